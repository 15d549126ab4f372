"""CPU: argument checking of the fp16 attention entry points (include/vitadapter_hip.h, *_f16).  Each one is the bf16
entry point's twin: for the same arguments it returns the same VAH_E_* code with the same message, the function name
changed.  Every call here is rejected (or has nothing to do) before anything touches a device."""
import pytest

import _vah

lib = _vah.lib
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
P = 4096           # a non-null, 16-byte aligned fake pointer: never dereferenced by a rejected call
S = 0.125


def _fwd(q=P, N=5, H=1, ld=192, out=P):
    return (q, P, P, ld, N * ld, 1, H, N, S, P, out, 64, P, None)


def _bwd(q=P, N=5, H=1, ld=192, dq=P):
    return (q, P, P, ld, N * ld, P, P, 64, P, 1, H, N, S, P, dq, P, P, 192, N * 192, None)


def _win_fwd(q=P, B=1, win=2, H=1, out=P):
    return (q, P, P, 192, B, 4, 6, win, H, S, P, out, 64, P, None)


def _win_bwd(q=P, B=1, win=2, H=1, dq=P):
    return (q, P, P, 192, P, P, 64, P, B, 4, 6, win, H, S, P, dq, P, P, 192, None)


def _bias_fwd(q=P, N=5, ldb=64, bias=P):
    return (q, P, P, 192, N * 192, 1, 1, N, S, bias, ldb, P, 64, P, None)


def _bias_bwd(q=P, N=5, ldb=64, bias=P):
    return (q, P, P, 192, N * 192, P, P, 64, P, 1, 1, N, S, bias, P, ldb, P, P, P, P, P, 192, N * 192, None)


def _relpos_build(table=P, N=5, ldb=64):
    return (table, P, 10, 2, N, ldb, P, P, None)


def _relpos_grad(ds=P, N=5, T=10):
    return (ds, P, 1, 2, N, 64, T, P, P, None)


# (bf16 entry, argument builder, [(case, kwargs, expected rc)])
CASES = [
    ('vah_attn_fwd_bf16', _fwd, [('bad dims', dict(H=0), E_SHAPE), ('null', dict(out=None), E_NULL),
                                 ('misaligned', dict(q=P + 2), E_ALIGN), ('ld', dict(ld=196), E_ALIGN),
                                 ('N == 0', dict(q=None, out=None, N=0), 0)]),
    ('vah_attn_bwd_bf16', _bwd, [('bad dims', dict(H=0), E_SHAPE), ('null', dict(dq=None), E_NULL),
                                 ('misaligned', dict(dq=P + 4), E_ALIGN), ('N == 0', dict(q=None, dq=None, N=0), 0)]),
    ('vah_attn_win_fwd_bf16', _win_fwd, [('bad dims', dict(win=0), E_SHAPE), ('bad window', dict(win=65), E_SHAPE),
                                         ('null', dict(out=None), E_NULL), ('misaligned', dict(q=P + 2), E_ALIGN),
                                         ('non-resident misaligned', dict(win=16, q=P + 2), E_ALIGN),
                                         ('no images', dict(q=None, out=None, B=0), 0)]),
    ('vah_attn_win_bwd_bf16', _win_bwd, [('bad dims', dict(win=0), E_SHAPE), ('null', dict(dq=None), E_NULL),
                                         ('misaligned', dict(q=P + 8), E_ALIGN),
                                         ('non-resident null', dict(win=16, dq=None), E_NULL),
                                         ('no images', dict(q=None, dq=None, B=0), 0)]),
    ('vah_attn_bias_fwd_bf16', _bias_fwd, [('bad dims', dict(ldb=60), E_SHAPE), ('ldb < N', dict(ldb=0), E_SHAPE),
                                           ('null', dict(bias=None), E_NULL), ('misaligned', dict(bias=P + 2), E_ALIGN),
                                           ('N == 0', dict(q=None, bias=None, N=0), 0)]),
    ('vah_attn_bias_bwd_bf16', _bias_bwd, [('bad dims', dict(ldb=60), E_SHAPE), ('null', dict(bias=None), E_NULL),
                                           ('misaligned', dict(q=P + 2), E_ALIGN), ('N == 0', dict(q=None, bias=None, N=0), 0)]),
    ('vah_relpos_bias_build', _relpos_build, [('bad dims', dict(ldb=4), E_SHAPE), ('null', dict(table=None), E_NULL),
                                              ('N == 0', dict(N=0), E_SHAPE)]),
    ('vah_relpos_bias_grad', _relpos_grad, [('bad dims', dict(T=1 << 20), E_SHAPE), ('null', dict(ds=None), E_NULL),
                                            ('N == 0', dict(N=0), E_SHAPE)]),
]


def _twin(name):
    return name[:-len('_bf16')] + '_f16' if name.endswith('_bf16') else name + '_f16'


@pytest.mark.parametrize('name,build,cases', CASES, ids=[c[0] for c in CASES])
def test_f16_entry_checks_arguments_like_its_bf16_twin(name, build, cases):
    f16 = _twin(name)
    assert f16 in _vah.EXPORTS
    for case, kw, want in cases:
        args = build(**kw)
        rc16 = getattr(lib, f16)(*args)
        msg16 = lib.vah_last_error().decode()
        rcb = getattr(lib, name)(*args)
        msgb = lib.vah_last_error().decode()
        assert rcb == want, (name, case, rcb, msgb)
        assert rc16 == want, (f16, case, rc16, msg16)
        if want:
            assert msg16.startswith(f16 + ':'), (case, msg16)
            assert msg16 == msgb.replace(name, f16), (case, msg16, msgb)
        else:
            assert msg16 == '', (case, msg16)


def test_f16_entries_share_the_workspace_queries():
    """The 16-bit sizes are the same for both types: one set of size queries serves both twins."""
    for n in ('vah_attn_padded_len', 'vah_attn_bwd_workspace_bytes', 'vah_relpos_bias_grad_ws_floats'):
        assert n in _vah.EXPORTS and n + '_f16' not in _vah.EXPORTS
    assert lib.vah_attn_bwd_workspace_bytes(2, 3, 100) == 3 * 2 * 3 * 64 * 128 * 2 + 2 * 3 * 100 * 4
    assert _vah.ABI_VERSION == lib.vah_abi_version() == 37
    for name, _, _ in CASES:
        assert getattr(lib, _twin(name)).argtypes == getattr(lib, name).argtypes
