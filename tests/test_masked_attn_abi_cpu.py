"""CPU: the masked cross-attention entry points (include/vitadapter_hip_masked_attn.h, csrc/masked_attn.hip), their binding
table (_vah.MCA_SIGNATURES) and the host-side argument checks.

The prototypes are held to the binding with the method of tests/test_resize_rows_abi_cpu.py, applied to the fifth header
and the fifth table; the other tables stay what they were.  Every call here is answered by the host-side validation
before anything touches a device (fake or null pointers that are never dereferenced)."""
import ctypes
import os
import re

import pytest

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_masked_attn.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
F32, BF16, F16 = 0, 1, 2
N, H, LQ, LK = 2, 8, 100, 1600
E = H * 32
NAMES = ('vah_mca_splits', 'vah_mca_ws_bytes', 'vah_mca_pack_mask', 'vah_mca_forward', 'vah_mca_backward')
KERNELS = NAMES[3:]
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}
FWD_OPS = ('q', 'k', 'v', 'out')
BWD_OPS = ('q', 'k', 'v', 'out', 'd_out', 'dq', 'dk', 'dv')


def _err():
    return lib.vah_last_error().decode()


def _param(text):
    if '*' in text:
        return (ctypes.c_void_p,)
    words = text.replace('const', '').split()
    assert len(words) == 2 and words[0] in SCALARS, 'parameter the test cannot read: %r' % text
    return (SCALARS[words[0]],)


def _prototypes():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r'\b(int64_t|int)\s*(vah_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        params = ' '.join(params.split())
        assert name not in out, name
        out[name] = (SCALARS[ret], [_param(p.strip()) for p in params.split(',')])
    return out


PROTOTYPES = _prototypes()


def _call(name, N=N, H=H, Lq=LQ, Lk=LK, D=32, scale=0.125, bits=P, lse=P, ws=P, ws_bytes=None, **ops):
    """ops: <operand>=(pointer, dtype, token stride, image stride) or <operand>_<field>=value for one field"""
    fwd = name.endswith('forward')

    def op(o):
        val = list(ops.get(o, (P, BF16, N * E, E)))
        for i, f in enumerate(('ptr', 'dt', 'ts', 'is')):
            if o + '_' + f in ops:
                val[i] = ops[o + '_' + f]
        return val

    ws_bytes = lib.vah_mca_ws_bytes(N, H, Lq, max(Lk, 1)) if ws_bytes is None else ws_bytes
    dims = [N, H, Lq, Lk, D, scale]
    if fwd:
        args = op('q') + op('k') + op('v') + [bits] + dims + op('out') + [lse, ws, ws_bytes, None]
    else:
        args = (op('q') + op('k') + op('v') + [bits] + op('out') + op('d_out') + [lse] + dims + op('dq') + op('dk') + op('dv')
                + [ws, ws_bytes, None])
    return getattr(lib, name)(*args)


def _ops(name):
    return FWD_OPS if name.endswith('forward') else BWD_OPS


def test_every_signature_matches_its_prototype():
    assert set(PROTOTYPES) == set(_vah.MCA_SIGNATURES) == set(NAMES)
    for name, (restype, params) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        got = list(fn.argtypes or [])
        assert got == list(_vah.MCA_SIGNATURES[name][1])
        assert len(got) == len(params), (name, len(got), len(params))
        for i, (g, allowed) in enumerate(zip(got, params)):
            assert g in allowed, (name, i, g, allowed)


@pytest.mark.parametrize('name', NAMES)
def test_library_exports_the_symbol(name):
    assert hasattr(ctypes.CDLL(_vah.LIB_PATH), name), name


def test_the_other_tables_are_untouched():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION
    assert len(_vah.EXPORTS) == 122 and len(_vah.SIGNATURES) == 79 and len(_vah.F16_TWINS) == 43
    assert len(_vah.GN_SIGNATURES) == 6 and len(_vah.BOX_SIGNATURES) == 2 and len(_vah.RESIZE_SIGNATURES) == 3
    others = set(_vah.EXPORTS) | set(_vah.BOX_SIGNATURES) | set(_vah.GN_SIGNATURES) | set(_vah.RESIZE_SIGNATURES)
    assert not set(_vah.MCA_SIGNATURES) & others
    for header in ('vitadapter_hip.h', 'vitadapter_hip_msda_box.h', 'vitadapter_hip_group_norm.h', 'vitadapter_hip_resize.h'):
        text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        assert 'vah_mca' not in text, header


def _rule(Lk):
    """the chunk rule as the header states it"""
    tiles = -(-Lk // 64)
    per = -(-tiles // min(16, tiles))
    return -(-tiles // per), 64 * per


def test_splits_and_workspace_follow_the_rule_in_the_header():
    text = open(HEADER).read()
    assert 'tiles_per_chunk = ceil(tiles / min(16, tiles))' in text and 'splits = ceil(tiles / tiles_per_chunk)' in text
    for Lk, want in ((1, 1), (64, 1), (65, 2), (129, 3), (400, 7), (1024, 16), (1025, 9), (1600, 13), (6400, 15), (100000, 16)):
        assert _rule(Lk)[0] == want, Lk
    for Lk in list(range(1, 300)) + [400, 1000, 1023, 1024, 1025, 1600, 1601, 6400, 25600, 100000, (1 << 30) - 1]:
        s, chunk = _rule(Lk)
        assert lib.vah_mca_splits(Lk) == s, Lk
        assert 1 <= s <= 16 and (s - 1) * chunk < Lk <= s * chunk, Lk       # no empty chunk
    assert lib.vah_mca_splits(0) == 0 and lib.vah_mca_splits(-5) == 0
    for n, h, lq, lk in ((1, 1, 1, 1), (2, 8, 100, 400), (2, 8, 100, 1600), (2, 8, 100, 6400), (1, 2, 33, 65), (3, 1, 1, 129)):
        R, S = n * h * lq, _rule(lk)[0]
        floats = 4 * -(-R // 4) + 34 * R * S
        assert lib.vah_mca_ws_bytes(n, h, lq, lk) == 16 * -(-floats // 4), (n, h, lq, lk)
    for dims in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-1, 1, 1, 1)):
        assert lib.vah_mca_ws_bytes(*dims) == 0


@pytest.mark.parametrize('name', KERNELS)
def test_bad_dims_and_unserved_shapes(name):
    for kw in (dict(N=-1), dict(H=0), dict(H=-1), dict(Lq=-1), dict(Lk=-1), dict(N=1 << 20), dict(H=1 << 16), dict(Lk=1 << 30)):
        assert _call(name, **kw) == E_SHAPE, (kw, _err())
        assert name in _err() and 'bad dims' in _err()
    assert _call(name, Lk=0) == E_SHAPE and 'no keys' in _err()
    for d in (16, 31, 64, 0):
        assert _call(name, D=d) == E_UNSUPPORTED and 'head_dim' in _err(), d
    assert _call(name, Lq=129) == E_UNSUPPORTED and '128' in _err()
    assert _call(name, Lq=128, ws=None) == E_NULL
    assert _call(name, D=64, N=0) == E_UNSUPPORTED                      # also where there is nothing to do
    for o in _ops(name):
        assert _call(name, **{o + '_dt': F32}) == E_UNSUPPORTED and 'fp32' in _err() and '(%s)' % o in _err()
        assert _call(name, **{o + '_dt': 3}) == E_UNSUPPORTED and 'dtype codes' in _err()
        assert _call(name, **{o + '_dt': -1}) == E_UNSUPPORTED
        assert _call(name, **{o + '_dt': F16}) == E_UNSUPPORTED and 'fp16 mixed with bf16' in _err()
    all_f16 = {o + '_dt': F16 for o in _ops(name)}
    assert _call(name, ws=None, **all_f16) == E_NULL and 'ws' in _err()     # passes every check up to the last


@pytest.mark.parametrize('name', KERNELS)
def test_null_pointers_and_empty_calls(name):
    for o in _ops(name):
        assert _call(name, **{o + '_ptr': None}) == E_NULL and 'null' in _err() and '(%s)' % o in _err() and name in _err()
    assert _call(name, bits=None) == E_NULL and 'bits' in _err()
    assert _call(name, lse=None) == E_NULL and 'lse' in _err()
    assert _call(name, ws=None) == E_NULL and 'ws' in _err()
    # nothing to write is not an error, and no pointer is read
    nothing = {o + '_ptr': None for o in _ops(name)}
    for kw in (dict(N=0), dict(Lq=0), dict(Lq=0, Lk=0)):
        assert _call(name, bits=None, lse=None, ws=None, ws_bytes=0, **kw, **nothing) == OK and _err() == '', kw
    assert _call(name, N=0, bits=None, lse=None, ws=None, ws_bytes=0, q_ptr=P + 2, k_ts=3) == OK


@pytest.mark.parametrize('name', KERNELS)
def test_alignment_strides_and_workspace(name):
    for o in _ops(name):
        for kw in ({o + '_ptr': P + 8}, {o + '_ptr': P + 2}, {o + '_ts': N * E + 4}, {o + '_is': E + 2}):
            assert _call(name, **kw) == E_ALIGN, (kw, _err())
            assert 'misaligned' in _err() and name in _err() and o in _err()
    assert _call(name, bits=P + 2) == E_ALIGN and _call(name, lse=P + 1) == E_ALIGN
    assert _call(name, bits=P + 4, lse=P + 4, ws=None) == E_NULL
    assert _call(name, ws=P + 8) == E_ALIGN and 'ws' in _err()
    need = lib.vah_mca_ws_bytes(N, H, LQ, LK)
    assert _call(name, ws_bytes=need - 1) == E_SHAPE and 'workspace too small' in _err()
    assert _call(name, ws_bytes=0) == E_SHAPE
    # the strided forms pass every check: k and v as column slices of a packed (Lk, N, 2E) projection, q as a slice of a
    # packed (Lq, N, 3E) one
    packed = dict(k=(P, BF16, N * 2 * E, 2 * E), v=(P + 2 * E, BF16, N * 2 * E, 2 * E), q_ts=N * 3 * E, q_is=3 * E)
    assert _call(name, ws=None, **packed) == E_NULL and 'ws' in _err()


def test_pack_mask_checks():
    def pack(x=P, dt=F32, rs=LK, is_=LQ * LK, N=N, Q=LQ, Lk=LK, bits=P):
        return lib.vah_mca_pack_mask(x, dt, rs, is_, N, Q, Lk, bits, None)
    for kw in (dict(N=-1), dict(Q=-1), dict(Lk=-1), dict(Lk=1 << 30), dict(N=1 << 20, Q=1 << 20)):
        assert pack(**kw) == E_SHAPE and 'bad dims' in _err(), kw
    assert pack(dt=3) == E_UNSUPPORTED and pack(dt=-1) == E_UNSUPPORTED and 'dtype codes' in _err()
    assert pack(x=None) == E_NULL and '(x)' in _err()
    assert pack(bits=None) == E_NULL and '(bits)' in _err()
    assert pack(x=P + 2) == E_ALIGN and pack(x=P + 2, dt=BF16, bits=None) == E_NULL and pack(bits=P + 2) == E_ALIGN
    assert pack(rs=-8) == E_SHAPE
    for kw in (dict(N=0), dict(Q=0), dict(Lk=0)):
        assert pack(x=None, bits=None, **kw) == OK and _err() == ''
