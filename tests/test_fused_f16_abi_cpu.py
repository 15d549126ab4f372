"""CPU: argument checking of the fp16 row-streaming entry points (include/vitadapter_hip.h, the `_f16` twins of the
LayerNorm / residual / DWConv kernels of csrc/fused_ops.hip).  Each one is its bf16 entry point's twin: for the same
arguments it returns the same VAH_E_* code with the same message, the function name changed.  Every call here is
rejected (or has nothing to do) before anything touches a device: the zero-row cases are those that return without a
memset of an output."""
import pytest

import _vah

lib = _vah.lib
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
P = 4096           # a non-null, 16-byte aligned fake pointer: never dereferenced by a rejected call
EPS = 1e-6


def _ln_fwd(x=P, rows=8, C=64, y=P):
    return (x, P, P, rows, C, EPS, y, P, P, None)


def _ln_bwd(x=P, g=P, rows=8, C=64, dw=P, gres=None):
    return (x, g, P, P, P, gres, rows, C, P, dw, P, P, None)


def _res_ln_fwd(x=P, z=P, gamma=None, batch=2, rpb=4, C=64, t=P, h=P):
    return (x, z, gamma, None, batch, rpb, C, P, P, EPS, t, h, P, P, None)


def _res_ln_bwd(t=P, gh=P, z=P, gamma=None, dgamma=None, batch=2, rpb=4, C=64, dz=P, dw=P):
    return (t, gh, P, P, P, None, z, gamma, None, batch, rpb, C, P, dz, dgamma, dw, P, P, None)


def _dual_fwd(x=P, rows=8, C=64, ya=P, yb=P):
    return (x, P, P, P, P, rows, C, EPS, ya, yb, P, P, None)


def _dual_bwd(x=P, ga=P, gb=P, rows=8, C=64, dparams=P, gres=None):
    return (x, ga, gb, P, P, P, P, gres, rows, C, P, dparams, P, None)


def _sr_fwd(x=P, z=P, gamma=None, batch=2, rpb=4, C=64, y=P):
    return (x, z, gamma, None, batch, rpb, C, y, None)


def _sr_bwd(g=P, z=P, gamma=None, batch=2, rpb=4, C=64, dz=P, dgamma=None, ws=None):
    return (g, z, gamma, None, batch, rpb, C, dz, dgamma, ws, None)


def _dwconv(x=P, bias=None, B=1, H=4, W=4, C=64, mode=0, y=P):
    return (x, P, bias, B, H, W, C, mode, y, None)


def _dwconv_wgrad(x=P, g=P, B=1, H=4, W=4, C=64, dw=P):
    return (x, g, B, H, W, C, dw, P, P, None)


# (bf16 entry, argument builder, [(case, kwargs, expected rc)])
CASES = [
    ('vah_layernorm_fwd_f32_bf16', _ln_fwd, [
        ('C % 4', dict(C=66), E_SHAPE), ('C too large', dict(C=4096), E_SHAPE), ('bad rows', dict(rows=-1), E_SHAPE),
        ('null', dict(y=None), E_NULL), ('misaligned x', dict(x=P + 8), E_ALIGN), ('misaligned y', dict(y=P + 2), E_ALIGN),
        ('zero rows', dict(x=None, y=None, rows=0), 0)]),
    ('vah_layernorm_bwd_f32_bf16', _ln_bwd, [
        ('C % 4', dict(C=66), E_SHAPE), ('C too large', dict(C=4096), E_SHAPE), ('null dw', dict(dw=None), E_NULL),
        ('zero rows, null dw', dict(rows=0, dw=None), E_NULL), ('null x', dict(x=None), E_NULL),
        ('misaligned g', dict(g=P + 4), E_ALIGN), ('misaligned gres', dict(gres=P + 8), E_ALIGN)]),
    ('vah_residual_layernorm_fwd', _res_ln_fwd, [
        ('bad dims', dict(batch=-1), E_SHAPE), ('null z', dict(z=None), E_NULL), ('null t', dict(t=None), E_NULL),
        ('misaligned z', dict(z=P + 4), E_ALIGN), ('misaligned gamma', dict(gamma=P + 8), E_ALIGN),
        ('C % 4', dict(C=66), E_SHAPE), ('null h', dict(h=None), E_NULL), ('zero rows', dict(z=None, t=None, batch=0), 0)]),
    ('vah_residual_layernorm_bwd', _res_ln_bwd, [
        ('bad dims', dict(rpb=-1), E_SHAPE), ('null z', dict(z=None), E_NULL), ('null dz', dict(dz=None), E_NULL),
        ('gamma without dgamma', dict(gamma=P), E_NULL), ('dgamma without gamma', dict(dgamma=P), E_NULL),
        ('misaligned dz', dict(dz=P + 2), E_ALIGN), ('C % 4', dict(C=66), E_SHAPE), ('null dw', dict(dw=None), E_NULL),
        ('misaligned gh', dict(gh=P + 4), E_ALIGN)]),
    ('vah_layernorm_dual_fwd', _dual_fwd, [
        ('C % 4', dict(C=66), E_SHAPE), ('C too large', dict(C=2048), E_SHAPE), ('null', dict(yb=None), E_NULL),
        ('misaligned x', dict(x=P + 4), E_ALIGN), ('misaligned ya', dict(ya=P + 4), E_ALIGN),
        ('zero rows', dict(x=None, ya=None, rows=0), 0)]),
    ('vah_layernorm_dual_bwd', _dual_bwd, [
        ('C % 4', dict(C=66), E_SHAPE), ('C too large', dict(C=2048), E_SHAPE), ('null dparams', dict(dparams=None), E_NULL),
        ('zero rows, null dparams', dict(rows=0, dparams=None), E_NULL), ('null x', dict(x=None), E_NULL),
        ('misaligned ga', dict(ga=P + 2), E_ALIGN), ('misaligned gres', dict(gres=P + 4), E_ALIGN)]),
    ('vah_scale_residual_fwd', _sr_fwd, [
        ('bad dims', dict(batch=-1), E_SHAPE), ('C % 4', dict(C=6), E_SHAPE), ('null', dict(z=None), E_NULL),
        ('misaligned z', dict(z=P + 4), E_ALIGN), ('misaligned y', dict(y=P + 8), E_ALIGN),
        ('zero rows', dict(x=None, z=None, y=None, rpb=0), 0)]),
    ('vah_scale_residual_bwd', _sr_bwd, [
        ('bad dims', dict(rpb=-1), E_SHAPE), ('C % 4', dict(C=6), E_SHAPE), ('null dz', dict(dz=None), E_NULL),
        ('dgamma without ws', dict(gamma=P, dgamma=P), E_NULL), ('misaligned dz', dict(dz=P + 4), E_ALIGN),
        ('misaligned g', dict(g=P + 8), E_ALIGN), ('zero rows', dict(g=None, z=None, dz=None, batch=0), 0)]),
    ('vah_dwconv3x3_tokens_bf16', _dwconv, [
        ('odd H', dict(H=3), E_SHAPE), ('C too large', dict(C=1028), E_SHAPE), ('C % 4', dict(C=6), E_SHAPE),
        ('null', dict(y=None), E_NULL), ('misaligned x', dict(x=P + 4), E_ALIGN), ('misaligned bias', dict(bias=P + 8), E_ALIGN),
        ('too many tokens', dict(B=1 << 20, H=64, W=64), E_SHAPE), ('no images', dict(x=None, y=None, B=0), 0),
        ('no images, dgrad', dict(x=None, y=None, B=0, mode=1), 0)]),
    ('vah_dwconv3x3_tokens_wgrad_bf16', _dwconv_wgrad, [
        ('odd W', dict(W=5), E_SHAPE), ('C too large', dict(C=1028), E_SHAPE), ('null dw', dict(dw=None), E_NULL),
        ('no images, null dw', dict(B=0, dw=None), E_NULL), ('null g', dict(g=None), E_NULL),
        ('misaligned g', dict(g=P + 2), E_ALIGN)]),
]


def _twin(name):
    return name[:-len('_bf16')] + '_f16' if name.endswith('_bf16') else name + '_f16'


def test_the_table_covers_the_ten_twins():
    assert sorted(_twin(c[0]) for c in CASES) == sorted(_vah.FUSED_F16_TWINS.values())
    assert all(_vah.FUSED_F16_TWINS[c[0]] == _twin(c[0]) for c in CASES) and len(CASES) == 10


@pytest.mark.parametrize('name,build,cases', CASES, ids=[c[0] for c in CASES])
def test_f16_entry_checks_arguments_like_its_bf16_twin(name, build, cases):
    f16 = _twin(name)
    assert f16 in _vah.EXPORTS
    assert getattr(lib, f16).argtypes == getattr(lib, name).argtypes
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


def test_f16_twins_share_the_workspace_query_and_the_abi_version():
    """Workspace sizes do not depend on the 16-bit type: one query serves both twins; adding symbols does not move the
    ABI version."""
    assert 'vah_reduce_ws_floats' in _vah.EXPORTS and 'vah_reduce_ws_floats_f16' not in _vah.EXPORTS
    assert lib.vah_reduce_ws_floats(3 * 768) == 512 * 3 * 768
    assert _vah.ABI_VERSION == lib.vah_abi_version() == 37


def test_host_gates_cpu():
    """fused.py's type questions without a device: which 16-bit types the row kernels take, the A/B switch, the symbol
    picked per type, and that CPU tensors take the torch expressions (the autocast side needs a device: GPU tier)."""
    import torch
    from vitadapter import fused
    assert fused.ENABLED['fp16_rows'] is True
    assert fused.takes_16(torch.bfloat16, 'fp16_rows') and fused.takes_16(torch.float16, 'fp16_rows') and not fused.takes_16(torch.float32, 'fp16_rows')
    assert fused.autocast_16('fp16_rows') is None
    fused.ENABLED['fp16_rows'] = False
    try:
        assert fused.takes_16(torch.bfloat16, 'fp16_rows') and not fused.takes_16(torch.float16, 'fp16_rows')
    finally:
        fused.ENABLED['fp16_rows'] = True
    for b16, f16 in _vah.FUSED_F16_TWINS.items():
        assert _vah.sym(b16, torch.bfloat16) is getattr(lib, b16)
        assert _vah.sym(b16, torch.float16) is getattr(lib, f16)
    norm = torch.nn.LayerNorm(8)
    x, z = torch.randn(2, 3, 8), torch.randn(2, 3, 8).half()
    t, h = fused.residual_ln(x, z, None, None, norm)
    assert torch.equal(t, x + z) and torch.equal(h, norm(x + z))
    assert torch.equal(fused.residual(x, z), x + z)
    assert fused.dwconv_tokens(torch.nn.Conv2d(8, 8, 3, 1, 1, groups=8), torch.randn(1, 21, 8).half(), 2, 2) is None
