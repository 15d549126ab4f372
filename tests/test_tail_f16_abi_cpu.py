"""CPU: argument checking of the fp16 output-tail entry points (include/vitadapter_hip.h, the `_f16` twins of the kernels
of csrc/tail_ops.hip: the four BatchNorm-tail passes, the token <-> plane transpose, the NCHW max-pool and the sub-pixel
interleave).  Each one is its bf16 entry point's twin: for the same arguments it returns the same VAH_E_* code with the
same message, the function name changed.  Every call here is rejected (or has nothing to do) before anything touches a
device: bad shapes, the two refusals of the tiling plan (N = 513; 256 x 256 at scale 4 with N = 171), null and
misaligned pointers, and the zero-size calls that return without a launch."""
import ctypes
import os
import re

import pytest

import _vah

lib = _vah.lib
E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer: never dereferenced by a rejected call

TWINS = {
    'vah_bn_tail_stats': 'vah_bn_tail_stats_f16', 'vah_bn_tail_apply': 'vah_bn_tail_apply_f16',
    'vah_bn_tail_bwd_stats': 'vah_bn_tail_bwd_stats_f16', 'vah_bn_tail_bwd_apply': 'vah_bn_tail_bwd_apply_f16',
    'vah_transpose_tokens': 'vah_transpose_tokens_f16', 'vah_maxpool3s2_fwd_bf16': 'vah_maxpool3s2_fwd_f16',
    'vah_maxpool3s2_bwd_bf16': 'vah_maxpool3s2_bwd_f16', 'vah_pixel_shuffle2_bf16': 'vah_pixel_shuffle2_f16',
}


def _ops(a=P, a16=1, b=None, b16=0, x=P, scale=4, N=2, C=8, H=32, W=32):
    return (a, a16, b, b16, x, scale, N, C, H, W)


def _stats(sums=P, ws=P, **kw):
    return _ops(**kw) + (None, sums, ws, None)


def _apply(mean=P, y=P, y16=0, **kw):
    return _ops(**kw) + (mean, P, None, None, 0, None, y, y16, None)


def _bwd_stats(mean=P, dy=P, dy16=0, sums=P, ws=P, **kw):
    return _ops(**kw) + (mean, P, None, None, 0, None, dy, dy16, sums, ws, None)


def _bwd_apply(mean=P, dy=P, dy16=0, mdy=P, da=P, db=None, dxlo=P, **kw):
    return _ops(**kw) + (mean, P, None, None, 0, None, dy, dy16, mdy, P, da, db, dxlo, None)


def _transpose(src=P, B=2, T_total=100, t0=0, T=50, C=50, dst=P, to_planes=1, planes16=1, vec=None):
    return (src, B, T_total, t0, T, C, dst, to_planes, planes16, vec, None)


def _pool_fwd(x=P, planes=4, H=8, W=8, y=P, idx=P):
    return (x, planes, H, W, y, idx, None)


def _pool_bwd(gy=P, idx=P, planes=4, H=8, W=8, gx=P):
    return (gy, idx, planes, H, W, gx, None)


def _shuffle(src=P, B=2, C=8, h=16, w=16, dst=P, inverse=0, add=None):
    return (src, B, C, h, w, dst, inverse, add, None)


# what every one of the four tail passes refuses through the shared shape rule / operand checks
_TAIL_COMMON = [
    ('W 30', dict(W=30), E_SHAPE), ('W 2', dict(W=2), E_SHAPE), ('W 8196', dict(W=8196, scale=1), E_SHAPE),
    ('N 0', dict(N=0), E_SHAPE), ('C 0', dict(C=0), E_SHAPE), ('H 0', dict(H=0), E_SHAPE),
    ('scale 3', dict(scale=3), E_SHAPE), ('scale 16', dict(scale=16), E_SHAPE),
    ('H not a multiple of the scale', dict(H=30), E_SHAPE), ('W / scale not a multiple of 4', dict(W=40, scale=4), E_SHAPE),
    ('too large', dict(N=512, C=1 << 16, H=1 << 10, W=1 << 12, scale=1), E_SHAPE),
    ('batch 513', dict(N=513), E_SHAPE),
    ('256 x 256 at scale 4, batch 171: the LDS tile', dict(N=171, C=2, H=256, W=256, scale=4), E_SHAPE),
    ('8192-wide rows at scale 8: the LDS tile', dict(N=1, C=1, H=64, W=8192, scale=8), E_SHAPE),
    ('null a', dict(a=None), E_NULL),
    ('misaligned 16-bit a', dict(a=P + 4), E_ALIGN), ('misaligned fp32 a', dict(a=P + 8, a16=0), E_ALIGN),
    ('misaligned fp32 b', dict(b=P + 8, b16=0), E_ALIGN), ('misaligned 16-bit b', dict(b=P + 2, b16=1), E_ALIGN),
    ('misaligned x', dict(x=P + 8), E_ALIGN),
]

# (bf16 entry, argument builder, [(case, kwargs, expected rc)])
CASES = [
    ('vah_bn_tail_stats', _stats, _TAIL_COMMON + [
        ('null sums', dict(sums=None), E_NULL), ('null ws', dict(ws=None), E_NULL)]),
    ('vah_bn_tail_apply', _apply, _TAIL_COMMON + [
        ('null mean', dict(mean=None), E_NULL), ('null y', dict(y=None), E_NULL),
        ('misaligned fp32 y', dict(y=P + 8), E_ALIGN), ('misaligned 16-bit y', dict(y=P + 4, y16=1), E_ALIGN)]),
    ('vah_bn_tail_bwd_stats', _bwd_stats, _TAIL_COMMON + [
        ('null mean', dict(mean=None), E_NULL), ('null dy', dict(dy=None), E_NULL), ('null sums', dict(sums=None), E_NULL),
        ('null ws', dict(ws=None), E_NULL), ('misaligned fp32 dy', dict(dy=P + 8), E_ALIGN),
        ('misaligned 16-bit dy', dict(dy=P + 4, dy16=1), E_ALIGN)]),
    ('vah_bn_tail_bwd_apply', _bwd_apply, _TAIL_COMMON + [
        ('null mean', dict(mean=None), E_NULL), ('null dy', dict(dy=None), E_NULL), ('null mdy', dict(mdy=None), E_NULL),
        ('misaligned 16-bit dy', dict(dy=P + 4, dy16=1), E_ALIGN), ('misaligned dxlo', dict(dxlo=P + 8), E_ALIGN),
        ('misaligned da', dict(da=P + 4), E_ALIGN), ('misaligned db', dict(db=P + 2), E_ALIGN)]),
    ('vah_transpose_tokens', _transpose, [
        ('range leaves the tokens', dict(t0=60), E_SHAPE), ('C 0', dict(C=0), E_SHAPE), ('negative B', dict(B=-1), E_SHAPE),
        ('B 65536', dict(B=65536), E_SHAPE), ('negative t0', dict(t0=-1), E_SHAPE),
        ('T 2^31', dict(T=1 << 31, T_total=1 << 32), E_SHAPE),
        ('null src', dict(src=None), E_NULL), ('null dst', dict(dst=None), E_NULL),
        ('vec with to_planes', dict(vec=P), E_UNSUPPORTED),
        ('no images', dict(src=None, dst=None, B=0), 0), ('no tokens', dict(src=None, dst=None, T=0), 0)]),
    ('vah_maxpool3s2_fwd_bf16', _pool_fwd, [
        ('H 0', dict(H=0), E_SHAPE), ('W 0', dict(W=0), E_SHAPE), ('negative planes', dict(planes=-1), E_SHAPE),
        ('H too large', dict(H=(1 << 20) + 1), E_SHAPE), ('too many planes', dict(planes=65536), E_SHAPE),
        ('null x', dict(x=None), E_NULL), ('null y', dict(y=None), E_NULL), ('null idx', dict(idx=None), E_NULL),
        ('no planes', dict(x=None, y=None, idx=None, planes=0), 0)]),
    ('vah_maxpool3s2_bwd_bf16', _pool_bwd, [
        ('H 0', dict(H=0), E_SHAPE), ('W too large', dict(W=(1 << 20) + 1), E_SHAPE), ('too many planes', dict(planes=65536), E_SHAPE),
        ('null gy', dict(gy=None), E_NULL), ('null idx', dict(idx=None), E_NULL), ('null gx', dict(gx=None), E_NULL),
        ('misaligned gx', dict(gx=P + 8), E_ALIGN), ('no planes', dict(gy=None, gx=None, idx=None, planes=0), 0)]),
    ('vah_pixel_shuffle2_bf16', _shuffle, [
        ('w 12', dict(w=12), E_SHAPE), ('w 4', dict(w=4), E_SHAPE), ('C 0', dict(C=0), E_SHAPE), ('h 0', dict(h=0), E_SHAPE),
        ('negative B', dict(B=-1), E_SHAPE), ('null src', dict(src=None), E_NULL), ('null dst', dict(dst=None), E_NULL),
        ('misaligned src', dict(src=P + 8), E_ALIGN), ('misaligned dst', dict(dst=P + 2), E_ALIGN),
        ('add with inverse', dict(inverse=1, add=P), E_SHAPE), ('misaligned add', dict(add=P + 8), E_SHAPE),
        ('no images', dict(src=None, dst=None, B=0), 0)]),
]


def _twin(name):
    return name[:-len('_bf16')] + '_f16' if name.endswith('_bf16') else name + '_f16'


def test_the_eight_symbols_are_exported_and_declared():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vitadapter_hip.h')).read()
    assert len(TWINS) == 8
    for b16, f16 in TWINS.items():
        assert f16 == _twin(b16)
        assert f16 in _vah.EXPORTS and b16 in _vah.EXPORTS
        assert re.search(r'^int %s\(' % f16, header, re.M), f16
        assert getattr(lib, f16).argtypes == getattr(lib, b16).argtypes and getattr(lib, f16).restype is ctypes.c_int
    assert _vah.TAIL_F16_TWINS == TWINS
    assert sorted(c[0] for c in CASES) == sorted(TWINS)


@pytest.mark.parametrize('name,build,cases', CASES, ids=[c[0] for c in CASES])
def test_f16_entry_checks_arguments_like_its_bf16_twin(name, build, cases):
    f16 = TWINS[name]
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
            assert msg16 == msgb.replace(name + ':', f16 + ':'), (case, msg16, msgb)
        else:
            assert msg16 == '', (case, msg16)


def test_the_plan_refusals_name_their_reason():
    """N = 513 is refused by the batch rule and 256 x 256 at scale 4 with N = 171 by the LDS tile, with the same words
    from either twin; N = 170 and N = 512 pass the plan (and stop at the null operand)."""
    for b16, f16 in list(TWINS.items())[:4]:
        build = dict((c[0], c[1]) for c in CASES)[b16]
        for name in (b16, f16):
            assert getattr(lib, name)(*build(N=513)) == E_SHAPE
            assert lib.vah_last_error().decode() == '%s: batch 513 above 512' % name
            assert getattr(lib, name)(*build(N=171, C=2, H=256, W=256, scale=4)) == E_SHAPE
            assert 'does not fit 150 KB of LDS' in lib.vah_last_error().decode()
            assert getattr(lib, name)(*build(N=170, C=2, H=256, W=256, scale=4, a=None)) == E_NULL
            assert getattr(lib, name)(*build(N=512, a=None)) == E_NULL


def test_f16_twins_share_the_shape_rule_the_workspace_query_and_the_abi_version():
    """The tiling plan and the workspace do not depend on the 16-bit type: vah_bn_tail_supported and
    vah_bn_tail_ws_floats serve both twins, vah_bn_finalize_stats is fp32 only; adding symbols does not move the ABI
    version."""
    for shared in ('vah_bn_tail_supported', 'vah_bn_tail_ws_floats', 'vah_bn_finalize_stats'):
        assert shared in _vah.EXPORTS and shared + '_f16' not in _vah.EXPORTS
        assert not hasattr(lib, shared + '_f16')
    assert lib.vah_bn_tail_ws_floats(768) == 512 * 2 * 768
    assert lib.vah_bn_tail_supported(2, 768, 256, 256, 4, 1) == 1
    assert lib.vah_bn_tail_supported(513, 8, 32, 32, 4, 1) == 0
    assert lib.vah_bn_tail_supported(171, 2, 256, 256, 4, 1) == 0 and lib.vah_bn_tail_supported(170, 2, 256, 256, 4, 1) == 1
    assert lib.vah_bn_tail_supported(171, 2, 256, 256, 4, 0) == 1          # without x there is no LDS tile
    # what vah_bn_tail_supported answers is what each twin does: same plan behind both
    for shape in ((513, 8, 32, 32, 4), (171, 2, 256, 256, 4), (170, 2, 256, 256, 4), (65, 2, 256, 256, 1), (1, 1, 64, 8192, 8)):
        N, C, H, W, s = shape
        ok = lib.vah_bn_tail_supported(N, C, H, W, s, 1)
        for name in ('vah_bn_tail_stats', 'vah_bn_tail_stats_f16'):
            rc = getattr(lib, name)(*_stats(N=N, C=C, H=H, W=W, scale=s, a=None))
            assert rc == (E_NULL if ok else E_SHAPE), (name, shape, rc)
    assert _vah.ABI_VERSION == lib.vah_abi_version() == 37


def test_host_gates_cpu():
    """The host's type questions without a device: the A/B switch, the symbol picked per type, and that nothing of the
    tail is fused without autocast (the autocast side needs a device: GPU tier)."""
    import torch
    from vitadapter import fused
    assert fused.ENABLED['fp16_tail'] is True
    assert fused.autocast_16('fp16_tail') is None and fused.tail_dtype() is None
    assert fused._maps_dtype() == torch.bfloat16
    for b16, f16 in TWINS.items():
        assert _vah.sym(b16, torch.bfloat16) is getattr(lib, b16)
        assert _vah.sym(b16, torch.float16) is getattr(lib, f16)
    for b16, f16 in _vah.FUSED_F16_TWINS.items():          # the row kernels' twins are still found
        assert _vah.sym(b16, torch.float16) is getattr(lib, f16)
    norm = torch.nn.BatchNorm2d(8)
    a = torch.randn(2, 8, 8, 8)
    assert not fused._bn_fusable(norm, a) and not fused.tail_takes_conv_bias(norm, a)
    y = fused.bn_tail(norm, a.half().float(), None, torch.randn(2, 8, 4, 4), 2)
    assert y.grad_fn is not None and not type(y.grad_fn).__name__.startswith('_BNTail')
