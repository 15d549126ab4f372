"""CPU: argument checking of the fp16 SpatialPriorModule entry points (include/vitadapter_hip.h, the `_f16` twins of the
convolution kernels of csrc/conv.hip and the BatchNorm / max-pool / layout kernels of csrc/spm_nhwc.hip).  Each one is
its bf16 entry point's twin: for the same arguments it returns the same VAH_E_* code with the same message, the function
name changed.  Every call here is rejected (or has nothing to do) before anything touches a device: the zero-size
cases are those that return without a launch or a memset (the weight gradient with no images clears dw and the two
statistics passes with no rows still write their sums, so they are not among them)."""
import ctypes
import os
import re

import pytest

import _vah

lib = _vah.lib
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
P = 4096           # a non-null, 16-byte aligned fake pointer: never dereferenced by a rejected call
TAPS = (ctypes.c_int * 9)(*range(-4, 5))

TWINS = {
    'vah_conv_taps_nhwc_bf16': 'vah_conv_taps_nhwc_f16', 'vah_conv3x3_dgrad_nhwc_bf16': 'vah_conv3x3_dgrad_nhwc_f16',
    'vah_conv3x3_wgrad_nhwc_bf16': 'vah_conv3x3_wgrad_nhwc_f16', 'vah_image_to_nhwc16_bf16': 'vah_image_to_nhwc16_f16',
    'vah_bn_nhwc_stats': 'vah_bn_nhwc_stats_f16', 'vah_bn_nhwc_apply': 'vah_bn_nhwc_apply_f16',
    'vah_bn_nhwc_bwd_stats': 'vah_bn_nhwc_bwd_stats_f16', 'vah_bn_nhwc_bwd_apply': 'vah_bn_nhwc_bwd_apply_f16',
    'vah_maxpool3s2_nhwc_fwd_bf16': 'vah_maxpool3s2_nhwc_fwd_f16', 'vah_maxpool3s2_nhwc_bwd_bf16': 'vah_maxpool3s2_nhwc_bwd_f16',
}


def _taps(x=P, N=1, IH=8, IW=8, Cin=64, w=P, Cout=64, T=9, ty=TAPS, tx=TAPS, S=1, out=P, ny=8, nx=8, OH=8, OW=8, OS=1,
          oy0=0, ox0=0):
    return (x, N, IH, IW, Cin, w, Cout, T, ty, tx, S, out, ny, nx, OH, OW, OS, oy0, ox0, None)


def _dgrad(gy=P, N=1, OH=8, OW=8, Cout=64, wt=P, Cin=64, S=1, gx=P, H=8, W=8):
    return (gy, N, OH, OW, Cout, wt, Cin, S, gx, H, W, None)


def _wgrad(x=P, N=1, IH=8, IW=8, Cin=64, dy=P, OH=8, OW=8, Cout=64, S=1, ws=P, ws_floats=1 << 40, dw=P):
    return (x, N, IH, IW, Cin, dy, OH, OW, Cout, S, ws, ws_floats, dw, None)


def _image(x=P, N=1, H=8, W=8, y=P):
    return (x, N, H, W, y, None)


def _stats(x=P, rows=64, C=64, sums=P, ws=P):
    return (x, rows, C, sums, ws, None)


def _apply(x=P, rows=64, C=64, mean=P, rstd=P, y=P):
    return (x, rows, C, mean, rstd, None, None, 1, y, None)


def _bwd_stats(x=P, dy=P, rows=64, C=64, mean=P, sums=P):
    return (x, dy, rows, C, mean, P, None, None, 1, sums, P, None)


def _bwd_apply(x=P, dy=P, rows=64, C=64, mean_g=P, dx=P):
    return (x, dy, rows, C, P, P, None, None, 1, mean_g, P, dx, None)


def _pool_fwd(x=P, N=1, H=8, W=8, C=64, y=P, idx=P):
    return (x, N, H, W, C, y, idx, None)


def _pool_bwd(gy=P, idx=P, N=1, H=8, W=8, C=64, gx=P):
    return (gy, idx, N, H, W, C, gx, None)


# (bf16 entry, argument builder, [(case, kwargs, expected rc)])
CASES = [
    ('vah_conv_taps_nhwc_bf16', _taps, [
        ('Cin 32', dict(Cin=32), E_SHAPE), ('Cin 8', dict(Cin=8), E_SHAPE), ('Cin 80', dict(Cin=80), E_SHAPE),
        ('Cout 32', dict(Cout=32), E_SHAPE), ('Cout 96', dict(Cout=96), E_SHAPE), ('10 taps', dict(T=10), E_SHAPE),
        ('stride 3', dict(S=3), E_SHAPE), ('null taps', dict(ty=None), E_SHAPE), ('outputs leave', dict(ny=9), E_SHAPE),
        ('tap offset 5', dict(ty=(ctypes.c_int * 9)(5, 0, 0, 0, 0, 0, 0, 0, 0)), E_SHAPE),
        ('null in', dict(x=None), E_NULL), ('null out', dict(out=None), E_NULL), ('misaligned in', dict(x=P + 8), E_ALIGN),
        ('misaligned w', dict(w=P + 2), E_ALIGN), ('misaligned out', dict(out=P + 4), E_ALIGN),
        ('Cin 16 passes the channel rule', dict(Cin=16, x=None), E_NULL),
        ('no images', dict(x=None, out=None, N=0), 0), ('no rows', dict(x=None, out=None, ny=0), 0)]),
    ('vah_conv3x3_dgrad_nhwc_bf16', _dgrad, [
        ('Cin 16', dict(Cin=16), E_SHAPE), ('Cin 96', dict(Cin=96), E_SHAPE), ('Cout 32', dict(Cout=32), E_SHAPE),
        ('stride 3', dict(S=3), E_SHAPE), ('OH of another stride', dict(S=2), E_SHAPE), ('null gy', dict(gy=None), E_NULL),
        ('null gx', dict(gx=None), E_NULL), ('misaligned gy', dict(gy=P + 8), E_ALIGN), ('misaligned gx', dict(gx=P + 4), E_ALIGN),
        ('no images', dict(gy=None, gx=None, N=0), 0)]),
    ('vah_conv3x3_wgrad_nhwc_bf16', _wgrad, [
        ('Cin 32', dict(Cin=32), E_SHAPE), ('Cin 80', dict(Cin=80), E_SHAPE), ('Cout 96', dict(Cout=96), E_SHAPE),
        ('OH of another stride', dict(S=2), E_SHAPE), ('null dw', dict(dw=None), E_NULL), ('null ws', dict(ws=None), E_NULL),
        ('no images, null dw', dict(N=0, dw=None), E_NULL), ('null x', dict(x=None), E_NULL),
        ('misaligned x', dict(x=P + 8), E_ALIGN), ('misaligned dy', dict(dy=P + 2), E_ALIGN),
        ('workspace too small', dict(ws_floats=64 * 9 * 64 - 1), E_SHAPE),
        ('workspace too small, Cin 16, stride 2', dict(Cin=16, S=2, OH=4, OW=4, ws_floats=1), E_SHAPE)]),
    ('vah_image_to_nhwc16_bf16', _image, [
        ('bad dims', dict(H=0), E_SHAPE), ('negative N', dict(N=-1), E_SHAPE), ('null x', dict(x=None), E_NULL),
        ('null y', dict(y=None), E_NULL), ('misaligned y', dict(y=P + 8), E_ALIGN), ('no images', dict(x=None, y=None, N=0), 0)]),
    ('vah_bn_nhwc_stats', _stats, [
        ('C 96', dict(C=96), E_SHAPE), ('C 512', dict(C=512), E_SHAPE), ('C 4', dict(C=4), E_SHAPE), ('bad rows', dict(rows=-1), E_SHAPE),
        ('null x', dict(x=None), E_NULL), ('null sums', dict(sums=None), E_NULL), ('null ws', dict(ws=None), E_NULL)]),
    ('vah_bn_nhwc_apply', _apply, [
        ('C 96', dict(C=96), E_SHAPE), ('C 512', dict(C=512), E_SHAPE), ('bad rows', dict(rows=-1), E_SHAPE),
        ('null x', dict(x=None), E_NULL), ('null y', dict(y=None), E_NULL), ('null mean', dict(mean=None), E_NULL),
        ('no rows', dict(x=None, y=None, rows=0), 0)]),
    ('vah_bn_nhwc_bwd_stats', _bwd_stats, [
        ('C 96', dict(C=96), E_SHAPE), ('C 512', dict(C=512), E_SHAPE), ('null dy', dict(dy=None), E_NULL),
        ('null mean', dict(mean=None), E_NULL), ('null sums', dict(sums=None), E_NULL),
        ('no rows, null sums', dict(rows=0, sums=None), E_NULL)]),
    ('vah_bn_nhwc_bwd_apply', _bwd_apply, [
        ('C 96', dict(C=96), E_SHAPE), ('C 512', dict(C=512), E_SHAPE), ('null dy', dict(dy=None), E_NULL),
        ('null dx', dict(dx=None), E_NULL), ('null mean_g', dict(mean_g=None), E_NULL),
        ('no rows', dict(x=None, dy=None, dx=None, rows=0), 0)]),
    ('vah_maxpool3s2_nhwc_fwd_bf16', _pool_fwd, [
        ('C 12', dict(C=12), E_SHAPE), ('C 4', dict(C=4), E_SHAPE), ('H too large', dict(H=32768), E_SHAPE),
        ('null x', dict(x=None), E_NULL), ('null idx', dict(idx=None), E_NULL), ('no images', dict(x=None, y=None, idx=None, N=0), 0)]),
    ('vah_maxpool3s2_nhwc_bwd_bf16', _pool_bwd, [
        ('C 12', dict(C=12), E_SHAPE), ('W 0', dict(W=0), E_SHAPE), ('null gy', dict(gy=None), E_NULL),
        ('null gx', dict(gx=None), E_NULL), ('no images', dict(gy=None, gx=None, idx=None, N=0), 0)]),
]


def _twin(name):
    return name[:-len('_bf16')] + '_f16' if name.endswith('_bf16') else name + '_f16'


def test_the_ten_symbols_are_exported_and_declared():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vitadapter_hip.h')).read()
    assert len(TWINS) == 10
    for b16, f16 in TWINS.items():
        assert f16 == _twin(b16)
        assert f16 in _vah.EXPORTS and b16 in _vah.EXPORTS
        assert re.search(r'^int %s\(' % f16, header, re.M), f16
        assert getattr(lib, f16).argtypes == getattr(lib, b16).argtypes and getattr(lib, f16).restype is ctypes.c_int
    assert _vah.SPM_F16_TWINS == TWINS
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


def test_f16_twins_share_the_workspace_queries_and_the_abi_version():
    """Workspace sizes do not depend on the 16-bit type: one query serves both twins, vah_bn_finalize_stats is fp32 only;
    adding symbols does not move the ABI version."""
    for shared in ('vah_conv3x3_wgrad_ws_floats', 'vah_bn_nhwc_ws_floats', 'vah_bn_finalize_stats'):
        assert shared in _vah.EXPORTS and shared + '_f16' not in _vah.EXPORTS
    assert lib.vah_bn_nhwc_ws_floats(64) == 512 * 2 * 64
    assert lib.vah_conv3x3_wgrad_ws_floats(64, 64) % (64 * 9 * 64) == 0
    assert _vah.ABI_VERSION == lib.vah_abi_version() == 37


def test_host_gates_cpu():
    """The host's type questions without a device: the A/B switch, the symbol picked per type, the operand layouts in
    either type, and that nothing is usable without autocast (the autocast side needs a device: GPU tier)."""
    import torch
    from vitadapter import conv, fused, spm_nhwc
    assert fused.ENABLED['fp16_spm'] is True
    assert spm_nhwc.autocast_dtype() is None
    for b16, f16 in TWINS.items():
        assert (_vah.sym(b16, torch.bfloat16), _vah.sym(b16, torch.bfloat16).__name__) == (getattr(lib, b16), b16)
        assert (_vah.sym(b16, torch.float16), _vah.sym(b16, torch.float16).__name__) == (getattr(lib, f16), f16)
        assert _vah.sym(b16, torch.float16) is getattr(lib, f16)
    with pytest.raises(ValueError):
        _vah.sym('vah_conv_taps_nhwc_bf16', torch.float32)
    w = torch.randn(64, 16, 3, 3)
    for dtype in (torch.bfloat16, torch.float16):
        w9, wt9 = conv.forward_weight(w, dtype), conv.dgrad_weight(w, dtype)
        assert w9.dtype == wt9.dtype == dtype and w9.shape == (64, 9, 16) and wt9.shape == (16, 9, 64)
        assert torch.equal(w9[5, 7], w[5, :, 2, 1].to(dtype)) and torch.equal(wt9[3, 2], w[:, 3, 0, 2].to(dtype))
    assert conv.forward_weight(w).dtype == torch.bfloat16 and conv.dgrad_weight(w).dtype == torch.bfloat16
