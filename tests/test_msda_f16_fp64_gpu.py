"""GPU: the fp16 instantiation of the fused MSDeformAttn core (dtype code 2 of include/vitadapter_hip.h) held to fp64.

One operand form: value / out / grad_out / grad_value and offsets / logits / d_offsets / d_logits all fp16 - what fp16
autocast hands MSDeformAttn.  The cases and the fp64 statement are oracle/msda_fused.py's: inputs(case, 'F4') rounded to
fp16 here, reference() on the rounded operands.  Direct calls of the C entry points (vah_msda_fused_forward, _forward_nref,
_forward_win, vah_msda_fused_backward_tiled, _backward_tiled_nref), every output and every workspace filled with NaN /
0xFF bytes first.

Tolerance, derived: the kernels widen fp16 exactly, compute in fp32 and round once at the store, so a result differs from
fp64 by half an fp16 ulp (2^-11 relative) plus the project's fp32 rule (1e-4 max(1, max|want|)); asserted per element is
    err <= 2^-10 |want| + 1e-4 max(1, max|want|)
- one full ulp, so that a value whose fp32 form sits on a rounding tie does not fail.  d_offsets under
oracle.msda_fused.smooth_mask (tests/test_msda_f16_abi_cpu.py pins that it keeps more than half of the samples with fp16
offsets).  Reports, not assertions (run with -s for the FIGURE lines): for grad_value err / (2^-21 abs_gv + 1e-6 max|want|),
the bound of an fp32 grad_value from weights split into fp16 hi + lo - behind an fp16 store it is dominated by the
store's own half ulp, 2^10 times larger - and therefore also the same ratio for the EXCESS of the error over half an
fp16 ulp of |want|, which bounds the error of the fp32 sum before the store, with the share of elements that are not
the correctly rounded fp64 value.  A matrix core that flushed the subnormal `lo` halves would lose up to 2^-14 per
weight: an excess ratio in the hundreds and a share of tens of percent."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import msda_fused as mfo

pytestmark = pytest.mark.gpu

H16 = torch.float16
F16 = 2                                     # dtype code
HALO = 5                                    # ops.functions.ms_deform_attn_fused.WIN_HALO
CASES = ['ext_ragged', 'inj_ragged', 'four_levels', 'shared_lists', 'wide_rows', 'borders', 'many_tiles']
PAD = 8


def _vah():
    import _vah
    return _vah


def _stream():
    return _vah().raw_stream(torch.device('cuda'))


def _nan(shape):
    return torch.full(tuple(shape), float('nan'), dtype=H16, device='cuda')


def _nan_bytes(n):
    return torch.full((max(int(n), 1),), 255, dtype=torch.uint8, device='cuda')     # 0xFFFF: NaN as fp16


def _call(name, *args):
    v = _vah()
    with v.on(torch.device('cuda')):
        rc = getattr(v.lib, name)(*args)
    v.check(rc, name)
    torch.cuda.synchronize()


def _f16_inputs(case, seed=0):
    """oracle inputs of form F4 with value, grad_out, offsets and logits rounded to fp16."""
    inp = mfo.inputs(case, 'F4', seed)
    inp.value, inp.grad_out = inp.value.to(H16), inp.grad_out.to(H16)
    inp.offsets, inp.logits = inp.offsets.to(H16).contiguous(), inp.logits.to(H16).contiguous()
    return inp


@functools.lru_cache(maxsize=None)
def _case(case, seed=0, backward=True):
    """(inputs, fp64 reference), computed once per case and shared by the tests; never modified."""
    inp = _f16_inputs(case, seed)
    return inp, mfo.reference(inp, backward=backward)


def _dev(inp, pad=None):
    """The operands on the GPU; pad: offsets / logits as views of one fp16 [offsets | logits | gap] matrix with rows of
    3 L P + pad halves and NaN in the gap."""
    N, M, D, P, Lq, L, S = inp.dims
    d = types.SimpleNamespace(value=inp.value.cuda(), gout=inp.grad_out.cuda(), ref=inp.ref.cuda().contiguous(),
                              shapes=inp.shapes.cuda(), lsi=inp.lsi.cuda(), params=None)
    if pad is None:
        d.offsets, d.logits = inp.offsets.cuda(), inp.logits.cuda()
        d.off, d.logit, d.os, d.ls = d.offsets.data_ptr(), d.logits.data_ptr(), 0, 0
    else:
        stride = 3 * L * P + pad
        d.params = _nan((N, Lq, M, stride))
        o, lg = mfo.param_views(d.params, L)
        o.copy_(inp.offsets)
        lg.copy_(inp.logits)
        d.off = d.params.data_ptr()
        d.logit = d.off + 2 * L * P * 2
        d.os = d.ls = stride
    return d


def _ref_arg(inp, d, per_image):
    """(ref tensor, ref_batch): the shared grid, or one copy of it per image (the same numbers through the rq term)."""
    N = inp.dims[0]
    if not per_image:
        return d.ref, 1
    return d.ref[None].repeat(N, 1, 1, 1).contiguous(), N


def _forward(inp, d, nref=None):
    N, M, D, P, Lq, L, S = inp.dims
    out = _nan((N, Lq, M * D))
    head = (d.value.data_ptr(), F16, d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit, F16, d.os, d.ls)
    tail = (N, S, M, D, L, Lq, P, out.data_ptr(), _stream())
    if nref is None:
        _call('vah_msda_fused_forward', *head, d.ref.data_ptr(), inp.ref_levels, *tail)
    else:
        ref, rb = _ref_arg(inp, d, nref)
        _call('vah_msda_fused_forward_nref', *head, ref.data_ptr(), inp.ref_levels, rb, *tail)
    return out


def _forward_win(inp, d):
    N, M, D, P, Lq, L, S = inp.dims
    out = _nan((N, Lq, M * D))
    n = _vah().lib.vah_msda_win_ws_bytes(S, Lq)
    assert n > 0
    ws = _nan_bytes(n)
    _call('vah_msda_fused_forward_win', d.value.data_ptr(), F16, d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit, F16,
          d.os, d.ls, d.ref.data_ptr(), N, S, M, D, Lq, P, HALO, ws.data_ptr(), ws.numel(), 0, out.data_ptr(), _stream())
    return out


def _backward(inp, d, nref=None, pad=None):
    """-> grad_value, d_offsets, d_logits (views for pad), the gradient matrix (pad) or None."""
    N, M, D, P, Lq, L, S = inp.dims
    gv = _nan((N, S, M, D))
    if pad is None:
        g = None
        d_off, d_logit = _nan((N, Lq, M, L, P, 2)), _nan((N, Lq, M, L * P))
        d_off_p, d_logit_p, dos, dls = d_off.data_ptr(), d_logit.data_ptr(), 0, 0
    else:
        stride = 3 * L * P + pad
        g = _nan_bytes(N * Lq * M * stride * 2).view(H16).view(N, Lq, M, stride)       # 0xFFFF words
        d_off, d_logit = mfo.param_views(g, L)
        d_off_p, d_logit_p, dos, dls = g.data_ptr(), g.data_ptr() + 2 * L * P * 2, stride, stride
    ws_bytes = _vah().lib.vah_msda_tile_ws_bytes(N, S, M, L, Lq, P)
    assert ws_bytes > 0
    ws = _nan_bytes(ws_bytes)
    head = (d.value.data_ptr(), F16, d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit, F16, d.os, d.ls)
    tail = (d.gout.data_ptr(), N, S, M, D, L, Lq, P, gv.data_ptr(), F16, d_off_p, d_logit_p, F16, dos, dls, ws.data_ptr(),
            ws_bytes, _stream())
    if nref is None:
        _call('vah_msda_fused_backward_tiled', *head, d.ref.data_ptr(), inp.ref_levels, *tail)
    else:
        ref, rb = _ref_arg(inp, d, nref)
        _call('vah_msda_fused_backward_tiled_nref', *head, ref.data_ptr(), inp.ref_levels, rb, *tail)
    return gv, d_off, d_logit, g


def _check(name, got, want, mask=None):
    """err <= 2^-10 |want| + 1e-4 max(1, max|want|) per element (module docstring)."""
    got = got.detach().double().cpu().numpy().reshape(want.shape)
    assert np.isfinite(got).all(), '%s: not finite' % name
    if mask is not None:
        assert mask.mean() > 0.5, 'more than half of the samples sit on a kink'
        got, want = np.where(mask, got, 0.0), np.where(mask, want, 0.0)
    err = np.abs(got - want)
    scale = float(np.abs(want).max())
    bound = 2.0 ** -10 * np.abs(want) + 1e-4 * max(1.0, scale)
    ratio = float((err / bound).max())
    print('FIGURE %s max_err %.3e scale %.3e ratio %.3f' % (name, float(err.max()), scale, ratio))
    assert (err <= bound).all(), '%s: %.3e, %.3f of its bound (max |ref| %.3e)' % (name, float(err.max()), ratio, scale)
    return err, scale


def _check_backward(tag, inp, want, gv, d_off, d_logit):
    err, scale = _check(tag + ' grad_value', gv, want.grad_value)
    hilo = float((err / (2.0 ** -21 * want.abs_gv + 1e-6 * scale)).max())
    print('FIGURE %s grad_value err / (2^-21 abs_gv + 1e-6 max|want|) = %.3f' % (tag, hilo))
    half_ulp = 0.5 * np.spacing(np.abs(want.grad_value).astype(np.float16)).astype(np.float64)
    excess = float(((err - half_ulp) / (2.0 ** -21 * want.abs_gv + 1e-6 * scale)).max())
    wrong = float((gv.cpu() != torch.from_numpy(want.grad_value).to(H16)).double().mean())
    print('FIGURE %s grad_value (err - half ulp) / (2^-21 abs_gv + 1e-6 max|want|) = %.3f, not correctly rounded: %.4f of the elements'
          % (tag, excess, wrong))
    _check(tag + ' d_logits', d_logit, want.d_logits)
    _check(tag + ' d_offsets', d_off, want.d_offsets, mask=mfo.smooth_mask(inp))


@pytest.mark.parametrize('case', CASES)
def test_forward(case):
    """vah_msda_fused_forward and _forward_nref (a shared grid, and one grid per image where the case has two images);
    on the single-level cases vah_msda_fused_forward_win as well."""
    inp, want = _case(case)
    d = _dev(inp)
    _check(case + ' out (8-lane)', _forward(inp, d), want.out)
    _check(case + ' out (8-lane, nref shared)', _forward(inp, d, nref=False), want.out)
    if inp.dims[0] > 1:
        _check(case + ' out (8-lane, nref per image)', _forward(inp, d, nref=True), want.out)
    if len(inp.levels) == 1:
        _check(case + ' out (windows)', _forward_win(inp, d), want.out)


@pytest.mark.parametrize('case', CASES)
def test_backward_tiled(case):
    inp, want = _case(case)
    d = _dev(inp)
    _check_backward(case + ' tiled', inp, want, *_backward(inp, d)[:3])
    per_image = inp.dims[0] > 1
    _check_backward(case + ' tiled nref %s' % ('per image' if per_image else 'shared'), inp, want,
                    *_backward(inp, d, nref=per_image)[:3])


def test_row_strided_parameters():
    """ext_ragged with offsets / logits in one fp16 matrix of row stride 3 L P + 8 (40 bytes: 8-byte aligned rows) and the
    gradients written into a second one: same results, and the NaN gap words are neither read nor overwritten."""
    inp, want = _case('ext_ragged')
    N, M, D, P, Lq, L, S = inp.dims
    d = _dev(inp, pad=PAD)
    stride = 3 * L * P + PAD
    assert stride == 20
    held = d.params.clone()
    _check('ext_ragged strided out (8-lane)', _forward(inp, d), want.out)
    _check('ext_ragged strided out (8-lane, nref per image)', _forward(inp, d, nref=True), want.out)
    _check('ext_ragged strided out (windows)', _forward_win(inp, d), want.out)
    for nref in (None, True):
        gv, d_off, d_logit, g = _backward(inp, d, nref=nref, pad=PAD)
        _check_backward('ext_ragged strided tiled%s' % (' nref' if nref else ''), inp, want, gv, d_off, d_logit)
        gap = g[..., stride - PAD:].contiguous().view(torch.int16)
        assert bool((gap == -1).all()), 'the gap words between the rows of the gradient matrix were written'
    assert torch.equal(d.params.view(torch.int16), held.view(torch.int16)), 'the parameter matrix was written'
    assert bool(torch.isnan(d.params[..., stride - PAD:]).all())


def test_invalid_level_contributes_nothing():
    """invalid_level_h0 (H = 0): every result is exactly zero, from every entry point."""
    inp = _f16_inputs('invalid_level_h0')
    d = _dev(inp)

    def zero(name, t):
        assert bool((t == 0).all()), '%s: %d of %d elements are not zero' % (name, int((t != 0).sum()), t.numel())

    zero('out (8-lane)', _forward(inp, d))
    zero('out (8-lane, nref)', _forward(inp, d, nref=False))
    zero('out (windows)', _forward_win(inp, d))
    for nref in (None, False):
        gv, d_off, d_logit, _ = _backward(inp, d, nref=nref)
        zero('grad_value', gv)
        zero('d_offsets', d_off)
        zero('d_logits', d_logit)


def test_grad_value_overflows_to_inf():
    """GradScaler finds an overflow by its infs: a grad_value beyond fp16's range has to be stored as +-inf, not
    saturated.  One 2 x 2 level, N = 1, M = 2, 256 queries on ONE reference point with zero offsets and equal logits,
    grad_out = 4096 (head 1: -4096): the samples sit at pixel (x, y) = (0.25, 0), so row 0 receives 256 * 4096 * (0.75,
    0.25) = (786 432, 262 144) - beyond 65 504 - and row 1 exactly nothing."""
    N, M, D, P, Lq, L, S = 1, 2, 32, 4, 256, 1, 4
    inp = types.SimpleNamespace(
        value=torch.randn(N, S, M, D, generator=torch.Generator().manual_seed(3)).to(H16),
        grad_out=torch.cat([torch.full((N, Lq, D), 4096.0), torch.full((N, Lq, D), -4096.0)], -1).to(H16),
        offsets=torch.zeros(N, Lq, M, L, P, 2, dtype=H16), logits=torch.zeros(N, Lq, M, L * P, dtype=H16),
        ref=torch.tensor([0.375, 0.25]).repeat(Lq, 1, 1).contiguous(), shapes=torch.tensor([[2, 2]]), lsi=torch.tensor([0]),
        levels=[(2, 2)], dims=(N, M, D, P, Lq, L, S), ref_levels=1)
    want = mfo.reference(inp)
    assert float(np.abs(want.grad_value[:, :2]).min()) > 65504.0 and float(np.abs(want.grad_value[:, 2:]).max()) == 0.0
    want16 = torch.from_numpy(want.grad_value).to(H16)
    inf = torch.isinf(want16)
    assert bool(inf[:, :2].all()) and not bool(inf[:, 2:].any())
    d = _dev(inp)
    _check('overflow out', _forward(inp, d), want.out)
    for nref in (None, False):
        gv, d_off, d_logit, _ = _backward(inp, d, nref=nref)
        gv = gv.cpu()
        assert torch.equal(gv[inf], want16[inf]), 'overflowing grad_value elements are not +-inf of the right sign'
        assert bool(torch.isfinite(gv[~inf]).all())
        assert bool((gv[~inf] == 0).all())
        assert bool(torch.isfinite(d_off).all()) and bool(torch.isfinite(d_logit).all())
        _check('overflow d_logits', d_logit, want.d_logits)
