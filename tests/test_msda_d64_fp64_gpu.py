"""GPU: the fused MSDeformAttn core at D = 64 (ViT-Adapter-S: 384 channels over 6 deformable heads) held to fp64.

Direct calls of the C entry points (vah_msda_fused_forward[_nref], vah_msda_fused_forward_win,
vah_msda_fused_backward_tiled[_nref]) in the style of tests/test_msda_fused_fp64_gpu.py: one call per entry point and
case, every output and every workspace filled with NaN / 0xFF bytes first.  The workspace of the tiled backward is
asked for 2 M head slices (include/vitadapter_hip.h: vah_msda_tile_ws_bytes counts 32-channel slices).

Operands: oracle.msda_fused.inputs(case, form, seed) for the geometry, offsets, logits and reference points - the
oracle's own offsets, so the share of samples off a kink is what its cases already have - with value and grad_out
replaced by oracle.seeded.randn tensors of width 64 under keys of their own, rounded to the form's dtype.  The fp64
statement (oracle.msda_fused.reference), smooth_mask, check and bounds(form) read the sizes from the operands and are
used as they stand: the bounds are storage-rounding rules plus the project's fp32 rule, and neither depends on the
length of the dot product once there is a single rounding.  The all-fp16 form has the cases and the derived bound of
tests/test_msda_f16_fp64_gpu.py: err <= 2^-10 |want| + 1e-4 max(1, max|want|).

At D = 64 the tile pass keeps a sample's {d(offset), d(out)/d(p)} as two fp32 partial records, one per 32-channel
half-head, added and rounded once by the finishing pass: d_offsets / d_logits are held to the same bounds as at D = 32.
Run with -s for one FIGURE line per checked tensor."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import msda as oracle_msda
from oracle import msda_fused as mfo
from oracle import seeded

pytestmark = pytest.mark.gpu

D64 = 64
H16 = torch.float16
_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
HALO = 5                                    # ops.functions.ms_deform_attn_fused.WIN_HALO
FIRST = ['ext_ragged', 'inj_ragged', 'four_levels']
ALL_FORMS = ('F1', 'F1p', 'F2', 'F3', 'F4', 'F5')
NON_TILING = 'non_tiling_overlapping_levels'

FORWARD = ([(c, f) for c in FIRST for f in ALL_FORMS] +
           [(c, 'F1') for c in ('inj_ragged_ref3', 'shared_lists', 'wide_rows', 'many_tiles', 'borders', NON_TILING)] +
           [(c, f) for c in ('long_queries', 'many_groups') for f in ('F1', 'F4')])
TILED = ([(c, f) for c in FIRST for f in ALL_FORMS] +
         [(c, 'F1') for c in ('inj_ragged_ref3', 'shared_lists', 'wide_rows', 'many_tiles', 'borders')] +
         [(NON_TILING, 'F1'), (NON_TILING, 'F4')])
F16_CASES = ['ext_ragged', 'inj_ragged', 'four_levels', 'shared_lists', 'wide_rows', 'borders', 'many_tiles']


def _vah():
    import _vah
    return _vah


def _stream():
    return _vah().raw_stream(torch.device('cuda'))


def _nan(shape, dtype):
    return torch.full(tuple(shape), float('nan'), dtype=dtype, device='cuda')


def _nan_bytes(n):
    return torch.full((max(int(n), 1),), 255, dtype=torch.uint8, device='cuda')     # 0xFF..: NaN as fp32, bf16 and fp16


def _call(name, *args):
    v = _vah()
    with v.on(torch.device('cuda')):
        rc = getattr(v.lib, name)(*args)
    v.check(rc, name)
    torch.cuda.synchronize()


def _inputs(case, form, seed=0):
    """oracle.msda_fused.inputs with 64-channel value / grad_out; form 'F16': everything fp16 (from F4, contiguous)."""
    f16 = form == 'F16'
    inp = mfo.inputs(case, 'F4' if f16 else form, seed)
    N, M, _, P, Lq, L, S = inp.dims
    vdt = H16 if f16 else inp.f.value
    key = 'msda_d64/' + case
    inp.value = seeded.randn(key + '/value', (N, S, M, D64), seed).to(vdt)
    inp.grad_out = seeded.randn(key + '/gout', (N, Lq, M * D64), seed).to(vdt)
    inp.dims = (N, M, D64, P, Lq, L, S)
    inp.vdt, inp.pdt = vdt, H16 if f16 else inp.f.param
    inp.gvdt, inp.gpdt = (H16, H16) if f16 else (inp.f.gv, inp.f.gparam)
    if f16:
        inp.offsets, inp.logits = inp.offsets.to(H16).contiguous(), inp.logits.to(H16).contiguous()
    return inp


@functools.lru_cache(maxsize=None)
def _case(case, form, seed=0, backward=True):
    """(inputs, reference), computed once per (case, form, seed) and shared by the tests; never modified."""
    inp = _inputs(case, form, seed)
    return inp, mfo.reference(inp, backward=backward and not inp.forward_only)


def _dev(inp, ref=None):
    """The operands on the GPU.  off / logit: device pointers; os / ls: row strides as the ABI takes them."""
    N, M, D, P, Lq, L, S = inp.dims
    d = types.SimpleNamespace(value=inp.value.cuda(), gout=inp.grad_out.cuda(),
                              ref=(inp.ref if ref is None else ref).cuda().contiguous(),
                              shapes=inp.shapes.cuda(), lsi=inp.lsi.cuda(), params=None)
    if inp.params is not None:
        d.params = inp.params.cuda()
        d.off = d.params.data_ptr()
        d.logit = d.off + 2 * L * P * d.params.element_size()
        d.os = d.ls = inp.stride
    else:
        d.offsets, d.logits = inp.offsets.cuda(), inp.logits.cuda()
        d.off, d.logit, d.os, d.ls = d.offsets.data_ptr(), d.logits.data_ptr(), 0, 0
    return d


def _forward(inp, d, ref_batch=None):
    N, M, D, P, Lq, L, S = inp.dims
    out = _nan((N, Lq, M * D), inp.vdt)
    head = (d.value.data_ptr(), _DT[inp.vdt], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit, _DT[inp.pdt], d.os, d.ls,
            d.ref.data_ptr(), inp.ref_levels)
    tail = (N, S, M, D, L, Lq, P, out.data_ptr(), _stream())
    if ref_batch is None:
        _call('vah_msda_fused_forward', *head, *tail)
    else:
        _call('vah_msda_fused_forward_nref', *head, ref_batch, *tail)
    return out


def _win_ws(inp):
    N, M, D, P, Lq, L, S = inp.dims
    n = _vah().lib.vah_msda_win_ws_bytes(S, Lq)
    assert n > 0
    return _nan_bytes(n)


def _forward_win(inp, d, ws, holds_schedule):
    N, M, D, P, Lq, L, S = inp.dims
    out = _nan((N, Lq, M * D), inp.vdt)
    _call('vah_msda_fused_forward_win', d.value.data_ptr(), _DT[inp.vdt], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit,
          _DT[inp.pdt], d.os, d.ls, d.ref.data_ptr(), N, S, M, D, Lq, P, HALO, ws.data_ptr(), ws.numel(), int(holds_schedule),
          out.data_ptr(), _stream())
    return out


def _backward_tiled(inp, d, ref_batch=None):
    """-> grad_value, d_offsets, d_logits (views of the gradient matrix for the interleaved forms), that matrix or None."""
    N, M, D, P, Lq, L, S = inp.dims
    gv = _nan((N, S, M, D), inp.gvdt)
    if inp.params is not None:
        esz = 2 if inp.gpdt != torch.float32 else 4
        g = _nan_bytes(N * Lq * M * inp.stride * esz).view(inp.gpdt).view(N, Lq, M, inp.stride)
        d_off, d_logit = mfo.param_views(g, L)
        d_off_p, d_logit_p, dos, dls = g.data_ptr(), g.data_ptr() + 2 * L * P * esz, inp.stride, inp.stride
    else:
        g = None
        d_off, d_logit = _nan((N, Lq, M, L, P, 2), inp.gpdt), _nan((N, Lq, M, L * P), inp.gpdt)
        d_off_p, d_logit_p, dos, dls = d_off.data_ptr(), d_logit.data_ptr(), 0, 0
    ws_bytes = _vah().lib.vah_msda_tile_ws_bytes(N, S, M * (D // 32), L, Lq, P)
    assert ws_bytes > 0
    ws = _nan_bytes(ws_bytes)
    head = (d.value.data_ptr(), _DT[inp.vdt], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit, _DT[inp.pdt], d.os, d.ls,
            d.ref.data_ptr(), inp.ref_levels)
    tail = (d.gout.data_ptr(), N, S, M, D, L, Lq, P, gv.data_ptr(), _DT[inp.gvdt], d_off_p, d_logit_p, _DT[inp.gpdt], dos, dls,
            ws.data_ptr(), ws_bytes, _stream())
    if ref_batch is None:
        _call('vah_msda_fused_backward_tiled', *head, *tail)
    else:
        _call('vah_msda_fused_backward_tiled_nref', *head, ref_batch, *tail)
    return gv, d_off, d_logit, g


def _check_backward(tag, want, mask, gv, d_off, d_logit, rules):
    mfo.check(tag + ' grad_value', gv, want.grad_value, rules['grad_value'], abs_gv=want.abs_gv)
    mfo.check(tag + ' d_logits', d_logit, want.d_logits, rules['d_logits'])
    mfo.check(tag + ' d_offsets', d_off, want.d_offsets, rules['d_offsets'], mask=mask)


@pytest.mark.parametrize('case,form', FORWARD)
def test_forward(case, form):
    """vah_msda_fused_forward (16 channel lanes per row) on every case; on the single-level ones
    vah_msda_fused_forward_win (a lane per half-head row) as well: once building its schedule, then with new offsets
    and logits on the untouched workspace."""
    inp, want = _case(case, form)
    d = _dev(inp)
    rule = mfo.bounds(form)['out']
    tag = 'd64 %s %s' % (case, form)
    mfo.check(tag + ' out (16-lane)', _forward(inp, d), want.out, rule)
    if len(inp.levels) > 1:
        return
    ws = _win_ws(inp)
    mfo.check(tag + ' out (windows)', _forward_win(inp, d, ws, False), want.out, rule)
    held = ws.clone()
    inp2, want2 = _case(case, form, 1, False)
    assert torch.equal(inp2.ref, inp.ref) and not torch.equal(inp2.logits, inp.logits)
    mfo.check(tag + ' out (windows, schedule reused)', _forward_win(inp2, _dev(inp2), ws, True), want2.out, rule)
    assert torch.equal(ws, held), 'the forward kernel wrote to its workspace'


@pytest.mark.parametrize('case,form', TILED)
def test_backward_tiled(case, form):
    inp, want = _case(case, form)
    d = _dev(inp)
    gv, d_off, d_logit, g = _backward_tiled(inp, d)
    _check_backward('d64 %s %s tiled' % (case, form), want, mfo.smooth_mask(inp), gv, d_off, d_logit, mfo.bounds(form))
    if inp.f.pad:
        gap = g[..., inp.stride - inp.f.pad:].contiguous().view(torch.int16)
        assert bool((gap == -1).all()), 'the gap words between the rows of the gradient matrix were written'
        assert bool(torch.isnan(d.params[..., inp.stride - inp.f.pad:]).all())


# ---- the all-fp16 form ------------------------------------------------------------------------------------------
def _check_f16(name, got, want, mask=None):
    """err <= 2^-10 |want| + 1e-4 max(1, max|want|) per element (tests/test_msda_f16_fp64_gpu.py)."""
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


@pytest.mark.parametrize('case', F16_CASES)
def test_f16_forward(case):
    inp, want = _case(case, 'F16')
    d = _dev(inp)
    _check_f16('d64 f16 %s out (16-lane)' % case, _forward(inp, d), want.out)
    if len(inp.levels) == 1:
        _check_f16('d64 f16 %s out (windows)' % case, _forward_win(inp, d, _win_ws(inp), False), want.out)


@pytest.mark.parametrize('case', F16_CASES)
def test_f16_backward_tiled(case):
    inp, want = _case(case, 'F16')
    gv, d_off, d_logit, _ = _backward_tiled(inp, _dev(inp))
    tag = 'd64 f16 %s tiled' % case
    _check_f16(tag + ' grad_value', gv, want.grad_value)
    _check_f16(tag + ' d_logits', d_logit, want.d_logits)
    _check_f16(tag + ' d_offsets', d_off, want.d_offsets, mask=mfo.smooth_mask(inp))


# ---- reference points per image ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _per_image_case(case, form):
    """(inputs, (N, Lq, RL, 2) grid, fp64 reference, kink mask): the case's grid times a ratio per image, jittered (the
    recipe of tests/test_msda_nref_fp64_gpu.py); the reference is oracle.msda_fused.reference's body with ref[n]."""
    inp = _inputs(case, form, 1)
    N, M, _, P, Lq, L, S = inp.dims
    assert N > 1
    key = 'msda_d64_nref/' + case
    ratio = 0.6 + 0.4 * seeded.rand(key + '/ratio', (N, 1, 1, 2), 1)
    ratio[0] = 1.0
    ref = (inp.ref[None].repeat(N, 1, 1, 1) * ratio + 0.01 * seeded.randn(key + '/jitter', (N,) + tuple(inp.ref.shape), 1))
    ref = ref.float().contiguous()
    assert float((ref[1] - ref[0]).abs().max()) >= 0.1          # a kernel that ignores n is wrong by far more than a bound
    wh = torch.tensor([[w, h] for h, w in inp.levels], dtype=torch.float64)[None, None, None, :, None, :]
    loc = ref.double()[:, :, None, :, None, :] + inp.offsets.double() / wh
    px = loc * wh - 0.5
    mask = ((px - px.round()).abs() > 1e-3).all(-1, keepdim=True).expand_as(px).numpy()
    v, g = inp.value.double().numpy(), inp.grad_out.double().numpy()
    p = torch.softmax(inp.logits.double(), -1)
    attn = p.view(N, Lq, M, L, P).numpy()
    hw, lsi, loc = inp.shapes.numpy(), inp.lsi.numpy(), loc.numpy()
    want = types.SimpleNamespace(out=oracle_msda.forward(v, hw, lsi, loc, attn))
    want.grad_value, gl, ga = oracle_msda.backward(v, hw, lsi, loc, attn, g)
    want.d_offsets = (torch.from_numpy(gl) / wh).numpy()
    ga = torch.from_numpy(ga).view(N, Lq, M, L * P)
    want.d_logits = (p * (ga - (p * ga).sum(-1, keepdim=True))).numpy()
    want.abs_gv = oracle_msda.backward(v, hw, lsi, loc, attn, np.abs(g))[0]
    return inp, ref, want, mask


def test_forward_nref_per_image():
    inp, ref, want, _ = _per_image_case('inj_ragged', 'F1')
    d = _dev(inp, ref)
    mfo.check('d64 inj_ragged F1 nref out', _forward(inp, d, ref_batch=inp.dims[0]), want.out, mfo.bounds('F1')['out'])


def test_backward_tiled_nref_per_image():
    inp, ref, want, mask = _per_image_case('inj_ragged', 'F1')
    d = _dev(inp, ref)
    gv, d_off, d_logit, _ = _backward_tiled(inp, d, ref_batch=inp.dims[0])
    _check_backward('d64 inj_ragged F1 tiled nref', want, mask, gv, d_off, d_logit, mfo.bounds('F1'))


# ---- a level that is no window of the value rows ---------------------------------------------------------------------
def test_invalid_level_contributes_nothing():
    """invalid_level_rows (start + H*W > S): both forward entry points return VAH_OK with out exactly zero - the window
    forward also on a workspace that holds such a schedule - and the tiled backward returns grad_value, d_offsets and
    d_logits exactly zero."""
    inp = _inputs('invalid_level_rows', 'F1')
    d = _dev(inp)

    def zero(name, t):
        assert bool((t == 0).all()), '%s: %d of %d elements are not zero' % (name, int((t != 0).sum()), t.numel())

    zero('out (16-lane)', _forward(inp, d))
    ws = _win_ws(inp)
    zero('out (windows)', _forward_win(inp, d, ws, False))
    zero('out (windows, schedule reused)', _forward_win(inp, d, ws, True))
    gv, d_off, d_logit, _ = _backward_tiled(inp, d)
    zero('grad_value', gv)
    zero('d_offsets', d_off)
    zero('d_logits', d_logit)
