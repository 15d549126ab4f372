"""GPU: the fused MSDeformAttn core with reference BOXES (include/vitadapter_hip_msda_box.h: vah_msda_fused_forward_box,
vah_msda_fused_backward_tiled_box; ref (ref_batch, Lq, ref_levels, 4) = (cx, cy, w, h)) held to fp64.

Direct calls in the style of tests/test_msda_nref_fp64_gpu.py: one call per entry point and case, every output filled
with NaN and every workspace with 0xFF bytes first.

Operands: oracle.msda_fused.inputs(case, form, SEED = 1); the two cases the oracle states with one image (shared_lists,
many_tiles) are made two images by stacking seeds 1 and 2, as in the nref test.  D = 64: value and grad_out replaced by
64-channel seeded tensors under the keys of tests/test_msda_d64_fp64_gpu.py::_inputs; the all-fp16 form ('F16'): form F4
rounded to fp16, as tests/test_msda_f16_fp64_gpu.py does.  Box centres per image: the case's shared grid times an
(x, y) ratio from [0.6, 1] (image 0: 1) plus 0.01 * randn - the nref recipe; box sizes 0.1 + 0.5 * rand.  borders and
wide_rows are not used: their offsets are built for the point form.

Three conditions on these INPUTS are asserted per case (_case; the two one-level cases each have one floor of their
own, see FLOORS), so that a kernel that ignored the box, or one that formed the point location, is wrong far beyond any
bound:
  * kink mask: the share of samples whose pixel coordinates are both more than 1e-3 px from an integer is >= 0.99
    (oracle.msda_fused.check's own floor is 0.5);
  * at least 0.9 of the samples fall inside the gate (-1 < px < W, -1 < py < H);
  * at least 0.8 of the samples land more than 0.5 px away from where the point form (c + off / (W, H)) puts them.

Reference, fp64 throughout: loc = c + off / P * wh * 0.5 (detection/ops/modules/ms_deform_attn.py:120-122), the C oracle
(oracle.msda.forward / backward), d_offsets = grad_loc * wh * 0.5 / P, d_logits and abs_gv as in
oracle.msda_fused.reference.  Bounds: oracle.msda_fused.bounds(form) / check unchanged; the all-fp16 form takes the
derived rule of tests/test_msda_f16_fp64_gpu.py, err <= 2^-10 |want| + 1e-4 max(1, max|want|).  These are
storage-rounding rules plus the project's fp32 rule; the box scale is an fp32 factor applied before the single
rounding, so they hold as they are.  Run with -s for one FIGURE line per checked tensor."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import msda as oracle_msda
from oracle import msda_fused as mfo
from oracle import seeded

pytestmark = pytest.mark.gpu

H16 = torch.float16
_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
SEED = 1
P = mfo.P
FIRST = ['ext_ragged', 'inj_ragged', 'four_levels']
FORMS32 = ('F1', 'F1p', 'F2', 'F3', 'F4', 'F5', 'F16')
CASES = ([(c, f, 32) for c in FIRST for f in FORMS32] +
         [(c, 'F1', 32) for c in ('inj_ragged_ref3', 'shared_lists', 'many_tiles')] +
         [(c, f, 64) for c in FIRST for f in ('F1', 'F4', 'F16')])
# Floors of the three input conditions: 0.99 / 0.9 / 0.8, which the recipe meets on ext_ragged, inj_ragged,
# inj_ragged_ref3 and four_levels (0.9956-0.9962 / 0.912-0.954 / 0.838-0.891).  The two one-level cases cannot meet all
# three with box sizes from [0.1, 0.6], whatever the seed; each keeps the two floors it meets and gets one of its own:
#   shared_lists  one 16 x 16 level: the point form moves a sample by `off` px, the box form by off / P * w * 0.5 * 16 =
#                 2 w off px, so they are |off| |1 - 2 w| px apart and four samples in ten are closer than 0.5 px
#                 (0.617 differ).  Six in ten still put a kernel that formed the point location wrong beyond any bound.
#   many_tiles    one 264 x 264 level: the box form moves a sample by 33 w off px - 3 to 20 px per px of offset - and a
#                 tenth of the samples of the queries near the border leave the map (0.895 inside).  The floor is there
#                 so that the gather, not the gate, is what the samples exercise: 0.85 does that.
FLOORS = {'shared_lists': dict(differs=0.6), 'many_tiles': dict(inside=0.85)}


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


# ---- operands -------------------------------------------------------------------------------------------------------
def _one(case, form, D, seed):
    """oracle.msda_fused.inputs in the test's forms: 'F16' = F4 rounded to fp16; D = 64: value / grad_out of width 64."""
    f16 = form == 'F16'
    inp = mfo.inputs(case, 'F4' if f16 else form, seed)
    N, M, _, _, Lq, L, S = inp.dims
    vdt = H16 if f16 else inp.f.value
    if D == 64:
        key = 'msda_d64/' + case
        inp.value = seeded.randn(key + '/value', (N, S, M, D), seed).to(vdt)
        inp.grad_out = seeded.randn(key + '/gout', (N, Lq, M * D), seed).to(vdt)
        inp.dims = (N, M, D, P, Lq, L, S)
    elif f16:
        inp.value, inp.grad_out = inp.value.to(H16), inp.grad_out.to(H16)
    if f16:
        inp.offsets, inp.logits = inp.offsets.to(H16).contiguous(), inp.logits.to(H16).contiguous()
    inp.vdt, inp.pdt = vdt, H16 if f16 else inp.f.param
    inp.gvdt, inp.gpdt = (H16, H16) if f16 else (inp.f.gv, inp.f.gparam)
    return inp


def _two_images(case, form, D):
    """Two images: as the oracle states the case, or seeds SEED and SEED + 1 stacked along the batch."""
    a = _one(case, form, D, SEED)
    if a.dims[0] > 1:
        return a
    b = _one(case, form, D, SEED + 1)
    assert a.dims[0] == 1 and torch.equal(a.ref, b.ref)
    _, M, _, _, Lq, L, S = a.dims
    a.dims = (2, M, D, P, Lq, L, S)
    a.value, a.grad_out = torch.cat((a.value, b.value)), torch.cat((a.grad_out, b.grad_out))
    if a.params is not None:
        a.params = torch.cat((a.params, b.params))
        a.offsets, a.logits = mfo.param_views(a.params, L)
    else:
        a.offsets, a.logits = torch.cat((a.offsets, b.offsets)), torch.cat((a.logits, b.logits))
    return a


def _boxes(inp):
    """(N, Lq, ref_levels, 4) fp32 boxes (cx, cy, w, h), one set per image."""
    N, Lq = inp.dims[0], inp.dims[4]
    key = 'msda_box/' + inp.case
    ratio = 0.6 + 0.4 * seeded.rand(key + '/ratio', (N, 1, 1, 2), SEED)
    ratio[0] = 1.0
    centre = inp.ref[None].repeat(N, 1, 1, 1) * ratio + 0.01 * seeded.randn(key + '/jitter', (N,) + tuple(inp.ref.shape), SEED)
    assert float((centre[1] - centre[0]).abs().max()) >= 0.1          # a kernel that ignores n is wrong by far more than a bound
    wh = 0.1 + 0.5 * seeded.rand(key + '/wh', (N, Lq, inp.ref_levels, 2), SEED)
    return torch.cat((centre, wh), -1).float().contiguous()


def _level_wh(levels):
    return torch.tensor([[w, h] for h, w in levels], dtype=torch.float64)[None, None, None, :, None, :]      # (W, H)


def _reference(inp, boxes):
    """fp64 results for boxes (RB, Lq, RL, 4), RB in (1, N) -> (results, kink mask of d_offsets, input statistics)."""
    N, M, _, _, Lq, L, S = inp.dims
    WH = _level_wh(inp.levels)
    b = boxes.double()[:, :, None, :, None, :]                      # (RB, Lq, 1, RL, 1, 4)
    off = inp.offsets.double()
    scale = b[..., 2:] * 0.5 / P                                     # d(loc) / d(off)
    loc = b[..., :2] + off / P * b[..., 2:] * 0.5
    px = loc * WH - 0.5
    mask = ((px - px.round()).abs() > 1e-3).all(-1, keepdim=True).expand_as(px).numpy()
    inside = ((px > -1) & (px < WH)).all(-1)
    px_point = (b[..., :2] + off / WH) * WH - 0.5
    differs = ((px - px_point).abs() > 0.5).any(-1)
    stats = dict(mask=float(mask.mean()), inside=float(inside.double().mean()), differs=float(differs.double().mean()))
    v = inp.value.double().numpy()
    p = torch.softmax(inp.logits.double(), -1)
    attn = p.view(N, Lq, M, L, P).numpy()
    hw, lsi, loc = inp.shapes.numpy(), inp.lsi.numpy(), loc.expand(N, Lq, M, L, P, 2).contiguous().numpy()
    g = inp.grad_out.double().numpy()
    want = types.SimpleNamespace(out=oracle_msda.forward(v, hw, lsi, loc, attn))
    gv, gl, ga = oracle_msda.backward(v, hw, lsi, loc, attn, g)
    want.grad_value = gv
    want.d_offsets = (torch.from_numpy(gl) * scale).numpy()
    ga = torch.from_numpy(ga).view(N, Lq, M, L * P)
    want.d_logits = (p * (ga - (p * ga).sum(-1, keepdim=True))).numpy()
    want.abs_gv = oracle_msda.backward(v, hw, lsi, loc, attn, np.abs(g))[0]
    return want, mask, stats


@functools.lru_cache(maxsize=None)
def _case(case, form, D, shared=False):
    """(inputs, boxes, reference, mask), computed once per (case, form, D), shared by the tests, never modified.
    shared: image 0's boxes for the whole batch (ref_batch = 1)."""
    inp = _two_images(case, form, D)
    boxes = _boxes(inp)
    if shared:
        boxes = boxes[:1].contiguous()
    want, mask, stats = _reference(inp, boxes)
    print('FIGURE %s %s D%d%s inputs %s' % (case, form, D, ' shared' if shared else '', stats))
    floors = dict(dict(mask=0.99, inside=0.9, differs=0.8), **FLOORS.get(case, {}))
    for k, floor in floors.items():                # conditions on the inputs, not on the kernels (module docstring)
        assert stats[k] >= floor, (k, floor, stats)
    return inp, boxes, want, mask


def _dev(inp, boxes):
    _, M, D, _, Lq, L, S = inp.dims
    d = types.SimpleNamespace(value=inp.value.cuda(), gout=inp.grad_out.cuda(), ref=boxes.cuda().contiguous(),
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


# ---- the calls ------------------------------------------------------------------------------------------------------
def _forward(inp, d, entry='box'):
    """entry 'box': vah_msda_fused_forward_box with ref_comps = d.ref.shape[-1]; 'nref': vah_msda_fused_forward_nref."""
    N, M, D, _, Lq, L, S = inp.dims
    out = _nan((N, Lq, M * D), inp.vdt)
    head = (d.value.data_ptr(), _DT[inp.vdt], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit, _DT[inp.pdt], d.os, d.ls,
            d.ref.data_ptr(), inp.ref_levels, d.ref.shape[0])
    tail = (N, S, M, D, L, Lq, P, out.data_ptr(), _stream())
    if entry == 'box':
        _call('vah_msda_fused_forward_box', *head, d.ref.shape[-1], *tail)
    else:
        _call('vah_msda_fused_forward_nref', *head, *tail)
    return out


def _backward(inp, d, entry='box'):
    """-> grad_value, d_offsets, d_logits (views of the gradient matrix for the interleaved forms), that matrix or None."""
    N, M, D, _, Lq, L, S = inp.dims
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
            d.ref.data_ptr(), inp.ref_levels, d.ref.shape[0])
    tail = (d.gout.data_ptr(), N, S, M, D, L, Lq, P, gv.data_ptr(), _DT[inp.gvdt], d_off_p, d_logit_p, _DT[inp.gpdt], dos, dls,
            ws.data_ptr(), ws_bytes, _stream())
    if entry == 'box':
        _call('vah_msda_fused_backward_tiled_box', *head, d.ref.shape[-1], *tail)
    else:
        _call('vah_msda_fused_backward_tiled_nref', *head, *tail)
    return gv, d_off, d_logit, g


# ---- the bounds -----------------------------------------------------------------------------------------------------
def _check_f16(name, got, want, mask=None):
    """err <= 2^-10 |want| + 1e-4 max(1, max|want|) per element (tests/test_msda_f16_fp64_gpu.py)."""
    got = got.detach().double().cpu().numpy().reshape(want.shape)
    assert np.isfinite(got).all(), '%s: not finite' % name
    if mask is not None:
        got, want = np.where(mask, got, 0.0), np.where(mask, want, 0.0)
    err = np.abs(got - want)
    scale = float(np.abs(want).max())
    bound = 2.0 ** -10 * np.abs(want) + 1e-4 * max(1.0, scale)
    ratio = float((err / bound).max())
    print('FIGURE %s max_err %.3e scale %.3e ratio %.3f' % (name, float(err.max()), scale, ratio))
    assert (err <= bound).all(), '%s: %.3e, %.3f of its bound (max |ref| %.3e)' % (name, float(err.max()), ratio, scale)


def _check(tag, form, which, got, want, mask=None):
    if form == 'F16':
        _check_f16('%s %s' % (tag, which), got, getattr(want, which), mask=mask)
    else:
        mfo.check('%s %s' % (tag, which), got, getattr(want, which), mfo.bounds(form)[which], mask=mask,
                  abs_gv=want.abs_gv if which == 'grad_value' else None)


def _check_backward(tag, form, want, mask, gv, d_off, d_logit):
    _check(tag, form, 'grad_value', gv, want)
    _check(tag, form, 'd_logits', d_logit, want)
    _check(tag, form, 'd_offsets', d_off, want, mask=mask)


# ---- the tests ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,form,D', CASES)
def test_forward(case, form, D):
    inp, boxes, want, _ = _case(case, form, D)
    _check('box %s %s D%d' % (case, form, D), form, 'out', _forward(inp, _dev(inp, boxes)), want)


@pytest.mark.parametrize('case,form,D', CASES)
def test_backward_tiled(case, form, D):
    inp, boxes, want, mask = _case(case, form, D)
    d = _dev(inp, boxes)
    gv, d_off, d_logit, g = _backward(inp, d)
    _check_backward('box %s %s D%d tiled' % (case, form, D), form, want, mask, gv, d_off, d_logit)
    if inp.params is not None and inp.f.pad:
        gap = g[..., inp.stride - inp.f.pad:].contiguous().view(torch.int16)
        assert bool((gap == -1).all()), 'the gap words between the rows of the gradient matrix were written'
        assert bool(torch.isnan(d.params[..., inp.stride - inp.f.pad:]).all())


@pytest.mark.parametrize('form', ['F1', 'F4'])
def test_boxes_shared_by_the_batch(form):
    """ref_batch = 1: image 0's boxes for both images (every other test has one set per image)."""
    inp, boxes, want, mask = _case('inj_ragged', form, 32, True)
    assert boxes.shape[0] == 1 and inp.dims[0] == 2
    d = _dev(inp, boxes)
    tag = 'box inj_ragged %s shared' % form
    _check(tag, form, 'out', _forward(inp, d), want)
    gv, d_off, d_logit, _ = _backward(inp, d)
    _check_backward(tag + ' tiled', form, want, mask, gv, d_off, d_logit)
    # and they differ from the per-image results: the batch term is live in the other tests
    _, _, per_image, _ = _case('inj_ragged', form, 32)
    assert float(np.abs(per_image.out[1] - want.out[1]).max()) > 0.1


def _same_up_to_summation_order(name, a, b):
    """grad_value of two calls of the SAME kernels.  The tile pass adds a tile's list entries up in the order in which the
    binning pass's atomics put them into the list, and that order changes from one call to the next (the *_nref entry
    point against itself is printed below): the fp32 sums of two calls differ in their last bits, and a stored element
    by at most one unit in the last place of its type (bf16: 2^-7 relative) where the two sums straddle a rounding
    boundary - a rare event: at most one element in a hundred; an fp32 element by the reordering of at most a few hundred
    terms, held to 1e-5 of the largest element - a tenth of the project's fp32 rule.  Measured on an MI355X, inj_ragged,
    the *_nref entry point against itself: F1 4 of 282 240 bf16 elements (largest difference 6.1e-5), F4 20 639 of 282 240
    fp32 elements (2.4e-7)."""
    a, b = a.double(), b.double()
    diff = (a - b).abs()
    n = int((diff > 0).sum())
    print('FIGURE %s: %d of %d elements differ, largest difference %.3e' % (name, n, diff.numel(), float(diff.max())))
    if name.endswith('f32'):
        bound = torch.full_like(diff, 1e-5 * float(b.abs().max()))
    else:
        bound = 2.0 ** -7 * torch.maximum(a.abs(), b.abs())
        assert n <= 0.01 * diff.numel(), '%s: %d of %d elements differ' % (name, n, diff.numel())
    assert bool((diff <= bound).all()), '%s: %d elements differ by more than the summation order allows' % (name, int((diff > bound).sum()))


@pytest.mark.parametrize('form', ['F1', 'F4'])
def test_ref_comps_2_is_the_nref_call_bit_for_bit(form):
    """Points through the new entry points: out, d_offsets and d_logits equal the *_nref entry points' bits; grad_value
    equals them as far as two calls of one entry point do (_same_up_to_summation_order)."""
    inp = _two_images('inj_ragged', form, 32)
    N = inp.dims[0]
    grid = (inp.ref[None].repeat(N, 1, 1, 1) * torch.tensor([[[[1.0, 1.0]]], [[[0.8, 0.7]]]])).float().contiguous()
    d = _dev(inp, grid)
    assert d.ref.shape[-1] == 2
    got, want = _forward(inp, d, 'box'), _forward(inp, d, 'nref')
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got, want), 'out: %d elements differ' % int((got != want).sum())
    box, nref, again = _backward(inp, d, 'box')[:3], _backward(inp, d, 'nref')[:3], _backward(inp, d, 'nref')[:3]
    for name, a, b in zip(('d_offsets', 'd_logits'), box[1:], nref[1:]):
        assert bool(torch.isfinite(b).all()), name
        assert torch.equal(a, b), '%s: %d elements differ' % (name, int((a != b).sum()))
    assert bool(torch.isfinite(nref[0]).all())
    kind = 'f32' if inp.gvdt == torch.float32 else 'bf16'
    _same_up_to_summation_order('%s grad_value nref against nref, %s' % (form, kind), again[0], nref[0])
    _same_up_to_summation_order('%s grad_value box entry against nref, %s' % (form, kind), box[0], nref[0])


@pytest.mark.parametrize('poison', [float('nan'), float('inf')])
@pytest.mark.parametrize('form,D', [('F1', 32), ('F4', 32), ('F1', 64)])
def test_a_non_finite_box_poisons_its_query_and_nothing_else(form, D, poison):
    """w of one (image, query) box, on every reference level it has, set to NaN / +inf: every location of that query is
    non-finite (such a sample is not dropped), so that query's rows of out, d_offsets and d_logits are
    non-finite - every element - and every other row has the bits of the unpoisoned run."""
    inp, boxes, _, _ = _case('inj_ragged', form, D)
    N, M, _, _, Lq, L, S = inp.dims
    n, q = 1, Lq // 3
    bad = boxes.clone()
    bad[n, q, :, 2] = poison
    clean, dirty = _dev(inp, boxes), _dev(inp, bad)
    out0, out1 = _forward(inp, clean), _forward(inp, dirty)
    _, off0, lg0, _ = _backward(inp, clean)
    _, off1, lg1, _ = _backward(inp, dirty)
    for name, a, b in (('out', out0.view(N, Lq, -1), out1.view(N, Lq, -1)),
                       ('d_offsets', off0.reshape(N, Lq, -1), off1.reshape(N, Lq, -1)),
                       ('d_logits', lg0.reshape(N, Lq, -1), lg1.reshape(N, Lq, -1))):
        assert bool(torch.isfinite(a).all()), name
        assert not bool(torch.isfinite(b[n, q]).any()), '%s: %d finite elements in the poisoned row' % (
            name, int(torch.isfinite(b[n, q]).sum()))
        keep = torch.ones(N, Lq, dtype=torch.bool, device=a.device)
        keep[n, q] = False
        assert torch.equal(a[keep], b[keep]), '%s: %d elements of other rows changed' % (name, int((a[keep] != b[keep]).sum()))
