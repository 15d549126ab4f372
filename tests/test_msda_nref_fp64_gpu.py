"""GPU: the fused MSDeformAttn core with reference points PER IMAGE (vah_msda_fused_forward_nref,
vah_msda_fused_backward_tiled_nref, vah_msda_fused_backward_nref; ref (N, Lq, ref_levels, 2)) held to fp64.

Direct calls in the style of tests/test_msda_fused_fp64_gpu.py: one call per entry point and case, every output and
workspace filled with NaN / 0xFF bytes first.  Operands: oracle.msda_fused.inputs(case, form, SEED); the two cases the
oracle states with one image (shared_lists, many_tiles) are made two images by stacking seeds SEED and SEED + 1 along
the batch, since one image has no per-image form (ref_batch == N == 1 is the shared grid).

The grid of image n is the case's shared grid times a per-image (x, y) ratio from [0.6, 1.0] (image 0: 1) - the role of
the pixel decoder's valid ratios, msdeformattn_pixel_decoder.py:224-240 - plus 0.01 * randn; the images' grids differ by
0.1 and more somewhere (asserted), so a kernel that ignores n is wrong by far more than any bound.  Reference: the body
of oracle.msda_fused.reference with loc = ref[n] + off / (W, H); kink mask from the same locations; bounds and check are
oracle.msda_fused.bounds / check, nothing new.  Run with -s for one FIGURE line per checked tensor."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import msda as oracle_msda
from oracle import msda_fused as mfo
from oracle import seeded

pytestmark = pytest.mark.gpu

_DT = {torch.float32: 0, torch.bfloat16: 1}
SEED = 1
FIRST = ['ext_ragged', 'inj_ragged', 'four_levels']
CASES = ([(c, f) for c in FIRST for f in ('F1', 'F1p', 'F2', 'F4')] +
         [(c, 'F1') for c in ('inj_ragged_ref3', 'shared_lists', 'many_tiles')])
ATOMICS = [(c, f) for c in ('ext_ragged', 'inj_ragged') for f in ('F2', 'F4')]
P = mfo.P


def _vah():
    import _vah
    return _vah


def _stream():
    return _vah().raw_stream(torch.device('cuda'))


def _nan(shape, dtype):
    return torch.full(tuple(shape), float('nan'), dtype=dtype, device='cuda')


def _nan_bytes(n):
    return torch.full((max(int(n), 1),), 255, dtype=torch.uint8, device='cuda')     # 0xFF..: NaN as fp32 and as bf16


def _call(name, *args):
    v = _vah()
    with v.on(torch.device('cuda')):
        rc = getattr(v.lib, name)(*args)
    v.check(rc, name)
    torch.cuda.synchronize()


def _two_images(case, form):
    """oracle.msda_fused.inputs with two images: as the oracle states the case, or seeds SEED and SEED + 1 stacked."""
    a = mfo.inputs(case, form, SEED)
    if a.dims[0] > 1:
        return a
    b = mfo.inputs(case, form, SEED + 1)
    assert a.dims[0] == 1 and torch.equal(a.ref, b.ref)
    N, M, D, _, Lq, L, S = a.dims
    inp = types.SimpleNamespace(**vars(a))
    inp.dims = (2, M, D, P, Lq, L, S)
    inp.value, inp.grad_out = torch.cat((a.value, b.value)), torch.cat((a.grad_out, b.grad_out))
    if a.f.interleaved:
        inp.params = torch.cat((a.params, b.params))
        inp.offsets, inp.logits = mfo.param_views(inp.params, L)
    else:
        inp.offsets, inp.logits = torch.cat((a.offsets, b.offsets)), torch.cat((a.logits, b.logits))
    return inp


def _per_image_grid(inp):
    """(N, Lq, ref_levels, 2) fp32: the shared grid times a ratio per image > 0, jittered."""
    N = inp.dims[0]
    key = 'msda_nref/' + inp.case
    ratio = 0.6 + 0.4 * seeded.rand(key + '/ratio', (N, 1, 1, 2), SEED)
    ratio[0] = 1.0
    ref = inp.ref[None].repeat(N, 1, 1, 1) * ratio + 0.01 * seeded.randn(key + '/jitter', (N,) + tuple(inp.ref.shape), SEED)
    assert float((ref[1] - ref[0]).abs().max()) >= 0.1
    return ref.float().contiguous()


def _wh(levels):
    return torch.tensor([[w, h] for h, w in levels], dtype=torch.float64)          # (L, 2) as (W, H)


def _reference(inp, ref):
    """oracle.msda_fused.reference with one grid per image -> (results, kink mask of d_offsets)."""
    N, M, _, _, Lq, L, S = inp.dims
    wh = _wh(inp.levels)[None, None, None, :, None, :]
    loc = ref.double()[:, :, None, :, None, :] + inp.offsets.double() / wh
    px = loc * wh - 0.5
    mask = ((px - px.round()).abs() > 1e-3).all(-1, keepdim=True).expand_as(px).numpy()
    v = inp.value.double().numpy()
    p = torch.softmax(inp.logits.double(), -1)
    attn = p.view(N, Lq, M, L, P).numpy()
    hw, lsi, loc = inp.shapes.numpy(), inp.lsi.numpy(), loc.numpy()
    g = inp.grad_out.double().numpy()
    want = types.SimpleNamespace(out=oracle_msda.forward(v, hw, lsi, loc, attn))
    gv, gl, ga = oracle_msda.backward(v, hw, lsi, loc, attn, g)
    want.grad_value = gv
    want.d_offsets = (torch.from_numpy(gl) / wh).numpy()
    ga = torch.from_numpy(ga).view(N, Lq, M, L * P)
    want.d_logits = (p * (ga - (p * ga).sum(-1, keepdim=True))).numpy()
    want.abs_gv = oracle_msda.backward(v, hw, lsi, loc, attn, np.abs(g))[0]
    return want, mask


@functools.lru_cache(maxsize=None)
def _case(case, form):
    """(inputs, per-image grid, reference, mask), computed once per (case, form), shared by the tests, never modified."""
    inp = _two_images(case, form)
    ref = _per_image_grid(inp)
    want, mask = _reference(inp, ref)
    return inp, ref, want, mask


def _dev(inp, ref):
    N, M, D, _, Lq, L, S = inp.dims
    d = types.SimpleNamespace(value=inp.value.cuda(), gout=inp.grad_out.cuda(), ref=ref.cuda().contiguous(),
                              shapes=inp.shapes.cuda(), lsi=inp.lsi.cuda())
    if inp.params is not None:
        d.params = inp.params.cuda()
        d.off = d.params.data_ptr()
        d.logit = d.off + 2 * L * P * d.params.element_size()
        d.os = d.ls = inp.stride
    else:
        d.offsets, d.logits = inp.offsets.cuda(), inp.logits.cuda()
        d.off, d.logit, d.os, d.ls = d.offsets.data_ptr(), d.logits.data_ptr(), 0, 0
    return d


def _forward_nref(inp, d, ref_batch):
    N, M, D, _, Lq, L, S = inp.dims
    out = _nan((N, Lq, M * D), inp.f.value)
    _call('vah_msda_fused_forward_nref', d.value.data_ptr(), _DT[inp.f.value], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off,
          d.logit, _DT[inp.f.param], d.os, d.ls, d.ref.data_ptr(), inp.ref_levels, ref_batch, N, S, M, D, L, Lq, P,
          out.data_ptr(), _stream())
    return out


def _forward_shared(inp, d):
    N, M, D, _, Lq, L, S = inp.dims
    out = _nan((N, Lq, M * D), inp.f.value)
    _call('vah_msda_fused_forward', d.value.data_ptr(), _DT[inp.f.value], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit,
          _DT[inp.f.param], d.os, d.ls, d.ref.data_ptr(), inp.ref_levels, N, S, M, D, L, Lq, P, out.data_ptr(), _stream())
    return out


def _check_backward(tag, want, mask, gv, d_off, d_logit, rules):
    mfo.check(tag + ' grad_value', gv, want.grad_value, rules['grad_value'], abs_gv=want.abs_gv)
    mfo.check(tag + ' d_logits', d_logit, want.d_logits, rules['d_logits'])
    mfo.check(tag + ' d_offsets', d_off, want.d_offsets, rules['d_offsets'], mask=mask)


@pytest.mark.parametrize('case,form', CASES)
def test_forward(case, form):
    """The 8-lane forward on every case (the window forward has no per-image form)."""
    inp, ref, want, _ = _case(case, form)
    d = _dev(inp, ref)
    mfo.check('%s %s nref out' % (case, form), _forward_nref(inp, d, inp.dims[0]), want.out, mfo.bounds(form)['out'])


@pytest.mark.parametrize('case,form', CASES)
def test_backward_tiled(case, form):
    inp, ref, want, mask = _case(case, form)
    d = _dev(inp, ref)
    N, M, D, _, Lq, L, S = inp.dims
    f = inp.f
    gv = _nan((N, S, M, D), f.gv)
    g = None
    if f.interleaved:
        esz = 2 if f.gparam == torch.bfloat16 else 4
        g = _nan_bytes(N * Lq * M * inp.stride * esz).view(f.gparam).view(N, Lq, M, inp.stride)
        d_off_p, d_logit_p, dos, dls = g.data_ptr(), g.data_ptr() + 2 * L * P * esz, inp.stride, inp.stride
        d_off, d_logit = mfo.param_views(g, L)
    else:
        d_off, d_logit = _nan((N, Lq, M, L, P, 2), f.gparam), _nan((N, Lq, M, L * P), f.gparam)
        d_off_p, d_logit_p, dos, dls = d_off.data_ptr(), d_logit.data_ptr(), 0, 0
    ws_bytes = _vah().lib.vah_msda_tile_ws_bytes(N, S, M, L, Lq, P)
    assert ws_bytes > 0
    ws = _nan_bytes(ws_bytes)
    _call('vah_msda_fused_backward_tiled_nref', d.value.data_ptr(), _DT[f.value], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off,
          d.logit, _DT[f.param], d.os, d.ls, d.ref.data_ptr(), inp.ref_levels, N, d.gout.data_ptr(), N, S, M, D, L, Lq, P,
          gv.data_ptr(), _DT[f.gv], d_off_p, d_logit_p, _DT[f.gparam], dos, dls, ws.data_ptr(), ws_bytes, _stream())
    _check_backward('%s %s nref tiled' % (case, form), want, mask, gv, d_off, d_logit, mfo.bounds(form))
    if f.pad:
        gap = g[..., inp.stride - f.pad:].contiguous().view(torch.int16)
        assert bool((gap == -1).all()), 'the gap words between the rows of the gradient matrix were written'


@pytest.mark.parametrize('case,form', ATOMICS)
def test_backward_atomics(case, form):
    """vah_msda_fused_backward_nref, the fallback of the tile pass: fp32 grad_value, zero on entry."""
    inp, ref, want, mask = _case(case, form)
    d = _dev(inp, ref)
    N, M, D, _, Lq, L, S = inp.dims
    f = inp.f
    gv = torch.zeros((N, S, M, D), dtype=torch.float32, device='cuda')
    d_off, d_logit = _nan((N, Lq, M, L, P, 2), f.param), _nan((N, Lq, M, L * P), f.param)
    _call('vah_msda_fused_backward_nref', d.value.data_ptr(), _DT[f.value], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit,
          _DT[f.param], d.ref.data_ptr(), inp.ref_levels, N, d.gout.data_ptr(), N, S, M, D, L, Lq, P, gv.data_ptr(),
          d_off.data_ptr(), d_logit.data_ptr(), _stream())
    par = 'bf16' if f.param == torch.bfloat16 else 'f32'
    _check_backward('%s %s nref atomics' % (case, form), want, mask, gv, d_off, d_logit,
                    dict(grad_value='f32', d_offsets=par, d_logits=par))


@pytest.mark.parametrize('case,form', [('ext_ragged', 'F1'), ('inj_ragged', 'F4'), ('four_levels', 'F2')])
def test_identical_copies_of_the_shared_grid_give_the_same_bits(case, form):
    """ref_batch = N with N copies of the shared grid is the arithmetic of vah_msda_fused_forward on that grid."""
    inp = mfo.inputs(case, form, SEED)
    N = inp.dims[0]
    assert N == 2
    shared = _dev(inp, inp.ref)
    want = _forward_shared(inp, shared)
    got = _forward_nref(inp, _dev(inp, inp.ref[None].repeat(N, 1, 1, 1)), N)
    assert torch.equal(got, want), '%d elements differ' % int((got != want).sum())
    got1 = _forward_nref(inp, shared, 1)
    assert torch.equal(got1, want), 'ref_batch = 1: %d elements differ' % int((got1 != want).sum())


def test_one_image_is_the_shared_form():
    """N = 1, ref_batch = 1 against the entry point without ref_batch."""
    inp = mfo.inputs('shared_lists', 'F1', SEED)
    assert inp.dims[0] == 1
    d = _dev(inp, inp.ref)
    got, want = _forward_nref(inp, d, 1), _forward_shared(inp, d)
    assert torch.equal(got, want), '%d elements differ' % int((got != want).sum())
