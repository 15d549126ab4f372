"""oracle/msda_fused.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Cases, operand forms and the fp64 statement of the fused MSDeformAttn core (include/vitadapter_hip.h:
vah_msda_fused_forward[_win], vah_msda_fused_backward[_tiled]) in the forms the model runs.

  inputs(case, form, seed)  CPU tensors already rounded to the dtypes of ``form``; everything comes from oracle.cases
                            (reference_grid, ring_offsets, level_start_index) and oracle.seeded, so the CPU test and the
                            GPU test see identical bits.
  reference(inp)            fp64 throughout: loc = ref + off / (W_l, H_l), softmax over the L*P logits, the C oracle
                            (oracle.msda.forward / backward), d_off = grad_loc / (W, H), d_logit = p (ga - sum p ga);
                            also abs_gv, the oracle's grad_value for |grad_out| (bilinear and attention weights are
                            non-negative: the sum of the absolute terms of every element).
  smooth_mask(inp)          samples whose pixel coordinates are both more than 1e-3 px away from an integer:
                            d(out)/d(loc) jumps at integers (and at the gate at -1 and H, which are integers); the fp32
                            location error is below 1e-4 px at every map here.
  bounds(form), check(...)  the project's numbers (tests/test_msda_fullsize_fused_gpu.py::_check), see bounds().

Forms (value / offsets, logits / their gradients / grad_value):
  F1   bf16 / fp32, one interleaved matrix, row strides 3LP / bf16, interleaved, strides 3LP / bf16   (production:
       vitadapter/fused.py::_MSDAPairCore)
  F1p  as F1 with row strides 3LP + 8 and a sentinel in the gap words
  F2   bf16 / bf16 contiguous / bf16 contiguous / bf16
  F3   bf16 / fp32 contiguous / fp32 contiguous / fp32
  F4   fp32 / fp32 contiguous / fp32 contiguous / fp32
  F5   fp32 / bf16 contiguous / bf16 contiguous / fp32
"""
import collections
import types

import numpy as np
import torch

from . import cases, seeded
from . import msda as oracle_msda

D, P = 32, 4
PAD = 8

Form = collections.namedtuple('Form', 'value param gparam gv interleaved pad')
_B, _F = torch.bfloat16, torch.float32
FORMS = {
    'F1': Form(_B, _F, _B, _B, True, 0),
    'F1p': Form(_B, _F, _B, _B, True, PAD),
    'F2': Form(_B, _B, _B, _B, False, 0),
    'F3': Form(_B, _F, _F, _F, False, 0),
    'F4': Form(_F, _F, _F, _F, False, 0),
    'F5': Form(_F, _B, _B, _F, False, 0),
}

# case -> levels (H, W), queries, N, M, offsets.  Each is the smallest shape at which its path still exists; which
# path that is: DESIGN.md ("fp64 checks of the fused MSDA core").
#   qgrids    query grids (reference points = pixel centres, oracle.cases.reference_grid)
#   qrandom   number of random reference points
#   noise     sigma of the N(0, noise) px added to the offsets; ring: add the module's ring bias
#   lsi, S    level starts / value rows when the levels do not tile [0, S)
#   ref_levels  1 (shared by the levels) or L
CASES = {
    'ext_ragged': dict(levels=[(13, 11)], qgrids=[(26, 22), (13, 11), (7, 6)], N=2, M=6, noise=1.0, ring=True),
    'inj_ragged': dict(levels=[(20, 28), (10, 14), (5, 7)], qgrids=[(10, 14)], N=2, M=6, noise=1.0, ring=True),
    'inj_ragged_ref3': dict(levels=[(20, 28), (10, 14), (5, 7)], qgrids=[(10, 14)], N=2, M=6, noise=1.0, ring=True,
                            ref_levels=3),
    'four_levels': dict(levels=[(16, 16), (8, 8), (4, 4), (1, 1)], qgrids=[(16, 16), (8, 8)], N=2, M=12, noise=1.0,
                        ring=True, ref_levels=4),
    'shared_lists': dict(levels=[(16, 16)], qgrids=[(64, 64)], N=1, M=2, noise=1.0, ring=True),
    'wide_rows': dict(levels=[(48, 80)], qgrids=[(24, 40)], N=1, M=2, noise=12.0, ring=True),
    'many_tiles': dict(levels=[(264, 264)], qgrids=[(66, 66)], N=1, M=1, noise=1.0, ring=True),
    'long_queries': dict(levels=[(16, 16)], qrandom=33000, N=1, M=1, noise=1.0, ring=False, forward_only=True),
    'many_groups': dict(levels=[(520, 520)], qrandom=2048, N=1, M=1, noise=1.0, ring=False, forward_only=True),
    'borders': dict(levels=[(12, 16)], qgrids=[(12, 16)], N=1, M=2, constructed=True),
    # the geometries of tests/test_msda_gpu.py::test_levels_that_do_not_tile_the_value_rows on three levels
    'non_tiling_trailing_rows': dict(levels=[(8, 8), (4, 4), (2, 2)], qgrids=[(8, 8)], N=2, M=6, noise=1.0, ring=True,
                                     lsi=[0, 64, 80], S=96),             # rows 84..95 belong to no level
    'non_tiling_gap_between_levels': dict(levels=[(8, 8), (4, 4), (2, 2)], qgrids=[(8, 8)], N=2, M=6, noise=1.0,
                                          ring=True, lsi=[0, 70, 86], S=90),      # rows 64..69 belong to no level
    'non_tiling_overlapping_levels': dict(levels=[(8, 8), (4, 4), (2, 2)], qgrids=[(8, 8)], N=2, M=6, noise=1.0,
                                          ring=True, lsi=[0, 60, 76], S=80),      # rows 60..63 belong to two levels
    # a level that is no window of the value rows: every result is zero (no reference() for these)
    'invalid_level_rows': dict(levels=[(8, 8)], qgrids=[(8, 8)], N=1, M=2, noise=1.0, ring=False, S=48, invalid=True),
    'invalid_level_h0': dict(levels=[(0, 8)], qgrids=[(8, 8)], N=1, M=2, noise=1.0, ring=False, S=64, invalid=True),
}

# borders: pixel coordinates (x, y) of the hand-placed samples on the 12 x 16 (H x W) map, by class.  Every
# fractional part is 1/4, 1/2 or 3/4: no sample is masked.  Tiles of the backward are 8 x 4 pixels (x, y).
BORDER_H, BORDER_W = 12, 16
BORDER_SAMPLES = {
    'band_left': [(-0.5, 5.25), (-0.25, 2.5)],                 # -1 < x < 0: only the right corners are in the map
    'band_right': [(15.5, 5.25), (15.75, 9.5)],                # W-1 < x < W
    'band_top': [(6.25, -0.5), (11.5, -0.75)],                 # -1 < y < 0
    'band_bottom': [(6.25, 11.5), (2.75, 11.25)],              # H-1 < y < H
    'corner_top_left': [(-0.5, -0.25)],                        # exactly one corner pixel in the map
    'corner_top_right': [(15.25, -0.75)],
    'corner_bottom_left': [(-0.75, 11.5)],
    'corner_bottom_right': [(15.5, 11.25)],
    'straddle_x': [(7.5, 1.25), (7.25, 9.5)],                  # x0 = 7: corners in two tiles side by side
    'straddle_y': [(2.25, 3.5), (12.5, 7.75)],                 # y0 = 3 (and 7): corners in two tiles above each other
    'straddle_xy': [(7.25, 3.75), (7.5, 7.5)],                 # corners in four tiles
    'gate_just_outside': [(-1.25, 5.5), (5.5, 12.25), (16.25, 3.5), (3.5, -1.25)],
    'far_outside': [(1e4 + 0.5, 5.5), (5.5, -1e4 - 0.5), (-1e4 - 0.25, 1e4 + 0.25)],
    'last_row_col': [(14.5, 10.25), (14.25, 5.5), (4.5, 10.75)],          # x0 + 1 = W - 1 / y0 + 1 = H - 1
    'interior': [(4.5, 5.5), (9.25, 1.75)],
}


def border_class(x, y, H=BORDER_H, W=BORDER_W):
    """Class of a sample at pixel coordinates (x, y), from the location alone (see BORDER_SAMPLES)."""
    if abs(x) > 1e3 or abs(y) > 1e3:
        return 'far_outside'
    if not (-1 < x < W and -1 < y < H):
        return 'gate_just_outside'
    lo_x, hi_x, lo_y, hi_y = x < 0, x > W - 1, y < 0, y > H - 1
    if (lo_x or hi_x) and (lo_y or hi_y):
        return 'corner_%s_%s' % ('top' if lo_y else 'bottom', 'left' if lo_x else 'right')
    if lo_x or hi_x:
        return 'band_left' if lo_x else 'band_right'
    if lo_y or hi_y:
        return 'band_top' if lo_y else 'band_bottom'
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    sx, sy = x0 % 8 == 7, y0 % 4 == 3
    if sx or sy:
        return 'straddle_xy' if sx and sy else 'straddle_x' if sx else 'straddle_y'
    if x0 + 1 == W - 1 or y0 + 1 == H - 1:
        return 'last_row_col'
    return 'interior'


def geometry(case):
    """-> (levels, lsi (L,) int64 tensor, S, Lq, ref_levels) of a case."""
    c = CASES[case]
    levels = c['levels']
    lsi = torch.tensor(c['lsi'], dtype=torch.long) if 'lsi' in c else cases.level_start_index(levels)
    S = c.get('S', sum(h * w for h, w in levels))
    Lq = c['qrandom'] if 'qrandom' in c else sum(h * w for h, w in c['qgrids'])
    return levels, lsi, S, Lq, c.get('ref_levels', 1)


def _reference_points(case):
    """(Lq, ref_levels, 2) fp32, the same for every seed of a case (the window schedule of one call serves the next)."""
    c = CASES[case]
    levels, _, _, Lq, RL = geometry(case)
    if 'qrandom' in c:
        r = seeded.rand(case + '/ref', (Lq, 1, 2))
        if case == 'long_queries':      # a third beyond the map on either side, some exactly on its edges
            r[::3] = r[::3] * 1.1 - 0.05
            r[1::50] = 0.0
            r[7::50] = 1.0
            r[13::50, 0, 0] = 1.0
            r[19::50, 0, 1] = 0.0
        return r.contiguous()
    r = cases.reference_grid(c['qgrids'])[0]                    # (Lq, 1, 2)
    if RL > 1:                                                  # per-level points: the grid, moved a little per level
        r = r.repeat(1, RL, 1) + 0.01 * seeded.randn(case + '/ref', (Lq, RL, 2))
    return r.contiguous()


def _border_offsets(N, Lq, M, ref):
    """Offsets (N, Lq, M, 1, P, 2) that put BORDER_SAMPLES, four per (query, head) row, at their pixel coordinates:
    the reference points are pixel centres, px = ref * (W, H) - 0.5 + off."""
    targets = [t for k in BORDER_SAMPLES for t in BORDER_SAMPLES[k]]
    T = len(targets)
    wh = torch.tensor([BORDER_W, BORDER_H], dtype=torch.float64)
    ref_px = ref[:, 0].double() * wh - 0.5                      # (Lq, 2): integers up to fp32 rounding
    off = torch.empty(N, Lq, M, 1, P, 2, dtype=torch.float64)
    for q in range(Lq):
        for m in range(M):
            for p in range(P):
                t = targets[((q * M + m) * 3 + p * 7) % T]      # rows mix the classes
                off[:, q, m, 0, p] = torch.tensor(t, dtype=torch.float64) - ref_px[q].round()
    return off.float()


def inputs(case, form, seed=0):
    """CPU operands of one call, rounded to the dtypes of ``form``.  Fields: value (N,S,M,D), offsets (N,Lq,M,L,P,2),
    logits (N,Lq,M,L*P), grad_out (N,Lq,M*D), ref (Lq, ref_levels, 2) fp32, shapes (L,2) / lsi (L,) int64, dims;
    interleaved forms: params (N,Lq,M,stride) with offsets / logits as views of it (gap words: NaN) and stride."""
    c, f = CASES[case], FORMS[form]
    levels, lsi, S, Lq, RL = geometry(case)
    N, M, L = c['N'], c['M'], len(levels)
    key = 'msda_fused/' + case
    value = seeded.randn(key + '/value', (N, S, M, D), seed).to(f.value)
    gout = seeded.randn(key + '/gout', (N, Lq, M * D), seed).to(f.value)
    logits = seeded.randn(key + '/logits', (N, Lq, M, L * P), seed)
    ref = _reference_points(case)
    if c.get('constructed'):
        off = _border_offsets(N, Lq, M, ref)
    else:
        off = c['noise'] * seeded.randn(key + '/off', (N, Lq, M, L, P, 2), seed)
        if c['ring']:
            off = off + cases.ring_offsets(M, L, P)[None, None]
    off, logits = off.to(f.param), logits.to(f.param)
    inp = types.SimpleNamespace(case=case, form=form, f=f, value=value, grad_out=gout, ref=ref,
                                shapes=torch.tensor(levels, dtype=torch.long).view(L, 2), lsi=lsi, levels=levels,
                                dims=(N, M, D, P, Lq, L, S), ref_levels=RL, params=None, stride=0,
                                forward_only=c.get('forward_only', False))
    if f.interleaved:
        inp.stride = 3 * L * P + f.pad
        inp.params = torch.full((N, Lq, M, inp.stride), float('nan'), dtype=f.param)
        inp.offsets, inp.logits = param_views(inp.params, L)
        inp.offsets.copy_(off)
        inp.logits.copy_(logits)
    else:
        inp.offsets, inp.logits = off.contiguous(), logits.contiguous()
    return inp


def param_views(matrix, L):
    """(offsets (N,Lq,M,L,P,2), logits (N,Lq,M,L*P)) as views of an interleaved (N,Lq,M,stride) matrix: an (n, q, m) row
    is [L*P*2 offsets | L*P logits | gap]."""
    return matrix[..., :2 * L * P].unflatten(-1, (L, P, 2)), matrix[..., 2 * L * P:3 * L * P]


def _wh(levels):
    return torch.tensor([[w, h] for h, w in levels], dtype=torch.float64)          # (L, 2) as (W, H)


def locations(inp):
    """fp64 sampling locations (N,Lq,M,L,P,2) from the rounded operands."""
    wh = _wh(inp.levels)
    r = inp.ref.double()[None, :, None, :, None, :]                                  # (1, Lq, 1, RL, 1, 2)
    return r + inp.offsets.double() / wh[None, None, None, :, None, :]


def pixel_coords(inp):
    """fp64 pixel coordinates (x, y) of every sample, (N,Lq,M,L,P,2)."""
    return locations(inp) * _wh(inp.levels)[None, None, None, :, None, :] - 0.5


def smooth_mask(inp):
    """(N,Lq,M,L,P,2) bool, True where d(offsets) is compared: both pixel coordinates of the sample more than 1e-3 px
    away from an integer."""
    px = pixel_coords(inp)
    return ((px - px.round()).abs() > 1e-3).all(-1, keepdim=True).expand_as(px).numpy()


def reference(inp, backward=True):
    """fp64 results from the rounded operands: out, and with backward grad_value, d_offsets, d_logits, abs_gv."""
    N, M, _, _, Lq, L, S = inp.dims
    v = inp.value.double().numpy()
    loc = locations(inp).numpy()
    p = torch.softmax(inp.logits.double(), -1)
    attn = p.view(N, Lq, M, L, P).numpy()
    hw = inp.shapes.numpy()
    lsi = inp.lsi.numpy()
    want = types.SimpleNamespace(out=oracle_msda.forward(v, hw, lsi, loc, attn))
    if backward:
        g = inp.grad_out.double().numpy()
        gv, gl, ga = oracle_msda.backward(v, hw, lsi, loc, attn, g)
        want.grad_value = gv
        want.d_offsets = (torch.from_numpy(gl) / _wh(inp.levels)[None, None, None, :, None, :]).numpy()
        ga = torch.from_numpy(ga).view(N, Lq, M, L * P)
        want.d_logits = (p * (ga - (p * ga).sum(-1, keepdim=True))).numpy()
        want.abs_gv = oracle_msda.backward(v, hw, lsi, loc, attn, np.abs(g))[0]
    return want


def forward_f64(inp, offsets=None, logits=None):
    """out in fp64 for other offsets / logits (fp64 tensors): what the finite differences of the CPU test evaluate."""
    N, M, _, _, Lq, L, S = inp.dims
    o = inp.offsets.double() if offsets is None else offsets
    lg = inp.logits.double() if logits is None else logits
    r = inp.ref.double()[None, :, None, :, None, :]
    loc = r + o / _wh(inp.levels)[None, None, None, :, None, :]
    attn = torch.softmax(lg, -1).view(N, Lq, M, L, P)
    return oracle_msda.forward(inp.value.double().numpy(), inp.shapes.numpy(), inp.lsi.numpy(), loc.numpy(), attn.numpy())


def bounds(form):
    """Result -> rule (see check): the numbers of tests/test_msda_fullsize_fused_gpu.py::_check, nothing new.
      'bf16'   stored in bf16: err - 2^-8 |want| <= 2e-3 max|want| per element and relative L2 <= 4e-3
      'f32'    stored in fp32: err <= 1e-4 max(1, max|want|)
      'f32_tile_bf16'  fp32 grad_value of bf16 operands from the tile pass (F3): the pass multiplies exact bf16 rows by
               weights split into bf16 hi + lo (relative error <= 2^-16) and accumulates in fp32, so per element
               err <= 2^-15 abs_gv + 1e-6 max|want|, with the 'f32' rule as a ceiling."""
    f = FORMS[form]
    par = 'bf16' if f.gparam == _B else 'f32'
    gv = 'bf16' if f.gv == _B else 'f32_tile_bf16' if f.value == _B else 'f32'
    return dict(out='bf16' if f.value == _B else 'f32', grad_value=gv, d_offsets=par, d_logits=par)


def check(name, got, want, rule, mask=None, abs_gv=None):
    """Assert ``got`` (tensor) against ``want`` (fp64 array) under ``rule``; -> the measured figures."""
    got = got.detach().double().cpu().numpy().reshape(want.shape)
    assert np.isfinite(got).all(), '%s: not finite' % name
    if mask is not None:
        assert mask.mean() > 0.5, 'more than half of the samples sit on a kink'
        got, want = np.where(mask, got, 0.0), np.where(mask, want, 0.0)
    err = np.abs(got - want)
    scale = np.abs(want).max()
    fig = dict(rule=rule, max_err=float(err.max()), scale=float(scale))
    if rule == 'bf16':
        excess = err - 2.0 ** -8 * np.abs(want)
        fig['excess'] = float(excess.max())
        fig['rel_l2'] = float(np.sqrt((err ** 2).sum() / max((want ** 2).sum(), 1e-300)))
        print('FIGURE %s %s' % (name, fig))
        assert excess.max() <= 2e-3 * scale, '%s: %.3e over the bf16 rounding band (max |ref| %.3e)' % (
            name, excess.max(), scale)
        assert fig['rel_l2'] <= 4e-3, '%s: relative L2 error %.3e' % (name, fig['rel_l2'])
    else:
        if rule == 'f32_tile_bf16':
            bound = np.minimum(2.0 ** -15 * abs_gv + 1e-6 * scale, 1e-4 * max(1.0, scale))
            fig['ratio'] = float((err / bound).max())
        else:
            assert rule == 'f32', rule
            bound = 1e-4 * max(1.0, scale)
            fig['ratio'] = float(err.max() / bound)
        print('FIGURE %s %s' % (name, fig))
        assert (err <= bound).all(), '%s: %.3e, %.3f of its bound (max |ref| %.3e)' % (name, err.max(), fig['ratio'], scale)
    return fig
