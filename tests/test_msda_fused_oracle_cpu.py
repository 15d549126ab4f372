"""CPU: pins oracle/msda_fused.py - the fp64 statement of the fused MSDeformAttn core and the inputs of
tests/test_msda_fused_fp64_gpu.py - so that the GPU test cannot hide behind its own reference or masks.

  * reference().out equals the torch restatement of the reference's pure-PyTorch core (oracle.msda.core_torch) in fp64;
  * d_offsets / d_logits equal central finite differences of the fp64 forward on 200 seeded unmasked samples;
  * the inputs reach what their case exists for, computed from the sampling locations alone: few samples masked,
    samples on both sides of the gate, lists long enough to be sliced but not to overflow, rows spread beyond the
    binning window, corners beyond the forward's LDS window, more tiles / groups / queries than the fast paths hold,
    every border class present.  If one of these fails the inputs change (seed, noise), never the cap."""
import numpy as np
import pytest
import torch

from oracle import msda as oracle_msda
from oracle import msda_fused as mfo

BACKWARD_CASES = ['ext_ragged', 'inj_ragged', 'inj_ragged_ref3', 'four_levels', 'shared_lists', 'wide_rows', 'many_tiles',
                  'borders', 'non_tiling_trailing_rows', 'non_tiling_gap_between_levels', 'non_tiling_overlapping_levels']

BF16_PARAMETER_CASES = ['ext_ragged', 'inj_ragged', 'four_levels']        # forms F2 and F5 run on these only


@pytest.mark.parametrize('case', ['ext_ragged', 'inj_ragged', 'inj_ragged_ref3', 'four_levels', 'borders'])
def test_reference_out_equals_core_torch(case):
    inp = mfo.inputs(case, 'F1')
    N, M, _, P, Lq, L, S = inp.dims
    want = mfo.reference(inp, backward=False).out
    attn = torch.softmax(inp.logits.double(), -1).view(N, Lq, M, L, P)
    got = oracle_msda.core_torch(inp.value.double(), inp.levels, mfo.locations(inp), attn).numpy()
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize('case', ['ext_ragged', 'inj_ragged', 'four_levels'])
def test_parameter_gradients_equal_finite_differences(case):
    """One sample per (n, q, m) row is moved in 200 seeded rows at once (a row's output depends on its own parameters
    only): two forward calls per tensor.  Bilinear interpolation is linear in each coordinate between two integers, and
    an unmasked sample is more than 1e-3 px away from one: a step of 1e-4 px crosses no kink."""
    inp = mfo.inputs(case, 'F1')
    N, M, D, P, Lq, L, S = inp.dims
    want = mfo.reference(inp)
    smooth = torch.from_numpy(mfo.smooth_mask(inp))
    g = inp.grad_out.double().view(N, Lq, M, D)
    gen = torch.Generator().manual_seed(11)
    rows = torch.randperm(N * Lq * M, generator=gen)[:200]
    n, q, m = rows // (Lq * M), rows // M % Lq, rows % M
    h = 1e-4

    def directional(out_p, out_m):
        d = torch.from_numpy(out_p - out_m).view(N, Lq, M, D)
        return ((d * g).sum(-1) / (2 * h))[n, q, m]

    def close(fd, an, scale):
        assert float(((fd - an).abs() - 1e-6 * (an.abs() + 1e-3 * scale)).max()) <= 0.0, float((fd - an).abs().max())

    # offsets: a seeded unmasked sample and coordinate per row
    pick = torch.randint(0, L * P * 2, (200,), generator=gen)
    flat = smooth.reshape(N, Lq, M, L * P * 2)
    for i in range(200):
        while not flat[n[i], q[i], m[i], pick[i]]:
            pick[i] = (pick[i] + 1) % (L * P * 2)
    step = torch.zeros(N, Lq, M, L * P * 2, dtype=torch.float64)
    step[n, q, m, pick] = h
    step = step.view(N, Lq, M, L, P, 2)
    o = inp.offsets.double()
    fd = directional(mfo.forward_f64(inp, offsets=o + step), mfo.forward_f64(inp, offsets=o - step))
    an = torch.from_numpy(want.d_offsets).reshape(N, Lq, M, L * P * 2)[n, q, m, pick]
    assert int((an != 0).sum()) > 100
    close(fd, an, np.abs(want.d_offsets).max())
    # logits (smooth everywhere)
    pick = torch.randint(0, L * P, (200,), generator=gen)
    step = torch.zeros(N, Lq, M, L * P, dtype=torch.float64)
    step[n, q, m, pick] = h
    lg = inp.logits.double()
    fd = directional(mfo.forward_f64(inp, logits=lg + step), mfo.forward_f64(inp, logits=lg - step))
    an = torch.from_numpy(want.d_logits)[n, q, m, pick]
    close(fd, an, np.abs(want.d_logits).max())


@pytest.mark.parametrize('case', BACKWARD_CASES)
def test_few_samples_are_masked(case):
    """d(offsets) is compared where the sample is more than 1e-3 px away from a kink: at most 1 % of the samples are
    left out with fp32 parameters, at most 5 % with bf16 parameters (multiples of 2^-7 px near 1..4 px), in the forms
    the GPU test runs the case in."""
    for form, cap in (('F1', 0.01), ('F2', 0.05)):
        if form == 'F2' and case not in BF16_PARAMETER_CASES:
            continue
        share = 1.0 - mfo.smooth_mask(mfo.inputs(case, form)).mean()
        print('masked share %s %s: %.4f' % (case, form, share))
        assert share <= cap, (form, share)


def _gate(px, levels):
    """(in the gate, all four corners in the map) per sample, from pixel coordinates (N,Lq,M,L,P,2)."""
    hi = torch.tensor([[w, h] for h, w in levels], dtype=torch.float64)[None, None, None, :, None, :]
    gate = ((px > -1) & (px < hi)).all(-1)
    inmap = ((px >= 0) & (px <= hi - 1)).all(-1)
    return gate, inmap


@pytest.mark.parametrize('case', ['ext_ragged', 'inj_ragged', 'four_levels'])
def test_samples_on_both_sides_of_the_gate(case):
    inp = mfo.inputs(case, 'F1')
    gate, inmap = _gate(mfo.pixel_coords(inp), inp.levels)
    print('gate coverage %s: in the map %.3f, outside the gate %.3f' % (case, inmap.double().mean(), 1 - gate.double().mean()))
    assert inmap.double().mean() >= 0.25
    assert 1 - gate.double().mean() >= 0.05


def _corners(px, H, W):
    """-> x, y (..., 4) integer corner coordinates and ok (..., 4): sample in the gate and corner in the map."""
    x0, y0 = px[..., 0].floor().long(), px[..., 1].floor().long()
    gate = (px[..., 0] > -1) & (px[..., 0] < W) & (px[..., 1] > -1) & (px[..., 1] < H)
    x = torch.stack([x0, x0 + 1, x0, x0 + 1], -1)
    y = torch.stack([y0, y0, y0 + 1, y0 + 1], -1)
    ok = gate[..., None] & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    return x, y, ok


def test_shared_lists_are_sliced_and_do_not_overflow():
    """csrc/msda_tile.hip: a (tile, head) list whose even load (2 tiles per row) exceeds kChunksPerWg * 64 = 512 entries
    is shared by several work items (partial tiles); one that exceeds its capacity is replaced by a walk over all
    queries, which tests/test_msda_fullsize_fused_gpu.py covers."""
    inp = mfo.inputs('shared_lists', 'F1')
    N, M, _, P, Lq, L, S = inp.dims
    H, W = inp.levels[0]
    ntx, nty = (W + 7) // 8, (H + 3) // 4
    x, y, ok = _corners(mfo.pixel_coords(inp)[:, :, :, 0], H, W)                    # (N, Lq, M, P, 4)
    tile = torch.where(ok, (y // 4) * ntx + x // 8, torch.full_like(x, -1)).flatten(3)       # (N, Lq, M, 16)
    touched = torch.stack([(tile == t).any(-1) for t in range(ntx * nty)], -1)       # (N, Lq, M, tiles)
    lists = touched.sum(1)                                                           # rows per (n, m, tile)
    even = 2 * Lq / (ntx * nty)
    print('shared_lists: even load %.0f, lists %d..%d' % (even, lists.min(), lists.max()))
    assert even > 512
    assert int(lists.max()) <= 4 * even
    assert int(lists.min()) > 512


def test_wide_rows_leave_the_binning_window_and_the_lds_window():
    inp = mfo.inputs('wide_rows', 'F1')
    N, M, _, P, Lq, L, S = inp.dims
    H, W = inp.levels[0]
    px = mfo.pixel_coords(inp)[:, :, :, 0]                                          # (N, Lq, M, P, 2)
    gate, _ = _gate(mfo.pixel_coords(inp), inp.levels)
    gate = gate[:, :, :, 0]
    lo = torch.where(gate[..., None], px, torch.full_like(px, 1e9)).amin(-2)
    hi = torch.where(gate[..., None], px, torch.full_like(px, -1e9)).amax(-2)
    wide = ((hi - lo) > 32).any(-1) & (gate.sum(-1) >= 2)
    print('wide_rows: %.3f of the rows spread over more than 32 px' % wide.double().mean())
    assert wide.double().mean() >= 0.10
    # the forward's window: the 8 x 8 group of the query's reference point + halo 5 + 1 pixels on every side
    x, y, ok = _corners(px, H, W)
    rp = inp.ref[:, 0].double()                                                     # (Lq, 2)
    gx = (rp[:, 0] * W / 8).floor().clamp(0, (W + 7) // 8 - 1).long()[None, :, None, None, None]
    gy = (rp[:, 1] * H / 8).floor().clamp(0, (H + 7) // 8 - 1).long()[None, :, None, None, None]
    inwin = (x >= gx * 8 - 6) & (x < gx * 8 + 14) & (y >= gy * 8 - 6) & (y < gy * 8 + 14)
    beyond = (ok & ~inwin).sum().item() / ok.sum().item()
    print('wide_rows: %.3f of the in-map corners lie beyond the window' % beyond)
    assert beyond >= 0.05


def test_sizes_beyond_the_fast_paths():
    (H, W), = mfo.CASES['many_tiles']['levels']
    assert ((H + 3) // 4) * ((W + 7) // 8) > 2048                  # kBinTable of csrc/msda_tile.hip
    assert ((H + 7) // 8) * ((W + 7) // 8) > 64                    # the slice scan of msda_win_schedule
    (H, W), = mfo.CASES['many_groups']['levels']
    assert ((H + 7) // 8) * ((W + 7) // 8) > 4096                  # kLdsGroups of csrc/msda_fwd_win.hip
    assert mfo.geometry('long_queries')[3] > 32 * 1024             # kRegQ * kSchedThreads
    ref = mfo.inputs('long_queries', 'F1').ref
    assert int((ref == 0).sum()) > 100 and int((ref == 1).sum()) > 100
    assert int(((ref < 0) | (ref > 1)).sum()) > 100


def test_borders_hold_every_class_and_nothing_is_masked():
    inp = mfo.inputs('borders', 'F1')
    assert mfo.smooth_mask(inp).all()
    px = mfo.pixel_coords(inp).reshape(-1, 2)
    frac = (px - px.floor())
    near = px.abs() < 1e3
    assert float(((frac * 4 - (frac * 4).round()).abs() * near).max()) < 1e-4       # multiples of 1/4 ...
    assert float(((frac - frac.round()).abs() + (~near)).min()) > 0.2               # ... away from the integers
    seen = {mfo.border_class(float(x), float(y)) for x, y in px.tolist()}
    assert seen == set(mfo.BORDER_SAMPLES), set(mfo.BORDER_SAMPLES) ^ seen
    # every class is where BORDER_SAMPLES says it is
    for k, pts in mfo.BORDER_SAMPLES.items():
        assert all(mfo.border_class(x, y) == k for x, y in pts), k
