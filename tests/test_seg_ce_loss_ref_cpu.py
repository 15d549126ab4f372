"""CPU: the fp64 restatement the GPU tests of csrc/seg_ce_loss.hip are held to (tests/seg_ce_loss_ref.py) against torch in
fp64 - F.interpolate + F.cross_entropy(reduction='none', ignore_index=255[, weight]) and autograd's gradient of scale * sum -
and the proof that its budgets can fail.

The restatement computes the tap fractions in fp32, as the kernels do; torch in fp64 computes them in fp64.  Where both give
the same fractions bit for bit (an exact size ratio) everything agrees to 1e-12.  Elsewhere the bound comes from the
fraction error: the source coordinate scale * (dst + 0.5) - 0.5 is three fp32 roundings of values up to max(in, out), with
the rounding of scale itself at most 4 u max(in, out) (u = 2^-24); a blended logit is linear in each fraction with a slope of
one difference of neighbouring logits, taken as max|v|, so per axis
    |dv| <= 4 * 2^-24 * max(in, out) * max|v|
and the two axes add.  lse and v_y each move by at most |dv| (both are 1-Lipschitz in the largest logit error), so a
per-pixel loss moves by at most w * 2 |dv|.  For the gradient, p_c moves by at most 2 |dv| (softmax's sensitivity, p_c <= 1),
the tap weights themselves by the fraction errors f = sum over the axes of 4 * 2^-24 * max(in, out), and an input element sums
at most K' - 6 output pixels with |g| <= |scale| w: |d dlogits| <= |scale| max(w) (K' - 6) (2 |dv| + 2 f)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_ce_loss_ref as ref  # noqa: E402
from resize_rows_ref import taps  # noqa: E402
from seg_logits_ref import BAND  # noqa: E402

U = 2.0 ** -24
SIZES = (((5, 7), (20, 28)), ((3, 3), (48, 48)), ((7, 5), (23, 18)), ((9, 11), (9, 11)), ((12, 10), (5, 4)), ((1, 1), (6, 5)))
SCALE = 0.37


def _taps64(n_in, n_out, align):
    dst = np.arange(n_out, dtype=np.float64)
    if align:
        src = ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0) * dst
    else:
        src = np.maximum(n_in / n_out * (dst + 0.5) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    return i0, np.clip(src - i0, 0.0, 1.0)


def _exact(n_in, n_out, align):
    """do the fp32 taps equal the fp64 ones bit for bit, and sum to one?"""
    i0, _, l0, l1 = taps(n_in, n_out, align)
    j0, m1 = _taps64(n_in, n_out, align)
    return bool(np.array_equal(i0, j0) and np.array_equal(l1.astype(np.float64), m1)
                and np.array_equal(l0.astype(np.float64) + l1.astype(np.float64), np.ones(n_out)))


def _case(C, hw, HW, seed, N=2):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((N, C) + hw, generator=g, dtype=torch.float64)
    labels = torch.randint(0, C, (N,) + HW, generator=g)
    labels[torch.rand((N,) + HW, generator=g) < 0.1] = 255
    weight = torch.rand((C,), generator=g, dtype=torch.float64) + 0.5
    return logits, labels, weight


def _torch_side(logits, labels, weight, align):
    x = logits.clone().requires_grad_(True)
    up = F.interpolate(x, size=labels.shape[1:], mode='bilinear', align_corners=align)
    loss = F.cross_entropy(up, labels, weight=weight, reduction='none', ignore_index=255)
    (SCALE * loss.sum()).backward()
    return up.detach(), loss.detach(), x.grad


@pytest.mark.parametrize('weighted', (False, True))
@pytest.mark.parametrize('align', (False, True))
@pytest.mark.parametrize('hw,HW', SIZES)
@pytest.mark.parametrize('C', (3, 19, 150))
def test_restatement_matches_torch_fp64(C, hw, HW, align, weighted):
    logits, labels, weight = _case(C, hw, HW, seed=C + 7 * hw[0] + HW[1])
    weight = weight if weighted else None
    up, loss, grad = _torch_side(logits, labels, weight, align)
    r = ref.reference(logits.numpy(), labels.numpy(), align, 255, None if weight is None else weight.numpy(), scale=SCALE)
    vmax = float(logits.abs().max())
    wmax = float(weight.max()) if weighted else 1.0
    if all(_exact(i, o, align) for i, o in zip(hw, HW)):
        bv = bl = bg = 1e-12
    else:
        f = sum(4 * U * max(i, o) for i, o in zip(hw, HW))
        bv = f * vmax
        bl = wmax * 2 * bv
        bg = SCALE * wmax * (r['Kp'] - 6) * (2 * bv + 2 * f)
    assert np.abs(r['v'] - up.numpy()).max() <= bv
    assert np.abs(r['lse'] - torch.logsumexp(up, dim=1).numpy()).max() <= bv
    assert np.abs(r['loss'] - loss.numpy()).max() <= bl
    assert abs(r['loss_sum'] - float(loss.sum())) <= bl * labels.numel()
    assert np.abs(r['dlogits'] - grad.numpy()).max() <= bg
    assert r['n_valid'] == int((labels != 255).sum())
    # outside the band the restatement's argmax is torch's everywhere, so the two counts that bracket n_correct hold torch's
    outside = r['gap'] >= BAND
    assert np.array_equal(r['argmax'][outside], up.argmax(dim=1).numpy()[outside])
    hit = (up.argmax(dim=1) == labels) & (labels != 255)
    assert r['n_correct_lo'] <= int(hit.sum()) <= r['n_correct_hi']
    assert r['band'] <= ref.MAX_BAND


def test_ignored_and_out_of_range_labels_count_for_nothing():
    logits, labels, _ = _case(19, (5, 7), (20, 28), seed=3)
    r0 = ref.reference(logits.numpy(), labels.numpy())
    labels2 = labels.clone()
    labels2[labels == 255] = 200                         # not ignore_index, not a class: ignored as well
    labels2[0, 0, 0] = -3
    r1 = ref.reference(logits.numpy(), labels2.numpy())
    valid0 = int((labels != 255).sum()) - int(labels[0, 0, 0] != 255)
    assert r1['n_valid'] == valid0
    poisoned = logits.clone()
    poisoned[1, :, 2, 3] = float('nan')
    lab = labels.clone()
    lab[1] = 255                                         # the NaN is tapped by ignored pixels only
    r2 = ref.reference(poisoned.numpy(), lab.numpy())
    assert np.isfinite(r2['loss_sum']) and np.isnan(r2['dlogits'][1]).any() and np.isfinite(r2['dlogits'][0]).all()
    assert np.isnan(r2['dlogits'][1, :, 2, 3]).all() and np.isfinite(r2['dlogits'][1, :, 0, 0]).all()
    assert r0['n_valid'] == int((labels != 255).sum())


def _as_got(r):
    return dict(lse=r['lse'].copy(), loss_sum=r['loss_sum'], n_valid=r['n_valid'], n_correct=r['n_correct_lo'],
                dlogits=r['dlogits'].copy())


def test_budgets_can_fail():
    """the comparison the GPU tests go through accepts the reference itself (rounded to fp32) and rejects a gradient whose
    class 1 is scaled by 1 + 1e-3, an lse shifted by 1e-5, one pixel too many and a NaN that went missing"""
    logits, labels, weight = _case(19, (5, 7), (20, 28), seed=11)
    x32 = logits.float()
    r = ref.reference(x32.numpy(), labels.numpy(), False, 255, weight.numpy(), scale=SCALE, K=20)
    good = _as_got(r)
    good['lse'] = good['lse'].astype(np.float32)
    good['dlogits'] = good['dlogits'].astype(np.float32)
    worst = ref.compare(good, r)
    assert all(v <= 1.0 for v in worst.values())
    bad = _as_got(r)
    bad['dlogits'][:, 1] *= 1 + 1e-3
    with pytest.raises(AssertionError, match='dlogits'):
        ref.compare(bad, r)
    bad = _as_got(r)
    bad['lse'] += 1e-5
    with pytest.raises(AssertionError, match='lse'):
        ref.compare(bad, r)
    bad = _as_got(r)
    bad['loss_sum'] *= 1 + 1e-4
    with pytest.raises(AssertionError, match='loss_sum'):
        ref.compare(bad, r)
    bad = _as_got(r)
    bad['n_valid'] += 1
    with pytest.raises(AssertionError):
        ref.compare(bad, r)
    bad = _as_got(r)
    bad['n_correct'] = r['n_correct_hi'] + 1
    with pytest.raises(AssertionError):
        ref.compare(bad, r)
    bad = _as_got(r)
    bad['dlogits'][0, 0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match='NaN'):
        ref.compare(bad, r)
