"""CPU: the restatement of tests/seg_logits_ref.py against torch's own fp64 operator sequence - the expressions of the
reference's encoder_decoder_mask2former.py (F.interpolate, F.pad, /, softmax, flip, argmax).

torch's fp64 upsample computes its taps in fp64, the restatement (like the kernels) in fp32.  A source coordinate is at most
~52 here, so its fp32 value is off by at most 52 * 2^-23 < 1e-5; the blend is continuous in it, with slope at most 2 max|v|
per axis: 1e-4 * (A + max|v| of the plane) bounds the difference with room to spare, and a wrong tap or a wrong weight order
is off by O(|v|).  The budgets are non-negative."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_logits_ref as ref  # noqa: E402


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize('align', (False, True))
@pytest.mark.parametrize('hw_in,hw_out', (((12, 13), (48, 52)), ((12, 13), (31, 45)), ((1, 13), (5, 52)), ((12, 1), (48, 3)),
                                          ((48, 52), (31, 45)), ((5, 7), (5, 7))))
def test_resize_matches_interpolate(hw_in, hw_out, align):
    v = _randn(2, 3, *hw_in, seed=1)
    want = F.interpolate(v, size=hw_out, mode='bilinear', align_corners=align).numpy()
    got, A = ref.resize(v.numpy(), hw_out, align)
    tol = 1e-4 * (A + np.abs(v.numpy()).max())
    err = np.abs(got - want)
    print('resize %s -> %s align %s: worst err / tol %.3g' % (hw_in, hw_out, align, (err / tol).max()))
    assert (err <= tol).all()
    assert (A >= np.abs(got) - 1e-12).all()


@pytest.mark.parametrize('accumulate', (False, True))
def test_resize_add_matches_pad_and_add(accumulate):
    src, prior = _randn(2, 3, 12, 13, seed=2), _randn(2, 3, 61, 67, seed=3)
    up = F.interpolate(src, size=(48, 52), mode='bilinear', align_corners=False)
    if accumulate:
        want = prior + F.pad(up, (7, 67 - 7 - 52, 5, 61 - 5 - 48))
    else:
        want = prior.clone()
        want[:, :, 5:53, 7:59] = up
    got, budget, mask = ref.resize_add(src.numpy(), prior.numpy(), 5, 7, (48, 52), False, accumulate)
    assert np.array_equal(got[~mask], prior.numpy()[~mask]) and (budget[~mask] == 0).all()
    assert mask.sum() == 2 * 3 * 48 * 52
    assert np.abs(got - want.numpy()).max() <= 1e-4 * 2 * np.abs(src.numpy()).max()
    assert (budget >= 0).all() and (budget[mask] > 0).all()


@pytest.mark.parametrize('flip', (0, 1, 2))
@pytest.mark.parametrize('size', (None, (31, 45), (70, 80)))
def test_finish_matches_the_reference_expression(size, flip):
    C = 5
    acc = _randn(2, C, 48, 52, seed=4)
    cy = torch.ones(48, dtype=torch.int32)
    cx = torch.ones(52, dtype=torch.int32)
    cy[16:32] += 1
    cx[20:30] += 1
    region = (44, 50)
    prior = _randn(2, C, *(size or region), seed=5).abs()
    v = (acc / (cy[:, None] * cx[None, :]).double())[:, :, :region[0], :region[1]]
    if size is not None:
        v = F.interpolate(v, size=size, mode='bilinear', align_corners=False)
    p = F.softmax(v, dim=1)
    if flip:
        p = p.flip(dims=(3,) if flip == 1 else (2,))
    r = ref.finish(acc.numpy(), cy.numpy(), cx.numpy(), region, size, False, flip, prior=prior.numpy())
    assert np.abs(r['p'] - p.numpy()).max() <= 1e-4
    assert np.abs(r['prob'] - (prior + p).numpy()).max() <= 1e-4
    sure = r['gap'] >= ref.BAND
    assert sure.mean() > 0.99
    assert np.array_equal(r['labels'][sure], p.argmax(1).numpy()[sure])
    assert (r['budget'] >= 0).all() and np.isfinite(r['budget']).all()
    # without counts, region or prior: whole mode
    r0 = ref.finish(acc.numpy(), size=size, flip=flip)
    v0 = acc if size is None else F.interpolate(acc, size=size, mode='bilinear', align_corners=False)
    p0 = F.softmax(v0, dim=1)
    if flip:
        p0 = p0.flip(dims=(3,) if flip == 1 else (2,))
    assert np.abs(r0['prob'] - p0.numpy()).max() <= 1e-4 and r0['prob'] is r0['p']


def test_non_finite_values_follow_torch():
    acc = _randn(1, 4, 6, 7, seed=6)
    acc[0, 1, 1, 1] = float('nan')
    acc[0, 2, 4, 5] = float('inf')
    acc[0, :, 2, 4] = float('-inf')
    acc[0, 0, 0, 6] = float('-inf')
    for size in (None, (13, 15)):
        v = acc if size is None else F.interpolate(acc, size=size, mode='bilinear', align_corners=False)
        p = F.softmax(v, dim=1)
        r = ref.finish(acc.numpy(), size=size)
        assert np.array_equal(np.isnan(r['p']), torch.isnan(p).numpy())
        ok = ~np.isnan(r['p'])
        assert np.abs(r['p'][ok] - p.numpy()[ok]).max() <= 1e-4
        assert np.array_equal(r['labels'][np.isnan(r['p']).all(1)], p.argmax(1).numpy()[np.isnan(r['p']).all(1)])
    assert np.isnan(ref.finish(acc.numpy())['p'][0, :, 2, 4]).all() and ref.finish(acc.numpy())['p'][0, 0, 0, 6] == 0


def test_argmax_rules():
    total = _randn(2, 6, 5, 7, seed=7).abs()
    total[0, 3] = total[0, 1]                       # a tie: the lower index wins
    total[1, 4, 2, 2] = float('nan')
    for divisor in (1, 3, 6):
        labels, gap = ref.argmax(total.numpy(), divisor)
        assert np.array_equal(labels, (total / divisor).argmax(1).numpy())
        assert not (labels[0] == 3).any() and labels[1, 2, 2] == 4
        assert (gap[~np.isnan(gap)] >= 0).all()
