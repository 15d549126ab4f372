"""CPU: the fp64 reference of tests/point_mask_loss_ref.py against fp64 autograd of torch's own expression (F.grid_sample +
binary_cross_entropy_with_logits + the dice line of fused.point_mask_losses): values, gx and dmaps on a 5 x 7 map with the
edge point set (0, 1 - 2^-24, every pixel centre, points outside [0, 1]), targets 11 x 9 in both dtypes, rows scrambled and
tgt_rows with a repeat.  Both sides are fp64 evaluations of the same real functions: they agree to 1e-12 of the largest
element.  Also: a budget is positive wherever its value is non-zero."""
import pytest
import torch
import torch.nn.functional as F

import point_loss_ref as base
import point_mask_loss_ref as ref

H, W, EPS_DICE = 5, 7, 1.0


def _case(dtype):
    g = torch.Generator().manual_seed(3)
    pred = torch.randn((6, H, W), generator=g) * 4
    tgt = torch.rand((4, 11, 9), generator=g)
    if dtype == torch.uint8:
        tgt = (tgt < 0.5).to(torch.uint8)
    edge = base.edge_points(H, W)
    rnd = torch.rand((edge.shape[0], 2), generator=g) * 1.2 - 0.1
    points = torch.stack([edge, rnd, edge.flip(0)])
    rows, tgt_rows = [4, 1, 3], [2, 0, 2]
    g_bce, g_dice = torch.tensor([0.5, -1.25, 2.0]), torch.tensor([3.0, 0.75, -1.5])
    return pred, tgt, points, rows, tgt_rows, g_bce, g_dice


def _torch_side(pred, tgt, points, rows, tgt_rows, g_bce, g_dice):
    maps = pred.double()[rows].clone().requires_grad_(True)
    x = base.grid_sample64(maps, points)
    x.retain_grad()
    t = base.grid_sample64(tgt.double()[tgt_rows], points)
    bce = F.binary_cross_entropy_with_logits(x, t, reduction='none').sum(1)
    s = x.sigmoid()
    dice = 1 - (2 * (s * t).sum(1) + EPS_DICE) / (s.sum(1) + t.sum(1) + EPS_DICE)
    (bce * g_bce.double() + dice * g_dice.double()).sum().backward()
    return x.detach(), t, bce.detach(), dice.detach(), x.grad, maps.grad


def _close(got, want):
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0), float((got - want).abs().max())


@pytest.mark.parametrize('dtype', [torch.float32, torch.uint8], ids=['f32', 'u8'])
def test_reference_is_torchs_expression_and_its_autograd(dtype):
    pred, tgt, points, rows, tgt_rows, g_bce, g_dice = _case(dtype)
    out = ref.reference(pred, tgt, points, rows, tgt_rows, EPS_DICE, g_bce, g_dice)
    x, t, bce, dice, gx, dm = _torch_side(pred, tgt, points, rows, tgt_rows, g_bce, g_dice)
    _close(out['xs'][0], x)
    _close(out['ts'][0], t)
    _close(out['bce'][0], bce)
    _close(out['dice'][0], dice)
    _close(out['sums'][0][:, 3], bce)
    _close(out['gx'][0], gx)
    _close(out['dmaps'][0], dm)
    # a pixel without a tap is exactly zero on both sides
    assert bool((out['dmaps'][0][~out['touched']] == 0).all()) and bool((dm[~out['touched']] == 0).all())
    assert bool(out['touched'].any()) and not bool(out['touched'].all())


@pytest.mark.parametrize('dtype', [torch.float32, torch.uint8], ids=['f32', 'u8'])
def test_budgets_are_positive_where_the_value_is_not_zero(dtype):
    pred, tgt, points, rows, tgt_rows, g_bce, g_dice = _case(dtype)
    out = ref.reference(pred, tgt, points, rows, tgt_rows, EPS_DICE, g_bce, g_dice)
    for name in ('xs', 'ts', 'bce', 'dice', 'sums', 'gx', 'dmaps'):
        val, budget = out[name]
        assert val.shape == budget.shape and bool(torch.isfinite(budget).all()), name
        assert bool((budget[val != 0] > 0).all()), name
        assert bool((budget >= 0).all()), name
    # and they are budgets of an fp32 evaluation, not slack: small against the values
    assert float((out['bce'][1] / out['bce'][0].abs()).max()) < 1e-4
    assert float(out['dice'][1].max()) < 1e-4


def test_sum_depth_follows_the_chunks():
    assert ref.sum_depth(1) == 13 and ref.sum_depth(1024) == 13 and ref.sum_depth(1025) == 14 and ref.sum_depth(12544) == 25
