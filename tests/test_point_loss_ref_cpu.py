"""CPU: the fp64 reference and the budgets of tests/point_loss_ref.py, held against things that are not the kernels they
judge: F.grid_sample in fp64 (mmcv's definition of point_sample) at random and at the edge points, the match costs written
as the reference writes them (models/losses/match_costs.py, models/utils/assigner.py:126-145), and an fp32 torch evaluation
of each quantity - this repository's CPU tier, fused.point_sample / fused.match_costs - which must stay within HALF of its
budget: a budget that an honest fp32 evaluation already fills is no budget for a kernel."""
import pytest
import torch
import torch.nn.functional as F

import point_loss_ref as ref
from vitadapter import fused

SHAPES = [(1, 1), (2, 3), (5, 7), (32, 48), (160, 160)]


def _case(h, w, dtype, P, seed):
    g = torch.Generator().manual_seed(seed)
    M = 3
    maps = (torch.rand((M, h, w), generator=g) < 0.5).to(torch.uint8) if dtype == torch.uint8 else torch.randn((M, h, w), generator=g) * 4
    pts = torch.rand((M, P, 2), generator=g) * 1.2 - 0.1
    edge = ref.edge_points(h, w)
    return maps, pts, edge[None].expand(M, -1, -1).contiguous()


@pytest.mark.parametrize('dtype', [torch.float32, torch.uint8], ids=['f32', 'u8'])
@pytest.mark.parametrize('hw', SHAPES, ids=lambda s: '%dx%d' % s)
def test_sample_reference_is_grid_sample_in_fp64(hw, dtype):
    h, w = hw
    maps, pts, edge = _case(h, w, dtype, 257, 3 + h)
    for p in (pts, edge):
        val, budget = ref.sample(maps, p)
        want = ref.grid_sample64(maps, p)
        assert val.dtype == torch.float64 and val.shape == want.shape == budget.shape
        # grid_sample forms the coordinate as ((2 p - 1) + 1) * w / 2 - 0.5: a few fp64 roundings at magnitude <= max(|p|, 1) w,
        # times the slope of the patch (at most 2 * max|v| per pixel)
        scale = float(maps.double().abs().max()) * max(h, w) * max(float(p.abs().max()), 1.0)
        big = p.abs().amax(-1) > 1e6                    # far outside: both are exactly 0
        assert float(val[big].abs().max()) == 0.0 if bool(big.any()) else True
        assert float((val - want)[~big].abs().max()) <= 64 * 2.0 ** -53 * max(scale, 1.0), (hw, float((val - want)[~big].abs().max()))
        assert bool((budget >= 0).all())
    # index arrays pick rows as plain indexing does
    mi, si = [2, 0, 2, 1], [1, 1, 0, 2]
    val, _ = ref.sample(maps, pts, mi, si)
    assert torch.equal(val, ref.grid_sample64(maps[mi], pts[si])) or float((val - ref.grid_sample64(maps[mi], pts[si])).abs().max()) <= 1e-9


def test_sample_reference_known_values():
    maps = torch.arange(8, dtype=torch.float32).reshape(1, 2, 4)
    pts = torch.tensor([[[0.125, 0.25], [0.5, 0.5], [0.0, 0.0], [1.0, 1.0], [-1.0, 0.5], [0.375, 0.75]]])
    val, _ = ref.sample(maps, pts)
    # pixel centre (0, 0); the middle of the map; the corners weigh one tap by 1 / 4; outside; a pixel centre (1, 1)
    assert torch.allclose(val[0], torch.tensor([0.0, 3.5, 0.0, 7.0 / 4, 0.0, 5.0], dtype=torch.float64), atol=1e-12)


@pytest.mark.parametrize('dtype', [torch.float32, torch.uint8], ids=['f32', 'u8'])
@pytest.mark.parametrize('hw', SHAPES, ids=lambda s: '%dx%d' % s)
def test_fp32_torch_sampling_stays_within_half_the_budget(hw, dtype):
    h, w = hw
    maps, pts, edge = _case(h, w, dtype, 257, 5 + h)
    for p in (pts, edge):
        got = fused.point_sample(maps, p)                          # CPU: F.grid_sample in fp32
        assert got.dtype == torch.float32
        val, budget = ref.sample(maps, p)
        r = ref.ratio(got, val, budget)
        assert r <= 0.5, (hw, r)


def _reference_costs(xs, ts, cls, labels, weights, eps):
    """one image, as ClassificationCost, CrossEntropyLossCost(use_sigmoid=True) and DiceCost(pred_act=True) write them"""
    w_cls, w_mask, w_dice = weights
    cls_cost = -cls.softmax(-1)[:, labels] * w_cls
    pos = F.binary_cross_entropy_with_logits(xs, torch.ones_like(xs), reduction='none')
    neg = F.binary_cross_entropy_with_logits(xs, torch.zeros_like(xs), reduction='none')
    mask_cost = (torch.einsum('nc,mc->nm', pos, ts) + torch.einsum('nc,mc->nm', neg, 1 - ts)) / xs.shape[1] * w_mask
    s = xs.sigmoid()
    numerator = 2 * torch.einsum('nc,mc->nm', s, ts)
    denominator = s.sum(-1)[:, None] + ts.sum(-1)[None, :]
    dice_cost = (1 - (numerator + eps) / (denominator + eps)) * w_dice
    return cls_cost + mask_cost + dice_cost


def _cost_case(N, Q, counts, P, C1, seed):
    g = torch.Generator().manual_seed(seed)
    G = sum(counts)
    xs = torch.randn((N * Q, P), generator=g) * 8
    ts = torch.rand((G, P), generator=g)
    ts[:, ::3] = (ts[:, ::3] > 0.5).float()
    cls = torch.randn((N, Q, C1), generator=g) * 3
    labels = torch.randint(0, C1 - 1, (G,), generator=g)
    return xs, ts, cls, labels


COST_CASES = [(1, 1, [1], 1, 6), (2, 8, [3, 0], 65, 6), (1, 100, [13], 12544, 151), (3, 5, [0, 2, 4], 300, 9)]


@pytest.mark.parametrize('N,Q,counts,P,C1', COST_CASES)
def test_match_cost_reference_and_budget(N, Q, counts, P, C1):
    weights, eps = (2.0, 5.0, 5.0), 1.0
    xs, ts, cls, labels = _cost_case(N, Q, counts, P, C1, 7 * Q + P)
    cost, budget = ref.match_cost(xs, ts, cls, labels, counts, weights, eps)
    assert cost.shape == (N, Q, max(counts)) and cost.dtype == torch.float64
    lo = 0
    for n, G in enumerate(counts):
        assert bool((cost[n, :, G:] == float('inf')).all())
        if G:
            want = _reference_costs(xs[n * Q:(n + 1) * Q].double(), ts[lo:lo + G].double(), cls[n].double(), labels[lo:lo + G], weights, eps)
            assert float((cost[n, :, :G] - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))
            assert bool((budget[n, :, :G] > 0).all())
        lo += G
    # the fp32 torch evaluation (the CPU tier) fills at most half of the budget
    got = fused.match_costs(xs, ts, cls, labels, counts, weights, eps)
    assert got.dtype == torch.float32
    r = ref.ratio(got, cost, budget)
    assert r <= 0.5, r


def test_ratio_compares_non_finite_entries_exactly():
    want = torch.tensor([1.0, float('inf'), float('nan')], dtype=torch.float64)
    budget = torch.full((3,), 1e-6, dtype=torch.float64)
    assert ref.ratio(torch.tensor([1.0 + 5e-7, float('inf'), float('nan')], dtype=torch.float64), want, budget) == pytest.approx(0.5, rel=1e-3)
    with pytest.raises(AssertionError):
        ref.ratio(torch.tensor([1.0, 3.0, float('nan')]), want, budget)
    with pytest.raises(AssertionError):
        ref.ratio(torch.tensor([1.0, float('-inf'), float('nan')]), want, budget)
    assert ref.sum_depth(12544, 256) == 49 + 6 + 3 and ref.sum_depth(1, 256) == 10
