"""GPU: the point kernels (csrc/point_loss.hip) by direct C calls against the fp64 reference and the budgets of
tests/point_loss_ref.py, every output NaN-filled first.

Sample: maps 1 x 1, 2 x 3, 5 x 7, 32 x 48 and 160 x 160, fp32 and uint8, P in {1, 63, 64, 65, 257} plus the edge set (0,
1 - 2^-24, every pixel centre, points outside [0, 1], |p| = 1e30), with and without index arrays, one point set shared by 8
rows, a row stride wider than the map.  Cost: (N, Q, G) in {(1, 1, 1), (2, 8, (3, 0)), (1, 100, 13)} x P in {1, 65, 12 544}; the
+inf padding is exact.

A ratio is max |err| / budget; every one must be <= 1, and one above 0.5 means the budget is to be
re-derived, not widened.  Worst ratios of a run on an MI355X (the RATIO lines; MEASURED repeats them):
    sample 0.250   cost 0.079
"""
import pytest
import torch

import _vah
import point_loss_ref as ref

pytestmark = pytest.mark.gpu

lib = _vah.lib
NAN = float('nan')
# worst ratios over all cases, copied from the RATIO lines of a run on an MI355X
MEASURED = {
    'sample': '0.250 over all cases of test_sample',
    'cost': '0.079 over all cases of test_match_cost',
}
WORST = {}


def _dev():
    return torch.device('cuda:0')


def _note(name, r):
    WORST[name] = max(WORST.get(name, 0.0), r)
    print('RATIO %s %.3f (worst so far %.3f)' % (name, r, WORST[name]))
    assert r <= 1.0, (name, r)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _points(P, seed, h, w):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((P, 2), generator=g) * 1.2 - 0.1


def c_sample(maps, points, map_idx, set_idx, R):
    dev = _dev()
    m, p = maps.to(dev), points.to(dev).contiguous()
    mi = None if map_idx is None else torch.as_tensor(map_idx, dtype=torch.int32, device=dev)
    si = None if set_idx is None else torch.as_tensor(set_idx, dtype=torch.int32, device=dev)
    out = torch.full((R, p.shape[1]), NAN, device=dev)
    code = {torch.float32: 0, torch.uint8: 3}[m.dtype]
    rc = lib.vah_pts_sample(m.data_ptr(), code, m.stride(0), m.stride(1), m.shape[0], m.shape[1], m.shape[2], p.data_ptr(), p.shape[0],
                            p.shape[1], _ptr(mi), _ptr(si), R, out.data_ptr(), _vah.raw_stream(dev))
    _vah.check(rc, 'vah_pts_sample')
    torch.cuda.synchronize()
    return out.cpu()


def _maps(M, h, w, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return (torch.rand((M, h, w), generator=g) < 0.5).to(torch.uint8)
    return torch.randn((M, h, w), generator=g) * 4


@pytest.mark.parametrize('dtype', [torch.float32, torch.uint8], ids=['f32', 'u8'])
@pytest.mark.parametrize('hw', [(1, 1), (2, 3), (5, 7), (32, 48), (160, 160)], ids=lambda s: '%dx%d' % s)
def test_sample(hw, dtype):
    h, w = hw
    M = 3 if h == 160 else 8
    maps = _maps(M, h, w, dtype, 11 + h)
    edge = ref.edge_points(h, w)
    for P in (1, 63, 64, 65, 257, edge.shape[0]):
        sets = torch.stack([_points(P, 100 * s + P, h, w) for s in range(M)])
        if P == edge.shape[0]:
            sets[0] = edge
        # identity rows
        want, budget = ref.sample(maps, sets)
        _note('sample', ref.ratio(c_sample(maps, sets, None, None, M), want, budget))
        # index arrays: 8 rows share point set 0 (the edge set where there is one), maps in a scrambled order with a repeat
        mi, si = [(3 * r + 1) % M for r in range(8)], [0] * 8
        want, budget = ref.sample(maps, sets, mi, si)
        _note('sample', ref.ratio(c_sample(maps, sets, mi, si, 8), want, budget))
        # one index array only
        want, budget = ref.sample(maps, sets, mi[:M], None)
        _note('sample', ref.ratio(c_sample(maps, sets, mi[:M], None, M), want, budget))
    # a row stride wider than the map, a map stride that is not h * row stride
    wide = torch.zeros((M, h + 1, w + 5), dtype=maps.dtype)
    wide[:, :h, :w] = maps
    view = wide.to(_dev())[:, :h, :w]
    sets = torch.stack([_points(65, 7 + s, h, w) for s in range(M)])
    want, budget = ref.sample(maps, sets)
    _note('sample', ref.ratio(c_sample(view, sets, None, None, M), want, budget))


def test_sample_nonfinite_values_reach_the_output_as_in_torch():
    """points on a dyadic grid, so that the fp32 and the exact coordinate agree: an in-range tap of weight 0 on an inf gives
    NaN, an out-of-range tap gives nothing"""
    maps = torch.arange(16, dtype=torch.float32).reshape(1, 4, 4).clone()
    maps[0, 1, 1], maps[0, 3, 3] = float('inf'), float('nan')
    pts = torch.tensor([[[0.125, 0.125], [0.375, 0.375], [0.25, 0.25], [0.125, 0.375], [0.875, 0.875], [1.0, 1.0], [0.875, 0.125],
                         [0.625, 0.625], [1.125, 0.875]]])
    want, budget = ref.sample(maps, pts)
    got = c_sample(maps, pts, None, None, 1)
    ref.ratio(got, want, budget)                                   # the non-finite pattern is compared exactly
    torch_way = ref.grid_sample64(maps, pts)
    assert torch.equal(torch.isnan(got), torch.isnan(torch_way)) and torch.equal(torch.isinf(got), torch.isinf(torch_way))
    assert bool(torch.isnan(got[0, 0])) and bool(torch.isinf(got[0, 1])) and float(got[0, 6]) == 3.0


@pytest.mark.parametrize('P', [1, 65, 12544])
@pytest.mark.parametrize('shape', [(1, 1, (1,)), (2, 8, (3, 0)), (1, 100, (13,))], ids=['1x1x1', '2x8x3+0', '1x100x13'])
def test_match_cost(shape, P):
    N, Q, counts = shape
    counts = list(counts)
    G, Gmax, C1 = sum(counts), max(counts), 6 if Q < 100 else 151
    g = torch.Generator().manual_seed(5 * Q + P)
    xs = torch.randn((N * Q, P), generator=g) * 8
    ts = torch.rand((G, P), generator=g)
    ts[:, ::3] = (ts[:, ::3] > 0.5).float()                        # many exact 0 / 1, as samples inside a mask are
    cls = torch.randn((N, Q, C1), generator=g) * 3
    labels = torch.randint(0, C1 - 1, (G,), generator=g)
    offsets = torch.tensor([sum(counts[:n]) for n in range(N + 1)], dtype=torch.int32)
    weights, eps = (2.0, 5.0, 5.0), 1.0
    dev = _dev()
    d = [t.to(dev) for t in (xs, ts, offsets, cls, labels)]
    cost = torch.full((N, Q, Gmax), NAN, device=dev)
    rc = lib.vah_pts_match_cost(*[t.data_ptr() for t in d], N, Q, C1, G, Gmax, P, *weights, eps, cost.data_ptr(), _vah.raw_stream(dev))
    _vah.check(rc, 'vah_pts_match_cost')
    torch.cuda.synchronize()
    want, budget = ref.match_cost(xs, ts, cls, labels, counts, weights, eps)
    got = cost.cpu()
    for n, c in enumerate(counts):
        assert bool((got[n, :, c:] == float('inf')).all()) and bool(torch.isfinite(got[n, :, :c]).all())
    _note('cost', ref.ratio(got, want, budget))
