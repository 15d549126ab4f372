"""fp64 reference of the point kernels (include/vitadapter_hip_points.h, csrc/point_loss.hip) and the error budgets their
tests use.  Every function starts from the fp32 operands the kernel it mirrors sees and evaluates in fp64 on the CPU.

Budgets (eps = 2^-24; a measured error / budget ratio above 0.5 means re-derive, not widen):
  sample      eps * (8 * sum|w_i v_i| + 4 * (w * Dx + h * Dy)).  Dx / Dy: the largest horizontal / vertical tap difference of the
              point's cell, out-of-range taps counted as 0.  First term: twice the rounding of the weights (1 - f, the product
              wy wx), the product with the value and the three adds (4 eps).  Second: twice the effect of the fp32 coordinate,
              |x_hat - x| <= 2 eps w pixels (the fma rounds once at magnitude <= w, and the point itself is exact), times the
              slope of the bilinear patch.  The value is continuous across a floor() flip, so no point is left out - but the
              slope is not: for a point within that coordinate error of a cell edge (every pixel centre is one) the fp32
              coordinate may fall into the neighbouring cell, so Dx / Dy are the largest over the cells within the error
              (tests/test_point_loss_ref_cpu.py: torch's fp32 grid_sample at the pixel centres of a 0 / 1 mask has a
              non-zero error where the point's own cell is flat).
  sums        a sum of n terms by `serial` adds per lane, a 6-level wave butterfly and `waves` waves in order has
              depth = serial + 6 + (waves - 1) roundings on any path: depth * eps * sum|term|, plus the terms' own budgets:
              8 eps (|x| + 1) per transcendental term (expf / log1pf to a few ulp, the adds of max(x, 0) and the product with t).
              match cost: 256 lanes (serial = ceil(P / 256), waves = 4).
"""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24


def _coords(points, h, w):
    """pixel coordinates of fp32 points (..., 2), exact in fp64"""
    p = points.double()
    return p[..., 0] * w - 0.5, p[..., 1] * h - 0.5


def _taps(maps, x, y):
    """maps (R, h, w) fp64, coordinates (R, P) -> four (value, weight, in range) triples, y major; an out-of-range tap has
    value and weight 0"""
    R, h, w = maps.shape
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    r = torch.arange(R)[:, None].expand_as(x)
    out = []
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            v = maps[r, yi.clamp(0, h - 1).long(), xi.clamp(0, w - 1).long()]
            out.append((torch.where(ok, v, torch.zeros_like(v)), torch.where(ok, wy * wx, torch.zeros_like(v)), ok))
    return out


def sample(maps, points, map_idx=None, set_idx=None):
    """-> (value (R, P) fp64, budget (R, P)) of vah_pts_sample; maps (M, h, w) any dtype, points (S, P, 2) fp32"""
    M, h, w = maps.shape
    m = maps.double() if map_idx is None else maps.double()[torch.as_tensor(map_idx).long()]
    p = points if set_idx is None else points[torch.as_tensor(set_idx).long()]
    R = min(m.shape[0], p.shape[0])
    m, p = m[:R], p[:R]
    x, y = _coords(p, h, w)
    taps = _taps(m, x, y)
    val = sum(torch.where(ok, v * wt, torch.zeros_like(v)) for v, wt, ok in taps)
    mag = sum(torch.where(ok, (v * wt).abs(), torch.zeros_like(v)) for v, wt, ok in taps)
    # the cell an fp32 evaluation sees: the coordinate may land on the other side of a cell edge that lies within its error
    ex = 2 * EPS * w * p[..., 0].double().abs().clamp(min=1)
    ey = 2 * EPS * h * p[..., 1].double().abs().clamp(min=1)
    Dx, Dy = torch.zeros_like(val), torch.zeros_like(val)
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            (v00, _, _), (v01, _, _), (v10, _, _), (v11, _, _) = _taps(m, x + sx * ex, y + sy * ey)
            Dx = torch.maximum(Dx, torch.maximum((v01 - v00).abs(), (v11 - v10).abs()))
            Dy = torch.maximum(Dy, torch.maximum((v10 - v00).abs(), (v11 - v01).abs()))
    return val, EPS * (8 * mag + 4 * (w * Dx + h * Dy))


def softplus(x):
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def sum_depth(P, lanes):
    return -(-P // lanes) + 6 + (lanes // 64 - 1)


def match_cost(xs, ts, cls, labels, counts, weights, eps):
    """-> (cost (N, Q, Gmax) fp64 with +inf padding, budget) of vah_pts_match_cost from its fp32 operands"""
    N, Q, C1 = cls.shape
    P = xs.shape[1]
    Gmax = max(counts) if counts else 0
    w_cls, w_mask, w_dice = weights
    cost = torch.full((N, Q, Gmax), float('inf'), dtype=torch.float64)
    budget = torch.zeros((N, Q, Gmax), dtype=torch.float64)
    depth = sum_depth(P, 256)
    lo = 0
    for n, G in enumerate(counts):
        if G == 0:
            continue
        x, t, lab = xs[n * Q:(n + 1) * Q].double(), ts[lo:lo + G].double(), labels[lo:lo + G].long()
        lo += G
        z = cls[n].double()
        zc = z - z.max(-1, keepdim=True)[0]
        prob = torch.softmax(z, -1)[:, lab]
        b_prob = prob * EPS * (C1 + 16 * (zc.abs().max(-1, keepdim=True)[0] + 1) + 4)
        s, own = torch.sigmoid(x), 8 * EPS * (x.abs() + 1)
        sp_pos, sp_neg = softplus(x), softplus(-x)
        m = sp_neg @ t.T + sp_pos @ (1 - t).T                       # terms are non-negative: sum|term| = the sum
        b_m = depth * EPS * m + own.sum(-1, keepdim=True)
        a, b, c = s @ t.T, s.sum(-1, keepdim=True), t.sum(-1)[None, :]
        b_a, b_b, b_c = depth * EPS * a + own @ t.T, depth * EPS * b + own.sum(-1, keepdim=True), depth * EPS * c
        D = b + c + eps
        dice = 1 - (2 * a + eps) / D
        b_dice = 2 * b_a / D + (2 * a + eps) / D ** 2 * (b_b + b_c) + 8 * EPS
        cost[n, :, :G] = w_cls * -prob + w_mask * m / P + w_dice * dice
        budget[n, :, :G] = (abs(w_cls) * b_prob + abs(w_mask) * (b_m / P + 4 * EPS * m / P) + abs(w_dice) * b_dice
                            + 4 * EPS * (abs(w_cls) * prob + abs(w_mask) * m / P + abs(w_dice) * dice.abs()))
    return cost, budget


def grid_sample64(maps, points):
    """mmcv point_sample restated on F.grid_sample, fp64: maps (R, h, w), points (R, P, 2) -> (R, P)"""
    return F.grid_sample(maps.double()[:, None], 2.0 * points.double()[:, None] - 1.0, mode='bilinear', padding_mode='zeros',
                         align_corners=False)[:, 0, 0]


def edge_points(h, w):
    """points the tests must include: 0, 1 - 2^-24, every pixel centre (i + 0.5) / w, and points outside [0, 1]"""
    one = 1.0 - 2.0 ** -24
    xs = [0.0, one, -0.25, 1.25, -1e-3, 1.0, 1.0 + 2.0 ** -20, -3.0, 7.5] + [(i + 0.5) / w for i in range(w)]
    ys = [0.0, one, -0.25, 1.25, 1.0, -1e-3] + [(i + 0.5) / h for i in range(h)]
    pts = [(x, ys[i % len(ys)]) for i, x in enumerate(xs)] + [(xs[i % len(xs)], y) for i, y in enumerate(ys)]
    pts += [(0.0, 0.0), (one, one), (0.0, one), (one, 0.0), (-5.0, 0.5), (0.5, 9.0), (1e30, 0.5), (0.5, -1e30)]
    return torch.tensor(pts, dtype=torch.float32)


def ratio(got, want, budget):
    """largest |got - want| / budget over the finite entries (0 / 0 counts as 0); non-finite entries must agree exactly"""
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = torch.isfinite(want)
    assert bool((torch.isfinite(got) == fin).all()), 'finite / non-finite pattern differs'
    assert bool(((got == want) | (torch.isnan(got) & torch.isnan(want)))[~fin].all()), 'non-finite entries differ'
    err = (got - want).abs()[fin]
    b = budget.double().expand_as(want)[fin]
    if err.numel() == 0:
        return 0.0
    r = torch.where(err == 0, torch.zeros_like(err), err / b.clamp(min=1e-300))
    return float(r.max())
