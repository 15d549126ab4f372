"""fp64 reference of the sampled mask losses and their backward (include/vitadapter_hip_point_mask_loss.h,
csrc/point_mask_loss.hip) and the error budgets their tests use.  Everything starts from the fp32 operands the kernels see and
is evaluated in fp64 on the CPU; samples and their budgets are point_loss_ref.sample's.

Budgets (eps = 2^-24; a measured error / budget ratio above 0.5 means re-derive, not widen).  b(.) is the budget of a
quantity, x / t the two samples, s = sigmoid(x), u = s (1 - s).
  xs, ts      point_loss_ref.sample's budget, per tap: b(x), b(t).
  terms       each of the four per-point terms has its own rounding and what the error of its samples does to it (first order,
              the derivative times b(x) / b(t)); own = 8 eps (|x| + 1) per transcendental term, as in point_loss_ref:
                  softplus(x) - x t   own + 2 eps |x t| + |s - t| b(x) + |x| b(t)        (d/dx = s - t, d/dt = -x)
                  s t                 own |t| + u |t| b(x) + s b(t)
                  s                   own + u b(x)
                  t                   b(t)
  sums        the order the header states: a serial run of 4 per lane, a butterfly of 6 levels, 3 adds over the four waves,
              then chunks - 1 adds over the ceil(P / 1024) chunks: depth = 4 + 6 + 3 + (chunks - 1) roundings on any path,
              depth * eps * sum|term| + the sum of the terms' budgets.  This gives b(bce), b(A), b(B), b(T).
  dice        D = (B + T) + eps: b(D) = b(B) + b(T) + 2 eps |D|;  dice = 1 - (2 A + eps) / D:
              2 b(A) / D + (2 A + eps) / D^2 b(D) + 8 eps (the product, the add, the division and the subtraction from 1 at O(1)).
  gx          gx = g_bce (s - t) + g_dice u v,  v = c - 2 t / D,  c = (2 A + eps) / D^2.  The kernel starts from its own xs, ts
              and sums, so their budgets enter:
                  b(s) = 8 eps (|x| + 1) + u b(x);  b(u) = b(s) + 2 eps u             (|d u / d s| = |1 - 2 s| <= 1)
                  b(c) = 2 b(A) / D^2 + 2 c b(D) / D + 4 eps c
                  b(v) = b(c) + 2 b(t) / D + 2 |t| b(D) / D^2 + 3 eps (c + |2 t / D|)
                  b(gx) = |g_bce| (b(s) + b(t) + eps |s - t|) + |g_dice| (b(u) |v| + u b(v) + 2 eps u |v|)
                          + 4 eps (|g_bce (s - t)| + |g_dice u v|)
  dmaps       a pixel is the serial sum of its list of weight * gx terms, n terms: n eps sum|weight gx| for the order, plus
              per term weight b(gx) + |gx| b(weight) + 3 eps weight |gx|.  b(weight): the fp32 coordinate is off by at most
              ex = 2 eps w max(|px|, 1) pixels (point_loss_ref: the fma rounds once at magnitude <= w), the same in y, and a
              weight is a product of two fractions in [0, 1] each rounded once more: b(weight) = ex + ey + 4 eps.  A point within
              that error of a cell edge may be binned into the neighbouring cell by the fp32 floor; its weights are continuous
              across the flip (the tap it gains has a weight below b(weight)), but the list it is in is not, so every distinct
              cell within the error contributes its terms to the budget (and to n), the point's own cell first.
"""
import torch

import point_loss_ref as base

EPS = base.EPS
CHUNK = 1024


def sum_depth(P):
    return 4 + 6 + 3 + (-(-P // CHUNK) - 1)


def forward(pred, tgt, points, rows, tgt_rows, eps):
    """pred (Mp, h, w) fp32, tgt (Mt, H, W) fp32 / uint8, points (K, P, 2) fp32, rows / tgt_rows lists or None ->
    dict of (value, budget) pairs for xs, ts (K, P), bce, dice (K,), sums (K, 4) = (A, B, T, bce), all fp64"""
    x, bx = base.sample(pred, points, rows, None)
    t, bt = base.sample(tgt, points, tgt_rows, None)
    P = points.shape[1]
    depth = sum_depth(P)
    s = torch.sigmoid(x)
    u = s * (1 - s)
    own = 8 * EPS * (x.abs() + 1)
    terms = {
        'bce': (base.softplus(x) - x * t, own + 2 * EPS * (x * t).abs() + (s - t).abs() * bx + x.abs() * bt),
        'A': (s * t, own * t.abs() + u * t.abs() * bx + s * bt),
        'B': (s, own + u * bx),
        'T': (t, bt),
    }
    tot = {k: (v.sum(1), depth * EPS * v.abs().sum(1) + b.sum(1)) for k, (v, b) in terms.items()}
    (A, bA), (B, bB), (T, bT), (bce, bbce) = tot['A'], tot['B'], tot['T'], tot['bce']
    D = B + T + eps
    bD = bB + bT + 2 * EPS * D.abs()
    dice = 1 - (2 * A + eps) / D
    bdice = 2 * bA / D.abs() + (2 * A + eps).abs() / D ** 2 * bD + 8 * EPS
    return {'xs': (x, bx), 'ts': (t, bt), 'bce': (bce, bbce), 'dice': (dice, bdice),
            'sums': (torch.stack([A, B, T, bce], 1), torch.stack([bA, bB, bT, bbce], 1)), 'D': (D, bD)}


def gx(fwd, g_bce, g_dice, eps):
    """-> (gx (K, P) fp64, budget) from forward()'s dict and the fp32 upstream gradients (K,)"""
    (x, bx), (t, bt), (D, bD) = fwd['xs'], fwd['ts'], fwd['D']
    A, bA = fwd['sums'][0][:, 0], fwd['sums'][1][:, 0]
    gb, gd = g_bce.double()[:, None], g_dice.double()[:, None]
    D, bD, A, bA = D[:, None], bD[:, None], A[:, None], bA[:, None]
    s = torch.sigmoid(x)
    u = s * (1 - s)
    c = (2 * A + eps) / D ** 2
    v = c - 2 * t / D
    val = gb * (s - t) + gd * u * v
    bs = 8 * EPS * (x.abs() + 1) + u * bx
    bu = bs + 2 * EPS * u
    bc = 2 * bA / D ** 2 + 2 * c.abs() * bD / D.abs() + 4 * EPS * c.abs()
    bv = bc + 2 * bt / D.abs() + 2 * t.abs() * bD / D ** 2 + 3 * EPS * (c.abs() + (2 * t / D).abs())
    budget = (gb.abs() * (bs + bt + EPS * (s - t).abs()) + gd.abs() * (bu * v.abs() + u * bv + 2 * EPS * u * v.abs())
              + 4 * EPS * ((gb * (s - t)).abs() + (gd * u * v).abs()))
    return val, budget


def _cell_taps(points, h, w, sx, sy):
    """the cell of every point with its coordinate moved by (sx, sy) times its fp32 error, and the four (pixel index, weight,
    in range) of that cell, y major.  -> (cell id (K, P), taps)"""
    x, y = base._coords(points, h, w)
    ex = 2 * EPS * w * points[..., 0].double().abs().clamp(min=1)
    ey = 2 * EPS * h * points[..., 1].double().abs().clamp(min=1)
    x, y = x + sx * ex, y + sy * ey
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    taps = []
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            taps.append(((yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long(), wy * wx, ok))
    return y0.clamp(-3, h + 1) * (w + 5) + x0.clamp(-3, w + 1), taps, ex + ey + 4 * EPS


def dmaps(points, g, bg, h, w):
    """the adjoint of the bilinear sample: points (K, P, 2) fp32, g / bg (K, P) fp64 (gx and its budget) ->
    (dmaps (K, h, w) fp64, budget, touched (K, h, w) bool: the pixels with a tap of the exact evaluation, reach: the pixels
    with a tap of any cell within the coordinate error - outside it no fp32 evaluation has a tap)"""
    K, P, _ = points.shape
    base_idx = (torch.arange(K) * h * w)[:, None]
    val, touched = torch.zeros(K * h * w, dtype=torch.float64), torch.zeros(K * h * w, dtype=torch.float64)
    terms, mag, count = torch.zeros_like(val), torch.zeros_like(val), torch.zeros_like(val)
    seen = []
    for sx, sy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)):
        cell, taps, bw = _cell_taps(points, h, w, sx, sy)
        new = torch.ones_like(cell, dtype=torch.bool)
        for c in seen:
            new &= c != cell
        seen.append(cell)
        for idx, wt, ok in taps:
            sel = ok & new
            i = (base_idx + idx)[sel]
            if (sx, sy) == (0, 0):
                val.index_add_(0, i, (wt * g)[sel])
                touched.index_add_(0, i, torch.ones_like(wt)[sel])
            gf = torch.where(torch.isfinite(g), g, torch.zeros_like(g)).abs()
            terms.index_add_(0, i, (wt * bg + gf * bw + 3 * EPS * wt * gf)[sel])
            mag.index_add_(0, i, (wt * gf)[sel])
            count.index_add_(0, i, torch.ones_like(wt)[sel])
    budget = terms + count * EPS * mag
    return val.view(K, h, w), budget.view(K, h, w), touched.view(K, h, w) > 0, count.view(K, h, w) > 0


def reference(pred, tgt, points, rows, tgt_rows, eps, g_bce, g_dice):
    """everything the two entry points write: dict name -> (value, budget), plus 'touched' and 'reach' of dmaps()"""
    fwd = forward(pred, tgt, points, rows, tgt_rows, eps)
    g, bg = gx(fwd, g_bce, g_dice, eps)
    h, w = pred.shape[1:]
    d, bd, touched, reach = dmaps(points, g, torch.where(torch.isfinite(bg), bg, torch.zeros_like(bg)), h, w)
    out = {k: fwd[k] for k in ('xs', 'ts', 'bce', 'dice', 'sums')}
    out['gx'], out['dmaps'], out['touched'], out['reach'] = (g, bg), (d, bd), touched, reach
    return out
