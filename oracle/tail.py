"""fp64 reference of the output-tail kernels (csrc/tail_ops.hip, all but bn_finalize_kernel, which oracle/spm.py
holds) and the per-element budgets they are held to (tests/test_tail_fp64_gpu.py).

Every reference starts from the exact operands the kernel saw (bf16 upcast, fp32 as it is) and, for the passes behind
the statistics, from the kernel's own fp32 mean / rstd / mdy / mdyx.  Each returns A next to the result: the same
computation on absolute values, the sum of |terms| behind every element.

The bilinear upsample (align_corners=False, explicit scale s = 2^k) is written from the integer form of its taps,

    n = max(2 d + 1 - s, 0)     i0 = min(n // 2s, n_lo - 1)     i1 = min(i0 + 1, n_lo - 1)     w1 = (n mod 2s) / 2s

as two separable index / weight applications (rows, then columns), not through F.interpolate; its adjoint is the
same two applications as index_add.  tests/test_tail_oracle_cpu.py compares both with torch's own fp64 interpolate
and autograd.

    t    = a + b + shift + upsample(x)                       sums  = [sum t | sum t^2]
    y    = [relu]((t - mean) rstd gamma + beta)              bsums = [sum dy' | sum dy' xhat]
    dt   = gamma rstd (dy' - mdy - xhat mdyx)                dxlo  = upsample^T(dt)
    planes[b][co][2y + dy][2x + dx] = U[b][(2 dy + dx) C + co][y w + x] (+ addend)
    planes[b][c][t] = tokens[b][t0 + t][c]                   tokens[b][t0 + t][c] = planes[b][c][t] + vec[c]

Budget, as in oracle/spm.py:   |got - ref| <= C 2^-24 A   (+ 2^-8 |ref| per bf16 rounding of the output).

The constants bound the longest dependent chain of fp32 operations behind an element (a chain of d roundings is off
by at most d 2^-24 A):

  * t itself (sum4).  a + (shift + b): 2 roundings, + u: 1.  u is two nested lerps c0 + w (c1 - c0).  One lerp is off
    by 2^-24 (w (|c0| + |c1|) + |result|); against its A = (1 - w) |c0| + w |c1| the first term is at most
    w / (1 - w) <= 2s - 1 times larger (w = (2s - 1) / 2s with all the weight of A on c0), so a lerp costs at most
    2s and the two nested ones 4s: t is off by at most (4s + 3) 2^-24 A_t, 35 at s = 8, 19 at s = 4, 3 at s = 1.
  * C_ELT = 48, the elementwise outputs.  y = t sc + sh: t's 35, sc = rstd gamma 1, sh = beta - mean sc 2, the fma
    1: 39.  dt = k (dy' - mdy - (t - mean) rstd mdyx): t's 35, three products, two differences, k and k's own
    product: 43.
  * C_LO = 128, dxlo.  A low-res pixel gathers at most 3s columns (one fma each), then at most 3s rows, and is added
    to the map once (a plain add or one float atomic): 6s + 1 = 49 at s = 8, on top of dt's 43: 92.
  * C_ACC = 256 (the project's largest, oracle/spm.py), the channel sums.  A thread adds its quads one after the
    other, q = ceil(rows_per_block W / 4 / 256) of them with 2 more roundings inside a quad; block_sum is 6 wave
    steps + 3; tail_finalize walks nparts / 8 rows and adds 8 columns, at most 512 / 8 + 8 = 72 at the cap; and
    every term carries its own error, 2 * 35 + 1 = 71 for t^2 at s = 8 (39 at s = 4; dy' (t - mean) rstd: 38).  With
    x and s > 1 the LDS limit of the plan (rows_per_block (W + W / s) floats <= 150 KB) holds q <= 38:
    38 + 2 + 9 + 72 + 71 = 192.  Without x, or at s = 1, the terms cost 7 and q is bounded by the 2^16 items of a
    workgroup only: 256 covers q <= 166, a workgroup tile of up to 170 000 pixels, which is every case of the test
    file and every shape with N H W <= 21 M pixels per channel (production: q = 8; N = 170 at 256 x 256: q = 22).
  * the GEMMs behind up_from_tokens (hipBLASLt, fp32 accumulation in MFMA steps of 16 or 32 along K): K / 16 = 64 for
    the product at K = 1024, 256 for d rows at K = 4 Co = 4096, both within C_ACC; the fp32 weight gradient is summed
    over K = h w tokens per image and over the images, which as a worst-case chain (1 050 at 128 x 128) is beyond
    any constant the project uses.  It is held to C_ACC like the others: the measured error is that of a random
    walk, and DESIGN 4.7 records how much of the budget it uses.

ReLU: RELU_EDGE of oracle/spm.py.  Elements whose fp64 pre-activation lies within RELU_EDGE (|t sc| + |sh|) of zero
may take either side of the fp32 mask: they are left out of da and enter the budgets of the backward sums with
|dy| and |dy xhat|.
"""
import torch

from oracle.spm import BF16_U, C_ACC, RELU_EDGE, U, bound, check, ratio, rounding_excess  # noqa: F401  (one set of budget functions)

C_ELT = 48.0
C_LO = 128.0
f64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------
# bilinear upsample and its adjoint
# ---------------------------------------------------------------------------------------------------------------
def taps(n_hi, s, device=None):
    """for every hi-res index d of an axis of n_hi = s n_lo: the two low-res indices and the weight of the second"""
    n_lo = n_hi // s
    d = torch.arange(n_hi, device=device)
    n = (2 * d + 1 - s).clamp_min(0)
    i0 = torch.div(n, 2 * s, rounding_mode='floor').clamp_max(n_lo - 1)
    i1 = (i0 + 1).clamp_max(n_lo - 1)
    w1 = (n % (2 * s)).to(f64) / (2 * s)
    return i0, i1, w1


def _up_last(x, s):
    i0, i1, w1 = taps(x.shape[-1] * s, s, x.device)
    return x[..., i0] * (1.0 - w1) + x[..., i1] * w1


def _up_last_t(g, s):
    i0, i1, w1 = taps(g.shape[-1], s, g.device)
    out = torch.zeros(g.shape[:-1] + (g.shape[-1] // s,), dtype=f64, device=g.device)
    out.index_add_(-1, i0, g * (1.0 - w1))
    out.index_add_(-1, i1, g * w1)
    return out


def _both_axes(f, x, s):
    return f(f(x.transpose(-1, -2), s).transpose(-1, -2), s)


def upsample(x, s):
    """(..., Hl, Wl) -> up, A: (..., s Hl, s Wl) fp64; s = 1: x itself"""
    xd = x.to(f64)
    if s == 1:
        return xd, xd.abs()
    return _both_axes(_up_last, xd, s), _both_axes(_up_last, xd.abs(), s)


def upsample_t(g, s):
    """the adjoint: (..., H, W) -> dxlo, A: (..., H / s, W / s) fp64"""
    gd = g.to(f64)
    if s == 1:
        return gd, gd.abs()
    return _both_axes(_up_last_t, gd, s), _both_axes(_up_last_t, gd.abs(), s)


# ---------------------------------------------------------------------------------------------------------------
# the tail passes; a, b (N, C, H, W), x (N, C, H / s, W / s), per-channel vectors (C,)
# ---------------------------------------------------------------------------------------------------------------
def _c(v):
    return v.to(f64).view(1, -1, 1, 1)


def tail_sum(a, b, x, s, shift):
    """t = a + b + shift + upsample(x) and A_t = the sum of the terms' absolute values"""
    t = a.to(f64)
    A = t.abs()
    if b is not None:
        t = t + b.to(f64)
        A = A + b.to(f64).abs()
    if shift is not None:
        t = t + _c(shift)
        A = A + _c(shift).abs()
    if x is not None:
        up, ua = upsample(x, s)
        t = t + up
        A = A + ua
    return t, A


def stats(t, At):
    """-> [sum t | sum t^2] (2C), A = [sum A_t | sum A_t^2]"""
    d = (0, 2, 3)
    return torch.cat([t.sum(d), (t * t).sum(d)]), torch.cat([At.sum(d), (At * At).sum(d)])


def affine(mean, rstd, gamma, beta):
    """the fp64 sc, sh of y = t sc + sh from the kernel's fp32 mean, rstd and the affine parameters, and beta"""
    mu, rs = mean.to(f64), rstd.to(f64)
    g = gamma.to(f64) if gamma is not None else torch.ones_like(mu)
    bt = beta.to(f64) if beta is not None else torch.zeros_like(mu)
    sc = rs * g
    return sc, bt - mu * sc, bt


def apply(t, At, mean, rstd, gamma, beta, relu):
    """y = [relu](t sc + sh), A = |sc| A_t + |beta| + |mean sc|, and the pre-activation with the ReLU-edge mask"""
    sc, sh, bt = affine(mean, rstd, gamma, beta)
    pre = t * _c(sc) + _c(sh)
    A = At * _c(sc).abs() + _c(bt).abs() + _c(mean.to(f64) * sc).abs()
    edge = pre.abs() <= RELU_EDGE * ((t * _c(sc)).abs() + _c(sh).abs()) if relu else torch.zeros_like(pre, dtype=torch.bool)
    return (pre.clamp_min(0.) if relu else pre), A, pre, edge


def _masked(dy, pre, relu):
    gd = dy.to(f64)
    return torch.where(pre > 0, gd, torch.zeros_like(gd)) if relu else gd


def bwd_stats(t, At, dy, mean, rstd, pre, edge, relu):
    """-> [sum dy' | sum dy' xhat] (2C) and A = [sum |dy'| | sum |dy'| (A_t + |mean|) rstd], both with the edge
    elements' |dy| and |dy xhat| added: xhat = (t - mean) rstd cancels, its error is that of t and mean"""
    d = (0, 2, 3)
    g = _masked(dy, pre, relu)
    mu, rs = _c(mean), _c(rstd)
    xh = (t - mu) * rs
    ge = torch.where(edge, dy.to(f64).abs(), torch.zeros_like(g))
    s = torch.cat([g.sum(d), (g * xh).sum(d)])
    xa = (At + mu.abs()) * rs
    A = torch.cat([(g.abs() + ge).sum(d), (g.abs() * xa + ge * xh.abs()).sum(d)])
    return s, A


def bwd_apply(t, At, dy, mean, rstd, gamma, pre, relu, mdy, mdyx):
    """dt = gamma rstd (dy' - mdy - xhat mdyx), A = |gamma rstd| (|dy'| + |mdy| + (A_t + |mean|) rstd |mdyx|)"""
    sc, _, _ = affine(mean, rstd, gamma, None)
    g = _masked(dy, pre, relu)
    mu, rs, m0, m1 = _c(mean), _c(rstd), _c(mdy), _c(mdyx)
    dt = _c(sc) * (g - m0 - (t - mu) * rs * m1)
    return dt, _c(sc).abs() * (g.abs() + m0.abs() + (At + mu.abs()) * rs * m1.abs())


# ---------------------------------------------------------------------------------------------------------------
# layouts (exact: index expressions only)
# ---------------------------------------------------------------------------------------------------------------
def interleave(U_, C, h, w):
    """U (B, 4 C, h w), rows (dy, dx, co) -> planes (B, C, 2h, 2w): planes[b][co][2y + dy][2x + dx] = U[b][(2 dy + dx) C + co][y w + x]"""
    B = U_.shape[0]
    out = U_.new_empty((B, C, 2 * h, 2 * w))
    for dy in range(2):
        for dx in range(2):
            out[:, :, dy::2, dx::2] = U_[:, (2 * dy + dx) * C:(2 * dy + dx + 1) * C].reshape(B, C, h, w)
    return out


def deinterleave(planes):
    """the inverse: planes (B, C, 2h, 2w) -> U (B, 4 C, h w)"""
    B, C, H2, W2 = planes.shape
    return torch.cat([planes[:, :, dy::2, dx::2].reshape(B, C, -1) for dy in range(2) for dx in range(2)], 1)


def tokens_to_planes(tokens, t0, T):
    """(B, T_total, C) -> (B, C, T): planes[b][c][t] = tokens[b][t0 + t][c]"""
    return tokens[:, t0:t0 + T].transpose(1, 2).contiguous()


def planes_to_tokens(planes, vec):
    """(B, C, T) -> the (B, T, C) fp32 token rows planes[b][c][t] + vec[c] (one fp32 addition, as the kernel's)"""
    rows = planes.float().transpose(1, 2)
    return (rows + vec.float()) if vec is not None else rows.contiguous()


def up_weight_rows(weight):
    """ConvTranspose2d weight (C, Co, 2, 2) -> Wcat (4 Co, C), rows (dy, dx, co)"""
    C, Co = weight.shape[:2]
    return weight.permute(2, 3, 1, 0).reshape(4 * Co, C)


def up_product(rows, wc):
    """U = Wcat rows^T per image on the bf16 operands: (B, T, C), (4 Co, C) -> U, A: (B, 4 Co, T) fp64"""
    r, w = rows.to(f64), wc.to(f64)
    return torch.matmul(w, r.transpose(1, 2)), torch.matmul(w.abs(), r.abs().transpose(1, 2))


# ---------------------------------------------------------------------------------------------------------------
# NCHW MaxPool2d(3, 2, 1): index statement
# ---------------------------------------------------------------------------------------------------------------
def maxpool_forward(x):
    """x (P, H, W) -> y (fp64, exact) and the window position 0..8 (3 ky + kx) of the first maximum in row-major
    order, -inf outside the image"""
    P, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.nn.functional.pad(x.to(f64), (1, 1, 1, 1), value=float('-inf'))
    win = torch.stack([xp[:, ky: ky + 2 * (OH - 1) + 1: 2, kx: kx + 2 * (OW - 1) + 1: 2] for ky in range(3) for kx in range(3)], 1)
    m = win.max(1).values
    pos = torch.arange(9, device=x.device).view(1, 9, 1, 1)
    idx = torch.where(win == m.unsqueeze(1), pos, 9).min(1).values.to(torch.uint8)
    return m, idx


def _pool_flat(idx, W):
    P, OH, OW = idx.shape
    k = idx.long()
    oy = torch.arange(OH, device=idx.device).view(1, OH, 1)
    ox = torch.arange(OW, device=idx.device).view(1, 1, OW)
    return ((2 * oy - 1 + k // 3) * W + (2 * ox - 1 + k % 3)).reshape(P, -1)


def maxpool_backward(gy, idx, H, W):
    """gx (P, H, W): every output gradient added, in fp64, to the input its window position names"""
    P = gy.shape[0]
    gx = torch.zeros((P, H * W), dtype=f64, device=gy.device)
    gx.scatter_add_(1, _pool_flat(idx, W), gy.to(f64).reshape(P, -1))
    return gx.view(P, H, W)


def maxpool_inexact(gy, idx, H, W):
    """pixels where an fp32 sum of the (at most four) bf16 gradients, in whatever order, need not be exact: the binary
    exponents of its non-zero terms lie more than 14 apart (8-bit significands, two carry bits: within 14 every
    partial sum fits 24 bits).  Computed from the reference alone; the kernel's last bf16 bit may differ only there."""
    P = gy.shape[0]
    g = gy.to(f64).reshape(P, -1)
    e = torch.frexp(g).exponent.to(f64)
    flat = _pool_flat(idx, W)
    hi = torch.full((P, H * W), -1e9, dtype=f64, device=gy.device)
    lo = torch.full((P, H * W), 1e9, dtype=f64, device=gy.device)
    hi.scatter_reduce_(1, flat, torch.where(g != 0, e, torch.full_like(e, -1e9)), 'amax')
    lo.scatter_reduce_(1, flat, torch.where(g != 0, e, torch.full_like(e, 1e9)), 'amin')
    return ((hi - lo > 14) & (hi > -1e8)).view(P, H, W)
