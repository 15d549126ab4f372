"""fp64 reference of the SpatialPriorModule kernels on NHWC bf16 (csrc/conv.hip, csrc/spm_nhwc.hip, and
bn_finalize_kernel of csrc/tail_ops.hip) and the per-element budgets they are held to (tests/test_spm_fp64_gpu.py,
DESIGN 4.4b).

Every reference starts from the exact operands the kernel saw: bf16 activations upcast, bf16 weights in the kernel's
own layouts (conv.forward_weight: (Cout, 9, Cin); conv.dgrad_weight: (Cin, 9, Cout)), and for the BatchNorm passes
the kernel's own fp32 mean / rstd / means.  The convolutions are written as tap decompositions, so that they rely
neither on MIOpen nor on torch's fp64 convolution: the input is padded by 1, and tap t = (dy, dx) (t = 3 dy + dx, the
weight's (ky, kx)) is one strided slice of it and one fp64 GEMM:

    forward   out     = sum_t X_t W_t^T            X_t = xpad[dy :: S, dx :: S] (OH x OW pixels)
    dgrad     dXpad[dy :: S, dx :: S] += dY W_t     then cropped to [1 : H + 1, 1 : W + 1]
    wgrad     dW_t    = dY^T X_t

Each returns A, the same computation on absolute values: the sum of |terms| behind every element.  Evaluated on the
operands' device one image at a time: at the production sizes of BASELINE no call holds more than about 0.6 GB of
fp64.

Budget (as in tests/test_reductions_fullsize_gpu.py):

    |got - ref| <= C_ACC * 2^-24 * A   (+ 2^-8 |ref| where the output is bf16)

2^-8 |ref| is the round-to-nearest bound of bf16 for the one rounding of each bf16 output.  C_ACC = 256 bounds the
longest dependent chain of fp32 operations behind an element (an fp32 sum whose longest chain is d additions long is
off by at most d * 2^-24 * A):
  * conv_taps_kernel: one accumulator per element walks 9 taps x Cin / 16 MFMA steps - 9 at Cin 16, 144 at Cin 256;
  * conv_wgrad_kernel: a workgroup adds its tiles in registers, WY * 32 / 16 MFMA steps of 16 pixels per tile:
    32 tiles x 4 steps at the configs[2] stem (8 192 tiles on 256 slots), 16 x 8 for its 64 -> 64 convs; then
    conv_wgrad_reduce: slots / 16 per chain (16 at 256 slots) + 2 + 2: about 150 in all;
  * bn_nhwc_stats: a thread walks rows / (parts * 256 / (C / 8)) rows (at most 32 at the 512-part cap and C 64),
    the row lanes of a workgroup (at most 32) are added in order, bn_nhwc_sum_parts adds 16 per chain + 2 + 8:
    about 90, each term formed by at most 3 roundings (g (x - mean) rstd).
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
C_ACC = 256.0
BF16_U = 2.0 ** -8
RELU_EDGE = 2.0 ** -20
f64 = torch.float64


def _out_hw(H, W, S):
    return (H - 1) // S + 1, (W - 1) // S + 1


def _tap(xp, t, S, OH, OW):
    """tap t of a padded image (H + 2, W + 2, C): the (OH, OW) pixels that meet weight position (t // 3, t % 3)"""
    dy, dx = divmod(t, 3)
    return xp[dy: dy + S * (OH - 1) + 1: S, dx: dx + S * (OW - 1) + 1: S]


def conv_forward(x, w9, S):
    """x (N, H, W, Cin) bf16, w9 (Cout, 9, Cin) -> out, A: (N, OH, OW, Cout) fp64"""
    N, H, W, Cin = x.shape
    Cout = w9.shape[0]
    OH, OW = _out_hw(H, W, S)
    wd = w9.to(f64)
    wa = wd.abs()
    out = torch.empty((N, OH, OW, Cout), dtype=f64, device=x.device)
    A = torch.empty_like(out)
    for n in range(N):
        xp = F.pad(x[n].to(f64), (0, 0, 1, 1, 1, 1))
        o = torch.zeros((OH * OW, Cout), dtype=f64, device=x.device)
        a = torch.zeros_like(o)
        for t in range(9):
            xt = _tap(xp, t, S, OH, OW).reshape(-1, Cin)
            o += xt @ wd[:, t].T
            a += xt.abs() @ wa[:, t].T
        out[n], A[n] = o.view(OH, OW, Cout), a.view(OH, OW, Cout)
    return out, A


def conv_input_grad(gy, wt9, S, H, W):
    """gy (N, OH, OW, Cout) bf16, wt9 (Cin, 9, Cout) -> dX, A: (N, H, W, Cin) fp64"""
    N, OH, OW, Cout = gy.shape
    Cin = wt9.shape[0]
    assert (OH, OW) == _out_hw(H, W, S)
    wd = wt9.to(f64)
    wa = wd.abs()
    out = torch.empty((N, H, W, Cin), dtype=f64, device=gy.device)
    A = torch.empty_like(out)
    for n in range(N):
        g = gy[n].to(f64).reshape(-1, Cout)
        ga = g.abs()
        dxp = torch.zeros((H + 2, W + 2, Cin), dtype=f64, device=gy.device)
        dap = torch.zeros_like(dxp)
        for t in range(9):
            _tap(dxp, t, S, OH, OW).add_((g @ wd[:, t].T).view(OH, OW, Cin))
            _tap(dap, t, S, OH, OW).add_((ga @ wa[:, t].T).view(OH, OW, Cin))
        out[n], A[n] = dxp[1:H + 1, 1:W + 1], dap[1:H + 1, 1:W + 1]
    return out, A


def conv_weight_grad(x, gy, S):
    """x (N, H, W, Cin), gy (N, OH, OW, Cout) bf16 -> dW, A: (Cout, 9, Cin) fp64 (the kernel's (Cout, 3, 3, Cin))"""
    N, H, W, Cin = x.shape
    _, OH, OW, Cout = gy.shape
    assert (OH, OW) == _out_hw(H, W, S)
    dw = torch.zeros((Cout, 9, Cin), dtype=f64, device=x.device)
    A = torch.zeros_like(dw)
    for n in range(N):
        xp = F.pad(x[n].to(f64), (0, 0, 1, 1, 1, 1))
        g = gy[n].to(f64).reshape(-1, Cout)
        ga = g.abs()
        for t in range(9):
            xt = _tap(xp, t, S, OH, OW).reshape(-1, Cin)
            dw[:, t] += g.T @ xt
            A[:, t] += ga.T @ xt.abs()
    return dw, A


def bn_stats(x):
    """x (rows, C) bf16 -> [sum x | sum x^2] (2C) fp64 and A = [sum |x| | sum x^2]"""
    xd = x.to(f64)
    s, q = xd.sum(0), (xd * xd).sum(0)
    return torch.cat([s, q]), torch.cat([xd.abs().sum(0), q])


def affine(mean, rstd, w, b):
    """the fp64 scale / shift of y = x sc + sh from the kernel's fp32 mean, rstd and the affine parameters"""
    mu, rs = mean.to(f64), rstd.to(f64)
    wd = w.to(f64) if w is not None else torch.ones_like(mu)
    bd = b.to(f64) if b is not None else torch.zeros_like(mu)
    sc = rs * wd
    return sc, bd - mu * sc, bd


def bn_apply(x, mean, rstd, w, b, relu):
    """y = relu?(x sc + sh) and A = |x sc| + |b| + |mean sc| (the terms of w rstd x + b - mean rstd w)"""
    xd = x.to(f64)
    sc, sh, bd = affine(mean, rstd, w, b)
    t = xd * sc + sh
    return (t.clamp_min(0.) if relu else t), (xd * sc).abs() + bd.abs() + (mean.to(f64) * sc).abs()


def relu_edge(x, mean, rstd, w, b):
    """elements whose fp64 pre-activation lies within 2^-20 (|x sc| + |sh|) of zero: the fp32 ReLU mask of the
    backward may go either way there"""
    xd = x.to(f64)
    sc, sh, _ = affine(mean, rstd, w, b)
    return (xd * sc + sh).abs() <= RELU_EDGE * ((xd * sc).abs() + sh.abs())


def bn_bwd_stats(x, dy, mean, rstd, w, b, relu):
    """-> [sum g' | sum g' xhat] (2C), A = [sum |g'| | sum |g' xhat|] and the ReLU-edge mask; g' = dy where the
    pre-activation is positive (all of dy without relu), xhat = (x - mean) rstd.  A flip of an edge element moves the
    sums by |dy| (1 + |xhat|): that is added to A."""
    xd, gd = x.to(f64), dy.to(f64)
    sc, sh, _ = affine(mean, rstd, w, b)
    xh = (xd - mean.to(f64)) * rstd.to(f64)
    if relu:
        g = torch.where(xd * sc + sh > 0, gd, torch.zeros_like(gd))
        edge = relu_edge(x, mean, rstd, w, b)
    else:
        g, edge = gd, torch.zeros_like(xd, dtype=torch.bool)
    ge = torch.where(edge, gd.abs(), torch.zeros_like(gd))
    s = torch.cat([g.sum(0), (g * xh).sum(0)])
    A = torch.cat([g.abs().sum(0) + ge.sum(0), (g * xh).abs().sum(0) + (ge * xh.abs()).sum(0)])
    return s, A, edge


def bn_bwd_apply(x, dy, mean, rstd, w, b, relu, mean_g, mean_gx):
    """dx = w rstd (g' - mean_g - xhat mean_gx) from the kernel's mean, rstd, mean_g, mean_gx;
    A = |sc| (|g'| + |mean_g| + (|x| + |mean|) rstd |mean_gx|)"""
    xd, gd = x.to(f64), dy.to(f64)
    mu, rs = mean.to(f64), rstd.to(f64)
    sc, sh, _ = affine(mean, rstd, w, b)
    g = torch.where(xd * sc + sh > 0, gd, torch.zeros_like(gd)) if relu else gd
    m0, m1 = mean_g.to(f64), mean_gx.to(f64)
    dx = sc * (g - m0 - (xd - mu) * rs * m1)
    return dx, sc.abs() * (g.abs() + m0.abs() + (xd.abs() + mu.abs()) * rs * m1.abs())


def finalize_stats(sums, C, eps, momentum, running_mean=None, running_var=None):
    """bn_finalize_kernel in fp64 from the kernel's fp32 sums [sum | sum of squares | count]: mean, rstd (biased
    variance) and the updated running statistics (unbiased variance), each with its budget.  var = E[x^2] - mean^2
    loses the leading bits of E[x^2] and mean^2: its error scales with E[x^2] + mean^2, not with var."""
    eps, momentum = (float(torch.tensor(v, dtype=torch.float32)) for v in (eps, momentum))     # as the kernel gets them
    s = sums.to(f64)
    cnt = s[2 * C]
    mu = s[:C] / cnt
    ex2 = s[C:2 * C] / cnt
    var = (ex2 - mu * mu).clamp_min(0.)
    rs = 1.0 / torch.sqrt(var + eps)
    cond = (ex2 + mu * mu) / (var + eps)
    out = {'mean': (mu, mu.abs()), 'rstd': (rs, rs * (1.0 + cond))}
    if running_mean is not None:
        m = momentum
        unb = cnt / max(float(cnt) - 1.0, 1.0)
        rm, rv = running_mean.to(f64), running_var.to(f64)
        out['running_mean'] = ((1 - m) * rm + m * mu, (1 - m) * rm.abs() + m * mu.abs())
        out['running_var'] = ((1 - m) * rv + m * var * unb, (1 - m) * rv.abs() + m * unb * (var + ex2 + mu * mu))
    return out


def _pool_windows(x):
    """one image (H, W, C) -> fp64 windows (OH, OW, 9, C) of MaxPool2d(3, 2, 1), -inf outside"""
    H, W, C = x.shape
    xp = F.pad(x.to(f64), (0, 0, 1, 1, 1, 1), value=float('-inf'))
    OH, OW = _out_hw(H, W, 2)
    return torch.stack([_tap(xp, t, 2, OH, OW) for t in range(9)], 2)


def maxpool_forward(x):
    """MaxPool2d(3, 2, 1) on (N, H, W, C): y (fp64, exact) and the window position 0..8 (3 ky + kx) of the first
    maximum in scan order, as uint8; one image at a time"""
    N, H, W, C = x.shape
    OH, OW = _out_hw(H, W, 2)
    y = torch.empty((N, OH, OW, C), dtype=f64, device=x.device)
    idx = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=x.device)
    for n in range(N):
        win = _pool_windows(x[n])
        m = win.max(2).values
        y[n] = m
        # first position equal to the maximum (argmax does not promise the first one on every device)
        pos = torch.arange(9, device=x.device).view(1, 1, 9, 1)
        idx[n] = torch.where(win == m.unsqueeze(2), pos, 9).min(2).values.to(torch.uint8)
    return y, idx


def pool_flat_index(idx, H, W):
    """window positions (N, OH, OW, C) -> flat input index iy * W + ix, what max_pool2d(return_indices=True) gives"""
    N, OH, OW, C = idx.shape
    k = idx.long()
    oy = torch.arange(OH, device=idx.device).view(1, OH, 1, 1)
    ox = torch.arange(OW, device=idx.device).view(1, 1, OW, 1)
    return (2 * oy - 1 + k // 3) * W + (2 * ox - 1 + k % 3)


def maxpool_backward(gy, idx, H, W):
    """gx (N, H, W, C) fp64: every output gradient added to the input its window position names; A = the same on |gy|
    (at most 4 terms per element)"""
    N, OH, OW, C = gy.shape
    flat = pool_flat_index(idx, H, W)
    gx = torch.zeros((N, H * W, C), dtype=f64, device=gy.device)
    A = torch.zeros_like(gx)
    g = gy.to(f64).reshape(N, OH * OW, C)
    fl = flat.reshape(N, OH * OW, C)
    gx.scatter_add_(1, fl, g)
    A.scatter_add_(1, fl, g.abs())
    return gx.view(N, H, W, C), A.view(N, H, W, C)


def image_to_nhwc16(x):
    """(N, 3, H, W) fp32 -> (N, H, W, 16) bf16, channels 3..15 zero"""
    N, _, H, W = x.shape
    y = torch.zeros((N, H, W, 16), dtype=torch.bfloat16, device=x.device)
    y[..., :3] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    return y


def bound(ref, A, bf16=False, c_acc=C_ACC):
    b = c_acc * U * A.to(f64)
    return b + BF16_U * ref.to(f64).abs() if bf16 else b


def ratio(got, ref, A, bf16=False, mask=None, c_acc=C_ACC):
    """worst |got - ref| / budget (inf for a NaN or an error where the budget is 0); mask: elements to check"""
    err = (got.to(f64) - ref.to(f64)).abs()
    b = bound(ref, A, bf16, c_acc)
    if mask is not None:
        err, b = err[mask], b[mask]
    if err.numel() == 0:
        return 0.0
    r = torch.where(err == 0, torch.zeros_like(err), err / b)
    return float(r.nan_to_num(float('inf')).max())


def rounding_excess(got, ref, A, mask=None, c_acc=C_ACC):
    """for a bf16 output: the worst part of |got - ref| beyond half a bf16 ulp of ref (the output's own rounding), over
    the accumulation budget C_ACC 2^-24 A: what the fp32 arithmetic behind the element used of its budget"""
    r = ref.to(f64)
    e = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -126)))
    ex = ((got.to(f64) - r).abs() - torch.exp2(e - 8)).clamp_min(0.)
    b = c_acc * U * A.to(f64)
    if mask is not None:
        ex, b = ex[mask], b[mask]
    if ex.numel() == 0:
        return 0.0
    return float(torch.where(ex == 0, torch.zeros_like(ex), ex / b).nan_to_num(float('inf')).max())


def check(what, got, ref, A, bf16=False, mask=None, c_acc=C_ACC):
    """assert every element within its budget; returns the worst ratio"""
    r = ratio(got, ref, A, bf16, mask, c_acc)
    if not r <= 1.0:
        err = (got.to(f64) - ref.to(f64)).abs()
        b = bound(ref, A, bf16, c_acc)
        bad = ~(err <= b)
        if mask is not None:
            bad &= mask
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError('%s: %d of %d elements over budget; first at %s (flat %d): got %r ref %r budget %.3e '
                             '(worst err / budget %.3g)' % (what, int(bad.sum()), bad.numel(),
                                                            tuple(int(v) for v in torch.unravel_index(torch.tensor(i), bad.shape)),
                                                            i, got.reshape(-1)[i].item(), ref.reshape(-1)[i].item(),
                                                            b.reshape(-1)[i].item(), r))
    return r
