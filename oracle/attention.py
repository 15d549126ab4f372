"""fp64 reference of the MFMA attention kernels (csrc/attn_flash.hip, attn_win.hip, attn_fwd.hip, attn_bwd.hip,
relpos.hip) and the per-element error budgets they are held to (tests/test_attention_fp64_gpu.py).

The reference starts from the exact operands a kernel saw: q, k, v and dO upcast from bf16 / fp16, and for the bias
paths the 16-bit ``bias * log2(e)`` operand divided back by log2(e).  It is evaluated in fp64 on the operands' device
(the GPU in the GPU tests), one head and a chunk of sequences at a time, so that no call holds more than about 1 GB of
fp64 however large N is.

Budgets.  u_T = 2^-8 (bf16) or 2^-11 (fp16), the round-to-nearest bounds of the two types.  The kernels' numerics
contract: scores, max, sum, lse, delta and every accumulator are fp32; only P and dS are rounded to T
(once each), and every output once more.  So an output is off by at most u_T relative per rounded operand of its sum,
plus its own rounding:

    o[i,d]   : C u_T sum_j p_ij |v_jd|                                 + u_T |o_ref|
    dv[j,d]  : C u_T sum_i p_ij |dO_id|                                + u_T |dv_ref|
    dq[i,d]  : C u_T scale sum_j (|dS_ij| + p_ij D_i) |k_jd|           + u_T |dq_ref|
    dk[j,d]  : C u_T scale sum_i (|dS_ij| + p_ij D_i) |q_id|           + u_T |dk_ref|
    dbias    : C u_T sum_b (|dS_bij| + p_bij D_bi)        (dtable: the same, summed over the index class)
    lse[i]   : 2 u_T + 2^-20 |lse_ref|
    with D_i = sum_d |dO_id| (|o_id| + sum_j p_ij |v_jd|)

D_i bounds the error of delta = rowsum(dO o O), which the kernels form from their T-rounded output.  C = 2: the
normaliser l of the whole-sequence kernels sums the same T-rounded P as the product (one u_T each for numerator and
denominator), the window kernels sum P in fp32.  No fp32-accumulation term: an fp32 sum of at most 4 200 terms is off
by 4 200 * 2^-24 = 2^-12 relative to the sum of its |terms| in the worst case and by far less in practice, and the
measured ratios below leave that room.

One term is added per rounded operand and per output: ETA, the absolute error of a rounding below the normal range
(fp16 P and dS underflow to subnormals, and fp32 values below 2^-126 may be flushed).  Measurement needed it.  Under
the 'late' regime, early keys carry p ~ 2^-60; their dS has no relative accuracy, and dK of those keys is all
underflow.  The term is C ETA times the column sum of the other operand (sum_j |v_jd| for o, and so on), plus ETA for
the output.  It is far below u_T of any output that is not itself near underflow.

Every tensor gets two checks: (a) every element within its budget, (b) ||got - ref||_2 <= 0.5 ||budget||_2, which
catches small systematic errors (an extra key, a wrong normaliser) that stay under the per-element bound.

Worst measured ratios on an MI355X ((a) max err / budget, (b) ||err|| / ||budget||, all 147 cases):
    whole sequence  bf16 0.47 / 0.16   fp16 0.46 / 0.15
    resident window bf16 0.55 / 0.15   fp16 0.92 / 0.15 (dQ of a 14 x 27 grid in 13 x 13 windows: mostly padding)
    general window  bf16 0.58 / 0.15   fp16 0.54 / 0.15
    bias            bf16 0.48 / 0.16   fp16 0.50 / 0.16
    relpos          bf16 0.47 / 0.15   fp16 0.49 / 0.15   (dtable per element: bf16 0.11, fp16 0.33)
"""
import math

import torch

LOG2E = 1.4426950408889634
C = 2.0
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# absolute error of one rounding below the normal range: fp16 keeps subnormals (half the smallest, 2^-25); bf16 has fp32's
# exponent range, and the GPU flushes fp32 subnormals (exp2, conversions), so a value below 2^-126 may become 0
ETA = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25}
L2_FRACTION = 0.5
CHUNK_ELEMS = 1 << 24          # (sequences x N x N) elements per fp64 score-sized matrix of one step: 128 MB


def make_inputs(B, N, H, regime, seed, scale=0.125):
    """fp32 packed projection qkv (B, N, 3, H, 64) and output gradient (B, N, H, 64) of an input regime:
    'peaked': q, k, v ~ 1.5 N(0, 1) (a dropped tile or row shows up far outside the budget);
    'flat':   q, k ~ 0.25 N(0, 1), v = 1 + 0.5 N(0, 1): every key carries about 1/N of the mass and every output is about
              1, so an extra or missing key or a wrong normaliser moves every output;
    'late':   'peaked' at 1/3 the size plus a ramp along d = 0 of k (q_0 = 4): the row maximum rises by 2 units of log2
              every 64 keys, so the online softmax rescales in every key tile."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((B, N, 3, H, 64), generator=g)
    dout = torch.randn((B, N, H, 64), generator=g)
    if regime == 'peaked':
        qkv *= 1.5
    elif regime == 'flat':
        qkv[:, :, :2] *= 0.25
        qkv[:, :, 2] = 1.0 + 0.5 * qkv[:, :, 2]
    elif regime == 'late':
        qkv *= 0.5
        qkv[:, :, 0, :, 0] = 4.0
        qkv[:, :, 1, :, 0] = torch.arange(N, dtype=torch.float32)[None, :, None] * (2.0 / (64 * 4.0 * scale * LOG2E))
    else:
        raise ValueError(regime)
    return qkv, dout


def reference(q, k, v, do, scale, bias=None):
    """fp64 forward and backward of softmax(scale q k^T + bias) v.

    q, k, v, do: (Z, H, N, 64), the exact operands (any float dtype; upcast here).  bias: (H, N, N) in natural-log
    units, shared by the Z sequences, or None.  Returns fp64 tensors: o, lse (log2 domain, (Z, H, N)), dq, dk, dv, and
    the absolute-value sums of the budgets: a_o = P|v|, a_dv = P^T|dO|, a_dq = scale W|k|, a_dk = scale W^T|q| with
    W = |dS| + P D; with a bias also dbias = sum_Z dS and a_dbias = sum_Z W, each (H, N, N)."""
    Z, H, N, hd = q.shape
    f64 = torch.float64
    out = {n: torch.empty((Z, H, N, hd), dtype=f64, device=q.device) for n in ('o', 'dq', 'dk', 'dv', 'a_o', 'a_dv', 'a_dq', 'a_dk')}
    out['lse'] = torch.empty((Z, H, N), dtype=f64, device=q.device)
    # column sums of |v|, |dO|, |k|, |q| per sequence: what one underflowed P or dS element per term can move
    for n, t in (('s_o', v), ('s_dv', do), ('s_dq', k), ('s_dk', q)):
        out[n] = t.to(f64).abs().sum(2, keepdim=True) * (scale if n in ('s_dq', 's_dk') else 1.0)
    if bias is not None:
        out['dbias'] = torch.zeros((H, N, N), dtype=f64, device=q.device)
        out['a_dbias'] = torch.zeros((H, N, N), dtype=f64, device=q.device)
        out['n_seq'] = Z
    zc = max(1, CHUNK_ELEMS // (N * N))
    for h in range(H):
        bh = bias[h].to(f64) if bias is not None else None
        for z0 in range(0, Z, zc):
            sl = slice(z0, min(Z, z0 + zc))
            qh, kh, vh, gh = (t[sl, h].to(f64) for t in (q, k, v, do))
            s = scale * (qh @ kh.transpose(1, 2))
            if bh is not None:
                s += bh
            lse = torch.logsumexp(s, -1)
            p = torch.exp(s - lse[..., None])
            del s
            o = p @ vh
            a_o = p @ vh.abs()
            out['o'][sl, h], out['a_o'][sl, h] = o, a_o
            out['lse'][sl, h] = lse * LOG2E
            out['dv'][sl, h] = p.transpose(1, 2) @ gh
            out['a_dv'][sl, h] = p.transpose(1, 2) @ gh.abs()
            delta = (gh * o).sum(-1, keepdim=True)
            dabs = (gh.abs() * (o.abs() + a_o)).sum(-1, keepdim=True)
            ds = gh @ vh.transpose(1, 2)
            ds -= delta
            ds *= p
            w = p * dabs
            w += ds.abs()
            del p
            out['dq'][sl, h] = scale * (ds @ kh)
            out['dk'][sl, h] = scale * (ds.transpose(1, 2) @ qh)
            out['a_dq'][sl, h] = scale * (w @ kh.abs())
            out['a_dk'][sl, h] = scale * (w.transpose(1, 2) @ qh.abs())
            if bh is not None:
                out['dbias'][h] += ds.sum(0)
                out['a_dbias'][h] += w.sum(0)
            del ds, w
    return out


def budget(ref, name, dtype):
    """Per-element budget of output `name` ('o', 'dq', 'dk', 'dv', 'lse', 'dbias') of a kernel with 16-bit type `dtype`."""
    u, eta = UNIT[dtype], ETA[dtype]
    if name == 'lse':
        return 2 * u + 2.0 ** -20 * ref['lse'].abs()
    if name == 'dbias':
        return C * (u * ref['a_dbias'] + eta * ref['n_seq'])
    return C * (u * ref['a_' + name] + eta * ref['s_' + name]) + u * ref[name].abs() + eta


def scatter_table(x, index, T):
    """(H, N, N) -> (T, H): the sum of x[h, i, j] over the (i, j) with index[i, j] = t (relpos table gradient)."""
    H = x.shape[0]
    out = torch.zeros((H, T), dtype=x.dtype, device=x.device)
    out.index_add_(1, index.reshape(-1).to(x.device), x.reshape(H, -1))
    return out.t().contiguous()


def ratios(got, ref, bud):
    """(max |got - ref| / budget, ||got - ref||_2 / ||budget||_2); NaN anywhere gives inf."""
    err = (got.double() - ref).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf, math.inf
    worst = (err / bud.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    bn = bud.norm().item()
    return worst, (err.norm().item() / bn if bn > 0 else (0.0 if err.norm().item() == 0 else math.inf))


def check(what, got, ref, bud):
    """Raises unless (a) every element of `got` is within its budget and (b) ||got - ref|| <= 0.5 ||budget||; returns the two
    ratios of `ratios` (for the record of the worst case)."""
    a, b = ratios(got, ref, bud)
    if not (a <= 1.0 and b <= L2_FRACTION):
        err = (got.double() - ref).abs()
        over = ~(err <= bud)
        msg = '%s: max err / budget %.3g, ||err|| / ||budget|| %.3g (limit %.2f); %d of %d elements over budget' % (
            what, a, b, L2_FRACTION, int(over.sum()), got.numel())
        if bool(over.any()):
            i = int(torch.nonzero(over.reshape(-1))[0])
            msg += '; first at flat %d: got %r ref %r budget %.3e' % (
                i, got.reshape(-1)[i].item(), ref.reshape(-1)[i].item(), bud.reshape(-1)[i].item())
        raise AssertionError(msg)
    return a, b
