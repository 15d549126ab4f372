"""fp64 reference of the masked cross-attention kernels (csrc/masked_attn.hip, include/vitadapter_hip_masked_attn.h): the
pack rule, and forward and backward of softmax(scale q k^T + (-inf where excluded)) v for Lq != Lk at head dim 32.

`reference` returns the dict oracle.attention.budget consumes (o, dq, dk, dv, lse, a_*, s_*), so the kernels are held to
the budgets of oracle/attention.py unchanged: the numerics contract is the same (scores, max, sum, lse, delta and every
accumulator fp32; P and dS rounded to T once each; every output once).  The a_* sums run over the kept keys only - an
excluded key has p = 0 exactly - and so do the s_* column sums of the underflow term: an excluded key contributes exactly 0,
so it gets no allowance.

tests/test_masked_attn_ref_cpu.py holds this file to F.scaled_dot_product_attention with a bool mask and to autograd."""
import numpy as np
import torch

LOG2E = 1.4426950408889634
HD = 32


def keep_rule(x):
    """(N, Q, Lk) logits -> bool keep mask: a key is kept iff not (x < 0) (so -0.0, +0.0 and NaN are kept); a row that keeps
    no key keeps every key."""
    keep = ~(x < 0)
    return keep | ~keep.any(-1, keepdim=True)


def pack_bits(keep):
    """bool (N, Q, Lk) -> int64 array (N, Q, ceil(Lk / 32)) of the 32-bit words as unsigned values: bit (j & 31) of word
    (j >> 5) is key j; bits at positions >= Lk are 0."""
    k = keep.cpu().numpy().astype(np.uint64)
    N, Q, Lk = k.shape
    W = (Lk + 31) // 32
    padded = np.zeros((N, Q, W * 32), dtype=np.uint64)
    padded[:, :, :Lk] = k
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (padded.reshape(N, Q, W, 32) * weights).sum(-1).astype(np.int64)


def words_of(bits):
    """int32 tensor of words (as the library writes them) -> int64 array of unsigned values"""
    return bits.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def make_inputs(N, H, Lq, Lk, regime, seed):
    """fp32 q, dout (Lq, N, H * 32) and k, v (Lk, N, H * 32) of an input regime in the sense of
    oracle.attention.make_inputs, restated for 32 channels and separate query / key lengths:
    'peaked': q, k, v ~ 1.5 N(0, 1): a dropped tile or row shows up far outside the budget;
    'flat':   q, k ~ 0.25 N(0, 1), v = 1 + 0.5 N(0, 1): every kept key carries about the same mass and every output is
              about 1, so an extra or missing key or a wrong normaliser moves every output."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((Lq, N, H * HD), generator=g)
    k = torch.randn((Lk, N, H * HD), generator=g)
    v = torch.randn((Lk, N, H * HD), generator=g)
    dout = torch.randn((Lq, N, H * HD), generator=g)
    if regime == 'peaked':
        q, k, v = 1.5 * q, 1.5 * k, 1.5 * v
    elif regime == 'flat':
        q, k, v = 0.25 * q, 0.25 * k, 1.0 + 0.5 * v
    else:
        raise ValueError(regime)
    return q, k, v, dout


def heads(t, H):
    """(L, N, H * 32) -> (N, H, L, 32)"""
    L, N, _ = t.shape
    return t.reshape(L, N, H, HD).permute(1, 2, 0, 3)


def rows(t):
    """(N, H, L, 32) -> (L, N, H * 32)"""
    N, H, L, _ = t.shape
    return t.permute(2, 0, 1, 3).reshape(L, N, H * HD)


def reference(q, k, v, do, keep, scale):
    """fp64 forward and backward.  q, do: (N, H, Lq, 32), k, v: (N, H, Lk, 32) - the exact operands, any float dtype -
    and keep: bool (N, Lq, Lk) with at least one kept key per row.  Returns fp64 tensors: o, dq (N, H, Lq, 32), dk, dv
    (N, H, Lk, 32), lse (N, H, Lq) in the log2 domain, and the sums of the budgets of oracle/attention.py:
    a_o = P|v|, a_dv = P^T|dO|, a_dq = scale W|k|, a_dk = scale W^T|q| with W = |dS| + P D,
    D_i = sum_d |dO_id| (|o_id| + sum_j p_ij |v_jd|); s_o, s_dv, s_dq, s_dk: the sums of |v|, |dO|, scale |k|, scale |q| over
    the keys (queries) that take part in the element."""
    f64 = torch.float64
    q, k, v, do = (t.to(f64) for t in (q, k, v, do))
    km = keep[:, None].to(q.device)
    kf = km.to(f64)
    s = scale * (q @ k.transpose(2, 3))
    s = s.masked_fill(~km, float('-inf'))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    out = {'lse': lse * LOG2E}
    out['o'] = p @ v
    out['a_o'] = p @ v.abs()
    out['dv'] = p.transpose(2, 3) @ do
    out['a_dv'] = p.transpose(2, 3) @ do.abs()
    delta = (do * out['o']).sum(-1, keepdim=True)
    dabs = (do.abs() * (out['o'].abs() + out['a_o'])).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(2, 3) - delta)
    w = ds.abs() + p * dabs
    out['dq'] = scale * (ds @ k)
    out['dk'] = scale * (ds.transpose(2, 3) @ q)
    out['a_dq'] = scale * (w @ k.abs())
    out['a_dk'] = scale * (w.transpose(2, 3) @ q.abs())
    out['s_o'] = kf @ v.abs()
    out['s_dv'] = kf.transpose(2, 3) @ do.abs()
    out['s_dq'] = scale * (kf @ k.abs())
    out['s_dk'] = scale * (kf.transpose(2, 3) @ q.abs())
    return out
