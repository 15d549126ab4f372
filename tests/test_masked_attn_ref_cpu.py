"""CPU: the fp64 reference of the masked cross-attention kernels (tests/masked_attn_ref.py) against
F.scaled_dot_product_attention with a bool mask and against autograd, in fp64 on small cases, and the torch expression of
vitadapter.fused.masked_cross_attention (what runs without the kernels) against the same reference."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import masked_attn_ref as mref
from oracle import attention as oa
from vitadapter import fused

SCALE = 1.0 / math.sqrt(32)


def _case(N, H, Lq, Lk, seed, special=True):
    q, k, v, do = mref.make_inputs(N, H, Lq, Lk, 'peaked', seed)
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn((N, Lq, Lk), generator=g)
    if special and Lq >= 3:
        x[0, 1] = -1.0 - x[0, 1].abs()                  # a row that keeps no key: keeps every key
        x[-1, 2] = -1.0 - x[-1, 2].abs()                # a row that keeps one key
        x[-1, 2, Lk // 2] = 0.5
    return q, k, v, do, x


def test_keep_rule_and_bits():
    x = torch.tensor([[[-1.0, -0.0, 0.0, float('nan'), float('inf'), float('-inf'), -1e-30, 1e-30],
                       [-1.0, -2.0, -3.0, -4.0, -5.0, -6.0, -7.0, float('-inf')]]])
    keep = mref.keep_rule(x)
    assert keep[0, 0].tolist() == [False, True, True, True, True, False, False, True]
    assert keep[0, 1].tolist() == [True] * 8
    assert mref.pack_bits(keep).tolist() == [[[0b10011110], [0xFF]]]
    keep = torch.zeros((1, 1, 70), dtype=torch.bool)
    keep[0, 0, [0, 31, 32, 69]] = True
    assert mref.pack_bits(keep).tolist() == [[[0x80000001, 0x1, 1 << 5]]]


@pytest.mark.parametrize('dims', [(1, 1, 1, 1), (2, 2, 5, 7), (1, 3, 9, 70), (2, 1, 33, 65)])
def test_reference_against_sdpa_and_autograd(dims):
    N, H, Lq, Lk = dims
    q, k, v, do, x = _case(N, H, Lq, Lk, 3)
    keep = mref.keep_rule(x)
    if Lq >= 3:
        assert bool(keep[0, 1].all()) and int(keep[-1, 2].sum()) == 1
    qh, kh, vh, gh = (mref.heads(t.double(), H).clone().requires_grad_(True) for t in (q, k, v, do))
    ref = mref.reference(qh.detach(), kh.detach(), vh.detach(), gh.detach(), keep, SCALE)
    o = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=keep[:, None], scale=SCALE)
    dq, dk, dv = torch.autograd.grad((o * gh.detach()).sum(), (qh, kh, vh))
    for name, got in (('o', o.detach()), ('dq', dq), ('dk', dk), ('dv', dv)):
        assert float((got - ref[name]).abs().max()) <= 1e-12 * max(1.0, float(ref[name].abs().max())), name
    s = (SCALE * qh.detach() @ kh.detach().transpose(2, 3)).masked_fill(~keep[:, None], float('-inf'))
    assert float((torch.logsumexp(s, -1) * mref.LOG2E - ref['lse']).abs().max()) <= 1e-12
    # the single kept key: that row's output is its v row
    if Lq >= 3:
        assert float((ref['o'][-1, :, 2] - vh.detach()[-1, :, Lk // 2]).abs().max()) <= 1e-14
    # the budget sums: p sums to one over the kept keys, and the column sums cover kept keys only
    for name in ('o', 'dq', 'dk', 'dv', 'lse'):
        b = oa.budget(ref, name, torch.bfloat16)
        assert b.shape == ref[name].shape and bool((b > 0).all()), name
    assert float((ref['s_o'] - keep[:, None].double() @ vh.detach().abs()).abs().max()) == 0.0


def test_rows_and_heads_are_inverse():
    q, _, _, _ = mref.make_inputs(2, 3, 5, 7, 'flat', 0)
    assert torch.equal(mref.rows(mref.heads(q, 3)), q)


@pytest.mark.parametrize('dims', [(2, 2, 5, 7), (1, 3, 9, 70)])
def test_torch_expression_of_the_glue(dims):
    """fused.masked_cross_attention on the CPU (no kernels): fp64 values and gradients equal the reference."""
    N, H, Lq, Lk = dims
    q, k, v, do, x = _case(N, H, Lq, Lk, 5)
    keep = mref.keep_rule(x)
    ref = mref.reference(*(mref.heads(t, H) for t in (q, k, v, do)), keep, SCALE)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    xr = x.clone().requires_grad_(True)
    out = fused.masked_cross_attention(qd, kd, vd, xr, H)
    assert out.shape == (Lq, N, H * 32)
    dq, dk, dv = torch.autograd.grad((out * do.double()).sum(), (qd, kd, vd))
    assert xr.grad is None
    for name, got in (('o', out.detach()), ('dq', dq), ('dk', dk), ('dv', dv)):
        want = mref.rows(ref[name])
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name


def test_the_switch_exists_and_is_on():
    assert fused.ENABLED['masked_attn'] is True
    assert np.dtype(np.int64) == mref.pack_bits(torch.ones((1, 1, 1), dtype=torch.bool)).dtype
