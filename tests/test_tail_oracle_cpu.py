"""CPU: oracle/tail.py (the fp64 statement tests/test_tail_fp64_gpu.py holds csrc/tail_ops.hip to) against torch's own
fp64 F.interpolate + BatchNorm2d autograd (+ F.relu), F.conv_transpose2d, max_pool2d and the slice / transpose / cat
lines of the pyramid assembly, on small odd shapes; and the budget functions return A >= |ref| elementwise."""
import pytest
import torch
import torch.nn.functional as F

from oracle import tail

f64 = torch.float64
# (N, C, H, W, scale): odd channel counts, batch 3, one-row low-res maps, Wl = 4 at scale 8
SHAPES = [(3, 5, 8, 32, 8), (1, 3, 16, 64, 8), (2, 3, 4, 16, 4), (3, 2, 12, 24, 4), (2, 5, 2, 8, 2), (1, 7, 6, 12, 2),
          (3, 4, 5, 12, 1)]


def _close(got, want, tol=1e-12):
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize('s', [2, 4, 8])
@pytest.mark.parametrize('hw', [(1, 4), (1, 1), (3, 5), (7, 4), (2, 9)])
def test_upsample_and_adjoint_match_interpolate(s, hw):
    torch.manual_seed(s * 100 + hw[0] * 10 + hw[1])
    x = torch.randn(3, 2, *hw, dtype=f64, requires_grad=True)
    want = F.interpolate(x, scale_factor=s, mode='bilinear', align_corners=False)
    up, A = tail.upsample(x.detach(), s)
    _close(up, want.detach(), 1e-14)
    assert bool((A >= up.abs()).all())
    _close(A, F.interpolate(x.detach().abs(), scale_factor=s, mode='bilinear', align_corners=False), 1e-14)
    g = torch.randn_like(want)
    want.backward(g)
    lo, LA = tail.upsample_t(g, s)
    _close(lo, x.grad, 1e-14)
    assert bool((LA >= lo.abs()).all())


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_tail_passes_match_batchnorm_autograd(shape, relu):
    N, C, H, W, s = shape
    torch.manual_seed(sum(shape) + relu)
    a = (torch.randn(N, C, H, W) + 2.0).to(torch.bfloat16)
    b = torch.randn(N, C, H, W).to(torch.bfloat16) if C % 2 else None
    x = torch.randn(N, C, H // s, W // s)
    shift, gamma, beta = torch.randn(C), torch.randn(C) * 0.3 + 1.0, torch.randn(C) * 0.5
    dy = torch.randn(N, C, H, W)
    eps = 1e-5

    leaves = [v.to(f64).requires_grad_(True) for v in (a, x, gamma, beta)]
    ad, xd, gd, bd = leaves
    tt = ad + (b.to(f64) if b is not None else 0.) + shift.to(f64).view(1, C, 1, 1)
    tt = tt + (xd if s == 1 else F.interpolate(xd, scale_factor=s, mode='bilinear', align_corners=False))
    bn = torch.nn.BatchNorm2d(C, eps=eps).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    y = bn(tt)
    y = F.relu(y) if relu else y
    y.backward(dy.to(f64))

    t, At = tail.tail_sum(a, b, x, s, shift)
    _close(t, tt.detach())
    assert bool((At >= t.abs()).all())
    sums, SA = tail.stats(t, At)
    cnt = N * H * W
    _close(sums[:C], tt.detach().sum((0, 2, 3)))
    _close(sums[C:], (tt.detach() ** 2).sum((0, 2, 3)))
    assert bool((SA >= sums.abs()).all())
    mean = sums[:C] / cnt
    rstd = 1.0 / torch.sqrt(sums[C:] / cnt - mean * mean + eps)
    yy, YA, pre, edge = tail.apply(t, At, mean, rstd, gamma, beta, relu)
    _close(yy, y.detach(), 1e-10)
    assert bool((YA >= yy.abs()).all()) and not bool(edge.any())
    bs, BA = tail.bwd_stats(t, At, dy, mean, rstd, pre, edge, relu)
    assert bool((BA >= bs.abs()).all())
    _close(bs[:C], bn.bias.grad, 1e-10)              # d beta = sum dy', d gamma = sum dy' xhat
    _close(bs[C:], bn.weight.grad, 1e-10)
    dt, DA = tail.bwd_apply(t, At, dy, mean, rstd, gamma, pre, relu, bs[:C] / cnt, bs[C:] / cnt)
    _close(dt, ad.grad, 1e-9)
    assert bool((DA >= dt.abs()).all())
    lo, LA = tail.upsample_t(dt, s)
    _close(lo, xd.grad, 1e-9)
    assert bool((LA >= lo.abs()).all())


def test_eval_mode_statistics_are_constants():
    """running statistics as mean / rstd, mdy = mdyx = 0: dt = gamma rstd dy"""
    torch.manual_seed(7)
    N, C, H, W, s = 2, 3, 8, 16, 4
    a, x, dy = torch.randn(N, C, H, W), torch.randn(N, C, H // s, W // s), torch.randn(N, C, H, W)
    bn = torch.nn.BatchNorm2d(C).double().eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C))
        bn.running_var.copy_(torch.rand(C) + 0.5)
        bn.weight.copy_(torch.randn(C))
    ad = a.to(f64).requires_grad_(True)
    bn(ad + F.interpolate(x.to(f64), scale_factor=s, mode='bilinear', align_corners=False)).backward(dy.to(f64))
    t, At = tail.tail_sum(a, None, x, s, None)
    mean, rstd = bn.running_mean, torch.rsqrt(bn.running_var + bn.eps)
    _, _, pre, edge = tail.apply(t, At, mean, rstd, bn.weight.detach(), bn.bias.detach(), False)
    z = torch.zeros(C, dtype=f64)
    dt, DA = tail.bwd_apply(t, At, dy, mean, rstd, bn.weight.detach(), pre, False, z, z)
    _close(dt, ad.grad)
    assert bool((DA >= dt.abs()).all())


def test_relu_edge_marks_preactivations_at_zero():
    t = torch.tensor([0.0, 1.0, 1.0 + 2.0 ** -30, -3.0], dtype=f64).view(1, 1, 1, 4)
    one, zero = torch.ones(1), torch.zeros(1)
    _, _, pre, edge = tail.apply(t, t.abs(), one, one, one, zero, True)          # pre = t - 1
    assert edge.view(-1).tolist() == [False, True, True, False]
    dy = torch.ones(1, 1, 1, 4)
    s, A = tail.bwd_stats(t, t.abs(), dy, one, one, pre, edge, True)
    assert float(s[0]) == 1.0 and float(A[0]) == 3.0          # one element passes the mask, the two edge ones join A


@pytest.mark.parametrize('addend', [False, True])
def test_interleave_matches_conv_transpose(addend):
    torch.manual_seed(3)
    B, C, Co, h, w = 3, 5, 7, 3, 5
    rows = torch.randn(B, h * w, C, dtype=f64)
    weight = torch.randn(C, Co, 2, 2, dtype=f64)
    want = F.conv_transpose2d(rows.transpose(1, 2).reshape(B, C, h, w), weight, None, stride=2)
    U_, A = tail.up_product(rows, tail.up_weight_rows(weight))
    planes = tail.interleave(U_, Co, h, w)
    _close(planes, want)
    assert bool((A >= U_.abs()).all())
    assert torch.equal(tail.deinterleave(planes), U_)
    assert torch.equal(tail.interleave(tail.deinterleave(want), Co, h, w), want)


def test_token_layouts_match_slice_transpose_cat():
    torch.manual_seed(4)
    B, C, hw = 3, 5, [(3, 7), (2, 3), (1, 5)]
    T = sum(h * w for h, w in hw)
    tokens = torch.randn(B, T, C)
    t0, maps = 0, []
    for h, w in hw:
        want = tokens[:, t0:t0 + h * w].transpose(1, 2).reshape(B, C, h, w).contiguous()
        assert torch.equal(tail.tokens_to_planes(tokens, t0, h * w).view(B, C, h, w), want)
        maps.append(want)
        t0 += h * w
    vecs = [torch.randn(C), None, torch.randn(C)]
    want = torch.cat([m.flatten(2).transpose(1, 2).float() + (v if v is not None else 0.) for m, v in zip(maps, vecs)], dim=1)
    got = torch.cat([tail.planes_to_tokens(m.flatten(2), v) for m, v in zip(maps, vecs)], dim=1)
    assert torch.equal(got, want)


@pytest.mark.parametrize('hw', [(17, 9), (1, 1), (1, 6), (2, 2), (5, 1), (8, 12)])
def test_maxpool_statement_matches_torch(hw):
    torch.manual_seed(hw[0] * 31 + hw[1])
    H, W = hw
    # few-valued: ties among maxima; torch routes the gradient to the first maximum in row-major order
    x = torch.randint(0, 3, (4, H, W)).to(f64).requires_grad_(True)
    y, pos = F.max_pool2d(x.unsqueeze(0), 3, 2, 1, return_indices=True)
    m, idx = tail.maxpool_forward(x.detach())
    assert torch.equal(m, y[0].detach())
    OH, OW = m.shape[1:]
    k = idx.long()
    flat = (2 * torch.arange(OH).view(1, OH, 1) - 1 + k // 3) * W + (2 * torch.arange(OW).view(1, 1, OW) - 1 + k % 3)
    assert torch.equal(flat, pos[0])
    gy = torch.randn(4, OH, OW).to(torch.bfloat16)
    y.backward(gy.to(f64).unsqueeze(0))
    assert torch.equal(tail.maxpool_backward(gy, idx, H, W), x.grad)
    assert not bool(tail.maxpool_inexact(gy, idx, H, W).any())


def test_maxpool_inexact_flags_far_apart_exponents():
    x = torch.zeros(1, 3, 3)
    x[0, 1, 1] = 1.0                                   # the centre is the maximum of all four windows
    _, idx = tail.maxpool_forward(x)
    gy = torch.tensor([[[1.0, 2.0 ** -20], [1.0, 1.0]]]).to(torch.bfloat16)
    bad = tail.maxpool_inexact(gy, idx, 3, 3)
    assert bool(bad[0, 1, 1]) and int(bad.sum()) == 1
    gy[0, 0, 1] = 2.0 ** -10
    assert not bool(tail.maxpool_inexact(gy, idx, 3, 3).any())
