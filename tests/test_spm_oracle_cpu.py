"""CPU: the fp64 references of the SpatialPriorModule kernels (oracle/spm.py) against torch's own fp64 convolution,
autograd and max-pool, and the budget helper against an honest fp32 evaluation and against results with a piece
missing.  The GPU file tests/test_spm_fp64_gpu.py holds the kernels to these references."""
import pytest
import torch
import torch.nn.functional as F

from oracle import spm

# (N, H, W, Cin, Cout, S): stride 1 and 2, odd sizes, H or W of 1, the 16-channel stem layout
SHAPES = [(2, 7, 9, 8, 16, 1), (2, 7, 9, 8, 16, 2), (1, 1, 5, 4, 8, 1), (1, 6, 1, 4, 8, 2), (3, 1, 1, 4, 8, 2),
          (2, 10, 13, 16, 8, 2), (1, 5, 6, 16, 8, 1)]


def _operands(N, H, W, Cin, Cout, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Cin, generator=g).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5).to(torch.bfloat16)
    if Cin == 16:                                           # the image: 3 channels, 3..15 zero in x and in w
        x[..., 3:] = 0
        w[:, 3:] = 0
    OH, OW = (H - 1) // S + 1, (W - 1) // S + 1
    gy = torch.randn(N, OH, OW, Cout, generator=g).to(torch.bfloat16)
    return x, w, gy


def _w9(w):          # conv.forward_weight
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).contiguous()


def _wt9(w):         # conv.dgrad_weight
    return w.permute(1, 2, 3, 0).reshape(w.shape[1], 9, w.shape[0]).contiguous()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_conv_references_match_torch_fp64(shape):
    N, H, W, Cin, Cout, S = shape
    x, w, gy = _operands(*shape)
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.double().requires_grad_(True)
    y = F.conv2d(xr, wr, None, S, 1)
    gx, gw = torch.autograd.grad(y, (xr, wr), gy.double().permute(0, 3, 1, 2))
    out, A = spm.conv_forward(x, _w9(w), S)
    assert out.shape == (N, y.shape[2], y.shape[3], Cout)
    assert _rel(out, y.detach().permute(0, 2, 3, 1)) <= 1e-12
    assert (A >= out.abs()).all()
    dx, Ad = spm.conv_input_grad(gy, _wt9(w), S, H, W)
    assert _rel(dx, gx.permute(0, 2, 3, 1)) <= 1e-12 and (Ad >= dx.abs()).all()
    dw, Aw = spm.conv_weight_grad(x, gy, S)
    assert _rel(dw, gw.permute(0, 2, 3, 1).reshape(Cout, 9, Cin)) <= 1e-12 and (Aw >= dw.abs()).all()
    if Cin == 16:
        assert (dw[..., 3:] == 0).all() and (Aw[..., 3:] == 0).all()


@pytest.mark.parametrize('shape', [(2, 9, 11, 8), (1, 1, 1, 8), (1, 2, 5, 8), (2, 6, 1, 8)])
def test_maxpool_reference_matches_torch(shape):
    g = torch.Generator().manual_seed(1)
    rand = torch.randn(*shape, generator=g).to(torch.bfloat16)
    relu = rand.clamp_min(0)                                            # ties among zeros
    few = torch.tensor([-1.0, 0.5, 1.5, 1.5])[torch.randint(0, 4, shape, generator=g)].to(torch.bfloat16)  # non-zero ties
    N, H, W, C = shape
    for x in (rand, relu, few):
        y, idx = spm.maxpool_forward(x)
        yr, ir = F.max_pool2d(x.double().permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
        assert torch.equal(y, yr.permute(0, 2, 3, 1))
        assert torch.equal(spm.pool_flat_index(idx, H, W), ir.permute(0, 2, 3, 1))
        gy = torch.randn(y.shape, generator=g).to(torch.bfloat16)
        xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
        F.max_pool2d(xr, 3, 2, 1).backward(gy.double().permute(0, 3, 1, 2))
        gx, A = spm.maxpool_backward(gy, idx, H, W)
        assert torch.equal(gx, xr.grad.permute(0, 2, 3, 1)) and (A >= gx.abs()).all()


def test_batchnorm_references_match_torch_fp64():
    g = torch.Generator().manual_seed(2)
    C, rows = 16, 300
    x = (torch.randn(rows, C, generator=g) * 2 + 5).to(torch.bfloat16)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    s, A = spm.bn_stats(x)
    xd = x.double()
    assert torch.allclose(s, torch.cat([xd.sum(0), (xd * xd).sum(0)]), rtol=1e-13, atol=0)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    fin = spm.finalize_stats(torch.cat([s.float(), torch.tensor([float(rows)])]), C, 1e-5, 0.1, rm, rv)
    bn = torch.nn.BatchNorm1d(C, eps=1e-5, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.copy_(w), bn.bias.copy_(b), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    xr = xd.clone().requires_grad_(True)
    y = F.relu(bn(xr))
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    rstd = 1 / torch.sqrt(var + 1e-5)
    # from the fp32-rounded sums: agreement to the rounding of the sums (scaled by the variance's conditioning)
    assert torch.allclose(fin['mean'][0], mean, rtol=1e-6)
    assert torch.allclose(fin['rstd'][0], rstd, rtol=1e-5)
    assert torch.allclose(fin['running_mean'][0], bn.running_mean, rtol=1e-6, atol=1e-7)
    assert torch.allclose(fin['running_var'][0], bn.running_var, rtol=1e-5)
    # apply and backward from exact fp64 statistics
    mf, rf = mean.float(), rstd.float()
    yr, Ay = spm.bn_apply(x, mf, rf, w, b, True)
    sc = rf.double() * w.double()
    assert torch.allclose(yr, F.relu((xd - mf.double()) * sc + b.double()), rtol=1e-12, atol=1e-12) and (Ay >= yr.abs()).all()
    dy = torch.randn(rows, C, generator=g).to(torch.bfloat16)
    sums, As, edge = spm.bn_bwd_stats(x, dy, mf, rf, w, b, True)
    assert not edge.any()
    gp = torch.where(yr > 0, dy.double(), torch.zeros((), dtype=torch.float64))
    xh = (xd - mf.double()) * rf.double()
    assert torch.allclose(sums, torch.cat([gp.sum(0), (gp * xh).sum(0)]), rtol=1e-12, atol=1e-12)
    means = sums / rows
    dx, Adx = spm.bn_bwd_apply(x, dy, mf, rf, w, b, True, means[:C], means[C:])
    assert (Adx >= dx.abs() - 1e-12).all()
    # with exact statistics the formula is the autograd gradient of relu(BatchNorm(x))
    y.backward(dy.double())
    dx_exact, _ = spm.bn_bwd_apply(x, dy, mean, rstd, w, b, True, *(lambda m: (m[:C], m[C:]))(
        spm.bn_bwd_stats(x, dy, mean, rstd, w, b, True)[0] / rows))
    assert torch.allclose(dx_exact, xr.grad, rtol=1e-9, atol=1e-11)


def test_image_to_nhwc16_reference():
    x = torch.randn(2, 3, 5, 7)
    y = spm.image_to_nhwc16(x)
    assert y.shape == (2, 5, 7, 16) and (y[..., 3:] == 0).all()
    assert torch.equal(y[..., :3], x.permute(0, 2, 3, 1).to(torch.bfloat16))


def _fp32_eval(N, H, W, Cin, Cout, S, seed):
    x, w, gy = _operands(N, H, W, Cin, Cout, S, seed)
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.float().requires_grad_(True)
    y = F.conv2d(xr, wr, None, S, 1)
    gx, gw = torch.autograd.grad(y, (xr, wr), gy.float().permute(0, 3, 1, 2))
    return (x, w, gy), (y.detach().permute(0, 2, 3, 1), gx.permute(0, 2, 3, 1), gw.permute(0, 2, 3, 1).reshape(Cout, 9, Cin))


@pytest.mark.parametrize('shape', [(2, 64, 64, 64, 64, 1), (2, 64, 96, 64, 64, 2), (1, 64, 64, 16, 64, 2)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_budget_passes_fp32_and_fails_a_missing_piece(shape):
    """An honest fp32 evaluation of the same bf16 operands uses under half of every budget (fp32 outputs: the
    accumulation term alone); one tap left out of the forward or the input gradient, or one 32-pixel row of dY left
    out of the weight gradient, fails."""
    N, H, W, Cin, Cout, S = shape
    (x, w, gy), (y32, gx32, gw32) = _fp32_eval(*shape, seed=3)
    out, A = spm.conv_forward(x, _w9(w), S)
    assert spm.ratio(y32, out, A) < 0.5
    dw, Aw = spm.conv_weight_grad(x, gy, S)
    assert spm.ratio(gw32, dw, Aw) < 0.5
    if Cin == 16:
        assert (gw32[..., 3:] == 0).all()
    else:
        dx, Ad = spm.conv_input_grad(gy, _wt9(w), S, H, W)
        assert spm.ratio(gx32, dx, Ad) < 0.5
        w_drop = w.clone()
        w_drop[:, :, 2, 1] = 0                                          # tap (2, 1) left out
        dx_drop, _ = spm.conv_input_grad(gy, _wt9(w_drop), S, H, W)
        assert spm.ratio(dx_drop.to(torch.bfloat16), dx, Ad, bf16=True) > 1
    w_drop = w.clone()
    w_drop[:, :, 0, 2] = 0
    out_drop, _ = spm.conv_forward(x, _w9(w_drop), S)
    assert spm.ratio(out_drop.to(torch.bfloat16), out, A, bf16=True) > 1
    gy_drop = gy.clone()
    gy_drop[-1, gy.shape[1] // 2, :32] = 0                              # one 32-pixel row of one image
    dw_drop, _ = spm.conv_weight_grad(x, gy_drop, S)
    assert spm.ratio(dw_drop.float(), dw, Aw) > 1
    with pytest.raises(AssertionError):
        spm.check('dw', dw_drop.float(), dw, Aw)
