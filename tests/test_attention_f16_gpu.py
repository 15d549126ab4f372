"""GPU: the fp16 instantiations of the MFMA attention kernels (csrc/attn_*.hip with T = _Float16; the path fp16 autocast
takes) against an fp32 PyTorch statement of the same expression: softmax(q k^T * scale [+ bias]) v.

Scores, softmax statistics and accumulators are fp32 in the kernels; only P and dS are rounded to fp16 as MFMA operands.
So the results carry fp16's 11 significant bits (bounds 6x tighter than the bf16 suite's), no score can overflow fp16's
range, and no (B, heads, N, N) tensor is ever formed."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 5e-3, 1.5e-2


def _ref(qkv, scale, bias=None):
    q, k, v = qkv.float().permute(2, 0, 3, 1, 4).unbind(0)
    s = (q @ k.transpose(-2, -1)) * scale
    if bias is not None:
        s = s + bias.unsqueeze(0)
    return (s.softmax(-1) @ v).transpose(1, 2)


def _max_err(a, b):
    return (a.float() - b.float()).abs().max().item()


def _run(qkv16, g):
    from vitadapter import kernels
    x = qkv16.detach().clone().requires_grad_(True)
    out = kernels.attention(x, 64 ** -0.5)
    out.backward(g.to(qkv16.dtype))
    return out, x.grad


@pytest.mark.parametrize('B,N,H', [(1, 64, 1), (2, 196, 3), (2, 333, 2), (1, 65, 1), (3, 1, 1), (2, 4096, 2)])
def test_f16_attention_forward_backward(B, N, H):
    torch.manual_seed(N + H)
    qkv = (torch.randn(B, N, 3, H, 64, device='cuda') * 1.5).half()
    g = torch.randn(B, N, H, 64, device='cuda').half().float()
    out, dqkv = _run(qkv, g)
    assert out.dtype == torch.float16 and out.shape == (B, N, H, 64)
    assert dqkv.dtype == torch.float16 and dqkv.shape == qkv.shape
    qr = qkv.float().requires_grad_(True)
    ref = _ref(qr, 64 ** -0.5)
    ref.backward(g)
    err, gerr = _max_err(out, ref), _max_err(dqkv, qr.grad)
    assert err <= FWD_TOL * max(1.0, ref.abs().max().item()), err
    assert gerr <= GRAD_TOL * max(1.0, qr.grad.abs().max().item()), gerr
    # the same inputs through the bf16 kernels: a path that went through bf16 anywhere would land near their error
    out_b, dqkv_b = _run(qkv.bfloat16(), g)
    assert out_b.dtype == torch.bfloat16
    assert err <= 0.5 * _max_err(out_b, ref), (err, _max_err(out_b, ref))
    assert gerr <= 0.5 * _max_err(dqkv_b, qr.grad), (gerr, _max_err(dqkv_b, qr.grad))


def test_f16_attention_identity_structure():
    """Exact-data check of the fragment maps in fp16: one-hot probabilities must pick the right value row of an
    asymmetric V (catches transposed / permuted k orders of the fp16 operands)."""
    from vitadapter import kernels
    B, N, H = 1, 200, 2
    q = torch.zeros(B, N, H, 64, device='cuda')
    k = torch.zeros(B, N, H, 64, device='cuda')
    idx = torch.arange(N, device='cuda')
    tgt = (idx * 7 + 3) % N
    code = torch.randn(N, 64, device='cuda').sign()
    k[0] = code[:, None, :]
    q[0] = code[tgt][:, None, :] * 4.0                         # dot = 256 for the target, ~0 otherwise
    v = torch.arange(N * 64, device='cuda', dtype=torch.float32).view(N, 64) % 251 - 125.0     # integers: exact in fp16
    v = v[None, :, None, :].expand(B, N, H, 64)
    qkv = torch.stack((q, k, v), 2).half()
    out = kernels.attention(qkv, 1.0)
    assert out.dtype == torch.float16
    want = v[0, tgt][:, 0, :]
    assert _max_err(out[0, :, 0], want) <= 0.0625
    assert _max_err(out[0, :, 1], want) <= 0.0625


def test_f16_attention_scores_beyond_fp16_range():
    """q = k = +-32 sign codes: q.k = 65536 > 65504 (fp16's largest value) on the diagonal.  The scores live in fp32
    inside the kernels: output and gradients are finite and match fp32.  (q @ k^T formed in fp16 gives inf, then NaN.)"""
    from vitadapter import kernels
    torch.manual_seed(3)
    B, N, H = 1, 256, 2
    code = torch.randn(B, N, H, 64, device='cuda').sign() * 32
    v = torch.randn(B, N, H, 64, device='cuda')
    qkv = torch.stack((code, code, v), 2).half().requires_grad_(True)
    scale = 0.125
    out = kernels.attention(qkv, scale)
    assert torch.isfinite(out).all()
    qr = qkv.detach().float().requires_grad_(True)
    ref = _ref(qr, scale)
    assert _max_err(out, ref) <= FWD_TOL * max(1.0, ref.abs().max().item())
    g = torch.randn_like(ref).half()
    out.backward(g)
    ref.backward(g.float())
    assert torch.isfinite(qkv.grad).all()
    assert _max_err(qkv.grad, qr.grad) <= GRAD_TOL * max(1.0, qr.grad.abs().max().item())


def test_f16_attention_memory_is_linear_in_tokens():
    """One global block of the headline shape (2 x 4096 tokens, 12 heads) in fp16, forward and backward: workspace is
    O(N).  The (2, 12, 4096, 4096) fp16 scores alone would take 805 MB."""
    from vitadapter import kernels
    torch.manual_seed(0)
    B, N, H = 2, 4096, 12
    qkv = (torch.randn(B, N, 3, H, 64, device='cuda') * 1.5).half().requires_grad_(True)
    g = torch.randn(B, N, H, 64, device='cuda').half()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = kernels.attention(qkv, 64 ** -0.5)
    out.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert torch.isfinite(qkv.grad).all()
    assert peak < 256 * 2 ** 20, peak / 2 ** 20


@pytest.mark.parametrize('B,H,W,heads,win', [(2, 28, 28, 2, 14), (1, 30, 45, 3, 14), (2, 64, 64, 2, 14), (1, 40, 40, 2, 16)])
def test_f16_window_attention(B, H, W, heads, win):
    """Windows cut by the kernels' addressing (resident kernels for 14 x 14, the general path for 16 x 16 = 256 tokens)
    against the reference's pad AFTER projection / partition / attend / merge / crop (base/vit.py:136-167) in fp32."""
    from vitadapter import kernels
    torch.manual_seed(H * W + win)
    C = heads * 64
    qkv = (torch.randn(B, H * W, 3, heads, 64, device='cuda') * 1.2).half().requires_grad_(True)
    scale = 64 ** -0.5
    out = kernels.window_attention(qkv, scale, H, W, win)
    assert out is not None and out.dtype == torch.float16 and out.shape == (B, H * W, heads, 64)
    g = torch.randn(B, H * W, heads, 64, device='cuda').half()
    out.backward(g)
    assert qkv.grad.dtype == torch.float16

    qr = qkv.detach().float().requires_grad_(True)
    Hp, Wp = math.ceil(H / win) * win, math.ceil(W / win) * win
    t = F.pad(qr.view(B, H, W, 3 * C), (0, 0, 0, Wp - W, 0, Hp - H))
    t = t.view(B, Hp // win, win, Wp // win, win, 3 * C).permute(0, 1, 3, 2, 4, 5)
    t = t.reshape(-1, win * win, 3, heads, 64)
    o = _ref(t, scale).reshape(B, Hp // win, Wp // win, win, win, C).permute(0, 1, 3, 2, 4, 5)
    ref = o.reshape(B, Hp, Wp, C)[:, :H, :W].reshape(B, H * W, heads, 64)
    ref.backward(g.float())
    assert _max_err(out, ref) <= FWD_TOL * max(1.0, ref.abs().max().item())
    gerr = _max_err(qkv.grad, qr.grad)
    assert gerr <= GRAD_TOL * max(1.0, qr.grad.abs().max().item()), gerr


def test_f16_attention_bias_and_relpos():
    """BEiT's shapes (14 x 14 patches + class token = 197 tokens, 16 heads): an explicit (heads, N, N) bias through
    attention_bias and a random (T, heads) table through attention_relpos.  Output, d(qkv), d(bias) and d(table) against
    fp32; the fp16 profiler rows of the bias entry points are the ones recorded."""
    import _vah
    from vitadapter import kernels
    from vitadapter.backbones.beit import relative_position_index
    torch.manual_seed(197)
    B, H, hw = 2, 16, (14, 14)
    N = hw[0] * hw[1] + 1
    scale = 64 ** -0.5
    index, T = relative_position_index(hw)
    index = index.cuda()
    table = (torch.randn(T, H, device='cuda') * 1.5).requires_grad_(True)
    bias = (torch.randn(H, N, N, device='cuda') * 1.5).requires_grad_(True)
    qkv = (torch.randn(B, N, 3, H, 64, device='cuda') * 1.5).half()
    g = torch.randn(B, N, H, 64, device='cuda').half()

    _vah.prof_enable(True, 'attn_')
    try:
        x1 = qkv.clone().requires_grad_(True)
        out1 = kernels.attention_bias(x1, bias, scale)
        out1.backward(g)
        x2 = qkv.clone().requires_grad_(True)
        out2 = kernels.attention_relpos(x2, table, index, scale)
        out2.backward(g)
        torch.cuda.synchronize()
    finally:
        _vah.prof_enable(False)
    rows = _vah.prof_report()
    for name in ('attn_bias_fwd_f16', 'attn_bias_bwd_f16', 'attn_bwd_dq_f16', 'attn_bwd_dkdv_f16'):
        assert rows.get(name, {}).get('calls') == 2, (name, sorted(rows))
    assert not any(n.endswith('_bf16') for n in rows), sorted(rows)

    def check(x, out, leaf, grad, to_bias):
        assert out is not None and out.dtype == torch.float16 and out.shape == (B, N, H, 64)
        qr = qkv.float().requires_grad_(True)
        lr = leaf.detach().clone().requires_grad_(True)
        ref = _ref(qr, scale, to_bias(lr))
        ref.backward(g.float())
        assert _max_err(out, ref) <= FWD_TOL * max(1.0, ref.abs().max().item())
        assert x.grad.dtype == torch.float16
        assert _max_err(x.grad, qr.grad) <= GRAD_TOL * max(1.0, qr.grad.abs().max().item())
        berr = _max_err(grad, lr.grad)
        assert grad.dtype == torch.float32 and berr <= 1e-2 * max(1.0, lr.grad.abs().max().item()), berr

    check(x1, out1, bias, bias.grad, lambda b: b)
    check(x2, out2, table, table.grad, lambda t: t[index.view(-1)].view(N, N, H).permute(2, 0, 1))
