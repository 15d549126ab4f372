"""GPU: reference points per image through the modules - the pixel decoder's encoder stack at batch 2 with real valid
ratios (msdeformattn_pixel_decoder.py:224-240), the drop-in MSDeformAttn with a padding mask, and reference points that
require grad.  The stack must run on the fused kernels (profile rows msda_fused_fwd / msda_fused_bwd and no other msda_*
row; under bf16 autocast the one-node pair core), and compute what the unfused sequence (VAH_MSDA_FUSED=0) and the oracle
composition on the CPU compute.  Bounds of the stack: those of tests/test_pixel_decoder.py::test_stack_matches_oracle_on_gpu,
which batch 1 already meets on these kernels - fp32 2e-4 on outputs, 3e-4 on parameter gradients; bf16 against the fp32 run
relative L2 <= 3e-2 on the output, median <= 6e-2 and worst <= 0.3 over the parameter gradients."""
import pytest
import torch
import torch.nn.functional as F

from oracle import msda as oracle_msda

pytestmark = pytest.mark.gpu

SHAPES = ((4, 6), (8, 12), (16, 24))          # tests/test_pixel_decoder.py::SHAPES
LAYERS = 2


@pytest.fixture(autouse=True)
def _fp32_math():
    tf = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = tf


def _stack(dev, seed=1):
    from vitadapter.pixel_decoder import MSDeformAttnEncoder
    torch.manual_seed(seed)
    m = MSDeformAttnEncoder(num_layers=LAYERS, embed_dims=64, num_heads=2, num_levels=3, num_points=4, feedforward_channels=256)
    with torch.no_grad():                       # away from the all-zero initial offsets / weights
        for layer in m.layers:
            layer.attentions[0].sampling_offsets.weight.normal_(0, 0.05)
            layer.attentions[0].attention_weights.weight.normal_(0, 0.2)
            for n in layer.norms:
                n.weight.normal_(1, 0.1)
                n.bias.normal_(0, 0.1)
    return m.to(dev)


def _expected_stack(m, query, pos, ref, ss):
    """tests/test_pixel_decoder.py::_expected: the stack's arithmetic on the oracle's torch core."""
    shapes = [tuple(x) for x in ss.tolist()]
    for layer in m.layers:
        a = layer.attentions[0]
        M, L, P = a.num_heads, a.num_levels, a.num_points
        q = (query + pos).permute(1, 0, 2)
        v = query.permute(1, 0, 2)
        N, Lq, E = q.shape
        value = F.linear(v, a.value_proj.weight, a.value_proj.bias).view(N, -1, M, E // M)
        off = F.linear(q, a.sampling_offsets.weight, a.sampling_offsets.bias).view(N, Lq, M, L, P, 2)
        w = F.linear(q, a.attention_weights.weight, a.attention_weights.bias).view(N, Lq, M, L * P).softmax(-1).view(N, Lq, M, L, P)
        norm = torch.stack([ss[..., 1], ss[..., 0]], -1).to(q.dtype)
        loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
        out = oracle_msda.core_torch(value, shapes, loc, w)
        x = F.linear(out, a.output_proj.weight, a.output_proj.bias).permute(1, 0, 2) + query
        x = F.layer_norm(x, (E,), layer.norms[0].weight, layer.norms[0].bias, layer.norms[0].eps)
        f = layer.ffns[0]
        h = F.linear(torch.relu(F.linear(x, f.layers[0][0].weight, f.layers[0][0].bias)), f.layers[1].weight, f.layers[1].bias)
        query = F.layer_norm(x + h, (E,), layer.norms[1].weight, layer.norms[1].bias, layer.norms[1].eps)
    return query


def _profiled(fn):
    """fn() with the msda_* entry points profiled -> (result, {row: calls})."""
    import _vah
    _vah.prof_enable(True, 'msda_')
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        _vah.prof_enable(False)
    return res, {k: r['calls'] for k, r in _vah.prof_report().items()}


def _stack_run(m, query, pos, ref, ss, lsi, gout, bf16):
    m.zero_grad(set_to_none=True)
    q = query.detach().clone().requires_grad_(True)

    def run():
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=bf16):
            out = m(query=q, query_pos=pos, spatial_shapes=ss, reference_points=ref, level_start_index=lsi)
        out.float().backward(gout)
        return out.detach().float()
    out, rows = _profiled(run)
    return out, q.grad.clone(), {k: p.grad.clone() for k, p in m.named_parameters()}, rows


def test_encoder_stack_at_batch_two_runs_fused(monkeypatch):
    from vitadapter import fused
    from vitadapter.pixel_decoder import encoder_inputs
    m = _stack('cuda')
    query, pos, ref, ss, lsi = encoder_inputs(SHAPES, 2, 64, 'cuda', seed=3)
    # valid ratios (N, L, 2) as (x, y): image 0 fills its maps, image 1 is padded on the right and at the bottom
    ratios = torch.tensor([[[1.0, 1.0]] * 3, [[0.75, 0.625], [0.75, 0.625], [0.75, 0.59375]]], device='cuda')
    ref = (ref * ratios[:, None]).contiguous()
    assert ref.shape == (2, query.shape[0], 3, 2) and float((ref[1] - ref[0]).abs().max()) >= 0.1
    gout = torch.randn(query.shape, generator=torch.Generator().manual_seed(3)).cuda()
    fused_rows = {'msda_fused_fwd': LAYERS, 'msda_fused_bwd': LAYERS}

    out, dq, g32, rows = _stack_run(m, query, pos, ref, ss, lsi, gout, False)
    assert rows == fused_rows, rows

    # fp32 against the oracle composition on the CPU
    m_cpu = _stack('cpu')
    m_cpu.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    cq = query.detach().cpu().requires_grad_(True)
    want = _expected_stack(m_cpu, cq, pos.cpu(), ref.cpu(), ss.cpu())
    want.backward(gout.cpu())
    assert (out.cpu() - want.detach()).abs().max().item() <= 2e-4
    assert (dq.cpu() - cq.grad).abs().max().item() <= 2e-4 * max(1.0, cq.grad.abs().max().item())
    for k, pc in m_cpu.named_parameters():
        assert (g32[k].cpu() - pc.grad).abs().max().item() <= 3e-4 * max(1.0, pc.grad.abs().max().item()), k

    # ... and against the same module on the unfused sequence
    monkeypatch.setenv('VAH_MSDA_FUSED', '0')
    out_u, dq_u, g_u, rows_u = _stack_run(m, query, pos, ref, ss, lsi, gout, False)
    monkeypatch.delenv('VAH_MSDA_FUSED')
    assert rows_u and not any(k.startswith('msda_fused') for k in rows_u), rows_u
    assert (out - out_u).abs().max().item() <= 2e-4
    assert (dq - dq_u).abs().max().item() <= 2e-4 * max(1.0, dq_u.abs().max().item())
    for k in g32:
        assert (g32[k] - g_u[k]).abs().max().item() <= 3e-4 * max(1.0, g_u[k].abs().max().item()), k

    # bf16 autocast: the one-node pair core, same two rows
    a = m.layers[0].attentions[0]
    with torch.autocast('cuda', dtype=torch.bfloat16):
        qn = (query + pos).permute(1, 0, 2)
        value = a.value_proj(query.permute(1, 0, 2)).view(2, -1, 2, 32)
        assert fused.msda_pair_core_ok(a, qn, value, ref)
    out16, _, g16, rows16 = _stack_run(m, query, pos, ref, ss, lsi, gout, True)
    assert rows16 == fused_rows, rows16
    rel = float((out16 - out).norm() / out.norm())
    assert rel <= 3e-2, rel
    rels = sorted(float((g16[k] - g32[k]).norm() / g32[k].norm()) for k in g32 if float(g32[k].norm()) > 0)
    assert rels[len(rels) // 2] <= 6e-2 and rels[-1] <= 0.3, (rels[len(rels) // 2], rels[-1])


def _plain(dev, d_model, heads, levels, seed=2):
    from ops.modules import MSDeformAttn
    torch.manual_seed(seed)
    m = MSDeformAttn(d_model=d_model, n_heads=heads, n_levels=levels, n_points=4)
    with torch.no_grad():
        m.sampling_offsets.weight.normal_(0, 0.05)
        m.attention_weights.weight.normal_(0, 0.2)
        m.attention_weights.bias.normal_(0, 0.3)
    return m.to(dev)


def _plain_inputs(N, Lq, C, shapes, seed=5):
    g = torch.Generator().manual_seed(seed)
    S = sum(h * w for h, w in shapes)
    query, feat = torch.randn(N, Lq, C, generator=g), torch.randn(N, S, C, generator=g)
    ref = torch.rand(N, Lq, len(shapes), 2, generator=g)
    mask = torch.zeros(N, S, dtype=torch.bool)
    mask[1, -7:] = True
    mask[N - 1, :3] = True
    ss = torch.tensor(shapes, dtype=torch.long)
    lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
    gout = torch.randn(N, Lq, C, generator=g)
    return query, feat, ref, mask, ss, lsi, gout


def _expected_plain(m, query, feat, ref, mask, ss):
    """MSDeformAttn.forward (ref ops/modules/ms_deform_attn.py:96-130) on the oracle's torch core."""
    M, L, P = m.n_heads, m.n_levels, m.n_points
    N, Lq, C = query.shape
    value = F.linear(feat, m.value_proj.weight, m.value_proj.bias).masked_fill(mask[..., None], 0.0).view(N, -1, M, C // M)
    off = F.linear(query, m.sampling_offsets.weight, m.sampling_offsets.bias).view(N, Lq, M, L, P, 2)
    w = F.linear(query, m.attention_weights.weight, m.attention_weights.bias).view(N, Lq, M, L * P).softmax(-1).view(N, Lq, M, L, P)
    norm = torch.stack([ss[..., 1], ss[..., 0]], -1).to(query.dtype)
    loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    out = oracle_msda.core_torch(value, [tuple(x) for x in ss.tolist()], loc, w)
    return F.linear(out, m.output_proj.weight, m.output_proj.bias)


def test_single_level_module_with_padding_mask_takes_the_8_lane_forward(monkeypatch):
    """One level, three images, a padding mask, one grid per image: the window forward builds its schedule from a grid
    the batch shares, so this call goes to the 8-lane kernel; results as the unfused path gives them (fp32 on both
    sides: the bounds of the fp32 stack, 2e-4 on outputs and 3e-4 on gradients)."""
    import _vah
    from ops.functions import ms_deform_attn_fused as mf
    N, Lq, C = 3, 77, 192
    m = _plain('cuda', C, 6, 1)
    query, feat, ref, mask, ss, lsi, gout = [t.cuda() for t in _plain_inputs(N, Lq, C, ((9, 11),))]
    assert Lq % 32 and mf.window_forward(1, 4, 1, Lq) and not mf.window_forward(1, 4, 1, Lq, N)
    calls = []
    for name in ('vah_msda_fused_forward_nref', 'vah_msda_fused_forward_win', 'vah_msda_fused_forward'):
        fn = getattr(_vah.lib, name)
        monkeypatch.setattr(_vah.lib, name, lambda *a, _fn=fn, _name=name: (calls.append(_name), _fn(*a))[1])

    def run():
        m.zero_grad(set_to_none=True)
        q, f = query.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        out = m(q, ref, f, ss, lsi, mask)
        out.backward(gout)
        return [out.detach(), q.grad, f.grad] + [p.grad.clone() for p in m.parameters()]
    got, rows = _profiled(run)
    assert calls == ['vah_msda_fused_forward_nref'], calls
    assert rows == {'msda_fused_fwd': 1, 'msda_fused_bwd': 1}, rows
    monkeypatch.setenv('VAH_MSDA_FUSED', '0')
    want, rows_u = _profiled(run)
    assert calls == ['vah_msda_fused_forward_nref'] and not any(k.startswith('msda_fused') for k in rows_u), (calls, rows_u)
    assert (got[0] - want[0]).abs().max().item() <= 2e-4
    for i, (a, b) in enumerate(zip(got[1:], want[1:])):
        assert (a - b).abs().max().item() <= 3e-4 * max(1.0, b.abs().max().item()), i


def test_reference_points_that_require_grad_keep_their_gradient():
    """Learned reference points of shape (N, ...): the fused Functions would detach them, so the gates send the call
    to the unfused expression; their gradient against the CPU composition, to 1e-4 of its largest entry.  Without grad
    mode, or without requires_grad, the same call is fused."""
    from ops.functions import ms_deform_attn_fused as mf
    N, Lq, C, shapes = 2, 45, 64, ((6, 8), (3, 4), (2, 2))
    m = _plain('cuda', C, 2, 3)
    query, feat, ref, mask, ss, lsi, gout = _plain_inputs(N, Lq, C, shapes)
    dev = [t.cuda() for t in (query, feat, ref, mask, ss, lsi, gout)]
    rg = dev[2].clone().requires_grad_(True)

    def run():
        out = m(dev[0], rg, dev[1], dev[4], dev[5], dev[3])
        out.backward(dev[6])
        return out.detach()
    out, rows = _profiled(run)
    assert rows == {'msda_fwd_f32': 1, 'msda_bwd_f32': 1}, rows
    m_cpu = _plain('cpu', C, 2, 3)
    m_cpu.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    rc = ref.clone().requires_grad_(True)
    want = _expected_plain(m_cpu, query, feat, rc, mask, ss)
    want.backward(gout)
    assert (out.cpu() - want.detach()).abs().max().item() <= 2e-4
    assert rg.grad is not None and rg.grad.shape == rc.grad.shape
    assert (rg.grad.cpu() - rc.grad).abs().max().item() <= 1e-4 * rc.grad.abs().max().item()
    # the gate itself: (N, ...) points that require grad are refused in grad mode only; a shared grid never is
    value = torch.zeros(N, dev[1].shape[1], 2, 32, device='cuda')
    off, lg = torch.zeros(N, Lq, 2, 3, 4, 2, device='cuda'), torch.zeros(N, Lq, 2, 12, device='cuda')
    assert not mf.fused_supported(value, off, lg, rg, 3, 4)
    assert mf.fused_supported(value, off, lg, rg.detach(), 3, 4)
    assert mf.fused_supported(value, off, lg, rg[:1], 3, 4)
    with torch.no_grad():
        assert mf.fused_supported(value, off, lg, rg, 3, 4)
        _, rows_ng = _profiled(lambda: m(dev[0], rg, dev[1], dev[4], dev[5], dev[3]))
    assert rows_ng == {'msda_fused_fwd': 1}, rows_ng
