"""GPU: MSDeformAttn with heads of 64 channels (ViT-Adapter-S: d_model 384, 6 heads, ratio 1.0) on the fused kernels,
against the unfused op sequence on the same weights, and the small_seg preset end to end.

The maps are the small ones of tests/test_backbone_gpu.py::test_fused_core_bf16_autocast_matches_unfused (L = 3 and L = 1,
powers of two: under fp16 the unfused sequence rounds offsets / (W, H) to fp16, exact for such maps, so both paths sample
at the same locations - tests/test_msda_f16_module_gpu.py).  Bounds, those of the tests that compare the same two paths
at D = 32: 4e-2 of each tensor's maximum for the fused core reading the 16-bit Linear outputs
(test_fused_core_bf16_autocast_matches_unfused), 2e-2 for the one-node pair + core with fp32 offsets against the module's
arithmetic with that Linear pair in fp32 (test_pair_core_matches_fp32_offsets_module)."""
import pytest
import torch

from oracle import cases

pytestmark = pytest.mark.gpu

C, M, P, N = 384, 6, 4, 2
GEOM = [(3, [(16, 16), (8, 8), (4, 4)], [(8, 8)]),
        (1, [(8, 8)], [(16, 16), (8, 8), (4, 4)])]


def _module(L):
    from ops.modules import MSDeformAttn
    torch.manual_seed(4)
    m = MSDeformAttn(d_model=C, n_levels=L, n_heads=M, n_points=P, ratio=1.0).cuda()
    with torch.no_grad():
        m.sampling_offsets.weight.normal_(0, 0.02)
        m.attention_weights.weight.normal_(0, 0.05)
        m.attention_weights.bias.normal_(0, 0.3)
    return m


def _operands(L, shapes, qshapes):
    S, Lq = sum(h * w for h, w in shapes), sum(h * w for h, w in qshapes)
    ref = cases.reference_grid(qshapes).cuda()
    if L > 1:
        ref = ref.expand(1, Lq, L, 2).contiguous()
    hw = torch.as_tensor(shapes, dtype=torch.long).cuda()
    lsi = cases.level_start_index(shapes).cuda()
    gen = torch.Generator().manual_seed(40 + L)
    query, feat, gout = (torch.randn(N, n, C, generator=gen).cuda() for n in (Lq, S, Lq))
    return ref, hw, lsi, query, feat, gout


NAMES = ('out', 'dquery', 'dfeat', 'd offsets.w', 'd offsets.b', 'd attn.w', 'd attn.b', 'd value.w', 'd output.w')


def _grads(m, out, qq, ff, gout):
    out.float().backward(gout)
    return (out.float().detach(), qq.grad, ff.grad, m.sampling_offsets.weight.grad.clone(),
            m.sampling_offsets.bias.grad.clone(), m.attention_weights.weight.grad.clone(),
            m.attention_weights.bias.grad.clone(), m.value_proj.weight.grad.clone(), m.output_proj.weight.grad.clone())


def _msda_rows(fn):
    """Run fn with the launch profiler on the msda_ rows -> (result, rows)."""
    import _vah
    try:
        _vah.prof_enable(True, 'msda_')
        res = fn()
        torch.cuda.synchronize()
        _vah.prof_enable(False)
        return res, _vah.prof_report()
    finally:
        _vah.prof_enable(False)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('L,shapes,qshapes', GEOM)
def test_fused_core_matches_unfused(monkeypatch, L, shapes, qshapes, dtype):
    """The fused core (MSDeformAttnFusedFunction: forward kernels + tile-pass backward at D = 64) reading the 16-bit Linear
    outputs, against VAH_MSDA_FUSED=0 on the same weights, under bf16 and under fp16 autocast."""
    from ops.functions import ms_deform_attn_fused as mf
    from vitadapter import fused as vfused
    # the one-node pair + core keeps the offsets in fp32 (its own test below): here both sides read the 16-bit outputs
    monkeypatch.setitem(vfused.ENABLED, 'pair_core', False)
    m = _module(L)
    ref, hw, lsi, query, feat, gout = _operands(L, shapes, qshapes)
    S, Lq = feat.shape[1], query.shape[1]
    value = torch.empty(N, S, M, C // M, dtype=dtype, device='cuda')
    assert value.shape[-1] == 64
    off, lg = torch.empty(N, Lq, M, L, P, 2, dtype=dtype, device='cuda'), torch.empty(N, Lq, M, L * P, dtype=dtype, device='cuda')
    assert mf.fused_supported(value, off, lg, ref, L, P)
    res, rows = [], []
    for fused in ('1', '0'):
        monkeypatch.setenv('VAH_MSDA_FUSED', fused)
        qq, ff = query.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        m.zero_grad()

        def run():
            with torch.autocast('cuda', dtype=dtype):
                out = m(qq, ref, ff, hw, lsi, None)
            return _grads(m, out, qq, ff, gout)
        r, rw = _msda_rows(run)
        res.append(r)
        rows.append(rw)
    sfx = '_f16' if dtype == torch.float16 else ''
    assert rows[0].get('msda_fused_fwd' + sfx, {}).get('calls', 0) == 1, sorted(rows[0])
    assert rows[0].get('msda_fused_bwd' + sfx, {}).get('calls', 0) == 1, sorted(rows[0])
    assert 'msda_fwd_f32' not in rows[0] and 'msda_bwd_f32' not in rows[0], sorted(rows[0])
    # the switch takes the fused kernels away (what runs the unfused core instead is the module's business)
    assert 'msda_fused_fwd' + sfx not in rows[1] and 'msda_fused_bwd' + sfx not in rows[1], sorted(rows[1])
    for a, b, nm in zip(res[0], res[1], NAMES):
        assert torch.isfinite(a).all(), nm
        err = (a - b).abs().max().item()
        print('FIGURE L=%d %s %s: max err %.3e, max |want| %.3e' % (L, sfx or '_bf16', nm, err, b.abs().max().item()))
        assert err <= 4e-2 * max(1.0, b.abs().max().item()), (nm, err)


@pytest.mark.parametrize('L,shapes,qshapes', GEOM)
def test_pair_core_matches_fp32_offsets_module(L, shapes, qshapes):
    """vitadapter/fused.py::_MSDAPairCore at D = 64 (what the small presets run under bf16 autocast) against the module's
    arithmetic with the offsets / logits Linear pair evaluated in fp32 on the same bf16-rounded operands, the unfused fp32
    core (MSDeformAttnFunction) and autograd: 2e-2 of each tensor's maximum."""
    from ops.functions import MSDeformAttnFunction
    from vitadapter import fused as vfused
    assert vfused.ENABLED['pair_core']
    m = _module(L)
    ref, hw, lsi, query, feat, gout = _operands(L, shapes, qshapes)
    S, Lq = feat.shape[1], query.shape[1]

    qq, ff = query.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    m.zero_grad()

    def run():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            assert vfused.msda_pair_core_ok(m, qq, m.value_proj(ff).view(N, S, M, C // M), ref)
            out = m(qq, ref, ff, hw, lsi, None)
        return _grads(m, out, qq, ff, gout)
    got, rows = _msda_rows(run)
    assert rows.get('msda_fused_fwd', {}).get('calls', 0) == 1 and rows.get('msda_fused_bwd', {}).get('calls', 0) == 1, sorted(rows)
    assert 'msda_fwd_f32' not in rows and 'msda_bwd_f32' not in rows, sorted(rows)

    def rounded(t):                     # bf16 value, fp32 gradient straight through
        return t + (t.to(torch.bfloat16).float() - t).detach()

    qq, ff = query.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    m.zero_grad()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        value = m.value_proj(ff)
    qr = rounded(qq).view(-1, C)
    offsets = (qr @ rounded(m.sampling_offsets.weight).t() + m.sampling_offsets.bias).view(N, Lq, M, L, P, 2)
    logits = (qr @ rounded(m.attention_weights.weight).t() + m.attention_weights.bias).view(N, Lq, M, L * P)
    weights = torch.softmax(logits, -1).view(N, Lq, M, L, P)
    wh = hw.flip(-1).float()
    loc = ref[:, :, None, :, None, :] + offsets / wh[None, None, None, :, None, :]
    core = MSDeformAttnFunction.apply(value.float().view(N, S, M, C // M), hw, lsi, loc, weights, 64)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = m.output_proj(core.to(torch.bfloat16))
    want = _grads(m, out, qq, ff, gout)
    for a, b, nm in zip(got, want, NAMES):
        assert torch.isfinite(a).all(), nm
        err = (a - b).abs().max().item()
        print('FIGURE L=%d pair core %s: max err %.3e, max |want| %.3e' % (L, nm, err, b.abs().max().item()))
        assert err <= 2e-2 * max(1e-3, b.abs().max().item()), (nm, err, b.abs().max().item())


def test_small_seg_preset_forward_backward_bf16():
    """build_preset('small_seg'), one pair of 64 x 64 images, forward + backward under bf16 autocast: finite outputs, the
    four pyramid shapes, a gradient for every parameter - with every deformable-attention call on the fused kernels."""
    from vitadapter.backbones.vit_adapter import build_preset
    torch.manual_seed(0)
    model = build_preset('small_seg').cuda().train()
    x = torch.randn(2, 3, 64, 64, device='cuda')

    def run():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            outs = model(x)
        sum(o.float().mean() for o in outs).backward()
        return outs
    outs, rows = _msda_rows(run)
    assert [tuple(o.shape) for o in outs] == [(2, 384, 16, 16), (2, 384, 8, 8), (2, 384, 4, 4), (2, 384, 2, 2)]
    assert all(torch.isfinite(o).all() for o in outs)
    missing = [k for k, p in model.named_parameters() if p.grad is None]
    assert not missing, missing
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    # 4 injectors + 6 extractors (two extra ones behind the last interaction)
    assert rows.get('msda_fused_fwd', {}).get('calls', 0) == 10 and rows.get('msda_fused_bwd', {}).get('calls', 0) == 10, rows
    assert 'msda_fwd_f32' not in rows and 'msda_bwd_f32' not in rows, sorted(rows)
