"""GPU: reference BOXES - reference_points (N, Lq, L, 4) = (cx, cy, w, h), what the iterative-refinement decoders pass
(segmentation/mmseg_custom/models/utils/transformer.py:595-615) - through ops.modules.MSDeformAttn, the mmcv-signature
shim and, under bf16 autocast, the one-node pair core.  The call must run on the fused kernels (one msda_fused_fwd* and
one msda_fused_bwd* profile row, no other msda_* row) and compute what the module's arithmetic on the oracle's torch core
computes on the CPU with loc = c + off / P * wh * 0.5 (detection/ops/modules/ms_deform_attn.py:120-122).

Setup: levels (6, 8), (3, 4), (2, 2), N = 2, Lq = 45, two heads of 32 (d_model 64) and of 64 (d_model 128) channels,
one set of boxes per image, a padding mask.  Tiers and bounds, none of them new:
  fp32           against the CPU composition and against VAH_MSDA_FUSED=0: 2e-4 on the output, 3e-4 max(1, max|want|) on
                 gradients (tests/test_msda_nref_module_gpu.py)
  bf16 autocast  takes the pair core (asserted); against the module's arithmetic with the offsets / logits Linear pair in
                 fp32 on the same bf16-rounded operands, the unfused fp32 core and autograd: 2e-2 of each tensor's maximum
                 (tests/test_msda_d64_module_gpu.py::test_pair_core_matches_fp32_offsets_module); against
                 VAH_MSDA_FUSED=0, which reads bf16 offsets: 4e-2 of each tensor's maximum (::test_fused_core_matches_unfused)
  fp16 autocast  against VAH_MSDA_FUSED=0 - the reference's sequence, which forms the box locations in fp32 as the
                 kernels do (fp16 offsets times fp32 boxes): at D = 32 the output within 2 fp16 ulps of max|out| and
                 gradients within relative L2 1e-2 (tests/test_msda_f16_module_gpu.py); at D = 64 4e-2 of each tensor's
                 maximum (tests/test_msda_d64_module_gpu.py)
Boxes that require grad keep the unfused pair of kernels and their gradient (held to the CPU composition, 1e-4 of its
largest entry), as tests/test_msda_nref_module_gpu.py pins for points.  Run with -s for the FIGURE lines."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import msda as oracle_msda

pytestmark = pytest.mark.gpu

SHAPES = ((6, 8), (3, 4), (2, 2))
N, LQ, HEADS, P = 2, 45, 2, 4
FUSED = {'msda_fused_fwd': 1, 'msda_fused_bwd': 1}
FUSED_F16 = {'msda_fused_fwd_f16': 1, 'msda_fused_bwd_f16': 1}
UNFUSED = {'msda_fwd_f32': 1, 'msda_bwd_f32': 1}
NAMES = ('out', 'dquery', 'dfeat', 'd offsets.w', 'd offsets.b', 'd attn.w', 'd attn.b', 'd value.w', 'd value.b', 'd output.w',
         'd output.b')


@pytest.fixture(autouse=True)
def _fp32_math():
    tf = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = tf


def _module(dev, d_model, cls=None, seed=2):
    from ops.modules import MSDeformAttn
    torch.manual_seed(seed)
    if cls is None:
        m = MSDeformAttn(d_model=d_model, n_heads=HEADS, n_levels=len(SHAPES), n_points=P)
    else:
        m = cls(embed_dims=d_model, num_heads=HEADS, num_levels=len(SHAPES), num_points=P, dropout=0.0, batch_first=False)
    with torch.no_grad():                       # away from the all-zero initial offsets / weights
        m.sampling_offsets.weight.normal_(0, 0.05)
        m.attention_weights.weight.normal_(0, 0.2)
        m.attention_weights.bias.normal_(0, 0.3)
    return m.to(dev)


def _inputs(C, Lq=LQ, seed=5):
    """CPU: query, feat, boxes (N, Lq, L, 4) with centres in [0, 1] and sizes in [0.1, 0.6], padding mask, shapes, lsi, gout."""
    g = torch.Generator().manual_seed(seed)
    S = sum(h * w for h, w in SHAPES)
    query, feat = torch.randn(N, Lq, C, generator=g), torch.randn(N, S, C, generator=g)
    boxes = torch.cat((torch.rand(N, Lq, len(SHAPES), 2, generator=g), 0.1 + 0.5 * torch.rand(N, Lq, len(SHAPES), 2, generator=g)), -1)
    mask = torch.zeros(N, S, dtype=torch.bool)
    mask[1, -7:] = True
    mask[N - 1, :3] = True
    ss = torch.tensor(SHAPES, dtype=torch.long)
    lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
    gout = torch.randn(N, Lq, C, generator=g)
    assert float((boxes[1] - boxes[0]).abs().max()) >= 0.1
    return query, feat, boxes.contiguous(), mask, ss, lsi, gout


def _box_loc(boxes, off):
    return boxes[:, :, None, :, None, :2] + off / P * boxes[:, :, None, :, None, 2:] * 0.5


def _expected_plain(m, query, feat, boxes, mask, ss):
    """MSDeformAttn.forward with reference boxes (ref ops/modules/ms_deform_attn.py:96-130) on the oracle's torch core."""
    M, L = m.n_heads, m.n_levels
    n, Lq, C = query.shape
    value = F.linear(feat, m.value_proj.weight, m.value_proj.bias).masked_fill(mask[..., None], 0.0).view(n, -1, M, C // M)
    off = F.linear(query, m.sampling_offsets.weight, m.sampling_offsets.bias).view(n, Lq, M, L, P, 2)
    w = F.linear(query, m.attention_weights.weight, m.attention_weights.bias).view(n, Lq, M, L * P).softmax(-1).view(n, Lq, M, L, P)
    out = oracle_msda.core_torch(value, [tuple(x) for x in ss.tolist()], _box_loc(boxes, off), w)
    return F.linear(out, m.output_proj.weight, m.output_proj.bias)


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


def _grads(m, out, q, f, gout):
    out.float().backward(gout)
    return [out.detach().float(), q.grad, f.grad] + [m.get_parameter(k).grad.clone() for k in (
        'sampling_offsets.weight', 'sampling_offsets.bias', 'attention_weights.weight', 'attention_weights.bias',
        'value_proj.weight', 'value_proj.bias', 'output_proj.weight', 'output_proj.bias')]


def _run(m, dev, autocast=None):
    """One forward + backward of the module on the device operands -> ([out, dquery, dfeat, parameter gradients], rows)."""
    query, feat, boxes, mask, ss, lsi, gout = dev

    def run():
        m.zero_grad(set_to_none=True)
        q, f = query.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        with torch.autocast('cuda', dtype=autocast or torch.bfloat16, enabled=autocast is not None):
            out = m(q, boxes, f, ss, lsi, mask)
        return _grads(m, out, q, f, gout)
    return _profiled(run)


def _close(tag, got, want, out_tol, grad_tol, floor=1.0):
    """|got - want| <= out_tol on the output, <= grad_tol * max(floor, max|want|) on every gradient."""
    for nm, a, b in zip(NAMES, got, want):
        a, b = a.float().cpu(), b.float().cpu()
        assert bool(torch.isfinite(a).all()), (tag, nm)
        err, top = float((a - b).abs().max()), float(b.abs().max())
        print('FIGURE %s %s: max err %.3e, max |want| %.3e' % (tag, nm, err, top))
        assert err <= (out_tol if nm == 'out' and out_tol is not None else grad_tol * max(floor, top)), (tag, nm, err, top)


@pytest.mark.parametrize('C', [64, 128], ids=['d32', 'd64'])
def test_fp32_boxes_run_fused_and_match_the_cpu_composition(monkeypatch, C):
    from ops.functions import ms_deform_attn_fused as mf
    m = _module('cuda', C)
    cpu = _inputs(C)
    dev = [t.cuda() for t in cpu]
    value = torch.zeros(N, cpu[1].shape[1], HEADS, C // HEADS, device='cuda')
    off, lg = torch.zeros(N, LQ, HEADS, 3, P, 2, device='cuda'), torch.zeros(N, LQ, HEADS, 3 * P, device='cuda')
    assert mf.fused_supported(value, off, lg, dev[2], 3, P)
    got, rows = _run(m, dev)
    assert rows == FUSED, rows

    m_cpu = _module('cpu', C)
    m_cpu.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    query, feat, boxes, mask, ss, lsi, gout = cpu
    q, f = query.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    want = _grads(m_cpu, _expected_plain(m_cpu, q, f, boxes, mask, ss), q, f, gout)
    _close('fp32 D%d vs cpu' % (C // HEADS), got, want, 2e-4, 3e-4)

    monkeypatch.setenv('VAH_MSDA_FUSED', '0')
    got_u, rows_u = _run(m, dev)
    monkeypatch.delenv('VAH_MSDA_FUSED')
    assert rows_u == UNFUSED, rows_u
    _close('fp32 D%d vs unfused' % (C // HEADS), got, got_u, 2e-4, 3e-4)


@pytest.mark.parametrize('C', [64, 128], ids=['d32', 'd64'])
def test_bf16_autocast_takes_the_pair_core(monkeypatch, C):
    from ops.functions import MSDeformAttnFunction
    from vitadapter import fused as vfused
    D = C // HEADS
    m = _module('cuda', C)
    dev = [t.cuda() for t in _inputs(C)]
    query, feat, boxes, mask, ss, lsi, gout = dev
    S = feat.shape[1]
    with torch.autocast('cuda', dtype=torch.bfloat16):
        assert vfused.msda_pair_core_ok(m, query, m.value_proj(feat).view(N, S, HEADS, D), boxes)
    calls = []
    core = vfused.msda_pair_core
    monkeypatch.setattr(vfused, 'msda_pair_core', lambda *a: (calls.append(1), core(*a))[1])
    got, rows = _run(m, dev, torch.bfloat16)
    assert calls == [1] and rows == FUSED, (calls, rows)

    # the module's arithmetic with the Linear pair in fp32 on the bf16-rounded operands, the unfused fp32 core, autograd
    def rounded(t):                     # bf16 value, fp32 gradient straight through
        return t + (t.to(torch.bfloat16).float() - t).detach()
    m.zero_grad(set_to_none=True)
    q, f = query.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        value = m.value_proj(f).masked_fill(mask[..., None], 0.0)
    qr = rounded(q).view(-1, C)
    offsets = (qr @ rounded(m.sampling_offsets.weight).t() + m.sampling_offsets.bias).view(N, LQ, HEADS, 3, P, 2)
    logits = (qr @ rounded(m.attention_weights.weight).t() + m.attention_weights.bias).view(N, LQ, HEADS, 3 * P)
    weights = torch.softmax(logits, -1).view(N, LQ, HEADS, 3, P)
    out = MSDeformAttnFunction.apply(value.float().view(N, S, HEADS, D), ss, lsi, _box_loc(boxes, offsets), weights, 64)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = m.output_proj(out.to(torch.bfloat16))
    want = _grads(m, out, q, f, gout)
    _close('bf16 D%d pair core vs fp32 offsets' % D, got, want, None, 2e-2, floor=1e-3)

    monkeypatch.setenv('VAH_MSDA_FUSED', '0')
    got_u, rows_u = _run(m, dev, torch.bfloat16)
    monkeypatch.delenv('VAH_MSDA_FUSED')
    assert calls == [1] and rows_u == UNFUSED, (calls, rows_u)
    _close('bf16 D%d vs unfused' % D, got, got_u, None, 4e-2)


@pytest.mark.parametrize('C', [64, 128], ids=['d32', 'd64'])
def test_fp16_autocast(monkeypatch, C):
    D = C // HEADS
    m = _module('cuda', C)
    dev = [t.cuda() for t in _inputs(C)]
    got, rows = _run(m, dev, torch.float16)
    assert rows == FUSED_F16, rows
    monkeypatch.setenv('VAH_MSDA_FUSED', '0')
    want, rows_u = _run(m, dev, torch.float16)
    monkeypatch.delenv('VAH_MSDA_FUSED')
    assert rows_u == UNFUSED, rows_u
    if D == 64:
        _close('fp16 D64 vs unfused', got, want, None, 4e-2)
        return
    assert all(bool(torch.isfinite(a).all()) for a in got)
    top = float(want[0].abs().max())
    ulp = 2.0 ** (math.floor(math.log2(top)) - 10)
    err = float((got[0] - want[0]).abs().max())
    print('FIGURE fp16 D32 out: max err %.3e = %.2f fp16 ulps of max|out| %.3e' % (err, err / ulp, top))
    figs = {nm: float((a.double() - b.double()).norm() / b.double().norm()) for nm, a, b in zip(NAMES[1:], got[1:], want[1:])}
    for nm in figs:
        print('FIGURE fp16 D32 grad %s: relative L2 %.3e' % (nm, figs[nm]))
    assert err <= 2 * ulp, (err, ulp)
    bad = {k: v for k, v in figs.items() if not v <= 1e-2}
    assert not bad, bad


def test_boxes_that_require_grad_keep_their_gradient():
    """Learned boxes of shape (N, ...): the fused Functions would detach them, so the gates send the call to the unfused
    expression; their gradient against the CPU composition, to 1e-4 of its largest entry.  Without grad mode, or without
    requires_grad, the same call is fused."""
    from ops.functions import ms_deform_attn_fused as mf
    C = 64
    m = _module('cuda', C)
    cpu = _inputs(C)
    query, feat, boxes, mask, ss, lsi, gout = cpu
    dev = [t.cuda() for t in cpu]
    rg = dev[2].clone().requires_grad_(True)

    def run():
        out = m(dev[0], rg, dev[1], dev[4], dev[5], dev[3])
        out.backward(dev[6])
        return out.detach()
    out, rows = _profiled(run)
    assert rows == UNFUSED, rows
    m_cpu = _module('cpu', C)
    m_cpu.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    rc = boxes.clone().requires_grad_(True)
    want = _expected_plain(m_cpu, query, feat, rc, mask, ss)
    want.backward(gout)
    assert (out.cpu() - want.detach()).abs().max().item() <= 2e-4
    assert rg.grad is not None and rg.grad.shape == rc.grad.shape
    assert float(rc.grad[..., 2:].abs().max()) > 0                       # the sizes have a gradient of their own
    assert (rg.grad.cpu() - rc.grad).abs().max().item() <= 1e-4 * rc.grad.abs().max().item()
    value = torch.zeros(N, dev[1].shape[1], HEADS, 32, device='cuda')
    off, lg = torch.zeros(N, LQ, HEADS, 3, P, 2, device='cuda'), torch.zeros(N, LQ, HEADS, 3 * P, device='cuda')
    assert not mf.fused_supported(value, off, lg, rg, 3, P)
    assert mf.fused_supported(value, off, lg, rg.detach(), 3, P)
    assert mf.fused_supported(value, off, lg, rg[:1], 3, P)
    with torch.no_grad():
        assert mf.fused_supported(value, off, lg, rg, 3, P)
        _, rows_ng = _profiled(lambda: m(dev[0], rg, dev[1], dev[4], dev[5], dev[3]))
    assert rows_ng == {'msda_fused_fwd': 1}, rows_ng


def test_mmcv_shim_with_query_pos_and_boxes():
    """vitadapter's MultiScaleDeformableAttention in (Lq, N, E) layout, value = query (Lq = S = 64), query_pos, a padding
    mask and boxes: the fused rows, and identity + the module's arithmetic on query + query_pos."""
    from vitadapter.mmcv_attention import MultiScaleDeformableAttention
    C = 64
    S = sum(h * w for h, w in SHAPES)
    m = _module('cuda', C, cls=MultiScaleDeformableAttention)
    _, _, boxes, mask, ss, lsi, _ = _inputs(C, Lq=S)
    g = torch.Generator().manual_seed(9)
    query, pos, gout = (torch.randn(S, N, C, generator=g) for _ in range(3))

    def run():
        m.zero_grad(set_to_none=True)
        q = query.cuda().requires_grad_(True)
        out = m(q, query_pos=pos.cuda(), key_padding_mask=mask.cuda(), reference_points=boxes.cuda(), spatial_shapes=ss.cuda(),
                level_start_index=lsi.cuda())
        out.backward(gout.cuda())
        return [out.detach(), q.grad] + [p.grad.clone() for p in m.parameters()]
    got, rows = _profiled(run)
    assert rows == FUSED, rows

    m_cpu = _module('cpu', C, cls=MultiScaleDeformableAttention)
    m_cpu.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    q = query.clone().requires_grad_(True)
    want = _expected_plain(m_cpu, (q + pos).permute(1, 0, 2), q.permute(1, 0, 2), boxes, mask, ss).permute(1, 0, 2) + q
    want.backward(gout)
    wants = [want.detach(), q.grad] + [p.grad for p in m_cpu.parameters()]
    assert (got[0].cpu() - wants[0]).abs().max().item() <= 2e-4
    for i, (a, b) in enumerate(zip(got[1:], wants[1:])):
        assert (a.cpu() - b).abs().max().item() <= 3e-4 * max(1.0, b.abs().max().item()), i
