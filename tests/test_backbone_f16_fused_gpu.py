"""GPU: whole backbones under fp16 autocast + GradScaler(init_scale=512) with the row-streaming layer of the blocks on
the fp16 kernels of csrc/fused_ops.hip (LayerNorm, residual + LayerNorm, dual LayerNorm, scale-residual, token DWConv).

Which of those rows a model launches depends on its block structure, so the expectation is taken from the model itself:
the rows of the four families under fp16 autocast must be the rows of the bf16-autocast run with `_f16` appended - same
names, same call counts - and no unsuffixed row may appear.  Against the same module in fp32 the bounds are those of
tests/test_backbone_f16_gpu.py (this project's fp16 tier): outputs within 0.08 of the max, parameter gradients median
relative L2 <= 0.08 and every one <= 0.25, with the two exclusions that file documents (the stem below the max-pool;
`sampling_offsets` of the one-head det_win_96x128 case at 1.0) and nothing else left out.  With
ENABLED['fp16_rows'] = False the same run launches none of the new rows and agrees with the fused run within the same
bounds.

The pixel decoder's post-norm encoder layers are the one place where a fused LayerNorm output feeds something that is
not a Linear (the FFN's and the next attention's identity adds): held to the fp32 run in the last test."""
import numpy as np
import pytest
import torch

from oracle import backbone_cases as bc
from oracle import seeded

pytestmark = pytest.mark.gpu

FAMILIES = ('layernorm', 'residual_layernorm', 'scale_residual', 'dwconv_tokens')
ALWAYS = ('residual_layernorm_fwd_f16', 'residual_layernorm_bwd_f16', 'dwconv_tokens_fwd_f16', 'dwconv_tokens_wgrad_f16')
DUAL = ('layernorm_dual_fwd_f16', 'layernorm_dual_bwd_f16')


@pytest.fixture(scope='module', autouse=True)
def _fp32_math():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    yield


def _vit(cfg):
    from vitadapter.backbones import ViTAdapter
    m = ViTAdapter(**cfg)
    m.load_state_dict(seeded.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 5))
    return m


def _beit(cfg):
    from vitadapter.backbones.beit_adapter import BEiTAdapter
    m = BEiTAdapter(**cfg)
    missing, unexpected = m.load_state_dict(seeded.seeded_state_dict(bc.float_shapes(m), 21), strict=False)
    assert not unexpected and all(k.endswith('relative_position_index') for k in missing)
    return m


CASES = {
    'tiny_seg_512': (lambda: (_vit(bc.FULLSIZE_CASES['tiny_seg_512']['cfg']), bc.fullsize_input('tiny_seg_512')), ALWAYS + DUAL),
    'det_win_96x128': (lambda: (_vit(bc.FULL_CASES['det_win_96x128']['cfg']), bc.full_input('det_win_96x128')), ALWAYS + DUAL),
    'beit_seg_96': (lambda: (_beit(bc.BEIT_CASES['beit_seg_96']['cfg']), bc.beit_input('beit_seg_96')), ALWAYS),
}


def _run(model, x, gouts, dtype):
    """One forward + backward (dtype None: fp32) with the row families profiled -> (outputs, gradients, rows, gouts)."""
    import _vah
    model.zero_grad(set_to_none=True)
    opt = torch.optim.SGD(model.parameters(), lr=0.)
    amp = dtype is not None
    scaler = torch.amp.GradScaler('cuda', init_scale=512., enabled=dtype == torch.float16)
    _vah.prof_enable(True, ','.join(FAMILIES))
    try:
        with torch.autocast('cuda', dtype=dtype, enabled=amp):
            o = model(x)
        if gouts is None:
            g = torch.Generator(device='cuda').manual_seed(7)
            gouts = [torch.randn(t.shape, device='cuda', generator=g) for t in o]
        # a mean per level, as a training loss is: fp16 gradients of a summed loss times 512 leave fp16's range
        scaler.scale(sum((t.float() * go).mean() for t, go in zip(o, gouts))).backward()
        scaler.unscale_(opt)
        torch.cuda.synchronize()
    finally:
        _vah.prof_enable(False)
    rows = {k: r['calls'] for k, r in _vah.prof_report().items()}
    outs = [t.detach().float() for t in o]
    grads = {k: p.grad.detach().double().clone() for k, p in model.named_parameters() if p.grad is not None}
    return outs, grads, rows, gouts


def _hold(name, outs, grads, outs32, grads32, what):
    for o16, o32 in zip(outs, outs32):
        assert torch.isfinite(o16).all(), what
        assert (o16 - o32).abs().max().item() <= 0.08 * max(1.0, o32.abs().max().item()), what
    assert set(grads) == set(grads32), what
    assert not [k for k, g in grads.items() if not bool(torch.isfinite(g).all())], what
    top = max(float(g.norm()) for g in grads32.values())
    errs = {k: float((grads[k] - g).norm()) / float(g.norm()) for k, g in grads32.items()
            if not k.startswith('spm.stem') and float(g.norm()) > 1e-5 * top}
    if name == 'det_win_96x128':
        loose = [k for k in errs if 'sampling_offsets' in k]
        assert all(errs[k] <= 1.0 for k in loose), (what, [(k, errs[k]) for k in loose])
        errs = {k: e for k, e in errs.items() if k not in loose}
    rels = sorted(errs.values())
    print('HOLD %s %s: %d gradients, median %.4f worst %.4f' % (name, what, len(rels), float(np.median(rels)), rels[-1]))
    assert len(rels) > 20 and float(np.median(rels)) <= 0.08 and rels[-1] <= 0.25, (
        what, len(rels), float(np.median(rels)), sorted(errs.items(), key=lambda kv: -kv[1])[:3])


@pytest.mark.parametrize('name', sorted(CASES))
def test_backbone_fp16_rows_run_fused(name):
    from vitadapter import fused
    make, at_least = CASES[name]
    torch.manual_seed(0)
    model, x = make()
    model = model.cuda().train()
    x = x.cuda()
    outs32, grads32, rows32, gouts = _run(model, x, None, None)
    assert rows32 == {}, rows32                         # fp32: torch's expressions
    _, _, rows_bf, _ = _run(model, x, gouts, torch.bfloat16)
    outs16, grads16, rows16, _ = _run(model, x, gouts, torch.float16)
    print('ROWS %s bf16 %s' % (name, sorted(rows_bf.items())))
    print('ROWS %s fp16 %s' % (name, sorted(rows16.items())))
    assert rows_bf and not any(r.endswith('_f16') for r in rows_bf), rows_bf
    assert rows16 == {r + '_f16': n for r, n in rows_bf.items()}, (rows16, rows_bf)
    for r in at_least:
        assert rows16.get(r, 0) > 0, (r, rows16)
    _hold(name, outs16, grads16, outs32, grads32, 'fused fp16 rows vs fp32')

    fused.ENABLED['fp16_rows'] = False
    try:
        outs_off, grads_off, rows_off, _ = _run(model, x, gouts, torch.float16)
    finally:
        fused.ENABLED['fp16_rows'] = True
    assert rows_off == {}, rows_off
    _hold(name, outs_off, grads_off, outs32, grads32, 'fp16_rows off vs fp32')
    # the two fp16 runs against each other, same bounds (the fused run as the reference)
    _hold(name, outs_off, grads_off, outs16, grads16, 'fp16_rows off vs fused')


def test_pixel_decoder_encoder_fp16_post_norm():
    """MSDeformAttnEncoder's layers are post-norm: the fused LayerNorm's output is the identity of the FFN's residual
    add and of the next layer's attention (and gets query_pos added), not only a Linear's input.  Under fp16 autocast
    that stream is therefore fp16 (torch's LayerNorm would return fp32): held to the fp32 run at the fp16 tier."""
    import _vah
    from vitadapter import fused
    from vitadapter.pixel_decoder import MSDeformAttnEncoder, encoder_inputs
    torch.manual_seed(0)
    enc = MSDeformAttnEncoder(num_layers=2).cuda().train()
    query, pos, ref, shapes, lsi = encoder_inputs([(8, 8), (16, 16), (32, 32)], 2, 256, 'cuda')
    gout = torch.randn(query.shape, device='cuda')
    res = {}
    for mode in ('fp32', 'fp16', 'fp16_off'):
        enc.zero_grad(set_to_none=True)
        fused.ENABLED['fp16_rows'] = mode != 'fp16_off'
        _vah.prof_enable(True, 'layernorm')
        try:
            with torch.autocast('cuda', dtype=torch.float16, enabled=mode != 'fp32'):
                out = enc(query=query, query_pos=pos, spatial_shapes=shapes, reference_points=ref, level_start_index=lsi)
            ((out.float() * gout).mean() * 512.).backward()
            torch.cuda.synchronize()
        finally:
            _vah.prof_enable(False)
            fused.ENABLED['fp16_rows'] = True
        rows = sorted(_vah.prof_report())
        grads = {k: p.grad.double() / 512. for k, p in enc.named_parameters() if p.grad is not None}
        res[mode] = (out.detach().float(), grads, rows)
    assert res['fp32'][2] == [] and res['fp16_off'][2] == []
    assert res['fp16'][2] == ['layernorm_bwd_f16', 'layernorm_fwd_f16'], res['fp16'][2]
    o32, g32, _ = res['fp32']
    for mode in ('fp16', 'fp16_off'):
        o, g, _ = res[mode]
        assert torch.isfinite(o).all()
        assert (o - o32).abs().max().item() <= 0.08 * max(1.0, o32.abs().max().item()), mode
        top = max(float(t.norm()) for t in g32.values())
        rels = sorted(float((g[k] - t).norm()) / float(t.norm()) for k, t in g32.items() if float(t.norm()) > 1e-5 * top)
        print('HOLD pixel decoder %s: %d gradients, median %.4f worst %.4f' % (mode, len(rels), float(np.median(rels)), rels[-1]))
        assert float(np.median(rels)) <= 0.08 and rels[-1] <= 0.25, (mode, float(np.median(rels)), rels[-1])
