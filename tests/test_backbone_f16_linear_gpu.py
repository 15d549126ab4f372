"""GPU: whole backbones under fp16 autocast + GradScaler(init_scale=512) with the Linear layers on the GEMM dispatcher
(csrc/gemm.hip: vah_gemm_f16 / vah_gemm_f16_fin) and their satellites on the fp16 kernels of csrc/fused_ops.hip.

The cases and bounds are those of tests/test_backbone_f16_fused_gpu.py: against the same module in fp32, outputs within
0.08 of the max, parameter gradients median relative L2 <= 0.08 and every one <= 0.25, with that file's two documented
exclusions (the stem below the max-pool; `sampling_offsets` of the one-head det_win_96x128 case at 1.0) and no others;
every gradient finite.  With ENABLED['fp16_linear'] = False the same run launches none of the new rows (the Linears are
torch's library calls) and stays within the same bounds.  Nothing tunes live: the dispatcher runs in mode 0 here."""
import os

import numpy as np
import pytest
import torch

from oracle import backbone_cases as bc
from oracle import seeded

pytestmark = pytest.mark.gpu

FILTER = 'gemm_,gelu_bwd,colsum_bf16,colsum_f16'
NEW_ROWS = ('gemm_nt_f16', 'gemm_nn_f16', 'gemm_tn_fin_f16')


@pytest.fixture(scope='module', autouse=True)
def _fp32_math_no_live_tuning():
    import _vah
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    _vah.check(_vah.lib.vah_gemm_set_tuning(0, 32), 'gemm_set_tuning')
    yield
    spec = [int(t) for t in os.environ.get('VAH_GEMM_TUNING', '1,32').split(',')]
    _vah.check(_vah.lib.vah_gemm_set_tuning(spec[0], spec[1] if len(spec) > 1 else 32), 'gemm_set_tuning')


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


# the trunk MLP of the BEiT flavour has no exact-GELU between two marked Linears in every configuration: gelu_bwd_f16 is
# required where the bf16 run of the same model launches gelu_bwd
CASES = {
    'tiny_seg_512': lambda: (_vit(bc.FULLSIZE_CASES['tiny_seg_512']['cfg']), bc.fullsize_input('tiny_seg_512')),
    'det_win_96x128': lambda: (_vit(bc.FULL_CASES['det_win_96x128']['cfg']), bc.full_input('det_win_96x128')),
    'beit_seg_96': lambda: (_beit(bc.BEIT_CASES['beit_seg_96']['cfg']), bc.beit_input('beit_seg_96')),
}


def _run(model, x, gouts, dtype):
    """One forward + backward (dtype None: fp32) with the Linear families profiled -> (outputs, gradients, rows, gouts)."""
    import _vah
    model.zero_grad(set_to_none=True)
    opt = torch.optim.SGD(model.parameters(), lr=0.)
    amp = dtype is not None
    scaler = torch.amp.GradScaler('cuda', init_scale=512., enabled=dtype == torch.float16)
    _vah.prof_enable(True, FILTER)
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
def test_backbone_fp16_linears_run_on_the_dispatcher(name):
    from vitadapter import fused
    torch.manual_seed(0)
    model, x = CASES[name]()
    model = model.cuda().train()
    x = x.cuda()
    outs32, grads32, _, gouts = _run(model, x, None, None)
    _, _, rows_bf, _ = _run(model, x, gouts, torch.bfloat16)
    outs16, grads16, rows16, _ = _run(model, x, gouts, torch.float16)
    print('ROWS %s bf16 %s' % (name, sorted(rows_bf.items())))
    print('ROWS %s fp16 %s' % (name, sorted(rows16.items())))
    for r in NEW_ROWS + (('gelu_bwd_f16',) if 'gelu_bwd' in rows_bf else ()):
        assert rows16.get(r, 0) > 0, (r, rows16)
    assert not [r for r in rows16 if not r.endswith('_f16')], rows16
    _hold(name, outs16, grads16, outs32, grads32, 'fp16 Linears on the dispatcher vs fp32')

    fused.ENABLED['fp16_linear'] = False
    try:
        outs_off, grads_off, rows_off, _ = _run(model, x, gouts, torch.float16)
    finally:
        fused.ENABLED['fp16_linear'] = True
    assert not [r for r in rows_off if r.endswith('_f16')], rows_off
    assert rows_off == {}, rows_off
    _hold(name, outs_off, grads_off, outs32, grads32, 'fp16_linear off vs fp32')
