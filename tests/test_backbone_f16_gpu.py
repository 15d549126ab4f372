"""GPU: whole backbones under fp16 autocast with a GradScaler at init_scale 512 - how the reference trains every published
model (`fp16 = dict(loss_scale=dict(init_scale=512))` in its configs).  Every ViT / BEiT attention of the blocks runs on
the fp16 MFMA kernels (the _f16 profiler rows, no bf16 row); the rest takes torch's own fp16 path (LayerNorm, Linear,
SPM convolutions) or, for MSDA, the fp32 kernels the reference's autocast cast forces.

Against the same module in fp32: outputs within 0.08 of the max, parameter gradients median relative L2 <= 0.08 and every
one <= 0.25 - the bf16 tier's bounds (tests/test_backbone_gpu.py, tests/test_beit_adapter.py)."""
import numpy as np
import pytest
import torch

from oracle import backbone_cases as bc
from oracle import seeded

pytestmark = pytest.mark.gpu


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


def _tiny_seg_512():
    c = bc.FULLSIZE_CASES['tiny_seg_512']
    return _vit(c['cfg']), bc.fullsize_input('tiny_seg_512')


def _det_win_96x128():
    return _vit(bc.FULL_CASES['det_win_96x128']['cfg']), bc.full_input('det_win_96x128')


def _beit_seg_96():
    return _beit(bc.BEIT_CASES['beit_seg_96']['cfg']), bc.beit_input('beit_seg_96')


GLOBAL_ROWS = ('attn_fwd_f16', 'attn_bwd_dq_f16', 'attn_bwd_dkdv_f16')
CASES = {
    # ViT-Adapter-T seg (configs/ade20k upernet_deit_adapter_tiny_512), 512 x 512, batch 2: 1024-token global attention
    'tiny_seg_512': (_tiny_seg_512, GLOBAL_ROWS),
    # det flavour, 14 x 14 windows on a 6 x 8 token grid (padded windows) and global blocks
    'det_win_96x128': (_det_win_96x128, GLOBAL_ROWS + ('attn_win_fwd_f16', 'attn_win_bwd_f16')),
    # BEiT-Adapter seg: class token + relative position bias table in every block
    'beit_seg_96': (_beit_seg_96, ('attn_bias_fwd_f16', 'attn_bias_bwd_f16', 'attn_bwd_dq_f16', 'attn_bwd_dkdv_f16')),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_backbone_fp16_autocast_with_grad_scaler(name):
    import _vah
    make, rows_expected = CASES[name]
    torch.manual_seed(0)
    model, x = make()
    model = model.cuda().train()
    x = x.cuda()
    opt = torch.optim.SGD(model.parameters(), lr=0.)
    outs, grads, gouts = {}, {}, None
    for amp in (False, True):
        model.zero_grad(set_to_none=True)
        scaler = torch.amp.GradScaler('cuda', init_scale=512., enabled=amp)
        if amp:
            _vah.prof_enable(True, 'attn_')
        try:
            with torch.autocast('cuda', dtype=torch.float16, enabled=amp):
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
        outs[amp] = [t.detach().float() for t in o]
        grads[amp] = {k: p.grad.detach().double().clone() for k, p in model.named_parameters() if p.grad is not None}

    rows = _vah.prof_report()
    for r in rows_expected:
        assert rows.get(r, {}).get('calls', 0) > 0, (r, sorted(rows))
    assert not any(r.endswith('_bf16') for r in rows), sorted(rows)

    for o16, o32 in zip(outs[True], outs[False]):
        assert torch.isfinite(o16).all()
        assert (o16 - o32).abs().max().item() <= 0.08 * max(1.0, o32.abs().max().item())
    assert set(grads[True]) == set(grads[False])
    assert not [k for k, g in grads[True].items() if not bool(torch.isfinite(g).all())]
    # as the bf16 tier: the stem below the max-pool (arg-max flips) and exact-zero gradients (a bias in front of a
    # BatchNorm) are left out
    top = max(float(g.norm()) for g in grads[False].values())
    errs = {k: float((grads[True][k] - g).norm()) / float(g.norm()) for k, g in grads[False].items()
            if not k.startswith('spm.stem') and float(g.norm()) > 1e-5 * top}
    if name == 'det_win_96x128':
        # one deformable head on a 6 x 8 map, batch 1: its sampling_offsets gradients are sums over a few hundred
        # bilinear samples, held to the bf16 tier's 1.0 (test_vit_adapter_bf16_autocast_vs_reference_goldens)
        loose = [k for k in errs if 'sampling_offsets' in k]
        assert all(errs[k] <= 1.0 for k in loose), [(k, errs[k]) for k in loose]
        errs = {k: e for k, e in errs.items() if k not in loose}
    rels = sorted(errs.values())
    assert len(rels) > 20 and float(np.median(rels)) <= 0.08 and rels[-1] <= 0.25, (
        len(rels), float(np.median(rels)), sorted(errs.items(), key=lambda kv: -kv[1])[:3])
