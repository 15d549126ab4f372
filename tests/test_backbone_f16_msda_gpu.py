"""GPU: whole backbones under fp16 autocast with a GradScaler at init_scale 512 (how the reference trains every published
model), with the deformable attention on the fp16 instantiation of the fused MSDA kernels: the `msda_fused_fwd_f16` /
`msda_fused_bwd_f16` profiler rows are there, and neither the unfused fp32 rows the reference's autocast cast used to force
(`msda_fwd_f32`, `msda_bwd_f32`) nor a bf16 row.

The models and the bounds are those of tests/test_backbone_f16_gpu.py, against the same module in fp32: outputs within
0.08 of the max, parameter gradients median relative L2 <= 0.08 and every one <= 0.25; the sampling_offsets gradients of
the one-head det case (sums over a few hundred bilinear samples on a 6 x 8 map) <= 1.0."""
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


def _vit(name):
    from vitadapter.backbones import ViTAdapter
    m = ViTAdapter(**bc.FULL_CASES[name]['cfg'])
    m.load_state_dict(seeded.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 5))
    return m, bc.full_input(name)


MSDA_ROWS = ('msda_fused_fwd_f16', 'msda_fused_bwd_f16')


# det_win_96x128: det flavour, ONE deformable head, 6 x 8 token grid, batch 1; seg_glob_64: seg flavour, two heads, batch 2
@pytest.mark.parametrize('name', ['det_win_96x128', 'seg_glob_64'])
def test_backbone_fp16_autocast_runs_the_fused_fp16_msda(name):
    import _vah
    from vitadapter import fused
    assert fused.ENABLED['fp16_msda']
    torch.manual_seed(0)
    model, x = _vit(name)
    model = model.cuda().train()
    x = x.cuda()
    opt = torch.optim.SGD(model.parameters(), lr=0.)
    outs, grads, gouts = {}, {}, None
    for amp in (False, True):
        model.zero_grad(set_to_none=True)
        scaler = torch.amp.GradScaler('cuda', init_scale=512., enabled=amp)
        if amp:
            _vah.prof_enable(True, 'msda_')
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
    for r in MSDA_ROWS:
        assert rows.get(r, {}).get('calls', 0) > 0, (r, sorted(rows))
    assert rows['msda_fused_fwd_f16']['calls'] == rows['msda_fused_bwd_f16']['calls']
    assert 'msda_fwd_f32' not in rows and 'msda_bwd_f32' not in rows, sorted(rows)
    assert not any(r.endswith('_bf16') or r in ('msda_fused_fwd', 'msda_fused_bwd') for r in rows), sorted(rows)

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
        loose = [k for k in errs if 'sampling_offsets' in k]
        assert loose
        print('FIGURE %s sampling_offsets: worst %.3f' % (name, max(errs[k] for k in loose)))
        assert all(errs[k] <= 1.0 for k in loose), [(k, errs[k]) for k in loose]
        errs = {k: e for k, e in errs.items() if k not in loose}
    rels = sorted(errs.values())
    print('FIGURE %s parameter gradients: %d, median %.4f worst %.4f' % (name, len(rels), float(np.median(rels)), rels[-1]))
    assert len(rels) > 20 and float(np.median(rels)) <= 0.08 and rels[-1] <= 0.25, (
        len(rels), float(np.median(rels)), sorted(errs.items(), key=lambda kv: -kv[1])[:3])
