"""GPU: whole backbones under fp16 autocast + GradScaler(init_scale=512) with the SpatialPriorModule on the fp16
instantiations of the NHWC convolution / BatchNorm / max-pool kernels (csrc/conv.hip, csrc/spm_nhwc.hip).

The rows of the families `conv_` and `spm_` under fp16 autocast must be the rows of the bf16-autocast run with the type
suffix swapped (`conv_taps_bf16` -> `conv_taps_f16`, `spm_bn_stats` -> `spm_bn_stats_f16`): same names, same call
counts, and no bf16 row.  Against the same module in fp32 the bounds are those of tests/test_backbone_f16_fused_gpu.py
(this project's fp16 tier): outputs within 0.08 of the max, parameter gradients median relative L2 <= 0.08 and every
one <= 0.25, with the two exclusions that file documents (the stem below the max-pool; `sampling_offsets` of the
one-head det_win_96x128 case at 1.0) and nothing else left out.  With ENABLED['fp16_spm'] = False the same run launches
none of the new rows and meets the same bounds against fp32 and against the fused run.

Cases: those of tests/test_backbone_f16_fused_gpu.py.  tiny_seg_512 (oracle/backbone_cases.py, conv_inplane 64) is
usable() as it stands.  The two small cases build their SPM with conv_inplane = 16, which the NHWC kernels do not take
(output channels in multiples of 64) and no configuration of the reference uses; oracle/backbone_cases.py has no small
case at the reference's width, so here they are built with `conv_inplane=64` and everything else - trunk, windows, heads,
input, seeds - as the file has it (`_wide`).  Every input is a multiple of 32 in both directions; usable() is asserted
in each test under both autocast types.  Two single-case tests: eval mode
(running statistics: no statistics pass), and two processes on the one card sharing the SyncBatchNorm sums over gloo."""
import os
import socket

import numpy as np
import pytest
import torch

from oracle import backbone_cases as bc
from oracle import seeded

pytestmark = pytest.mark.gpu

FAMILIES = ('conv_', 'spm_')
TRAIN_ROWS = ('conv_taps_f16', 'conv_dgrad_f16', 'conv_wgrad_f16', 'spm_image_to_nhwc_f16', 'spm_bn_stats_f16', 'spm_bn_apply_f16',
              'spm_bn_bwd_stats_f16', 'spm_bn_bwd_apply_f16', 'spm_maxpool_fwd_f16', 'spm_maxpool_bwd_f16')


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


def _wide(cfg):
    """the case's configuration with the SPM at the reference's width (every published config: conv_inplane=64)"""
    assert cfg['conv_inplane'] == 16
    return dict(cfg, conv_inplane=64)


CASES = {
    'tiny_seg_512': lambda: (_vit(bc.FULLSIZE_CASES['tiny_seg_512']['cfg']), bc.fullsize_input('tiny_seg_512')),
    'det_win_96x128': lambda: (_vit(_wide(bc.FULL_CASES['det_win_96x128']['cfg'])), bc.full_input('det_win_96x128')),
    'beit_seg_96': lambda: (_beit(_wide(bc.BEIT_CASES['beit_seg_96']['cfg'])), bc.beit_input('beit_seg_96')),
}


def _f16_name(row):
    return row[:-len('_bf16')] + '_f16' if row.endswith('_bf16') else row + '_f16'


def _usable(model, x, dtype):
    from vitadapter import spm_nhwc
    with torch.autocast('cuda', dtype=dtype):
        return spm_nhwc.usable(model.spm, x)


def _run(model, x, gouts, dtype, backward=True):
    """One forward + backward (dtype None: fp32) with the two families profiled -> (outputs, gradients, rows, gouts)."""
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
        if backward:
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


def _hold_outputs(outs, outs32, what):
    for o16, o32 in zip(outs, outs32):
        assert torch.isfinite(o16).all(), what
        assert (o16 - o32).abs().max().item() <= 0.08 * max(1.0, o32.abs().max().item()), what


def _hold(name, outs, grads, outs32, grads32, what):
    _hold_outputs(outs, outs32, what)
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
def test_backbone_fp16_spm_runs_on_the_nhwc_kernels(name):
    from vitadapter import fused
    torch.manual_seed(0)
    model, x = CASES[name]()
    model = model.cuda().train()
    x = x.cuda()
    assert x.shape[2] % 32 == 0 and x.shape[3] % 32 == 0
    assert _usable(model, x, torch.bfloat16) and _usable(model, x, torch.float16)
    outs32, grads32, rows32, gouts = _run(model, x, None, None)
    assert rows32 == {}, rows32                         # fp32: torch's module
    _, _, rows_bf, _ = _run(model, x, gouts, torch.bfloat16)
    outs16, grads16, rows16, _ = _run(model, x, gouts, torch.float16)
    print('ROWS %s bf16 %s' % (name, sorted(rows_bf.items())))
    print('ROWS %s fp16 %s' % (name, sorted(rows16.items())))
    assert rows_bf and not any(r.endswith('_f16') for r in rows_bf), rows_bf
    assert rows16 == {_f16_name(r): n for r, n in rows_bf.items()}, (rows16, rows_bf)
    assert not any(r in rows16 for r in rows_bf), rows16                # no bf16 conv / spm row under fp16
    for r in TRAIN_ROWS:
        assert rows16.get(r, 0) > 0, (r, rows16)
    _hold(name, outs16, grads16, outs32, grads32, 'fp16 NHWC SPM vs fp32')

    fused.ENABLED['fp16_spm'] = False
    try:
        assert not _usable(model, x, torch.float16) and _usable(model, x, torch.bfloat16)
        outs_off, grads_off, rows_off, _ = _run(model, x, gouts, torch.float16)
    finally:
        fused.ENABLED['fp16_spm'] = True
    assert rows_off == {}, rows_off
    _hold(name, outs_off, grads_off, outs32, grads32, 'fp16_spm off vs fp32')
    # the two fp16 runs against each other, same bounds (the NHWC run as the reference)
    _hold(name, outs_off, grads_off, outs16, grads16, 'fp16_spm off vs NHWC')


def test_backbone_fp16_spm_eval_mode():
    """Running statistics: the BatchNorm apply kernels take mean / rstd from the module's buffers, no statistics pass
    runs, nothing is tracked; outputs against the fp32 eval run."""
    name = 'det_win_96x128'
    torch.manual_seed(0)
    model, x = CASES[name]()
    model = model.cuda().eval()
    x = x.cuda()
    assert _usable(model, x, torch.float16)
    tracked = model.spm.stem[1].num_batches_tracked.clone()
    with torch.no_grad():
        outs32, _, rows32, gouts = _run(model, x, None, None, backward=False)
        outs16, _, rows16, _ = _run(model, x, gouts, torch.float16, backward=False)
    print('ROWS %s eval fp16 %s' % (name, sorted(rows16.items())))
    assert rows32 == {}
    assert rows16 == {'spm_image_to_nhwc_f16': 1, 'conv_taps_f16': 6, 'spm_bn_apply_f16': 6, 'spm_maxpool_fwd_f16': 1}, rows16
    assert torch.equal(model.spm.stem[1].num_batches_tracked, tracked)
    _hold_outputs(outs16, outs32, 'eval fp16 NHWC SPM vs fp32')


# ---------------------------------------------------------------- SyncBatchNorm, two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


SYNC_SHAPE = (4, 128, 128, 64)           # batch (both ranks), H, W, embed_dim


def _sync_make():
    from vitadapter.backbones.adapter_modules import SpatialPriorModule
    N, H, W, E = SYNC_SHAPE
    torch.manual_seed(3)
    spm = SpatialPriorModule(inplanes=64, embed_dim=E)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, 3, H, W, generator=g)
    g1 = torch.randn(N, E, H // 4, W // 4, generator=g)
    gc = torch.randn(N, (H // 8) * (W // 8) + (H // 16) * (W // 16) + (H // 32) * (W // 32), E, generator=g)
    return spm, x, g1, gc


def _sync_loss(c1, c, g1, gc, total):
    # each rank's share of one mean over the whole batch, times the loss scale
    return ((c1.float() * g1).sum() + (c.float() * gc).sum()) / total * 512.


def _sync_worker(rank, world, port, out_path):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'vit-adapter_amd'))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from vitadapter import spm_nhwc
        spm, x, g1, gc = _sync_make()
        spm = spm.cuda().train()
        per = x.shape[0] // world
        sl = slice(rank * per, (rank + 1) * per)
        xl, g1l, gcl = (t[sl].cuda() for t in (x, g1, gc))
        level = torch.zeros(3, SYNC_SHAPE[3], device='cuda')
        with torch.autocast('cuda', dtype=torch.float16):
            assert spm_nhwc.usable(spm, xl)
            c1, c = spm_nhwc.forward(spm, xl, level, c1_bias=True)
        assert c1.dtype == torch.float16 and c.dtype == torch.float32
        _sync_loss(c1, c, g1l, gcl, g1.numel() + gc.numel()).backward()
        torch.cuda.synchronize()
        torch.save(dict(c1=c1.detach().float().cpu(), c=c.detach().cpu(),
                        grads={k: (p.grad.float() / 512.).cpu() for k, p in spm.named_parameters() if p.grad is not None},
                        stats={k: b.float().cpu() for k, b in spm.named_buffers() if 'running_' in k}), out_path % rank)
    finally:
        dist.destroy_process_group()


def test_spm_fp16_syncbn_two_ranks(tmp_path):
    """Each rank runs half the batch through spm_nhwc.forward under fp16 autocast; the BatchNorm sums are all-reduced
    (fp32, as under bf16).  Outputs, running statistics and the rank-summed parameter gradients against ONE process
    running the module in fp32 over the whole batch.  Running statistics are the sharp check on the all-reduce: at 4 x 4
    pixels x 2 images per rank the local statistics of conv4 are far from the batch's; they must also be the same bits
    on both ranks.  Bounds: the fp16 tier's (outputs 0.08 of the max, gradients median 0.08 / worst 0.25 relative L2,
    the stem below the max-pool left out); running statistics to 2^-8 of their largest value (fp16 activations: 2^-11
    per element, averaged; the bound leaves a factor 8)."""
    import torch.multiprocessing as mp
    world = 2
    out_path = str(tmp_path / 'rank%d.pt')
    mp.spawn(_sync_worker, args=(world, _free_port(), out_path), nprocs=world, join=True)
    spm, x, g1, gc = _sync_make()
    spm = spm.cuda().train()
    xc, g1c, gcc = x.cuda(), g1.cuda(), gc.cuda()
    c1, c2, c3, c4 = spm(xc)
    c = torch.cat([c2, c3, c4], dim=1)
    (_sync_loss(c1, c, g1c, gcc, g1.numel() + gc.numel()) / 512.).backward()
    ref_grads = {k: p.grad.double().cpu() for k, p in spm.named_parameters() if p.grad is not None}
    ref_stats = {k: b.float().cpu() for k, b in spm.named_buffers() if 'running_' in k}
    got = [torch.load(out_path % r, weights_only=True) for r in range(world)]
    per = x.shape[0] // world
    for r in range(world):
        sl = slice(r * per, (r + 1) * per)
        _hold_outputs([got[r]['c1'], got[r]['c']], [c1.detach()[sl].cpu(), c.detach()[sl].cpu()], 'rank %d outputs' % r)
        assert set(got[r]['stats']) == set(ref_stats) and len(ref_stats) == 12
        for k, ref in ref_stats.items():
            assert torch.equal(got[r]['stats'][k], got[0]['stats'][k]), (r, k)
            err = (got[r]['stats'][k] - ref).abs().max().item()
            assert err <= 2.0 ** -8 * max(1.0, ref.abs().max().item()), (r, k, err)
    assert set(got[0]['grads']) == set(ref_grads)
    top = max(float(g.norm()) for g in ref_grads.values())
    errs = {k: float((sum(got[r]['grads'][k].double() for r in range(world)) - g).norm()) / float(g.norm())
            for k, g in ref_grads.items() if not k.startswith('stem') and float(g.norm()) > 1e-5 * top}
    rels = sorted(errs.values())
    print('HOLD syncbn two ranks: %d gradients, median %.4f worst %.4f' % (len(rels), float(np.median(rels)), rels[-1]))
    assert len(rels) >= 10 and float(np.median(rels)) <= 0.08 and rels[-1] <= 0.25, sorted(errs.items(), key=lambda kv: -kv[1])[:3]
