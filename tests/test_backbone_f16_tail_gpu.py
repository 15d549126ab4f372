"""GPU: whole backbones under fp16 autocast + GradScaler(init_scale=512) with the output tail on the fp16 instantiations
of csrc/tail_ops.hip: the BatchNorm tail (norm1..norm3), the token <-> plane transposes, the sub-pixel interleave of
`up` (whose two products are torch's fp16 GEMMs) and, where the NHWC SpatialPriorModule does not take the image, the
BatchNorm + ReLU pairs and the NCHW max-pool of the module as written.

The rows of the families `bn_tail`, `transpose_tokens`, `pixel_shuffle2` and `maxpool` under fp16 autocast must be the
rows of the bf16-autocast run with `_f16` appended: same names, same call counts, and no bf16 row.  Against the same
module in fp32 the bounds are those of tests/test_backbone_f16_fused_gpu.py (this project's fp16 tier): outputs within
0.08 of the max, parameter gradients median relative L2 <= 0.08 and every one <= 0.25, with the two exclusions that file
documents (the stem below the max-pool; `sampling_offsets` of the one-head det_win_96x128 case at 1.0) and nothing else
left out.  With ENABLED['fp16_tail'] = False the same run launches none of the new rows (the fp32 token -> plane
transposes keep their unsuffixed row, as before the switch existed) and meets the same bounds against fp32 and against
the fused run.

Cases: those of tests/test_backbone_f16_spm_gpu.py (tiny_seg_512; det_win_96x128 and beit_seg_96 with
`conv_inplane=64`), one of them in eval mode.  beit_seg_96 has a 6 x 6 patch grid: its three tails are 24, 12 and 6
columns wide, none a multiple of 4 x scale, so under bf16 and fp16 alike fused.bn_tail and fused.up_from_tokens take the
reference expression there and the token -> plane transposes are the only rows of the four families; that case asks for
those.  `beit_seg_128` is the same configuration on a 128 x 128 image (8 x 8 grid; tails 32, 16 and 8 wide), where the
BEiT adapter's tail does run on the kernels.

The module as written (fused.bn_relu, fused.max_pool, fused.maps_to_tokens in their fp16 forms) runs where
spm_nhwc.usable() refuses.  An image whose sides are not multiples of 32 is such a refusal, but no whole backbone runs
on one: the SPM's stride-32 map is ceil(H / 32) rows while the pyramid assembly splits the tokens at H // 32, so the
token count does not add up.  Two cases between them cover it: det_win_96x128 as oracle/backbone_cases.py has it
(conv_inplane = 16: refused by usable() for its widths) through the whole backbone, and the SpatialPriorModule alone,
with the token layout, on an 80 x 128 image (refused for its height; every map width a multiple of 4, as bn_relu
needs).  bn_relu's size threshold is a tuning constant far above these maps; the tests lower it so that the kernels under
test run.

SyncBatchNorm: two processes on the one card over gloo run fused.bn_tail under fp16 autocast on half the batch each,
in the form of tests/test_bn_tail_sync_gpu.py; the children are started fresh, joined under a time limit, never retried."""
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import backbone_cases as bc
from oracle import seeded
from test_backbone_f16_spm_gpu import CASES, _beit, _free_port, _hold, _hold_outputs, _usable, _vit

pytestmark = pytest.mark.gpu

FAMILIES = ('bn_tail', 'transpose_tokens', 'pixel_shuffle2', 'maxpool')
TRAIN_ROWS = ('bn_tail_stats_f16', 'bn_tail_apply_f16', 'bn_tail_bwd_stats_f16', 'bn_tail_bwd_apply_f16', 'transpose_tokens_f16',
              'pixel_shuffle2_f16')
MODULE_ROWS = ('maxpool_fwd_f16', 'maxpool_bwd_f16')
F16, BF = torch.float16, torch.bfloat16


@pytest.fixture(scope='module', autouse=True)
def _fp32_math():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    yield


def _run(model, x, gouts, dtype, backward=True):
    """One forward + backward (dtype None: fp32) with the four families profiled -> (outputs, gradients, rows, gouts)."""
    import _vah
    model.zero_grad(set_to_none=True)
    opt = torch.optim.SGD(model.parameters(), lr=0.)
    amp = dtype is not None
    scaler = torch.amp.GradScaler('cuda', init_scale=512., enabled=dtype == F16)
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


def _ab(name, model, x, rows_wanted):
    """fp32, bf16 and fp16 runs, then fp16 with the switch off"""
    from vitadapter import fused
    outs32, grads32, rows32, gouts = _run(model, x, None, None)
    assert not any(r.endswith('_f16') for r in rows32), rows32
    _, _, rows_bf, _ = _run(model, x, gouts, BF)
    outs16, grads16, rows16, _ = _run(model, x, gouts, F16)
    print('ROWS %s bf16 %s' % (name, sorted(rows_bf.items())))
    print('ROWS %s fp16 %s' % (name, sorted(rows16.items())))
    assert rows_bf and not any(r.endswith('_f16') for r in rows_bf), rows_bf
    assert rows16 == {r + '_f16': n for r, n in rows_bf.items()}, (rows16, rows_bf)
    assert not any(r in rows16 for r in rows_bf), rows16                # no bf16 row of the four families under fp16
    for r in rows_wanted:
        assert rows16.get(r, 0) > 0, (r, rows16)
    _hold(name, outs16, grads16, outs32, grads32, 'fp16 tail vs fp32')

    fused.ENABLED['fp16_tail'] = False
    try:
        outs_off, grads_off, rows_off, _ = _run(model, x, gouts, F16)
    finally:
        fused.ENABLED['fp16_tail'] = True
    print('ROWS %s fp16, fp16_tail off %s' % (name, sorted(rows_off.items())))
    # the behaviour before the switch existed: only the fp32 token -> plane transposes are this library's
    assert set(rows_off) <= {'transpose_tokens'}, rows_off
    _hold(name, outs_off, grads_off, outs32, grads32, 'fp16_tail off vs fp32')
    # the two fp16 runs against each other, same bounds (the fused run as the reference)
    _hold(name, outs_off, grads_off, outs16, grads16, 'fp16_tail off vs fused')


def _beit_128():
    cfg = dict(bc.BEIT_CASES['beit_seg_96']['cfg'], img_size=128, conv_inplane=64)
    return _beit(cfg), seeded.randn('beit/beit_seg_128/x', (bc.BEIT_CASES['beit_seg_96']['batch'], 3, 128, 128), 13)


TAIL_CASES = dict(CASES, beit_seg_128=_beit_128)
# the tail kernels want widths in multiples of 4 x scale: beit_seg_96's 24 / 12 / 6 columns take the reference expression
ROWS_WANTED = {'beit_seg_96': ('transpose_tokens_f16',)}


@pytest.mark.parametrize('name', sorted(TAIL_CASES))
def test_backbone_fp16_tail_runs_on_the_fused_kernels(name):
    torch.manual_seed(0)
    model, x = TAIL_CASES[name]()
    model = model.cuda().train()
    x = x.cuda()
    assert _usable(model, x, BF) and _usable(model, x, F16)
    _ab(name, model, x, ROWS_WANTED.get(name, TRAIN_ROWS))


def test_backbone_fp16_tail_with_the_module_as_written(monkeypatch):
    """det_win_96x128 at its own conv_inplane = 16: usable() refuses, the SpatialPriorModule runs as written, with
    fused.bn_relu, fused.max_pool and fused.maps_to_tokens in their fp16 forms and c1 handed over without fc1's bias."""
    from vitadapter import fused
    monkeypatch.setattr(fused, 'BN_RELU_MIN_NUMEL', 1)
    name = 'det_win_96x128'
    torch.manual_seed(0)
    model, x = _vit(bc.FULL_CASES[name]['cfg']), bc.full_input(name)
    model = model.cuda().train()
    x = x.cuda()
    assert not _usable(model, x, BF) and not _usable(model, x, F16)
    with torch.autocast('cuda', dtype=F16):
        assert fused.tail_takes_conv_bias(model.norm1, x)
    _ab(name, model, x, TRAIN_ROWS + MODULE_ROWS)


def test_spm_as_written_fp16_on_an_image_usable_refuses(monkeypatch):
    """80 x 128: a height that is a multiple of 16 only.  The module as written under fp16 autocast - six bn_relu, the
    max-pool, the token layout - launches the `_f16` rows the bf16 run launches and agrees with the fp32 module."""
    import _vah
    from vitadapter import fused, spm_nhwc
    from vitadapter.backbones.adapter_modules import SpatialPriorModule
    monkeypatch.setattr(fused, 'BN_RELU_MIN_NUMEL', 1)
    torch.manual_seed(3)
    E = 64
    spm = SpatialPriorModule(inplanes=64, embed_dim=E).cuda().train()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 80, 128, generator=g).cuda()
    vecs = [torch.randn(E, generator=g).cuda() for _ in range(3)]

    def run(dtype):
        spm.zero_grad(set_to_none=True)
        _vah.prof_enable(True, ','.join(FAMILIES))
        try:
            with torch.autocast('cuda', dtype=dtype, enabled=dtype is not None):
                assert not spm_nhwc.usable(spm, x)
                c1, m2, m3, m4 = spm(x, bias_free_c1=dtype is not None, raw_maps=True)
                c = fused.maps_to_tokens([m2, m3, m4], vecs)
            gg = torch.Generator(device='cuda').manual_seed(5)
            loss = (c1.float() * torch.randn(c1.shape, device='cuda', generator=gg)).mean() + \
                (c * torch.randn(c.shape, device='cuda', generator=gg)).mean()
            (loss * 512.).backward()
            torch.cuda.synchronize()
        finally:
            _vah.prof_enable(False)
        rows = {k: r['calls'] for k, r in _vah.prof_report().items()}
        grads = {k: p.grad.double() / 512. for k, p in spm.named_parameters() if p.grad is not None}
        return [c1.detach().float(), c.detach()], grads, rows, (m2.dtype, c1.dtype)

    outs32, grads32, _, _ = run(None)
    outs32[0] = outs32[0] - spm.fc1.bias.detach().view(1, -1, 1, 1)          # the 16-bit runs hand c1 over without the bias
    _, _, rows_bf, _ = run(BF)
    outs16, grads16, rows16, dts = run(F16)
    print('ROWS spm 80x128 bf16 %s' % sorted(rows_bf.items()))
    print('ROWS spm 80x128 fp16 %s' % sorted(rows16.items()))
    assert dts == (F16, F16)
    assert rows16 == {r + '_f16': n for r, n in rows_bf.items()}, (rows16, rows_bf)
    assert rows16 == {'bn_tail_stats_f16': 6, 'bn_tail_apply_f16': 6, 'bn_tail_bwd_stats_f16': 6, 'bn_tail_bwd_apply_f16': 6,
                      'maxpool_fwd_f16': 1, 'maxpool_bwd_f16': 1, 'transpose_tokens_f16': 6}, rows16
    _hold_outputs(outs16, outs32, 'SPM as written, fp16 vs fp32')
    top = max(float(g.norm()) for g in grads32.values())
    errs = {k: float((grads16[k] - g).norm()) / float(g.norm()) for k, g in grads32.items()
            if not k.startswith('stem') and k != 'fc1.bias' and float(g.norm()) > 1e-5 * top}
    rels = sorted(errs.values())
    print('HOLD spm 80x128: %d gradients, median %.4f worst %.4f' % (len(rels), float(np.median(rels)), rels[-1]))
    assert len(rels) >= 10 and float(np.median(rels)) <= 0.08 and rels[-1] <= 0.25, sorted(errs.items(), key=lambda kv: -kv[1])[:3]


def test_backbone_fp16_tail_eval_mode():
    """Running statistics: the three tails are one apply pass each, no statistics pass runs, nothing is tracked; outputs
    against the fp32 eval run."""
    name = 'det_win_96x128'
    torch.manual_seed(0)
    model, x = CASES[name]()
    model = model.cuda().eval()
    x = x.cuda()
    tracked = model.norm1.num_batches_tracked.clone()
    with torch.no_grad():
        outs32, _, rows32, gouts = _run(model, x, None, None, backward=False)
        _, _, rows_bf, _ = _run(model, x, gouts, BF, backward=False)
        outs16, _, rows16, _ = _run(model, x, gouts, F16, backward=False)
    print('ROWS %s eval fp16 %s' % (name, sorted(rows16.items())))
    assert not any(r.endswith('_f16') for r in rows32)
    assert rows16 == {r + '_f16': n for r, n in rows_bf.items()}, (rows16, rows_bf)
    assert rows16.get('bn_tail_apply_f16') == 3 and rows16.get('pixel_shuffle2_f16') == 1 and rows16.get('transpose_tokens_f16', 0) > 0
    assert not any('stats' in r for r in rows16), rows16
    assert torch.equal(model.norm1.num_batches_tracked, tracked)
    _hold_outputs(outs16, outs32, 'eval fp16 tail vs fp32')


# ---------------------------------------------------------------- SyncBatchNorm, two ranks
SYNC_SHAPE = (4, 12, 32, 32, 4)


def _sync_make(seed, N, C, H, W, scale):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(N, C, H, W, generator=g).to(F16)
    b = (torch.randn(N, C, H, W, generator=g) + 0.3).to(F16)
    x = torch.randn(N, C, H // scale, W // scale, generator=g)
    dy = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(C, generator=g) * 0.3 + 1
    bias = torch.randn(C, generator=g) * 0.3
    return a, b, x, dy, w, bias


def _sync_worker(rank, world, port, shape, out_path):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'vit-adapter_amd'))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import _vah
        from vitadapter import fused
        N, C, H, W, scale = shape
        a, b, x, dy, w, bias = (t.cuda() for t in _sync_make(11, N, C, H, W, scale))
        per = N // world
        sl = slice(rank * per, (rank + 1) * per)
        bn = torch.nn.SyncBatchNorm(C).cuda().train()
        with torch.no_grad():
            bn.weight.copy_(w)
            bn.bias.copy_(bias)
        al, bl, xl = (t[sl].clone().requires_grad_(True) for t in (a, b, x))
        _vah.prof_enable(True, 'bn_tail')
        with torch.autocast('cuda', dtype=torch.float16):
            y = fused.bn_tail(bn, al, bl, xl, scale)
        assert type(y.grad_fn).__name__ == '_BNTailBackward', 'fused path not taken'
        y.backward(dy[sl])
        torch.cuda.synchronize()
        _vah.prof_enable(False)
        rows = sorted(_vah.prof_report())
        assert rows == ['bn_tail_apply_f16', 'bn_tail_bwd_apply_f16', 'bn_tail_bwd_stats_f16', 'bn_tail_stats_f16'], rows
        assert al.grad.dtype == torch.float16 and bl.grad.dtype == torch.float16 and y.dtype == torch.float32
        torch.save(dict(y=y.detach().cpu(), da=al.grad.float().cpu(), db=bl.grad.float().cpu(), dx=xl.grad.cpu(),
                        dw=bn.weight.grad.cpu(), dbias=bn.bias.grad.cpu(), rm=bn.running_mean.cpu(),
                        rv=bn.running_var.cpu()), out_path % rank)
    finally:
        dist.destroy_process_group()


def test_bn_tail_fp16_syncbn_two_ranks(tmp_path):
    """Every rank's output and gradients equal those of one process running plain BatchNorm in fp32 over the whole batch on
    the same fp16 operands.  Tolerances: tests/test_bn_tail_sync_gpu.py's for the fp32 results (y, dx, running statistics,
    d weight, d bias: the operands are upcast exactly); da / db are rounded once to fp16: 2^-11 of the value, held to
    2^-10 of the tensor's largest."""
    import torch.multiprocessing as mp
    world = 2
    out_path = str(tmp_path / 'rank%d.pt')
    port = _free_port()
    ctx = mp.get_context('spawn')
    children = []
    for r in range(world):
        p = ctx.Process(target=_sync_worker, args=(r, world, port, SYNC_SHAPE, out_path))
        p.start()
        children.append((p, time.monotonic() + 120.))          # each child's own time limit, from its own start
    try:
        for r, (p, deadline) in enumerate(children):
            p.join(max(0., deadline - time.monotonic()))
            assert not p.is_alive(), 'rank %d did not finish within its time limit' % r
            assert p.exitcode == 0, 'rank %d ended with exit code %r' % (r, p.exitcode)
    finally:
        for p, _ in children:
            if p.is_alive():
                p.kill()
            p.join(10.)
    N, C, H, W, scale = SYNC_SHAPE
    a, b, x, dy, w, bias = _sync_make(11, N, C, H, W, scale)
    a2, b2, x2 = (t.float().requires_grad_(True) for t in (a, b, x))
    bn = torch.nn.BatchNorm2d(C).train()
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(bias)
    y = bn(a2 + b2 + F.interpolate(x2, scale_factor=scale, mode='bilinear', align_corners=False))
    y.backward(dy)
    per = N // world
    dw = torch.zeros(C)
    dbias = torch.zeros(C)
    for r in range(world):
        got = torch.load(out_path % r, weights_only=True)
        sl = slice(r * per, (r + 1) * per)
        for name, ref, tol in (('y', y.detach()[sl], 3e-5), ('da', a2.grad[sl], 2.0 ** -10), ('db', b2.grad[sl], 2.0 ** -10),
                               ('dx', x2.grad[sl], 1e-4), ('rm', bn.running_mean, 1e-5), ('rv', bn.running_var, 1e-5)):
            err = (got[name] - ref).abs().max().item()
            assert err <= tol * max(1.0, ref.abs().max().item()), (r, name, err)
        dw += got['dw']
        dbias += got['dbias']
    # weight / bias gradients are per-rank sums (DDP averages them afterwards)
    assert (dw - bn.weight.grad).abs().max().item() <= 1e-3 * bn.weight.grad.abs().max().item()
    assert (dbias - bn.bias.grad).abs().max().item() <= 1e-3 * max(1.0, bn.bias.grad.abs().max().item())
