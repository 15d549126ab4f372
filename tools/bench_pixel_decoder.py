#!/usr/bin/env python
"""GroupNorm and bilinear-resize kernels and the whole MSDeformAttnPixelDecoder at the shapes of BASELINE configs[4] (one 800 x 1344 image:
maps 200 x 336 .. 25 x 42, 256 channels, 32 groups), bf16 autocast.  Needs the GPU.

    python tools/bench_pixel_decoder.py [--reps 20] [--warmup 5] [--sections group_norm,resize,decoder]

Prints, after a warm-up, with device events, the two sides alternating inside this process:
  1. per GroupNorm kernel (profile rows gn_*; the event pair the library puts around each entry point's launches, so a
     statistics row holds both of its launches): median / min / max time over the repetitions, the algorithmic bytes the
     launch accounts for, and their rate as a fraction of 6.3 TB/s;
  2. the same tensors through torch.nn.functional.group_norm forward + backward in the form a torch user has today (NCHW,
     fp32 under autocast: the 16-bit map is cast up, the result cast down), against fused.group_norm forward + backward
     on the channels-last rows;
  3. the FPN tail's upsample, 100 x 168 -> 200 x 336 from the strided fp32 level of an (Lq, 1, 256) buffer to bf16 rows:
     fused.resize_bilinear_rows forward + backward against the expression it replaces (F.interpolate on the NCHW-shaped
     fp32 view, then .to(bf16), with its autograd backward), and the profile rows resize_rows_fwd / resize_rows_bwd;
  4. the whole decoder's forward + backward with ENABLED['group_norm'], then ENABLED['bilinear_rows'], on and off.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'vit-adapter_amd'))

import _vah                                                  # noqa: E402
from vitadapter import fused                                 # noqa: E402
from vitadapter.pixel_decoder import MSDeformAttnPixelDecoder  # noqa: E402

PEAK = 6.3e12
SIZES = ((200, 336), (100, 168), (50, 84), (25, 42))
C, G = 256, 32


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(v):
    return '%8.3f ms median (min %.3f, max %.3f, n %d)' % (statistics.median(v), min(v), max(v), len(v))


def alternate(sides, reps, warmup):
    """{name: fn} -> {name: [ms]}, the sides taking turns"""
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            out[k].append(timed(fn))
    return out


def resize_section(args, gen):
    dev = 'cuda'
    (hi, wi), (ho, wo) = SIZES[1], SIZES[0]
    lq = sum(h * w for h, w in SIZES[1:])
    memory = torch.randn(lq, 1, C, device=dev, generator=gen).requires_grad_(True)        # the encoder's (Lq, N, C) buffer, fp32
    start = lq - hi * wi                                                                  # its finest level comes last
    dy = torch.randn(1, ho * wo, C, device=dev, generator=gen).to(torch.bfloat16)
    print('== bilinear resize %d x %d -> %d x %d, %d channels, strided fp32 level -> bf16 rows, forward + backward ==' % (hi, wi, ho, wo, C))

    def kernels():
        memory.grad = None
        fused.resize_bilinear_rows(memory[start:].permute(1, 0, 2), (hi, wi), (ho, wo), out_dtype=torch.bfloat16).backward(dy)

    def torch_nchw():
        memory.grad = None
        up = F.interpolate(memory[start:].permute(1, 2, 0).reshape(1, C, hi, wi), size=(ho, wo), mode='bilinear', align_corners=False)
        up.permute(0, 2, 3, 1).reshape(1, ho * wo, C).to(torch.bfloat16).backward(dy)
    res = alternate({'kernels': kernels, 'torch': torch_nchw}, args.reps, args.warmup)
    print('  fused.resize_bilinear_rows fwd+bwd    %s' % spread(res['kernels']))
    print('  F.interpolate + .to(bf16) fwd+bwd     %s' % spread(res['torch']))
    per = {}
    for _ in range(args.reps):
        _vah.prof_enable(True, 'resize_rows')
        kernels()
        for name, r in _vah.prof_report().items():
            per.setdefault(name, []).append((r['total_ms'] / r['calls'], r['bytes'] // r['calls']))
        _vah.prof_enable(False)
    for name in ('resize_rows_fwd', 'resize_rows_bwd'):
        ms = [m for m, _ in per[name]]
        nbytes = per[name][0][1]
        med = statistics.median(ms)
        print('  %-16s %s  %6.1f MB  %5.1f %% of 6.3 TB/s' % (name, spread(ms), nbytes / 1e6, 100 * nbytes / (med * 1e-3) / PEAK))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--sections', default='group_norm,resize,decoder')
    args = ap.parse_args()
    sections = args.sections.split(',')
    if not torch.cuda.is_available():
        sys.exit('bench_pixel_decoder.py needs the GPU')
    dev = 'cuda'
    norm = torch.nn.GroupNorm(G, C).to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    print('device: %s' % torch.cuda.get_device_name(0))
    if 'group_norm' in sections:
        print('== GroupNorm (%d channels, %d groups), bf16 rows, forward (ReLU) + backward ==' % (C, G))
    for h, w in SIZES if 'group_norm' in sections else ():
        T = h * w
        rows = torch.randn(1, T, C, device=dev, generator=gen).to(torch.bfloat16).requires_grad_(True)
        dy = torch.randn(1, T, C, device=dev, generator=gen).to(torch.bfloat16)
        planes = rows.detach().transpose(1, 2).reshape(1, C, h, w).contiguous().requires_grad_(True)
        dyp = dy.transpose(1, 2).reshape(1, C, h, w).contiguous()

        def kernels():
            rows.grad = None
            fused.group_norm(norm, rows, relu=True).backward(dy)

        def torch_nchw():
            planes.grad = None
            with torch.autocast('cuda', dtype=torch.bfloat16):
                y = torch.relu(F.group_norm(planes, G, norm.weight, norm.bias, norm.eps)).to(torch.bfloat16)
            y.backward(dyp)
        res = alternate({'kernels': kernels, 'torch': torch_nchw}, args.reps, args.warmup)
        print('map %3d x %3d (%6d rows, %5.1f MB bf16)' % (h, w, T, T * C * 2 / 1e6))
        print('  fused.group_norm fwd+bwd, rows   %s' % spread(res['kernels']))
        print('  F.group_norm fwd+bwd, NCHW fp32  %s' % spread(res['torch']))
        # per kernel: the library's own event pairs, one collection per repetition
        per = {}
        for _ in range(args.reps):
            _vah.prof_enable(True, 'gn_')
            kernels()
            for name, r in _vah.prof_report().items():
                per.setdefault(name, []).append((r['total_ms'] / r['calls'], r['bytes'] // r['calls']))
            _vah.prof_enable(False)
        for name in ('gn_stats', 'gn_apply', 'gn_bwd_stats', 'gn_bwd_apply'):
            ms = [m for m, _ in per[name]]
            nbytes = per[name][0][1]
            med = statistics.median(ms)
            print('  %-13s %s  %6.1f MB  %5.1f %% of 6.3 TB/s' % (name, spread(ms), nbytes / 1e6, 100 * nbytes / (med * 1e-3) / PEAK))

    if 'resize' in sections:
        resize_section(args, gen)
    if 'decoder' not in sections:
        return
    print('== MSDeformAttnPixelDecoder, in_channels 1024 x 4, bf16 autocast, forward + backward ==')
    torch.manual_seed(0)
    m = MSDeformAttnPixelDecoder(in_channels=(1024,) * 4)
    m.init_weights()
    m = m.to(dev).train()
    with torch.no_grad():
        for layer in m.encoder.layers:
            layer.attentions[0].sampling_offsets.weight.normal_(0, 0.02)
            layer.attentions[0].attention_weights.weight.normal_(0, 0.05)
    feats = [torch.randn(1, 1024, h, w, device=dev, generator=gen).to(torch.bfloat16).requires_grad_(True) for h, w in SIZES]

    def step(switch, on):
        def run():
            fused.ENABLED[switch] = on
            try:
                m.zero_grad(set_to_none=True)
                with torch.autocast('cuda', dtype=torch.bfloat16):
                    mf, ms = m(feats)
                (mf.float().pow(2).mean() + sum(o.float().pow(2).mean() for o in ms)).backward()
            finally:
                fused.ENABLED[switch] = True
        return run
    res = alternate({'on': step('group_norm', True), 'off': step('group_norm', False)}, args.reps, args.warmup)
    print('  group_norm on  (kernels)         %s' % spread(res['on']))
    print('  group_norm off (F.group_norm)    %s' % spread(res['off']))
    res = alternate({'on': step('bilinear_rows', True), 'off': step('bilinear_rows', False)}, args.reps, args.warmup)
    print('  bilinear_rows on  (kernels)      %s' % spread(res['on']))
    print('  bilinear_rows off (F.interpolate) %s' % spread(res['off']))


if __name__ == '__main__':
    main()
