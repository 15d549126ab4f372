#!/usr/bin/env python
"""The training loss of the UperNet heads - resize to the label map, cross-entropy with ignore_index 255, top-1 count, and
the backward to the logits' gradient - at the reference's crop sizes.  Needs the GPU.

    python tools/bench_seg_ce_loss.py [--reps 10] [--warmup 3]

What is timed is one call of vitadapter.fused.seg_cross_entropy on seeded logits (N 2, C 150) and seeded labels with about
10 % of the pixels at 255, the mean over all pixels mmseg takes of it, and ``backward()`` to ``seg_logit.grad``.  Shapes: the
decode head (stride 4) and the auxiliary head (stride 16) of the 512 and the 640 crop, each with fp32 and with fp16 logits
(what conv_seg hands over without and under fp16 autocast).

Per shape, after a warm-up, with device events, ENABLED['seg_ce_loss'] on (csrc/seg_ce_loss.hip) and off (the torch
expression: F.interpolate of the upcast logits, F.cross_entropy, argmax - the only path before the kernels existed)
alternating inside this process: median / min / max, torch.cuda.max_memory_allocated of one forward + backward of each side
above what was allocated before it (logits and labels are allocated before), and the profile rows sce_* of one call with the
bytes the library counts from the shapes as a share of the 8.0 TB/s HBM peak of MI355X_MICROARCH.md."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'vit-adapter_amd'))

import _vah                                                  # noqa: E402
from vitadapter import fused                                 # noqa: E402

N, C = 2, 150
HBM_PEAK = 8.0e12
SHAPES = (('512 crop, decode head', 128, 512), ('512 crop, auxiliary head', 32, 512),
          ('640 crop, decode head', 160, 640), ('640 crop, auxiliary head', 40, 640))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def switched(on, fn):
    def run():
        fused.ENABLED['seg_ce_loss'] = on
        try:
            return fn()
        finally:
            fused.ENABLED['seg_ce_loss'] = True
    return run


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def section(title, fn, reps, warmup):
    sides = {'kernels': switched(True, fn), 'torch': switched(False, fn)}
    for _ in range(warmup):
        for f in sides.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, f in sides.items():
            ms[k].append(timed(f))
    peaks = {k: peak_of(f) for k, f in sides.items()}
    print('== %s ==' % title)
    for k, label in (('kernels', 'seg_ce_loss on  (seg_ce_loss.hip)'), ('torch', 'seg_ce_loss off (torch)          ')):
        print('  %s %8.3f ms median (min %.3f, max %.3f, n %d)   peak %7.1f MB'
              % (label, statistics.median(ms[k]), min(ms[k]), max(ms[k]), len(ms[k]), peaks[k] / 1e6))
    gain = statistics.median(ms['torch']) - statistics.median(ms['kernels'])
    widest = max(max(v) - min(v) for v in ms.values())
    print('  median gain %.3f ms, larger spread %.3f ms: %s; peak %s' % (gain, widest, 'met' if gain > widest else 'MISSED',
                                                                         'lower' if peaks['kernels'] < peaks['torch'] else 'NOT LOWER'))
    _vah.prof_enable(True, 'sce_')
    sides['kernels']()
    for name, r in sorted(_vah.prof_report().items()):
        per = r['total_ms'] / r['calls']
        print('    %-16s %2d x %8.3f ms   %8.1f MB each   %5.1f %% of the HBM peak'
              % (name, r['calls'], per, r['bytes'] / r['calls'] / 1e6, 100 * r['bytes'] / r['calls'] / (per * 1e-3) / HBM_PEAK))
    _vah.prof_enable(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_seg_ce_loss.py needs the GPU')
    dev = torch.device('cuda')
    print('device: %s' % torch.cuda.get_device_name(0))
    for title, src, out in SHAPES:
        for dtype in (torch.float32, torch.float16):
            gen = torch.Generator(device=dev).manual_seed(src + out)
            logits = torch.randn(N, C, src, src, device=dev, generator=gen).to(dtype).requires_grad_(True)
            labels = torch.randint(0, C, (N, 1, out, out), device=dev, generator=gen)
            labels[torch.rand(N, 1, out, out, device=dev, generator=gen) < 0.1] = 255

            def step():
                logits.grad = None
                loss_sum, n_valid, n_correct = fused.seg_cross_entropy(logits, labels, False, 255)
                (loss_sum / labels.numel()).backward()
                return logits.grad, n_correct

            section('%s: N %d, C %d, %d x %d -> %d x %d, %s logits' % (title, N, C, src, src, out, out, str(dtype)[6:]), step,
                    args.reps, args.warmup)
            del logits, labels


if __name__ == '__main__':
    main()
