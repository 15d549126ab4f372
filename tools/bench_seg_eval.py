#!/usr/bin/env python
"""The counting pass of the mIoU evaluation - label maps in, 3 x C int64 totals added to - at evaluation sizes.  Needs the GPU.

    python tools/bench_seg_eval.py [--reps 20] [--warmup 5]

Shapes: (1) 1 x 1024 x 2048, C 19, uint8 labels (Cityscapes); (2) 2 x 512 x 683, C 150, reduce_zero_label, uint8 (ADE20K);
(3) 1 x 896 x 896, C 171, int64 (COCO-Stuff crops).  Three kinds of maps for each, the prediction being the ground truth with
5 % of its pixels redrawn:
  const   one class everywhere: every add of a workgroup meets on three counters (the worst contention)
  blobs   argmax of upsampled low-resolution noise: the realistic case
  iid     independent random labels: runs of length 1, so no add is saved (the worst case for the LDS atomic rate)
Per shape and kind, after a warm-up, with device events, alternating inside this process: the kernel path
(ENABLED['seg_eval'] on, csrc/seg_eval.hip), the torch expression on the device (the switch off: masks and torch.bincount,
which synchronises) and the bare ``.cpu()`` copy of the int64 label map that evaluation on the host costs before it counts
anything: median / min / max.  Then the profile rows seg_eval_count and seg_eval_merge of one call with the bytes the
library counts - N * H * W * (8 + label bytes) plus the partial rows - as a share of the 8.0 TB/s HBM peak of
MI355X_MICROARCH.md."""
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

HBM_PEAK = 8.0e12
SHAPES = [('1 x 1024 x 2048, C 19, uint8', (1, 1024, 2048), 19, torch.uint8, False),
          ('2 x 512 x 683, C 150, reduce_zero_label, uint8', (2, 512, 683), 150, torch.uint8, True),
          ('1 x 896 x 896, C 171, int64', (1, 896, 896), 171, torch.int64, False)]


def make_maps(kind, shape, C, reduce_zero, dev, gen):
    """-> (pred int64, label int64) on the device; with reduce_zero_label the labels are 1-based and 0 is background"""
    N, H, W = shape
    if kind == 'const':
        cls = torch.full(shape, C // 2, dtype=torch.int64, device=dev)
    elif kind == 'blobs':
        low = torch.randn(N, C, (H + 31) // 32, (W + 31) // 32, device=dev, generator=gen)
        cls = F.interpolate(low, size=(H, W), mode='bilinear', align_corners=False).argmax(1)
    else:
        cls = torch.randint(0, C, shape, device=dev, generator=gen)
    redraw = torch.rand(shape, device=dev, generator=gen) < 0.05
    pred = torch.where(redraw, torch.randint(0, C, shape, device=dev, generator=gen), cls) if kind != 'const' else cls.clone()
    label = cls + 1 if reduce_zero else cls.clone()
    label[:, :8] = 0 if reduce_zero else 255                 # a band that counts for nothing
    return pred, label


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def section(title, pred, label, C, reduce_zero, reps, warmup):
    totals = torch.zeros((3, C), dtype=torch.int64, device=pred.device)

    def update(on):
        def run():
            fused.ENABLED['seg_eval'] = on
            try:
                fused.seg_eval_update(pred, label, totals, C, 255, reduce_zero)
            finally:
                fused.ENABLED['seg_eval'] = True
        return run

    sides = {'kernels': update(True), 'torch': update(False), 'copy': lambda: pred.cpu()}
    for _ in range(warmup):
        for f in sides.values():
            f()
    torch.cuda.synchronize()
    totals.zero_()
    sides['kernels']()
    a = totals.clone()
    totals.zero_()
    sides['torch']()
    same = torch.equal(a, totals)
    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, f in sides.items():
            ms[k].append(timed(f))
    print('  -- %s: totals of both sides %s' % (title, 'equal' if same else 'DIFFER'))
    for k, text in (('kernels', 'seg_eval on  (seg_eval.hip)  '), ('torch', 'seg_eval off (torch, device)'), ('copy', 'pred.cpu() alone            ')):
        print('     %s %8.3f ms median (min %.3f, max %.3f, n %d)' % (text, statistics.median(ms[k]), min(ms[k]), max(ms[k]), len(ms[k])))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print('     torch / kernels %.1f x, copy / kernels %.1f x' % (med['torch'] / med['kernels'], med['copy'] / med['kernels']))
    _vah.prof_enable(True, 'seg_eval')
    for _ in range(5):
        sides['kernels']()
    for name, r in sorted(_vah.prof_report().items()):
        per = r['total_ms'] / r['calls']
        print('       %-15s %2d x %8.4f ms   %8.2f MB each   %5.1f %% of the HBM peak'
              % (name, r['calls'], per, r['bytes'] / r['calls'] / 1e6, 100 * r['bytes'] / r['calls'] / (per * 1e-3) / HBM_PEAK))
    _vah.prof_enable(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_seg_eval.py needs the GPU')
    dev = torch.device('cuda')
    print('device: %s' % torch.cuda.get_device_name(0))
    gen = torch.Generator(device=dev).manual_seed(7)
    for title, shape, C, dtype, reduce_zero in SHAPES:
        print('== %s ==' % title)
        for kind in ('const', 'blobs', 'iid'):
            pred, label = make_maps(kind, shape, C, reduce_zero, dev, gen)
            section(kind, pred, label.to(dtype), C, reduce_zero, args.reps, args.warmup)


if __name__ == '__main__':
    main()
