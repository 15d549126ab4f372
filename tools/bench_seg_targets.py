#!/usr/bin/env python
"""Mask2Former's training targets from the label map - labels and binary masks per image - at training sizes.  Needs the GPU.

    python tools/bench_seg_targets.py [--reps 20] [--warmup 5] [--steps 12]

Shapes: (1) 2 x 512 x 512 with about 12 of 150 classes an image (ADE20K crops); (2) 2 x 896 x 896 with 19 classes (Cityscapes /
Mapillary crops); (3) 2 x 1024 x 1024 with 19 classes.  The maps are the argmax of upsampled low-resolution noise with an
ignored band, int64 as the reference's DefaultFormatBundle delivers them, and once more as uint8.

Three routes per shape, alternating inside this process after a warm-up, each timed on the host clock from its first call to
a device synchronisation (median / min / max):
  kernels    fused.seg_targets on the device map (csrc/seg_target.hip; ENABLED['seg_targets'] on)
  torch      the same call with the switch off: torch.unique and a comparison per image, on the device
  reference  the reference's route: vitadapter.ToMask - its ToMask step, line for line the same numpy calls - per image on
             one core of the host, then the int64 masks and labels copied to the device and reduced to uint8 there, as
             Mask2FormerHead._gt_groups does
with the bytes each route moves over PCIe in its own direction (the label map itself is on the device for the first two: the
UperNet path already trains that way; its upload is listed separately).  Then the three profile rows of one kernel call with
the bytes the library counts, the mask launch as GB/s.

Last, the claim that ``finish()`` does not stall a training step, on the real composition of
tests/test_segmentor_gpu.py::_real_segmentor (ViT-Adapter backbone, pixel decoder, query decoder, losses; bf16 autocast, N 2,
64 x 64): step times (forward_train + backward, synchronised) of the label-map route against the explicit-list route with the
lists already on the device as uint8 - the best case of that route -, and the host time spent inside ``finish()`` within a
step against the same ``finish()`` called directly after ``begin`` with nothing in between."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'vit-adapter_amd'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _vah                                                  # noqa: E402
import vitadapter                                            # noqa: E402
from vitadapter import fused                                 # noqa: E402

SHAPES = [('2 x 512 x 512, ~12 of 150 classes', (2, 512, 512), 150, 12),
          ('2 x 896 x 896, 19 classes', (2, 896, 896), 19, 19),
          ('2 x 1024 x 1024, 19 classes', (2, 1024, 1024), 19, 19)]


def make_map(shape, classes, present, dev, gen):
    """(N, H, W) int64 on the device: blobs of ``present`` of the ``classes`` labels an image, an ignored band"""
    N, H, W = shape
    low = torch.randn(N, present, (H + 63) // 64, (W + 63) // 64, device=dev, generator=gen)
    cls = F.interpolate(low, size=(H, W), mode='bilinear', align_corners=False).argmax(1)
    pick = torch.stack([torch.randperm(classes, device=dev, generator=gen)[:present] for _ in range(N)])
    out = torch.gather(pick, 1, cls.flatten(1)).view(N, H, W)
    out[:, :8] = 255
    return out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def reference_route(host_map, dev):
    """ToMask per image on the host, then the copies and the uint8 reduction of the head; -> (masks, labels, bytes copied)"""
    step = vitadapter.ToMask(255)
    masks, labels, moved = [], [], 0
    for n in range(host_map.shape[0]):
        r = step(dict(gt_semantic_seg=host_map[n], pad_shape=host_map[n].shape + (3,)))
        m, lab = torch.from_numpy(r['gt_masks']).to(dev), torch.from_numpy(r['gt_labels']).to(dev)
        moved += r['gt_masks'].nbytes + r['gt_labels'].nbytes
        masks.append((m != 0).view(torch.uint8))
        labels.append(lab)
    return torch.cat(masks), torch.cat(labels), moved


def stats(v):
    return '%8.3f ms median (min %.3f, max %.3f, n %d)' % (statistics.median(v), min(v), max(v), len(v))


def section(title, g, reps, warmup):
    host_map = g.cpu().numpy()
    N = g.shape[0]

    def kernels():
        return fused.seg_targets(g)

    def torch_route():
        fused.ENABLED['seg_targets'] = False
        try:
            return fused.seg_targets(g)
        finally:
            fused.ENABLED['seg_targets'] = True

    sides = {'kernels': kernels, 'torch': torch_route, 'reference': lambda: reference_route(host_map, g.device)}
    for _ in range(warmup):
        for f in sides.values():
            f()
    a, b, (rm, rl, moved) = kernels(), torch_route(), sides['reference']()
    same = all(torch.equal(x, y) for x, y in ((a.masks, b.masks), (a.labels, b.labels), (a.image_of, b.image_of), (a.masks, rm),
                                              (a.labels, rl))) and a.counts == b.counts
    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, f in sides.items():
            ms[k].append(wall(f))
    G = sum(a.counts)
    print('  -- %s: %d targets (%s), results of the three routes %s' % (title, G, a.counts, 'equal' if same else 'DIFFER'))
    pcie = {'kernels': '%d B down (meta)' % ((N + 2) * 4), 'torch': 'counts and labels down, %d synchronisations' % (2 * N),
            'reference': '%.1f MB up (int64 masks and labels)' % (moved / 1e6)}
    for k, text in (('kernels', 'seg_targets on  (seg_target.hip) '), ('torch', 'seg_targets off (torch, device)  '),
                    ('reference', 'numpy ToMask + copy + uint8      ')):
        print('     %s %s   PCIe: %s' % (text, stats(ms[k]), pcie[k]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print('     torch / kernels %.1f x, reference / kernels %.1f x; the label map itself: %.1f MB up as %s, %.1f MB as uint8'
          % (med['torch'] / med['kernels'], med['reference'] / med['kernels'], g.numel() * g.element_size() / 1e6,
             str(g.dtype).replace('torch.', ''), g.numel() / 1e6))
    _vah.prof_enable(True, 'seg_target')
    for _ in range(5):
        kernels()
    for name, r in sorted(_vah.prof_report().items()):
        per = r['total_ms'] / r['calls']
        print('       %-18s %2d x %8.4f ms   %8.2f MB each   %7.1f GB/s' % (name, r['calls'], per, r['bytes'] / r['calls'] / 1e6,
                                                                           r['bytes'] / r['calls'] / (per * 1e-3) / 1e9))
    _vah.prof_enable(False)


def composition(steps, warmup):
    import test_segmentor_gpu as seg_helpers
    import seg_targets_ref as ref
    seg, meta = seg_helpers._real_segmentor()
    dev = next(seg.parameters()).device
    gen = torch.Generator().manual_seed(3)
    img = torch.randn(2, 3, 64, 64, generator=gen).to(dev)
    rng = np.random.RandomState(9)
    gt = rng.randint(0, meta['things'] + meta['stuff'], size=(2, 4, 4)).repeat(16, axis=1).repeat(16, axis=2).astype(np.int64)
    gt[0, 5:20, 7:30] = 255
    gt_dev = torch.from_numpy(gt).to(dev)
    labels, masks = ref.lists(gt, 255)
    gt_labels = [torch.from_numpy(x).to(dev) for x in labels]
    gt_masks = [torch.from_numpy(x.astype(np.uint8)).to(dev) for x in masks]
    seg.train()
    inside = []
    keep = fused._PendingSegTargets._finish

    def timed_finish(self):
        t = time.perf_counter()
        out = keep(self)
        inside.append((time.perf_counter() - t) * 1e3)
        return out

    def step(route):
        seg.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            if route == 'label map':
                losses = seg.forward_train(img, [None, None], gt_dev)
            else:
                losses = seg.forward_train(img, [None, None], None, gt_labels=gt_labels, gt_masks=gt_masks)
        sum(losses.values()).backward()

    fused._PendingSegTargets._finish = timed_finish
    try:
        ms = {'label map': [], 'explicit lists': []}
        for i in range(warmup + steps):
            for route in ms:
                t = wall(lambda: step(route))
                if i >= warmup:
                    ms[route].append(t)
        in_step = inside[-steps:]
        del inside[:]
        for _ in range(steps):
            torch.cuda.synchronize()
            fused.seg_targets_begin(gt_dev).finish()
        alone = list(inside)
    finally:
        fused._PendingSegTargets._finish = keep
    print('== real composition, N 2, 64 x 64, bf16 autocast: forward_train + backward, synchronised ==')
    for route, v in ms.items():
        print('     %-15s %s' % (route, stats(v)))
    print('     host time inside finish(): within a step %s' % stats(in_step))
    print('                                directly after begin %s' % stats(alone))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_seg_targets.py needs the GPU')
    dev = torch.device('cuda')
    print('device: %s' % torch.cuda.get_device_name(0))
    gen = torch.Generator(device=dev).manual_seed(7)
    for title, shape, classes, present in SHAPES:
        print('== %s ==' % title)
        g = make_map(shape, classes, present, dev, gen)
        section('int64', g, args.reps, args.warmup)
        section('uint8', g.to(torch.uint8), args.reps, args.warmup)
    composition(args.steps, args.warmup)


if __name__ == '__main__':
    main()
