"""Mask2FormerHead.loss forward + backward at the shapes of BASELINE configs[4], ENABLED['point_loss'] on against off.

    python tools/bench_mask2former_loss.py [--reps 10] > profiles/r15_mask2former_loss.txt

Shapes: N 2, Q 100, 10 decoder outputs, 150 classes, mask_pred 160 x 160, ground truth 640 x 640 uint8 with 12 masks per image
(random ellipses), P 12 544, oversample 3.0, ratio 0.75, the losses and assigner of configs/_base_/models/mask2former_beit.py.
The head is the small one of tests/golden/mask2former_head.npz with these loss settings: ``loss`` reads none of its weights.

Timed: ``loss`` and the backward of sum(losses) into the twenty prediction tensors, host clock around a device synchronise,
median and minimum of --reps runs per side, the sides alternating; then, in a run of its own, the rows of the library's launch
timer for the point kernels (pts_sample, pts_match_cost).  "off" is this repository's torch expression (F.grid_sample and the
reference's cost formulas, still with one host round trip per step), not the reference's loss.  What is NOT on kernels on
either side: the sampled BCE / dice of the matched masks and their backward (F.grid_sample), topk, cross-entropy, and scipy's
linear_sum_assignment on the host.  Nothing is gated on these numbers."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'vit-adapter_amd')]

import _vah                                              # noqa: E402
from vitadapter import Mask2FormerHead, fused            # noqa: E402

N, Q, L, CLASSES, HW, GT_HW, G, P = 2, 100, 10, 150, (160, 160), (640, 640), 12, 12544


def build(dev):
    cfg = copy.deepcopy(json.loads(str(np.load(os.path.join(ROOT, 'tests', 'golden', 'mask2former_head.npz'))['meta']))['config'])
    cfg.update(num_things_classes=100, num_stuff_classes=50, num_queries=Q,
               loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=2.0, reduction='mean', class_weight=[1.0] * CLASSES + [0.1]),
               loss_mask=dict(type='CrossEntropyLoss', use_sigmoid=True, reduction='mean', loss_weight=5.0),
               loss_dice=dict(type='DiceLoss', use_sigmoid=True, activate=True, reduction='mean', naive_dice=True, eps=1.0, loss_weight=5.0),
               train_cfg=dict(num_points=P, oversample_ratio=3.0, importance_sample_ratio=0.75,
                              assigner=dict(type='MaskHungarianAssigner', cls_cost=dict(type='ClassificationCost', weight=2.0),
                                            mask_cost=dict(type='CrossEntropyLossCost', weight=5.0, use_sigmoid=True),
                                            dice_cost=dict(type='DiceCost', weight=5.0, pred_act=True, eps=1.0)),
                              sampler=dict(type='MaskPseudoSampler')))
    return Mask2FormerHead(**cfg).to(dev)


def inputs(dev):
    g = torch.Generator().manual_seed(0)
    masks = [(torch.randn((N, Q) + HW, generator=g) * 4).to(dev).requires_grad_(True) for _ in range(L)]
    clss = [(torch.randn((N, Q, CLASSES + 1), generator=g) * 2).to(dev).requires_grad_(True) for _ in range(L)]
    H, W = GT_HW
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    gts, labels = [], []
    for _ in range(N):
        ms = []
        for _ in range(G):
            cy, cx, ry, rx = (torch.rand(4, generator=g) * torch.tensor([H, W, H / 3, W / 3]) + torch.tensor([0, 0, 20, 20])).tolist()
            ms.append((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).to(torch.uint8))
        gts.append(torch.stack(ms).to(dev))
        labels.append(torch.randint(0, CLASSES, (G,), generator=g).to(dev))
    return masks, clss, labels, gts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: a CPU run says nothing about these times'
    dev = torch.device('cuda:0')
    head = build(dev)
    masks, clss, labels, gts = inputs(dev)

    def step(on):
        fused.ENABLED['point_loss'] = on
        for t in masks + clss:
            t.grad = None
        torch.manual_seed(1)
        losses = head.loss(clss, masks, labels, gts, [None] * N)
        sum(losses.values()).backward()
        return losses

    def timed(on):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(on)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for on in (True, False, True, False):
        step(on)                                          # warm-up of both sides
    torch.cuda.synchronize()
    times = {True: [], False: []}
    for _ in range(args.reps):
        for on in (True, False):
            times[on].append(timed(on))
    print('Mask2FormerHead.loss forward + backward on %s, %s' % (torch.cuda.get_device_name(0), time.strftime('%Y-%m-%d')))
    print('N %d, Q %d, %d outputs, mask_pred %d x %d, ground truth %d x %d with %d masks per image, P %d, %d reps per side'
          % (N, Q, L, HW[0], HW[1], GT_HW[0], GT_HW[1], G, P, args.reps))
    print('%-28s %12s %12s' % ('', 'point_loss on', 'off (torch)'))
    print('%-28s %12.3f %12.3f' % ('median ms', statistics.median(times[True]), statistics.median(times[False])))
    print('%-28s %12.3f %12.3f' % ('min ms', min(times[True]), min(times[False])))
    print('%-28s %12.3f %12.3f' % ('max ms', max(times[True]), max(times[False])))
    a, b = step(True), step(False)
    worst = max(abs(float(a[k].detach()) - float(b[k].detach())) / max(abs(float(b[k].detach())), 1e-6) for k in a)
    print('largest relative difference of a loss between the sides (same draws): %.3e' % worst)
    _vah.prof_enable(True, 'pts_')
    step(True)
    torch.cuda.synchronize()
    rows = _vah.prof_report()
    _vah.prof_enable(False)
    print('per-kernel rows of one step (launch timer, a run of its own):')
    for name in sorted(rows):
        r = rows[name]
        print('  %-18s calls %4d   total %8.3f ms   %8.1f us / call' % (name, r['calls'], r['total_ms'], 1e3 * r['total_ms'] / max(r['calls'], 1)))


if __name__ == '__main__':
    main()
