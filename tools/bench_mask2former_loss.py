"""Mask2FormerHead.loss forward + backward at the shapes of BASELINE configs[4], ENABLED['point_loss'] on against off, and
with it on, ENABLED['point_mask_loss'] on against off (the third side: the sampled BCE / dice of the matched masks and their
backward on csrc/point_mask_loss.hip against torch's F.grid_sample expression, which is what the step ran before those kernels).

    python tools/bench_mask2former_loss.py [--reps 10] > profiles/r15_mask2former_loss.txt
    python tools/bench_mask2former_loss.py --pml [--reps 20] > profiles/r17_point_mask_loss.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_mask2former_loss.py --trace on|off [--reps 5]

--pml times only the third pair, with device events around each step (the sides alternate in one process; host clock beside
it, since the step is launch-bound), compares the two sides' losses and mask_pred gradients, checks that two steps of the kernel
side give the same gradient bits, and prints the launch-timer rows pml_forward / pml_backward.  --trace runs --reps steps of one
side after two warm-up steps and nothing else: the kernel trace of such a run, divided by the steps, is the launch count of a step.

Shapes: N 2, Q 100, 10 decoder outputs, 150 classes, mask_pred 160 x 160, ground truth 640 x 640 uint8 with 12 masks per image
(random ellipses), P 12 544, oversample 3.0, ratio 0.75, the losses and assigner of configs/_base_/models/mask2former_beit.py.
The head is the small one of tests/golden/mask2former_head.npz with these loss settings: ``loss`` reads none of its weights.

Timed: ``loss`` and the backward of sum(losses) into the twenty prediction tensors, host clock around a device synchronise,
median and minimum of --reps runs per side, the sides alternating; then, in a run of its own, the rows of the library's launch
timer for the point kernels (pts_sample, pts_match_cost).  "off" is this repository's torch expression (F.grid_sample and the
reference's cost formulas, still with one host round trip per step), not the reference's loss.  The "on" side of the first
pair has the sampled BCE / dice on their kernels too (ENABLED['point_mask_loss'], the default).  What is NOT on kernels on
either side: topk, cross-entropy, and scipy's linear_sum_assignment on the host.  Nothing is gated on these numbers."""
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
    ap.add_argument('--pml', action='store_true', help="time ENABLED['point_mask_loss'] on against off, point_loss on in both")
    ap.add_argument('--trace', choices=['on', 'off'], help='run only steps of one side of the --pml pair (for a kernel trace)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: a CPU run says nothing about these times'
    dev = torch.device('cuda:0')
    head = build(dev)
    masks, clss, labels, gts = inputs(dev)

    def step(on, pml=True):
        fused.ENABLED['point_loss'], fused.ENABLED['point_mask_loss'] = on, pml
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

    if args.trace:
        for _ in range(2 + args.reps):
            step(True, args.trace == 'on')
        torch.cuda.synchronize()
        print('%d steps of point_mask_loss %s after 2 warm-up steps (%d decoder outputs per step)' % (args.reps, args.trace, L))
        return
    if args.pml:
        return pml_pair(step, masks, args.reps)
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


def pml_pair(step, masks, reps):
    """ENABLED['point_mask_loss'] on against off with point_loss on in both, alternating; device events and host clock"""
    def timed(pml):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        step(True, pml)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), 1e3 * (time.perf_counter() - t0)

    for pml in (True, False, True, False):
        step(True, pml)
    torch.cuda.synchronize()
    ev, host = {True: [], False: []}, {True: [], False: []}
    for _ in range(reps):
        for pml in (True, False):
            e, h = timed(pml)
            ev[pml].append(e)
            host[pml].append(h)
    print('Mask2FormerHead.loss forward + backward on %s, %s' % (torch.cuda.get_device_name(0), time.strftime('%Y-%m-%d')))
    print('N %d, Q %d, %d outputs, mask_pred %d x %d, ground truth %d x %d with %d masks per image, P %d, %d reps per side, alternating'
          % (N, Q, L, HW[0], HW[1], GT_HW[0], GT_HW[1], G, P, reps))
    print("ENABLED['point_loss'] on in both sides; off = torch's F.grid_sample expression for the sampled BCE / dice and their backward")
    print('%-28s %18s %18s' % ('', 'point_mask_loss on', 'off (torch)'))
    for name, t in (('device events', ev), ('host clock', host)):
        print('%-28s %18.3f %18.3f' % (name + ': median ms', statistics.median(t[True]), statistics.median(t[False])))
        print('%-28s %18.3f %18.3f' % (name + ': min ms', min(t[True]), min(t[False])))
        print('%-28s %18.3f %18.3f' % (name + ': max ms', max(t[True]), max(t[False])))
    spread = max(max(ev[True]) - min(ev[True]), max(ev[False]) - min(ev[False]))
    gain = statistics.median(ev[False]) - statistics.median(ev[True])
    print('device events: median(off) - median(on) = %.3f ms, the larger min - max spread %.3f ms: %s'
          % (gain, spread, 'the kernel side is faster by more than the spread' if gain > spread else
             'NOT faster by more than the spread'))
    a = step(True, True)
    ga = [m.grad.clone() for m in masks]
    b = step(True, False)
    gb = [m.grad.clone() for m in masks]
    step(True, True)
    worst = max(abs(float(a[k].detach()) - float(b[k].detach())) / max(abs(float(b[k].detach())), 1e-6) for k in a)
    print('largest relative difference of a loss between the sides (same draws): %.3e' % worst)
    print('largest difference of a mask_pred gradient element between the sides, over the largest element: %.3e'
          % max(float((x - y).abs().max()) / float(y.abs().max()) for x, y in zip(ga, gb)))
    print('two steps of the kernel side give the same mask_pred gradient bits: %s'
          % all(torch.equal(x.view(torch.int32), m.grad.view(torch.int32)) for x, m in zip(ga, masks)))
    _vah.prof_enable(True, 'pml_')
    step(True, True)
    torch.cuda.synchronize()
    rows = _vah.prof_report()
    _vah.prof_enable(False)
    print('launch-timer rows of one step (a run of its own; pml_forward = 2 launches, pml_backward = a memset and 5 launches):')
    for name in sorted(rows):
        r = rows[name]
        print('  %-18s calls %4d   total %8.3f ms   %8.1f us / call' % (name, r['calls'], r['total_ms'], 1e3 * r['total_ms'] / max(r['calls'], 1)))


if __name__ == '__main__':
    main()
