"""Mask2FormerHead.loss forward + backward at the shapes of BASELINE configs[4], ENABLED['point_loss'] on against off, and
with it on, ENABLED['point_mask_loss'] on against off (the third side: the sampled BCE / dice of the matched masks and their
backward on csrc/point_mask_loss.hip against torch's F.grid_sample expression, which is what the step ran before those kernels).

    python tools/bench_mask2former_loss.py [--reps 10] > profiles/r15_mask2former_loss.txt
    python tools/bench_mask2former_loss.py --pml [--reps 20] > profiles/r17_point_mask_loss.txt
    python tools/bench_mask2former_loss.py --hungarian [--reps 20] > profiles/r22_hungarian_match.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_mask2former_loss.py --trace on|off [--reps 5]

--hungarian times ENABLED['hungarian'] on (the assignment on csrc/assign.hip, nothing read back) against off (the path before that
kernel: costs to the host, scipy per problem, table back), alternating, device events and host clock: on the workload below, on
the same with 100 masks per image (the solver's bad case), and on forward_train + backward of the full head with the targets
from prepare_targets.  It also checks that both sides choose the same table and give the same bits, prints the launch-timer row
assign_solve and counts the solver's search steps per problem with the host restatement of tests/hungarian_ref.py.

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


def inputs(dev, G=G):
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
    ap.add_argument('--hungarian', action='store_true', help="time ENABLED['hungarian'] on against off, everything else on in both")
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: a CPU run says nothing about these times'
    dev = torch.device('cuda:0')
    if args.hungarian:
        return hungarian_pairs(dev, args.reps)
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


def _ab(sides, reps):
    """{name: fn} alternating in this process -> ({name: [device-event ms]}, {name: [host-clock ms]})"""
    for _ in range(2):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ev, host = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            host[k].append(1e3 * (time.perf_counter() - t0))
            ev[k].append(a.elapsed_time(b))
    return ev, host


def _report(ev, host):
    names = list(ev)
    print('%-28s' % '' + ''.join('%22s' % k for k in names))
    for title, t in (('device events', ev), ('host clock', host)):
        for stat, f in (('median', statistics.median), ('min', min), ('max', max)):
            print('%-28s' % ('%s: %s ms' % (title, stat)) + ''.join('%22.3f' % f(t[k]) for k in names))
    on, off = names
    spread = max(max(host[k]) - min(host[k]) for k in names)
    diff = statistics.median(host[on]) - statistics.median(host[off])
    print('host clock: median(%s) - median(%s) = %+.3f ms, the larger min - max spread %.3f ms: %s'
          % (on, off, diff, spread, 'not slower by more than the spread' if diff <= spread else 'SLOWER by more than the spread'))


def hungarian_pairs(dev, reps):
    """ENABLED['hungarian'] on (csrc/assign.hip, no host trip) against off (one copy to the host, scipy per problem, one copy
    back: the path before the kernel), alternating in one process: (a) the workload of this file, (b) 100 masks per image, the
    solver's bad case, (c) Mask2FormerHead.forward_train + backward of the full head of tools/bench_mask2former_head.py
    under bf16 autocast with the targets from prepare_targets, where a host that is not stopped can run ahead."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import hungarian_ref
    print('Mask2FormerHead.loss forward + backward on %s, %s' % (torch.cuda.get_device_name(0), time.strftime('%Y-%m-%d')))
    print("ENABLED['hungarian'] on = vah_assign_solve on the device; off = costs to the host, scipy per (output, image), table back")
    head = build(dev)
    for tag, masks_per_image in (('(a)', G), ('(b)', 100)):
        masks, clss, labels, gts = inputs(dev, masks_per_image)

        def step(on):
            fused.ENABLED['hungarian'] = on
            for t in masks + clss:
                t.grad = None
            torch.manual_seed(1)
            losses = head.loss(clss, masks, labels, gts, [None] * N)
            sum(losses.values()).backward()
            return losses
        print('== %s N %d, Q %d, %d outputs, mask_pred %d x %d, ground truth %d x %d with %d masks per image, P %d, %d reps per side =='
              % (tag, N, Q, L, HW[0], HW[1], GT_HW[0], GT_HW[1], masks_per_image, P, reps))
        ev, host = _ab({'hungarian on': lambda: step(True), 'off (scipy)': lambda: step(False)}, reps)
        _report(ev, host)
        a = step(True)
        ga = [m.grad.clone() for m in masks]
        table_on = head._last_match[0].clone()
        b = step(False)
        print('the two sides choose the same table: %s; every loss and mask_pred gradient has the same bits: %s'
              % (torch.equal(table_on, head._last_match[0]),
                 all(torch.equal(a[k].detach(), b[k].detach()) for k in a) and all(torch.equal(x, m.grad) for x, m in zip(ga, masks))))
        seen = {}
        real = fused.hungarian_match

        def spy(costs, counts, gt_offsets=None):
            seen['costs'], seen['counts'] = torch.stack(list(costs)).cpu().numpy(), list(counts)
            return real(costs, counts, gt_offsets=gt_offsets)
        fused.hungarian_match = spy
        try:
            _vah.prof_enable(True, 'assign_')
            step(True)
            torch.cuda.synchronize()
            rows = _vah.prof_report()
            _vah.prof_enable(False)
        finally:
            fused.hungarian_match = real
        for name in sorted(rows):
            r = rows[name]
            print('launch-timer row (a run of its own): %-14s calls %d   %8.1f us / call (%d problems a call)'
                  % (name, r['calls'], 1e3 * r['total_ms'] / max(r['calls'], 1), L * N))
        steps = [hungarian_ref.solve(seen['costs'][i, n, :, :seen['counts'][n]])[3] for i in range(L) for n in range(N)]
        print('search steps per problem (host restatement of the solver on the recorded costs): median %d, min %d, max %d; the bound '
              'min(Q, G) (min(Q, G) + 1) / 2 is %d' % (statistics.median(steps), min(steps), max(steps),
                                                       min(Q, masks_per_image) * (min(Q, masks_per_image) + 1) // 2))
        if 'assign_solve' in rows and max(steps):
            print('launch time over the longest problem of the launch: %.3f us per search step (one wave per problem, all in flight at once)'
                  % (1e3 * rows['assign_solve']['total_ms'] / rows['assign_solve']['calls'] / max(steps)))
        fused.ENABLED['hungarian'] = True
    train_pair(dev, reps)


def train_pair(dev, reps):
    from bench_mask2former_head import head_config
    cfg = head_config()
    small = build('cpu')
    cfg.update(loss_cls=small.loss_cls, loss_mask=small.loss_mask, loss_dice=small.loss_dice, train_cfg=small.train_cfg)
    torch.manual_seed(0)
    head = Mask2FormerHead(**cfg)
    head.init_weights()
    head = head.to(dev).train()
    g = torch.Generator().manual_seed(0)
    feats = [torch.randn((N, 1024, s, s), generator=g).to(dev) for s in (160, 80, 40, 20)]
    label = torch.randint(0, G, (N, 20, 20), generator=g).repeat_interleave(32, 1).repeat_interleave(32, 2).to(torch.uint8).to(dev)

    def step(on):
        fused.ENABLED['hungarian'] = on
        head.zero_grad(set_to_none=True)
        targets = head.prepare_targets(label)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            losses = head.forward_train(feats, [None] * N, None, gt_targets=targets)
        sum(losses.values()).backward()
    print('== (c) Mask2FormerHead.forward_train + backward, the head of tools/bench_mask2former_head.py (profiles/r14_mask2former_head.txt), '
          'bf16 autocast, N %d, features of a 640 x 640 image, targets from prepare_targets (up to %d classes an image), %d reps per side =='
          % (N, G, reps))
    ev, host = _ab({'hungarian on': lambda: step(True), 'off (scipy)': lambda: step(False)}, reps)
    _report(ev, host)
    fused.ENABLED['hungarian'] = True


if __name__ == '__main__':
    main()
