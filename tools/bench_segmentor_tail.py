#!/usr/bin/env python
"""The logit tail of the Mask2Former segmentor - everything after decode_head.forward_test - at ADE20K sizes.  Needs the GPU.

    python tools/bench_segmentor_tail.py [--reps 10] [--warmup 3]

Backbone and head are stand-ins that cost nothing: the head hands out seeded logits at stride 4 of the crop it is asked
about, so what is timed is vitadapter.segmentor's own work on them (the crop copies of 3-channel windows included).  Shapes:
  1. one slide view, N 1, C 150, 896 x 1195 -> two 896 x 896 windows (stride 512), ori_shape 512 x 683, to labels; unflipped
     and flipped horizontally;
  2. aug_test of three such views (896 x 1195 unflipped, 1024 x 1366 flipped, 768 x 1024 unflipped) to labels;
  3. whole mode, 512 x 512 with ori_shape 512 x 512, to labels.
Nothing is copied to the host: the sections end where simple_test / aug_test would call .cpu().

Per shape, after a warm-up, with device events, ENABLED['seg_logits'] on (csrc/seg_logits.hip) and off (the reference's torch
expressions) alternating inside this process: median / min / max, torch.cuda.max_memory_allocated of one call of each
side above what was allocated before it, and the profile rows seg_* of one call with the bytes the library counts from the
shapes (what each launch must move at least) as a share of the 8.0 TB/s HBM peak of MI355X_MICROARCH.md."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'vit-adapter_amd'))

import _vah                                                  # noqa: E402
from vitadapter import fused                                 # noqa: E402
from vitadapter.segmentor import EncoderDecoderMask2Former   # noqa: E402

C = 150
HBM_PEAK = 8.0e12


class SeededHead(nn.Module):
    """forward_test: seeded logits (N, C, h / 4, w / 4), one tensor per crop size, made on first use"""
    num_classes = C
    align_corners = False

    def __init__(self):
        super().__init__()
        self.made = {}

    def forward_test(self, x, img_metas, test_cfg):
        key = tuple(x.shape)
        if key not in self.made:
            gen = torch.Generator(device=x.device).manual_seed(len(self.made))
            self.made[key] = torch.randn(x.shape[0], C, x.shape[2] // 4, x.shape[3] // 4, device=x.device, generator=gen)
        return self.made[key]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def switched(on, fn):
    def run():
        fused.ENABLED['seg_logits'] = on
        try:
            return fn()
        finally:
            fused.ENABLED['seg_logits'] = True
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
    for k, label in (('kernels', 'seg_logits on  (seg_logits.hip)'), ('torch', 'seg_logits off (torch)        ')):
        print('  %s %8.3f ms median (min %.3f, max %.3f, n %d)   peak %7.1f MB'
              % (label, statistics.median(ms[k]), min(ms[k]), max(ms[k]), len(ms[k]), peaks[k] / 1e6))
    gain = statistics.median(ms['torch']) - statistics.median(ms['kernels'])
    widest = max(max(v) - min(v) for v in ms.values())
    print('  median gain %.3f ms, larger spread %.3f ms: %s; peak %s' % (gain, widest, 'met' if gain > widest else 'MISSED',
                                                                         'lower' if peaks['kernels'] < peaks['torch'] else 'NOT LOWER'))
    _vah.prof_enable(True, 'seg_')
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
        sys.exit('bench_segmentor_tail.py needs the GPU')
    dev = torch.device('cuda')
    print('device: %s' % torch.cuda.get_device_name(0))

    def build(mode):
        cfg = dict(mode=mode, crop_size=(896, 896), stride=(512, 512))
        return EncoderDecoderMask2Former(nn.Identity(), SeededHead(), test_cfg=cfg).to(dev).eval()

    def meta(hw, ori, flip=False):
        return [dict(ori_shape=ori + (3,), img_shape=hw + (3,), flip=flip, flip_direction='horizontal')]

    slide, whole = build('slide'), build('whole')
    views = [((896, 1195), False), ((1024, 1366), True), ((768, 1024), False)]
    imgs = [torch.zeros(1, 3, *hw, device=dev) for hw, _ in views]
    ori = (512, 683)

    def labels_of(seg, img, m):
        with torch.no_grad():
            return seg._finish(img, m, True, True, prob=False, labels=True)[1]

    def aug():
        with torch.no_grad():
            total = None
            for img, (hw, flip) in zip(imgs, views):
                total = slide._finish(img, meta(hw, ori, flip), True, True, out=total, accumulate=total is not None)[0]
            return fused.seg_argmax(total, len(imgs))

    section('slide view 896 x 1195 -> 512 x 683, C 150, N 1, to labels', lambda: labels_of(slide, imgs[0], meta(views[0][0], ori)),
            args.reps, args.warmup)
    section('the same view flipped horizontally', lambda: labels_of(slide, imgs[0], meta(views[0][0], ori, True)), args.reps, args.warmup)
    section('aug_test, three views (896 x 1195, 1024 x 1366 flipped, 768 x 1024) -> 512 x 683', aug, args.reps, args.warmup)
    img512 = torch.zeros(1, 3, 512, 512, device=dev)
    section('whole mode 512 x 512, ori_shape 512 x 512, to labels', lambda: labels_of(whole, img512, meta((512, 512), (512, 512))),
            args.reps, args.warmup)


if __name__ == '__main__':
    main()
