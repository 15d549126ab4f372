"""Mask2FormerHead.loss / forward_test golden from the reference's own code.  Container only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_mask2former_loss.py

Runs the reference's ``Mask2FormerHead.loss`` (with ``loss_single``, ``get_targets``, ``_get_target_single``) and the lines of its
``forward_test`` (segmentation/mmseg_custom/models/decode_heads/mask2former_head.py:154-402, :575-579), its
``MaskHungarianAssigner`` (models/utils/assigner.py), ``ClassificationCost`` / ``CrossEntropyLossCost`` / ``DiceCost``
(models/losses/match_costs.py), ``DiceLoss`` and ``CrossEntropyLoss`` (models/losses/), ``MaskPseudoSampler`` (core/box/samplers)
and ``get_uncertain_point_coords_with_randomness`` (models/utils/point_sample.py) under in-memory stand-ins, on top of the ones
tools/gen_golden_mask2former_head.py has: ``mmcv.ops.point_sample`` restated on F.grid_sample (mmcv's definition:
grid_sample(input, 2 * points - 1, align_corners=False)), mmseg's ``weight_reduce_loss`` / ``get_class_weight`` restated, the
registries and builders as dictionaries of the loaded classes, ``multi_apply`` and ``reduce_mean`` (no process group: identity).
The head object is the reference's class without its constructor (which needs mmcv's builders): only the attributes ``loss``
reads are set.

Evaluation is in fp64 on fp32-representable inputs: ``Tensor.float`` is ``Tensor.double`` while the fp64 run is on (the
reference casts inside CrossEntropyLossCost, DiceLoss and on the ground-truth masks).  ``torch.rand`` is wrapped: every draw is
made in fp32, recorded, and handed out in the run's dtype, so the fp32 run replays the fp64 run's points.

Case: N 2, Q 8, 3 + 1 decoder outputs, 3 + 2 classes, mask_pred 32 x 48, ground truth 64 x 96, P 32, oversample 3.0, ratio 0.75,
the losses and assigner of configs/_base_/models/mask2former_beit.py:93-123.  Variants by ground-truth count per image:
'full' (3, 2), 'one_empty' (3, 0: the second image has no ground truth), 'none' (0, 0: the zero-match branch :327-331).

Two discontinuities are guarded; seeds are walked until both hold for every variant (``meta`` records seed and margins):
  * assignment: d = the largest |fp32 - fp64| cost entry; the Hungarian assignment of every (output, image) must be unchanged
    under 32 perturbations of the fp64 cost by uniform noise of amplitude 16 d;
  * topk: per matched mask, the k-th and (k + 1)-th largest uncertainties (-|logit| at the oversampled points) must differ by at
    least 16 x the largest fp32 - fp64 difference of that mask's sampled logits.

Stored (fp64 results as float64 unless said): ``mask_pred<i>_q`` int8 with ``mask_pred_scale``, ``cls_score<i>_q`` / ``cls_scale``,
``gt_masks<n>`` uint8, ``gt_labels<n>``; per variant v: ``<v>_match_<i>_<n>``, ``<v>_over_<i>``, ``<v>_rand_<i>`` (the draws, fp32),
``<v>_cost_<i>_<n>`` (Q, G_n), ``<v>_assign_<i>_<n>`` (2, matches: queries ascending, their gts), ``<v>_points_<i>`` (K, P, 2) fp32,
``<v>_losses`` (12,) in the order of ``meta['loss_keys']``, ``<v>_gmask<i>`` / ``<v>_gcls<i>`` (gradients of sum(losses), fp32);
``seg_mask`` (fp32).
"""
import contextlib
import importlib
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import gen_golden as gg                                   # noqa: E402
import gen_golden_pixel_decoder as gpd                    # noqa: E402
import gen_golden_mask2former_head as ggh                 # noqa: E402

N, Q, L, THINGS, STUFF, HW, GT_HW, P = 2, 8, 4, 3, 2, (32, 48), (64, 96), 32
CLASSES = THINGS + STUFF
OVERSAMPLE, RATIO, GUARD, TRIALS = 3.0, 0.75, 16.0, 32
VARIANTS = {'full': (3, 2), 'one_empty': (3, 0), 'none': (0, 0)}
LOSS_CLS = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=2.0, reduction='mean', class_weight=[1.0] * CLASSES + [0.1])
LOSS_MASK = dict(type='CrossEntropyLoss', use_sigmoid=True, reduction='mean', loss_weight=5.0)
LOSS_DICE = dict(type='DiceLoss', use_sigmoid=True, activate=True, reduction='mean', naive_dice=True, eps=1.0, loss_weight=5.0)
TRAIN_CFG = dict(num_points=P, oversample_ratio=OVERSAMPLE, importance_sample_ratio=RATIO,
                 assigner=dict(type='MaskHungarianAssigner', cls_cost=dict(type='ClassificationCost', weight=2.0),
                               mask_cost=dict(type='CrossEntropyLossCost', weight=5.0, use_sigmoid=True),
                               dice_cost=dict(type='DiceCost', weight=5.0, pred_act=True, eps=1.0)),
                 sampler=dict(type='MaskPseudoSampler'))
LOSS_KEYS = ['loss_cls', 'loss_mask', 'loss_dice'] + ['d%d.%s' % (i, k) for i in range(L - 1) for k in ('loss_cls', 'loss_mask', 'loss_dice')]


def point_sample(input, points, align_corners=False, **kwargs):
    """mmcv.ops.point_sample for (N, P, 2) points"""
    assert points.dim() == 3 and not align_corners
    out = F.grid_sample(input.to(points.dtype), 2.0 * points.unsqueeze(2) - 1.0, align_corners=False, **kwargs)
    return out.squeeze(3)


def weight_reduce_loss(loss, weight=None, reduction='mean', avg_factor=None):
    """mmseg.models.losses.utils.weight_reduce_loss"""
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        return loss.mean() if reduction == 'mean' else (loss.sum() if reduction == 'sum' else loss)
    if reduction == 'mean':
        return loss.sum() / avg_factor
    assert reduction == 'none'
    return loss


class Draws:
    """torch.rand for the reference's modules: records fp32 draws, or replays recorded ones; hands them out in ``dtype``"""

    def __init__(self, gen):
        self.gen, self.log, self.replay, self.dtype = gen, [], None, torch.float64

    def rand(self, *size, device=None):
        size = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list)) else tuple(size)
        if self.replay is not None:
            t = self.replay.pop(0)
            assert tuple(t.shape) == size, (t.shape, size)
        else:
            t = torch.rand(size, generator=self.gen, dtype=torch.float32)
        self.log.append(t)
        return t.to(self.dtype)


class TorchProxy:
    def __init__(self, draws):
        self._draws = draws

    def __getattr__(self, name):
        return self._draws.rand if name == 'rand' else getattr(torch, name)


@contextlib.contextmanager
def float_is_double(on):
    keep = torch.Tensor.float
    if on:
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.Tensor.float = keep


def load_reference():
    """-> (head module, assigner module, dict of the loaded classes by registry name)"""
    mod = ggh.load_reference()
    sys.modules['mmcv.ops'].point_sample = point_sample
    gg._mod('mmdet'), gg._mod('mmdet.utils', util_mixins=types.SimpleNamespace(NiceRepr=object))
    gg._mod('mmseg.models.losses'), gg._mod('mmseg.models.losses.utils', weight_reduce_loss=weight_reduce_loss, get_class_weight=lambda w: w)
    sys.modules['mmseg.models.builder'].LOSSES = gpd.Registry()
    builder = sys.modules['ref_pd.models.builder']
    builder.MASK_ASSIGNERS, builder.MATCH_COST = gpd.Registry(), gpd.Registry()
    for name, sub in (('ref_pd.models.losses', 'models/losses'), ('ref_pd.core.box', 'core/box'), ('ref_pd.core.box.samplers', 'core/box/samplers')):
        gg._mod(name).__path__ = [os.path.join(gpd.REF, sub)]
    gg._mod('ref_pd.core.box.builder', BBOX_SAMPLERS=gpd.Registry())
    costs = importlib.import_module('ref_pd.models.losses.match_costs')
    builder.build_match_cost = lambda cfg: getattr(costs, cfg['type'])(**{k: v for k, v in cfg.items() if k != 'type'})
    assigner = importlib.import_module('ref_pd.models.utils.assigner')
    classes = dict(DiceLoss=importlib.import_module('ref_pd.models.losses.dice_loss').DiceLoss,
                   CrossEntropyLoss=importlib.import_module('ref_pd.models.losses.cross_entropy_loss').CrossEntropyLoss,
                   MaskHungarianAssigner=assigner.MaskHungarianAssigner,
                   MaskPseudoSampler=importlib.import_module('ref_pd.core.box.samplers.mask_pseudo_sampler').MaskPseudoSampler)
    pts = importlib.import_module('ref_pd.models.utils.point_sample')
    mod.point_sample = point_sample
    mod.get_uncertain_point_coords_with_randomness = pts.get_uncertain_point_coords_with_randomness
    mod.multi_apply = _multi_apply
    mod.reduce_mean = lambda t: t
    return mod, assigner, pts, classes


def _multi_apply(func, *args, **kwargs):
    """mmdet's multi_apply (core/utils/misc.py)"""
    results = map(lambda *a: func(*a, **kwargs), *args)
    return tuple(map(list, zip(*results)))


def build(cfg):
    cfg = dict(cfg)
    return cfg.pop('type'), cfg


def make_head(mod, classes):
    head = mod.Mask2FormerHead.__new__(mod.Mask2FormerHead)
    nn.Module.__init__(head)
    head.num_queries, head.num_classes = Q, CLASSES
    head.num_points, head.oversample_ratio, head.importance_sample_ratio = P, OVERSAMPLE, RATIO
    head.class_weight = LOSS_CLS['class_weight']
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for name, cfg in (('loss_cls', LOSS_CLS), ('loss_mask', LOSS_MASK), ('loss_dice', LOSS_DICE)):
            t, kw = build(cfg)
            setattr(head, name, classes[t](**kw))
    t, kw = build(TRAIN_CFG['assigner'])
    head.assigner = classes[t](**kw)
    head.sampler = classes[TRAIN_CFG['sampler']['type']]()
    return head


def inputs(seed):
    g = torch.Generator().manual_seed(1000 + seed)
    mask_q = [torch.randint(-127, 128, (N, Q) + HW, generator=g, dtype=torch.int16).to(torch.int8) for _ in range(L)]
    cls_q = [torch.randint(-127, 128, (N, Q, CLASSES + 1), generator=g, dtype=torch.int16).to(torch.int8) for _ in range(L)]
    gts, labels = [], []
    H, W = GT_HW
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    for n in range(N):
        ms = []
        for j in range(3):
            cy, cx, ry, rx = (torch.rand(4, generator=g) * torch.tensor([H, W, H / 2, W / 2]) + torch.tensor([0, 0, 4, 4])).tolist()
            ms.append((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).to(torch.uint8))
        gts.append(torch.stack(ms))
        labels.append(torch.randint(0, CLASSES, (3,), generator=g))
    return mask_q, cls_q, gts, labels


MASK_SCALE, CLS_SCALE = 1.0 / 16, 1.0 / 32


def run(head, assigner, pts_mod, draws, mask_q, cls_q, gts, labels, counts, dtype, replay=None):
    """one evaluation of the reference's loss -> dict of everything recorded"""
    draws.log, draws.replay, draws.dtype = [], (list(replay) if replay is not None else None), dtype
    masks = [(m.to(dtype) * MASK_SCALE).requires_grad_(True) for m in mask_q]
    clss = [(c.to(dtype) * CLS_SCALE).requires_grad_(True) for c in cls_q]
    seen = []
    real = assigner.__dict__['linear_sum_assignment_real']

    def lsa(cost):
        seen.append(cost.clone())
        return real(cost)
    assigner.linear_sum_assignment = lsa
    with float_is_double(dtype == torch.float64):
        out = head.loss(clss, masks, [lab[:c] for lab, c in zip(labels, counts)], [g[:c] for g, c in zip(gts, counts)], [None] * N)
        total = sum(out[k] for k in LOSS_KEYS)
        grads = torch.autograd.grad(total, masks + clss, allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(t) for g, t in zip(grads, masks + clss)]
    return dict(losses=out, costs=seen, draws=list(draws.log), gmask=grads[:L], gcls=grads[L:], masks=masks, clss=clss)


def split_draws(log, counts):
    """the reference's draw order -> {('match', i, n) | ('over', i) | ('rand', i): draw}"""
    K = sum(min(Q, c) for c in counts)
    out, it = {}, iter(log)
    for i in range(L):
        for n in range(N):
            out['match', i, n] = next(it)
        if K:
            out['over', i], out['rand', i] = next(it), next(it)
    assert next(it, None) is None
    return out


def assignments(costs, counts):
    """per (output, image): (queries ascending, their gts), from the costs the assigner handed to scipy"""
    from scipy.optimize import linear_sum_assignment
    out, it = {}, iter(costs)
    for i in range(L):
        for n in range(N):
            if counts[n]:
                c = next(it)
                r, g = linear_sum_assignment(c)
                o = np.argsort(r, kind='stable')
                out[i, n] = (c, np.stack([r[o], g[o]]))
            else:
                out[i, n] = (torch.zeros((Q, 0), dtype=torch.float64), np.zeros((2, 0), dtype=np.int64))
    return out


def guards(r64, r32, counts, seed):
    """-> (ok, margins)"""
    from scipy.optimize import linear_sum_assignment
    a64, a32 = assignments(r64['costs'], counts), assignments(r32['costs'], counts)
    d = max([float((a32[k][0].double() - a64[k][0].double()).abs().max()) for k in a64 if a64[k][0].numel()] + [0.0])
    ok = all(np.array_equal(a64[k][1], a32[k][1]) for k in a64)
    rng = np.random.default_rng(seed)
    for k, (c, a) in a64.items():
        if not c.numel():
            continue
        for _ in range(TRIALS):
            noise = rng.uniform(-GUARD * d, GUARD * d, size=tuple(c.shape))
            r, g = linear_sum_assignment(c.double().numpy() + noise)
            o = np.argsort(r, kind='stable')
            ok = ok and np.array_equal(np.stack([r[o], g[o]]), a)
    dr = split_draws(r64['draws'], counts)
    gaps = []
    n_unc = int(RATIO * P)
    if sum(counts):
        for i in range(L):
            rows = np.concatenate([a64[i, n][1][0] + n * Q for n in range(N)])
            lg = {}
            for dt, res in ((torch.float64, r64), (torch.float32, r32)):
                m = res['masks'][i].detach().flatten(0, 1)[rows]
                lg[dt] = point_sample(m.unsqueeze(1), dr['over', i].to(dt)).squeeze(1).double()
            diff = (lg[torch.float64] - lg[torch.float32]).abs().max(1)[0]
            u = torch.sort(-lg[torch.float64].abs(), dim=1, descending=True)[0]
            gap = u[:, n_unc - 1] - u[:, n_unc]
            gaps += [(float(a), float(b)) for a, b in zip(gap, diff)]
            ok = ok and bool((gap >= GUARD * diff).all())
    return ok, dict(d=d, least_topk_gap=min([g for g, _ in gaps] + [float('inf')]), largest_logit_diff=max([b for _, b in gaps] + [0.0]))


def main():
    mod, assigner, pts_mod, classes = load_reference()
    assigner.linear_sum_assignment_real = assigner.linear_sum_assignment
    assert assigner.linear_sum_assignment_real is not None, 'scipy is needed'
    draws = Draws(None)
    mod.torch = TorchProxy(draws)
    pts_mod.torch = TorchProxy(draws)
    head = make_head(mod, classes)
    for seed in range(200):
        mask_q, cls_q, gts, labels = inputs(seed)
        results, margins, ok = {}, {}, True
        for v, counts in VARIANTS.items():
            draws.gen = torch.Generator().manual_seed(77 * seed + len(v))
            r64 = run(head, assigner, pts_mod, draws, mask_q, cls_q, gts, labels, counts, torch.float64)
            r32 = run(head, assigner, pts_mod, draws, mask_q, cls_q, gts, labels, counts, torch.float32, replay=r64['draws'])
            good, margins[v] = guards(r64, r32, counts, seed)
            ok = ok and good
            results[v] = r64
        print('seed %d: %s -> %s' % (seed, margins, ok), flush=True)
        if ok:
            break
    else:
        raise SystemExit('no seed passes the guards')
    g = {'mask_pred_scale': np.float64(MASK_SCALE), 'cls_scale': np.float64(CLS_SCALE)}
    for i in range(L):
        g['mask_pred%d_q' % i], g['cls_score%d_q' % i] = mask_q[i].numpy(), cls_q[i].numpy()
    for n in range(N):
        g['gt_masks%d' % n], g['gt_labels%d' % n] = gts[n].numpy(), labels[n].numpy()
    f32 = lambda t: t.detach().to(torch.float32).numpy()                   # noqa: E731
    for v, counts in VARIANTS.items():
        r = results[v]
        K = sum(min(Q, c) for c in counts)
        dr = split_draws(r['draws'], counts)
        for key, t in dr.items():
            g['%s_%s' % (v, '_'.join(str(k) for k in key))] = t.numpy()
        a = assignments(r['costs'], counts)
        n_unc = int(RATIO * P)
        for i in range(L):
            for n in range(N):
                g['%s_cost_%d_%d' % (v, i, n)], g['%s_assign_%d_%d' % (v, i, n)] = a[i, n][0].double().numpy(), a[i, n][1]
            if K:
                rows = np.concatenate([a[i, n][1][0] + n * Q for n in range(N)])
                lg = point_sample(r['masks'][i].detach().flatten(0, 1)[rows].unsqueeze(1), dr['over', i].double()).squeeze(1)
                idx = torch.topk(-lg.abs(), k=n_unc, dim=1)[1]
                g['%s_points_%d' % (v, i)] = torch.cat((torch.gather(dr['over', i], 1, idx[:, :, None].expand(-1, -1, 2)), dr['rand', i]), 1).numpy()
            g['%s_gmask%d' % (v, i)], g['%s_gcls%d' % (v, i)] = f32(r['gmask'][i]), f32(r['gcls'][i])
        g['%s_losses' % v] = np.array([float(r['losses'][k].detach()) for k in LOSS_KEYS], dtype=np.float64)
    r = results['full']
    cls_score, mask_pred = F.softmax(r['clss'][-1].detach(), dim=-1)[..., :-1], r['masks'][-1].detach().sigmoid()
    g['seg_mask'] = f32(torch.einsum('bqc,bqhw->bchw', cls_score, mask_pred))
    meta = dict(seed=seed, guard=GUARD, trials=TRIALS, margins=margins, variants={v: list(c) for v, c in VARIANTS.items()}, loss_keys=LOSS_KEYS,
                loss_cls=LOSS_CLS, loss_mask=LOSS_MASK, loss_dice=LOSS_DICE, train_cfg=TRAIN_CFG, N=N, Q=Q, L=L, P=P,
                things=THINGS, stuff=STUFF)
    g['meta'] = np.array(json.dumps(meta))
    dst = os.path.join(ROOT, 'tests', 'golden', 'mask2former_loss.npz')
    np.savez_compressed(dst, **g)
    print(dst, os.path.getsize(dst), 'bytes,', len(g), 'arrays')


if __name__ == '__main__':
    main()
