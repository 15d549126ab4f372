"""CPU: Mask2FormerHead.loss / forward_test against tests/golden/mask2former_loss.npz (computed in fp64 by the reference's own
loss, assigner, match costs, losses and point selection, see tools/gen_golden_mask2former_loss.py), with ``_draw`` replaying the
golden's draws: the assignments and the chosen points equal the golden's exactly (two guards of the generator make that a fair
demand), the twelve losses, ``seg_mask`` and the gradients of sum(losses) are held to fp32 bounds.  On the CPU every point
operator is its torch expression (F.grid_sample), the CPU tier of fused.point_sample / match_costs / point_mask_losses.

Bounds: a loss is a mean of O(1) terms evaluated in fp32: 1e-5 relative (floor 1e-6); a gradient element 1e-5 of the gradient's
largest element; seg_mask 1e-5.  The helpers are shared with tests/test_mask2former_loss_gpu.py."""
import copy
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'mask2former_loss.npz')
HEAD_GOLD = os.path.join(ROOT, 'tests', 'golden', 'mask2former_head.npz')


@pytest.fixture(scope='module')
def gold():
    g = np.load(GOLD)
    return g, json.loads(str(g['meta']))


def head_config(meta):
    """the small head of tests/golden/mask2former_head.npz with the loss golden's loss and training configs"""
    cfg = copy.deepcopy(json.loads(str(np.load(HEAD_GOLD)['meta']))['config'])
    cfg.update(num_things_classes=meta['things'], num_stuff_classes=meta['stuff'], num_queries=meta['Q'],
               loss_cls=copy.deepcopy(meta['loss_cls']), loss_mask=copy.deepcopy(meta['loss_mask']),
               loss_dice=copy.deepcopy(meta['loss_dice']), train_cfg=copy.deepcopy(meta['train_cfg']))
    return cfg


def build_head(meta, dev):
    from vitadapter import Mask2FormerHead
    return Mask2FormerHead(**head_config(meta)).to(dev)


def inputs(g, meta, variant, dev):
    """fp32 predictions (leaves) and the ground truth of a variant"""
    masks = [(torch.from_numpy(g['mask_pred%d_q' % i].astype(np.float32)) * float(g['mask_pred_scale'])).to(dev).requires_grad_(True)
             for i in range(meta['L'])]
    clss = [(torch.from_numpy(g['cls_score%d_q' % i].astype(np.float32)) * float(g['cls_scale'])).to(dev).requires_grad_(True)
            for i in range(meta['L'])]
    counts = meta['variants'][variant]
    gt_masks = [torch.from_numpy(g['gt_masks%d' % n])[:c].to(dev) for n, c in enumerate(counts)]
    gt_labels = [torch.from_numpy(g['gt_labels%d' % n])[:c].to(dev) for n, c in enumerate(counts)]
    return masks, clss, gt_labels, gt_masks


def replay(head, g, variant):
    """replace ``_draw`` by the golden's recorded draws; -> the list of draws asked for"""
    asked = []

    def draw(kind, layer, image, shape, device):
        key = {'match': '%s_match_%d_%s' % (variant, layer, image), 'oversample': '%s_over_%d' % (variant, layer),
               'random': '%s_rand_%d' % (variant, layer)}[kind]
        asked.append((kind, layer, image))
        t = torch.from_numpy(g[key])
        assert tuple(t.shape) == tuple(shape), (key, t.shape, shape)
        return t.to(device)
    head._draw = draw
    return asked


def run_loss(head, g, meta, variant, dev):
    masks, clss, gt_labels, gt_masks = inputs(g, meta, variant, dev)
    asked = replay(head, g, variant)
    losses = head.loss(clss, masks, gt_labels, gt_masks, [None] * meta['N'])
    return masks, clss, losses, asked


def check_choices(head, g, meta, variant):
    """the discontinuous parts: exact"""
    counts = meta['variants'][variant]
    for i in range(meta['L']):
        for n in range(meta['N']):
            want = g['%s_assign_%d_%d' % (variant, i, n)]
            got = torch.stack(head.last_assignment[i][n]).numpy()
            assert np.array_equal(got, want), (
                'output %d image %d is assigned %s, the golden %s: the assignment guard of the generator (16 x the fp32 - fp64 '
                'cost difference, meta margins %s) did not hold here' % (i, n, got.tolist(), want.tolist(), meta['margins'][variant]))
        if sum(counts):
            want = g['%s_points_%d' % (variant, i)]
            got = head.last_points[i].cpu().numpy()
            assert got.shape == want.shape and got.dtype == np.float32
            assert np.array_equal(got, want), (
                'output %d: %d chosen points differ from the golden: the topk guard of the generator (meta margins %s) did not '
                'hold here' % (i, int((got != want).any(-1).sum()), meta['margins'][variant]))
        else:
            assert head.last_points[i] is None


def errors(g, meta, variant, masks, clss, losses):
    """-> ({loss key: |err|}, {gradient name: max |err|}, {gradient name: max |golden|}) after backward of sum(losses)"""
    want = g['%s_losses' % variant]
    assert list(losses) == meta['loss_keys']
    sum(losses[k] for k in meta['loss_keys']).backward()
    e_loss = {k: abs(float(losses[k].detach()) - want[j]) for j, k in enumerate(meta['loss_keys'])}
    e_grad, top = {}, {}
    for i in range(meta['L']):
        for name, t in (('gmask%d' % i, masks[i]), ('gcls%d' % i, clss[i])):
            w = g['%s_%s' % (variant, name)]
            got = t.grad.float().cpu().numpy() if t.grad is not None else np.zeros_like(w)
            e_grad[name], top[name] = float(np.abs(got - w).max()), float(np.abs(w).max())
    return e_loss, e_grad, top


def test_dict_keys_and_settings(gold):
    g, meta = gold
    head = build_head(meta, 'cpu')
    assert (head.num_points, head.oversample_ratio, head.importance_sample_ratio) == (32, 3.0, 0.75)
    assert head.match_weights == (2.0, 5.0, 5.0) and head.dice_cost_eps == 1.0 and head.dice_loss_eps == 1.0
    assert (head.cls_loss_weight, head.mask_loss_weight, head.dice_loss_weight) == (2.0, 5.0, 5.0)
    assert head.loss_cls == meta['loss_cls'] and head.train_cfg == meta['train_cfg']
    _, _, losses, asked = run_loss(head, g, meta, 'full', 'cpu')
    L = meta['L']
    assert list(losses) == ['loss_cls', 'loss_mask', 'loss_dice'] + ['d%d.%s' % (i, k) for i in range(L - 1)
                                                                       for k in ('loss_cls', 'loss_mask', 'loss_dice')]
    assert all(v.dim() == 0 and v.dtype == torch.float32 for v in losses.values())
    # every 'match' draw comes first, then per output the oversample and the random draw
    assert asked == [('match', i, n) for i in range(L) for n in range(meta['N'])] + [(k, i, None) for i in range(L)
                                                                                     for k in ('oversample', 'random')]


@pytest.mark.parametrize('variant', ['full', 'one_empty', 'none'])
def test_cpu_loss_matches_golden(gold, variant):
    g, meta = gold
    head = build_head(meta, 'cpu')
    masks, clss, losses, _ = run_loss(head, g, meta, variant, 'cpu')
    check_choices(head, g, meta, variant)
    want = g['%s_losses' % variant]
    e_loss, e_grad, top = errors(g, meta, variant, masks, clss, losses)
    for j, k in enumerate(meta['loss_keys']):
        assert e_loss[k] <= 1e-5 * max(abs(want[j]), 0.1), (k, float(losses[k]), want[j])
    for name in e_grad:
        assert e_grad[name] <= 1e-5 * max(top[name], 1e-3), (name, e_grad[name], top[name])
    if variant == 'none':                         # :327-331: zero with a zero gradient
        for k in meta['loss_keys']:
            if not k.endswith('loss_cls'):
                assert float(losses[k].detach()) == 0.0
        assert all(float(m.grad.abs().max()) == 0.0 for m in masks)
    if variant == 'one_empty':                    # the image without ground truth: no match, all of its queries background
        assert all(head.last_assignment[i][1][0].numel() == 0 for i in range(meta['L']))
        assert all(float(m.grad[1].abs().max()) == 0.0 for m in masks)


def test_forward_test_lines(gold):
    g, meta = gold
    from vitadapter import Mask2FormerHead
    masks, clss, _, _ = inputs(g, meta, 'full', 'cpu')
    seg = Mask2FormerHead.semantic_inference(clss[-1].detach(), masks[-1].detach())
    assert seg.dtype == torch.float32 and tuple(seg.shape) == g['seg_mask'].shape
    assert float(np.abs(seg.numpy() - g['seg_mask']).max()) <= 1e-5


def test_masks_of_different_sizes_take_the_per_image_path(gold):
    """the second image's masks at another resolution (nearest-resized by 2 in x): per-image calls, finite losses, the same
    assignment machinery; against the one-group path on equal sizes the first image's matches are unchanged"""
    g, meta = gold
    head = build_head(meta, 'cpu')
    masks, clss, gt_labels, gt_masks = inputs(g, meta, 'full', 'cpu')
    gt_masks = [gt_masks[0], gt_masks[1].repeat_interleave(2, dim=2)]
    replay(head, g, 'full')
    losses = head.loss(clss, masks, gt_labels, gt_masks, [None] * meta['N'])
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    assert all(bool(torch.isfinite(m.grad).all()) for m in masks)


def test_constructor_and_loss_errors(gold):
    from vitadapter import Mask2FormerHead
    _, meta = gold

    def cfg(**edit):
        c = head_config(meta)
        for path, v in edit.items():
            d = c
            keys = path.split('__')
            for k in keys[:-1]:
                d = d[k]
            d[keys[-1]] = v
        return c
    Mask2FormerHead(**cfg())
    with pytest.raises(ValueError, match='loss_mask'):
        Mask2FormerHead(**cfg(loss_mask__use_sigmoid=False))
    with pytest.raises(ValueError, match='loss_dice'):
        Mask2FormerHead(**cfg(loss_dice__naive_dice=False))
    with pytest.raises(ValueError, match='loss_cls'):
        Mask2FormerHead(**cfg(loss_cls__use_sigmoid=True))
    with pytest.raises(ValueError, match='assigner'):
        Mask2FormerHead(**cfg(train_cfg__assigner__type='HungarianAssigner'))
    with pytest.raises(ValueError, match='assigner'):
        Mask2FormerHead(**cfg(train_cfg__assigner__mask_cost=dict(type='FocalLossCost', weight=2.0)))
    with pytest.raises(ValueError, match='assigner'):
        Mask2FormerHead(**cfg(train_cfg__assigner__dice_cost__pred_act=False))
    with pytest.raises(ValueError, match='sampler'):
        Mask2FormerHead(**cfg(train_cfg__sampler=dict(type='RandomSampler')))
    head = Mask2FormerHead(**cfg(train_cfg=None))
    assert head.num_points is None and head.match_weights is None
    with pytest.raises(ValueError, match='train_cfg'):
        head.loss([torch.zeros(1, 8, 6)], [torch.zeros(1, 8, 4, 4)], [torch.zeros(0, dtype=torch.long)],
                  [torch.zeros(0, 8, 8, dtype=torch.uint8)], [None])
    for name in ('loss', 'forward_train', 'forward_test', '_draw'):
        assert callable(getattr(head, name))


def test_draw_is_uniform_rand():
    from vitadapter import Mask2FormerHead
    torch.manual_seed(3)
    a = Mask2FormerHead._draw(None, 'match', 0, 0, (2, 5, 2), 'cpu')
    torch.manual_seed(3)
    assert torch.equal(a, torch.rand((2, 5, 2))) and a.dtype == torch.float32
