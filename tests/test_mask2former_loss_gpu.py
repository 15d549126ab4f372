"""GPU: Mask2FormerHead.loss with its matching on the point kernels against tests/golden/mask2former_loss.npz, with ENABLED['point_loss'] on and
off from the golden's fp32 mask_pred / cls_score, so that both sides see identical inputs.

Rule (that of tests/test_mask2former_head_gpu.py, with a floor because both sides are fp32 here): the assignments and chosen
points are the golden's exactly on both sides; each loss and each gradient of the kernel side has an error against the golden
of at most 2 x the torch side's or 16 * 2^-24 * |golden| (a gradient: its largest element), whichever is larger.
What the two sides share: the sampled BCE / dice of the matched masks and their backward are F.grid_sample on both, so for the
losses and the mask_pred gradients the rule holds the kernel side only through what the kernels feed them - the sampled ground
truth, and the assignments and chosen points, which the exact comparison above pins.  The kernels themselves are held to fp64
in tests/test_point_loss_fp64_gpu.py.
Also: one forward_train of the small head under bf16 autocast gives finite losses and a finite gradient in every parameter."""
import json

import numpy as np
import pytest
import torch

import test_mask2former_head_cpu as head_helpers
import test_mask2former_loss_cpu as helpers

pytestmark = pytest.mark.gpu
FLOOR = 16 * 2.0 ** -24


@pytest.fixture(scope='module')
def gold():
    g = np.load(helpers.GOLD)
    return g, json.loads(str(g['meta']))


def _side(g, meta, variant, on):
    from vitadapter import fused
    dev = torch.device('cuda:0')
    keep = fused.ENABLED['point_loss']
    fused.ENABLED['point_loss'] = on
    try:
        head = helpers.build_head(meta, dev)
        masks, clss, losses, _ = helpers.run_loss(head, g, meta, variant, dev)
        helpers.check_choices(head, g, meta, variant)
        return helpers.errors(g, meta, variant, masks, clss, losses)
    finally:
        fused.ENABLED['point_loss'] = keep


@pytest.mark.parametrize('variant', ['full', 'one_empty', 'none'])
def test_loss_on_the_kernels_against_golden_and_torch(gold, variant):
    g, meta = gold
    k_loss, k_grad, top = _side(g, meta, variant, True)
    t_loss, t_grad, _ = _side(g, meta, variant, False)
    want = g['%s_losses' % variant]
    for j, key in enumerate(meta['loss_keys']):
        print('ERR %s %s kernel %.3e torch %.3e golden %.6f' % (variant, key, k_loss[key], t_loss[key], want[j]))
    for name in k_grad:
        print('ERR %s %s kernel %.3e torch %.3e top %.3e' % (variant, name, k_grad[name], t_grad[name], top[name]))
    for j, key in enumerate(meta['loss_keys']):
        assert k_loss[key] <= max(2 * t_loss[key], FLOOR * abs(want[j])), (key, k_loss[key], t_loss[key], want[j])
    for name in k_grad:
        assert k_grad[name] <= max(2 * t_grad[name], FLOOR * top[name]), (name, k_grad[name], t_grad[name], top[name])


def test_forward_train_under_bf16_autocast(gold):
    g, meta = gold
    dev = torch.device('cuda:0')
    pdg = np.load(head_helpers.PD_GOLD)
    torch.manual_seed(0)
    head = helpers.build_head(meta, 'cpu')
    head.init_weights()
    head = head.to(dev)
    feats = head_helpers.feats_of(pdg, dev)
    _, _, gt_labels, gt_masks = helpers.inputs(g, meta, 'full', dev)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        losses = head.forward_train(feats, [None] * meta['N'], None, gt_labels, gt_masks)
    assert list(losses) == meta['loss_keys']
    assert all(v.dtype == torch.float32 and bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for k, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert all(f.grad is not None and bool(torch.isfinite(f.grad).all()) for f in feats)
