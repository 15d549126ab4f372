"""GPU: fused.point_mask_losses on the kernels of csrc/point_mask_loss.hip through autograd, against the same function with
ENABLED['point_mask_loss'] off (torch's F.grid_sample expression; ENABLED['point_loss'] stays on on both sides), on the inputs of
tests/golden/mask2former_loss.npz with the helpers of tests/test_mask2former_loss_cpu.py.

Rule (that of tests/test_mask2former_loss_gpu.py): the assignments and chosen points are the golden's exactly on both sides; each
loss and each gradient of the kernel side has an error against the golden of at most 2 x the torch side's or 16 * 2^-24 *
|golden| (a gradient: its largest element), whichever is larger.  Whether the path ran is read from the launch profile: one
pml_forward and one pml_backward row per decoder output with a match, none with the switch off.
Also: ``rows`` with a repeat gives the sum of the two rows' gradients, bit for bit; loss + backward twice gives bit-equal
mask_pred gradients; masks of different sizes (per-image calls) run on the kernels and stay finite."""
import json

import numpy as np
import pytest
import torch

import test_mask2former_loss_cpu as helpers

pytestmark = pytest.mark.gpu
FLOOR = 16 * 2.0 ** -24


@pytest.fixture(scope='module')
def gold():
    g = np.load(helpers.GOLD)
    return g, json.loads(str(g['meta']))


def _counted(fn):
    """fn() with the pml rows of the launch profile counted -> fn's result, {row: calls}"""
    import _vah
    _vah.prof_enable(True, 'pml_')
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        _vah.prof_enable(False)
    return res, {k: r['calls'] for k, r in _vah.prof_report().items()}


class _Switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from vitadapter import fused
        assert fused.ENABLED['point_mask_loss'] and fused.ENABLED['point_loss']
        fused.ENABLED['point_mask_loss'] = self.on

    def __exit__(self, *exc):
        from vitadapter import fused
        fused.ENABLED['point_mask_loss'] = True
        return False


def _side(g, meta, variant, on):
    dev = torch.device('cuda:0')
    with _Switch(on):
        head = helpers.build_head(meta, dev)

        def run():
            masks, clss, losses, _ = helpers.run_loss(head, g, meta, variant, dev)
            helpers.check_choices(head, g, meta, variant)
            return helpers.errors(g, meta, variant, masks, clss, losses), masks
        return _counted(run)


@pytest.mark.parametrize('variant', ['full', 'one_empty', 'none'])
def test_losses_and_gradients_against_golden_and_torch(gold, variant):
    g, meta = gold
    ((k_loss, k_grad, top), _), k_calls = _side(g, meta, variant, True)
    ((t_loss, t_grad, _), _), t_calls = _side(g, meta, variant, False)
    n = meta['L'] if sum(meta['variants'][variant]) else 0
    assert k_calls == ({'pml_forward': n, 'pml_backward': n} if n else {}), k_calls
    assert t_calls == {}, t_calls
    want = g['%s_losses' % variant]
    for j, key in enumerate(meta['loss_keys']):
        print('ERR %s %s kernel %.3e torch %.3e golden %.6f' % (variant, key, k_loss[key], t_loss[key], want[j]))
    for name in k_grad:
        print('ERR %s %s kernel %.3e torch %.3e top %.3e' % (variant, name, k_grad[name], t_grad[name], top[name]))
    for j, key in enumerate(meta['loss_keys']):
        assert k_loss[key] <= max(2 * t_loss[key], FLOOR * abs(want[j])), (key, k_loss[key], t_loss[key], want[j])
    for name in k_grad:
        assert k_grad[name] <= max(2 * t_grad[name], FLOOR * top[name]), (name, k_grad[name], t_grad[name], top[name])


def test_loss_and_backward_twice_give_the_same_bits(gold):
    g, meta = gold
    (_, masks_a), calls = _side(g, meta, 'full', True)
    (_, masks_b), _ = _side(g, meta, 'full', True)
    assert calls.get('pml_backward') == meta['L']
    for a, b in zip(masks_a, masks_b):
        assert a.grad is not None and float(a.grad.abs().max()) > 0
        assert torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32))


def _direct(g, meta, rows, tgt_rows, points, weights):
    from vitadapter import fused
    dev = torch.device('cuda:0')
    masks, _, _, gt_masks = helpers.inputs(g, meta, 'full', dev)
    pred, tgt = masks[0], torch.cat(gt_masks)
    bce, dice = fused.point_mask_losses(pred, rows, tgt, tgt_rows, points.to(dev), 1.0)
    wb, wd = weights
    ((bce * wb.to(dev)).sum() + (dice * wd.to(dev)).sum()).backward()
    return bce.detach().cpu(), dice.detach().cpu(), pred.grad.cpu()


def test_rows_with_a_repeat_give_the_sum_of_the_two_gradients(gold):
    g, meta = gold
    gen = torch.Generator().manual_seed(1)
    P = 65
    points = torch.rand((3, P, 2), generator=gen)
    wb, wd = torch.tensor([0.5, -1.0, 2.0]), torch.tensor([1.5, 0.25, -0.75])
    (both, calls) = _counted(lambda: _direct(g, meta, [3, 1, 3], [0, 1, 2], points, (wb, wd)))
    assert calls == {'pml_forward': 1, 'pml_backward': 1}, calls
    first = _direct(g, meta, [3, 1], [0, 1], points[:2], (wb[:2], wd[:2]))
    second = _direct(g, meta, [3], [2], points[2:], (wb[2:], wd[2:]))
    assert torch.equal(both[0], torch.cat([first[0], second[0]])) and torch.equal(both[1], torch.cat([first[1], second[1]]))
    assert float(second[2].flatten(0, 1)[3].abs().max()) > 0 and float(first[2].flatten(0, 1)[3].abs().max()) > 0
    assert torch.equal(both[2], first[2] + second[2])
    # against the torch path: the same gradient to fp32
    with _Switch(False):
        ref, calls = _counted(lambda: _direct(g, meta, [3, 1, 3], [0, 1, 2], points, (wb, wd)))
    assert calls == {}, calls
    top = float(ref[2].abs().max())
    assert float((both[2] - ref[2]).abs().max()) <= 64 * 2.0 ** -24 * top
    assert float((both[0] - ref[0]).abs().max()) <= 64 * 2.0 ** -24 * float(ref[0].abs().max())


def test_masks_of_different_sizes_run_on_the_kernels_and_stay_finite(gold):
    """the input of test_masks_of_different_sizes_take_the_per_image_path: the second image's masks at another resolution"""
    g, meta = gold
    dev = torch.device('cuda:0')
    head = helpers.build_head(meta, dev)
    masks, clss, gt_labels, gt_masks = helpers.inputs(g, meta, 'full', dev)
    gt_masks = [gt_masks[0], gt_masks[1].repeat_interleave(2, dim=2)]
    helpers.replay(head, g, 'full')

    def run():
        losses = head.loss(clss, masks, gt_labels, gt_masks, [None] * meta['N'])
        sum(losses.values()).backward()
        return losses
    losses, calls = _counted(run)
    assert calls.get('pml_forward', 0) >= meta['L'] and calls.get('pml_backward', 0) == calls['pml_forward'], calls
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert all(bool(torch.isfinite(m.grad).all()) for m in masks)
