"""GPU: Mask2FormerHead.loss with the assignment on the device (fused.hungarian_match on csrc/assign.hip), with the helpers and the
golden of tests/test_mask2former_loss_cpu.py.

(a) With scipy's linear_sum_assignment replaced by a function that raises, the three variants of the golden pass
    ``check_choices`` (the assignments and chosen points are the golden's exactly), and every loss and every gradient is
    BIT-EQUAL to a run of the same process with ENABLED['hungarian'] off and scipy back: the two paths hand identical tables to
    identical kernels.
(b) With the targets a fused.SegTargets, ``loss`` + ``backward`` run under torch.cuda.set_sync_debug_mode('error') after one
    warm-up call: no host synchronisation at all.  Reading ``last_assignment`` afterwards (outside the mode: that read is the
    copy) gives scipy's assignment of the costs the step recorded.
(c) ``check_last_match`` raises after a step whose cls_score holds a NaN, that step's losses are NaN, and it is silent after a
    clean step."""
import json

import numpy as np
import pytest
import torch

import hungarian_ref as ref
import test_mask2former_loss_cpu as helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    g = np.load(helpers.GOLD)
    return g, json.loads(str(g['meta']))


def dev():
    return torch.device('cuda:0')


def _no_scipy(*args, **kwargs):
    raise AssertionError('scipy.optimize.linear_sum_assignment was called on the device path')


def _run(g, meta, variant, check):
    head = helpers.build_head(meta, dev())
    masks, clss, losses, _ = helpers.run_loss(head, g, meta, variant, dev())
    if check:
        helpers.check_choices(head, g, meta, variant)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in losses.items()}, [None if t.grad is None else t.grad.clone() for t in masks + clss],
            head)


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('variant', ['full', 'one_empty', 'none'])
def test_device_matching_gives_the_goldens_choices_and_the_host_paths_bits(gold, variant, monkeypatch):
    import scipy.optimize
    from vitadapter import fused
    g, meta = gold
    assert fused.ENABLED['hungarian'] is True
    with monkeypatch.context() as m:
        m.setattr(scipy.optimize, 'linear_sum_assignment', _no_scipy)
        on_losses, on_grads, head = _run(g, meta, variant, check=True)
        if sum(meta['variants'][variant]):
            assert head._last_match[1] is not None and not bool(head._last_match[1].any())
            head.check_last_match()
    monkeypatch.setitem(fused.ENABLED, 'hungarian', False)
    off_losses, off_grads, head_off = _run(g, meta, variant, check=True)
    assert head_off._last_match[1] is None
    assert list(on_losses) == list(off_losses) == meta['loss_keys']
    for k in on_losses:
        assert _same_bits(on_losses[k], off_losses[k]), (k, float(on_losses[k]), float(off_losses[k]))
    assert len(on_grads) == len(off_grads) == 2 * meta['L']
    for j, (a, b) in enumerate(zip(on_grads, off_grads)):
        assert _same_bits(a, b), j


def _sync_mode_reports():
    probe = torch.ones(1, device=dev())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        probe.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return False


def _small_step(meta, seed):
    """random predictions at the golden's shapes and a label map with a few classes per image"""
    gen = torch.Generator().manual_seed(seed)
    N, Q, L = meta['N'], meta['Q'], meta['L']
    C1 = meta['things'] + meta['stuff'] + 1
    masks = [(torch.randn((N, Q, 16, 16), generator=gen) * 3).to(dev()).requires_grad_(True) for _ in range(L)]
    clss = [(torch.randn((N, Q, C1), generator=gen) * 2).to(dev()).requires_grad_(True) for _ in range(L)]
    label = torch.randint(0, min(4, C1 - 1), (N, 8, 8), generator=gen).repeat_interleave(8, 1).repeat_interleave(8, 2).to(torch.uint8)
    label[:, :5, :] = 255                                            # some ignored pixels
    return masks, clss, label.to(dev())


def test_no_host_synchronisation_with_device_targets(gold, monkeypatch):
    from vitadapter import fused
    if not _sync_mode_reports():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not report a .item() on this build")
    _, meta = gold
    head = helpers.build_head(meta, dev())
    masks, clss, label = _small_step(meta, 3)
    targets = fused.seg_targets(label)
    assert isinstance(targets, fused.SegTargets) and sum(targets.counts) > 0
    seen = {}
    real = fused.hungarian_match

    def spy(costs, counts, gt_offsets=None):
        seen['costs'], seen['counts'] = torch.stack(list(costs)).clone(), list(counts)
        return real(costs, counts, gt_offsets=gt_offsets)
    monkeypatch.setattr(fused, 'hungarian_match', spy)
    metas = [None] * meta['N']
    sum(head.loss(clss, masks, targets, None, metas).values()).backward()          # warm-up: constants, code objects
    torch.cuda.synchronize()
    for t in masks + clss:
        t.grad = None
    torch.cuda.set_sync_debug_mode('error')
    try:
        losses = head.loss(clss, masks, targets, None, metas)
        sum(losses.values()).backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in masks + clss)
    head.check_last_match()
    costs, counts = seen['costs'].cpu().numpy(), seen['counts']
    assert counts == targets.counts
    for i in range(meta['L']):
        for n in range(meta['N']):
            got = torch.stack(head.last_assignment[i][n]).numpy()
            q, t = ref.scipy_pairs(costs[i, n, :, :counts[n]].astype(np.float64)) if counts[n] else (np.zeros(0), np.zeros(0))
            assert np.array_equal(got, np.stack([q, t])), (i, n)


def test_check_last_match_raises_after_an_invalid_step_only(gold):
    from vitadapter import fused
    _, meta = gold
    head = helpers.build_head(meta, dev())
    masks, clss, label = _small_step(meta, 4)
    targets = fused.seg_targets(label)
    metas = [None] * meta['N']
    losses = head.loss(clss, masks, targets, None, metas)
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    head.check_last_match()                                          # a clean step: silent
    with torch.no_grad():
        poisoned = [c.detach().clone() for c in clss]
        poisoned[0][1, 2, 0] = float('nan')                          # decoder output 0, image 1
    losses = head.loss(poisoned, masks, targets, None, metas)
    assert list(losses) == meta['loss_keys'] and all(bool(torch.isnan(v)) for v in losses.values())      # every output's, not only output 0's
    with pytest.raises(ValueError, match=ref.INVALID) as info:
        head.check_last_match()
    assert 'decoder output 0, image 1' in str(info.value)
    assert head._last_match[1].cpu().tolist()[0] == [0, 1] and not bool(head._last_match[1][1:].any())
    losses = head.loss(clss, masks, targets, None, metas)
    head.check_last_match()
    assert all(bool(torch.isfinite(v)) for v in losses.values())
