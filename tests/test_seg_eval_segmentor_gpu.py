"""GPU: evaluate_batch of vitadapter.segmentor on the toy segmentor of tests/segmentor_case.py: image in, totals out,
without leaving the device.

For slide and whole mode and for aug_test with a flipped view, ``evaluate_batch`` + ``SegEvaluator.compute()`` must equal
the reference of tests/seg_eval_ref.py fed with the numpy output of ``simple_test`` / ``aug_test`` (exactly: counts of the
same label maps), those two must still return the golden's label maps, and ENABLED['seg_eval'] off must give the same
totals."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_eval_ref as ref  # noqa: E402
import segmentor_case  # noqa: E402

from vitadapter import EncoderDecoderMask2Former, EncoderDecoderMask2FormerAug, SegEvaluator, fused  # noqa: E402

pytestmark = pytest.mark.gpu

CASE = segmentor_case.Case()
C = CASE.meta['classes']
ORI = tuple(CASE.ori[:2])


def dev():
    return torch.device('cuda:0')


def ground_truth(seed=0):
    """(1, H, W) uint8: blobs over the classes with an ignored band, at ori_shape"""
    rng = np.random.default_rng(seed)
    gt = ref.blobs(rng, (1,) + ORI, C, cell=6).astype(np.uint8)
    gt[:, :3] = 255
    return gt


def _inputs(aug):
    if aug:
        return ([CASE.image(v, torch.float32, dev()) for v in CASE.views], [CASE.metas(v) for v in CASE.views])
    v0 = CASE.views[0]
    return CASE.image(v0, torch.float32, dev()), CASE.metas(v0)


@pytest.mark.parametrize('cls,mode,aug,gold', [(EncoderDecoderMask2Former, 'slide', False, 'b_simple_test'),
                                               (EncoderDecoderMask2FormerAug, 'slide', False, 'a_simple_test'),
                                               (EncoderDecoderMask2Former, 'whole', False, 'b_whole_simple_test'),
                                               (EncoderDecoderMask2FormerAug, 'slide', True, 'a_aug_test'),
                                               (EncoderDecoderMask2Former, 'slide', True, 'b_aug_test')],
                         ids=['slide', 'slide-aug-class', 'whole', 'aug_test', 'aug_test-base-class'])
def test_evaluate_batch_equals_the_reference_on_the_numpy_output(cls, mode, aug, gold):
    assert any(v['flip'] for v in CASE.views)                       # aug_test sees a flipped view
    seg = CASE.build(cls, mode=mode, dtype=torch.float32, device=dev())
    img, metas = _inputs(aug)
    gt = ground_truth()
    with torch.no_grad():
        host = seg.aug_test(img, metas) if aug else seg.simple_test(img, metas)
        assert isinstance(host, list) and host[0].dtype == np.int64 and np.array_equal(np.stack(host), CASE.gold[gold])
        want = ref.counts(np.stack(host), gt, C)
        assert want[0].sum() > 0
        totals = {}
        for on in (True, False):
            keep = fused.ENABLED['seg_eval']
            fused.ENABLED['seg_eval'] = on
            try:
                ev = SegEvaluator(C)
                for gt_in in (torch.from_numpy(gt).to(dev()), gt[:, None]):      # a device tensor; an (N, 1, H, W) array
                    labels = seg.evaluate_batch(img, metas, gt_in, ev)
                    assert labels.is_cuda and labels.dtype == torch.int64 and np.array_equal(labels.cpu().numpy(), np.stack(host))
            finally:
                fused.ENABLED['seg_eval'] = keep
            assert ev.totals.is_cuda
            totals[on] = ev.totals.cpu().numpy()
            got, r = ev.compute(), ref.metrics(2 * want)
            for k in r:
                assert np.allclose(got[k], r[k], rtol=1e-12, atol=0, equal_nan=True), k
        assert np.array_equal(totals[True], 2 * want) and np.array_equal(totals[False], totals[True])
        with pytest.raises(ValueError):
            seg.evaluate_batch(img, metas, torch.from_numpy(gt[:, :-1]).to(dev()), SegEvaluator(C))


def test_the_labels_methods_are_the_tests_without_the_copy():
    seg = CASE.build(EncoderDecoderMask2FormerAug, dtype=torch.float32, device=dev())
    img, metas = _inputs(False)
    imgs, all_metas = _inputs(True)
    with torch.no_grad():
        lab = seg.simple_test_labels(img, metas)
        assert lab.is_cuda and lab.shape == (1,) + ORI and np.array_equal(lab.cpu().numpy(), np.stack(seg.simple_test(img, metas)))
        lab = seg.aug_test_labels(imgs, all_metas)
        assert lab.is_cuda and np.array_equal(lab.cpu().numpy(), np.stack(seg.aug_test(imgs, all_metas)))
        raw = seg.simple_test_labels(img, metas, rescale=False)
        assert np.array_equal(raw.cpu().numpy(), np.stack(seg.simple_test(img, metas, rescale=False)))
