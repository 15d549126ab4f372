"""CPU: the counting rule and the metrics of the mIoU evaluation (vitadapter/evaluation.py, vitadapter.fused.seg_eval_update)
against tests/seg_eval_ref.py.

The reference is first held to a hand-counted 3 x 4 case and to mmseg 0.20's torch.histc formulation (C >= 2: for C == 1 histc
counts everything, a documented difference); then the torch fallback of seg_eval_update must give the reference's counts
exactly, and every metric the reference's float64 value to 1e-12 relative (the same formula in the same type: a few ulps).
SegEvaluator: several updates equal one over the concatenation, reset, the keys and rounding of summary(), and all_reduce
over a 2-process gloo group by the method of tests/test_data_parallel_cpu.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_eval_ref as ref  # noqa: E402

import vitadapter  # noqa: E402
from vitadapter import SegEvaluator, evaluation, fused  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_CASES = [(C, ig, rz) for C in (2, 3, 19, 150) for ig in (255, 0, 7) for rz in (False, True)]


def _maps(seed, C, shape=(2, 23, 31)):
    """predictions and labels with values outside [0, C) among the valid ones"""
    rng = np.random.default_rng(seed)
    pred = rng.integers(-2, C + 3, size=shape).astype(np.int64)
    label = rng.integers(0, min(C + 40, 256), size=shape).astype(np.uint8)
    label[rng.random(shape) < 0.1] = 255
    return pred, label


def test_hand_counted_case():
    pred = np.array([[0, 1, 1, 2],
                     [2, 2, 0, 3],
                     [-1, 1, 0, 1]])
    label = np.array([[0, 1, 2, 2],
                      [255, 2, 1, 0],
                      [1, 255, 0, 5]])
    # ignored: (1, 0) and (2, 1).  pred 3 and -1 and label 5 are outside [0, 3)
    want = np.array([[2, 1, 2],             # agree: (0,0) (2,2) | (0,1) | (0,3) (1,1)
                     [3, 3, 2],             # pred 0: (0,0) (1,2) (2,2); 1: (0,1) (0,2) (2,3); 2: (0,3) (1,1), not the ignored (1,0)
                     [3, 3, 3]])            # label 0: (0,0) (1,3) (2,2); 1: (0,1) (1,2) (2,0); 2: (0,2) (0,3) (1,1)
    assert np.array_equal(ref.counts_loop(pred, label, 3), want)
    assert np.array_equal(ref.counts(pred, label, 3), want)
    # reduce_zero_label: labels 0 and 255 are ignored, the others move down by one.  Kept pixels (0,1) (0,2) (0,3) (1,1) (1,2)
    # (2,0) (2,3) with preds 1 1 2 2 0 -1 1 and labels 0 1 1 1 0 0 4
    want = np.array([[1, 1, 0],             # agree: (1,2) | (0,2)
                     [1, 3, 2],
                     [3, 3, 0]])
    assert np.array_equal(ref.counts_loop(pred, label, 3, reduce_zero_label=True), want)
    assert np.array_equal(ref.counts(pred, label, 3, reduce_zero_label=True), want)
    # a label_map chain applies to the original values: 1 -> 2 and 2 -> 0 leaves no 1, and the old 1s are 2s
    got = ref.counts_loop(pred, label, 3, label_map={1: 2, 2: 0})
    assert np.array_equal(got[2], [6, 0, 3]) and np.array_equal(got, ref.counts(pred, label, 3, label_map={1: 2, 2: 0}))


@pytest.mark.parametrize('C,ignore,reduce_zero', FLAG_CASES)
def test_reference_against_histc(C, ignore, reduce_zero):
    pred, label = _maps(C, C)
    want = ref.histc_counts(pred, label, C, ignore, reduce_zero)
    assert np.array_equal(ref.counts(pred, label, C, ignore, reduce_zero), want)
    assert np.array_equal(ref.counts_loop(pred, label, C, ignore, reduce_zero), want)


@pytest.mark.parametrize('C,ignore,reduce_zero', FLAG_CASES + [(1, 255, False), (1, 0, True), (4096, 255, False)])
@pytest.mark.parametrize('label_map', [None, {0: 3, 3: 1, 1: 255, 200: 0}])
def test_fallback_equals_the_reference(C, ignore, reduce_zero, label_map):
    pred, label = _maps(C + 1, C)
    want = ref.counts(pred, label, C, ignore, reduce_zero, label_map)
    for lab in (torch.from_numpy(label), torch.from_numpy(label).long(), torch.from_numpy(label)[:, None], torch.from_numpy(label).int()):
        totals = torch.full((3, C), 5, dtype=torch.int64)
        out = fused.seg_eval_update(torch.from_numpy(pred), lab, totals, C, ignore, reduce_zero, label_map)
        assert out is totals and totals.dtype == torch.int64
        assert np.array_equal(totals.numpy() - 5, want)
    areas = evaluation.intersect_and_union(pred[0], label[0], C, ignore, label_map, reduce_zero)
    one = ref.counts(pred[0], label[0], C, ignore, reduce_zero, label_map)
    assert all(a.dtype == torch.int64 for a in areas)
    assert np.array_equal(areas[0].numpy(), one[0]) and np.array_equal(areas[1].numpy(), one[1] + one[2] - one[0])
    assert np.array_equal(areas[2].numpy(), one[1]) and np.array_equal(areas[3].numpy(), one[2])


def test_int64_labels_and_a_negative_ignore_index():
    rng = np.random.default_rng(3)
    pred = rng.integers(0, 5, size=(1, 9, 11)).astype(np.int64)
    label = rng.integers(-1, 5, size=(1, 9, 11)).astype(np.int64)
    totals = torch.zeros((3, 5), dtype=torch.int64)
    fused.seg_eval_update(torch.from_numpy(pred), torch.from_numpy(label), totals, 5, ignore_index=-1)
    assert np.array_equal(totals.numpy(), ref.counts(pred, label, 5, -1))
    with pytest.raises(ValueError):
        fused.seg_eval_update(torch.from_numpy(pred), torch.from_numpy(label)[:, :8], totals, 5)
    with pytest.raises(ValueError):
        fused.seg_eval_update(torch.from_numpy(pred), torch.from_numpy(label), totals.float(), 5)


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok]))


def test_metrics_against_the_reference():
    C = 6
    pred, label = _maps(11, C - 1)
    pred, label = np.clip(pred, -2, 4), np.where(label >= 5, 255, label).astype(np.uint8)    # class 5 is absent from both maps: 0 / 0
    totals = ref.counts(pred, label, C)
    assert totals[1, 5] == 0 and totals[2, 5] == 0
    ev = SegEvaluator(C)
    ev.update(torch.from_numpy(pred), torch.from_numpy(label))
    assert np.array_equal(ev.totals.numpy(), totals)
    for names, kw in ((('mIoU',), {}), (('mDice',), {}), (('mFscore',), dict(beta=2)), (('mIoU', 'mDice', 'mFscore'), dict(beta=0.5)),
                      (('mIoU', 'mFscore'), dict(nan_to_num=-1))):
        got, want = ev.compute(names, **kw), ref.metrics(totals, names, **kw)
        assert list(got) == list(want)
        for k in want:
            _close(got[k], want[k])
    got = ev.compute()
    assert np.isnan(got['IoU'][5]) and np.isnan(got['Acc'][5]) and not np.isnan(got['IoU'][:5]).any()
    s = ev.summary()
    assert s['mIoU'] == round(float(np.nanmean(got['IoU'])) * 100, 2) / 100          # the absent class is skipped
    assert ev.compute(nan_to_num=0)['IoU'][5] == 0 and ev.summary(nan_to_num=0)['mIoU'] < s['mIoU']
    fs = ev.compute(('mFscore',), beta=2)
    p, r = fs['Precision'][:5], fs['Recall'][:5]
    _close(fs['Fscore'][:5], 5 * p * r / (4 * p + r))
    _close(ev.compute(('mDice',))['Dice'][:5], 2 * totals[0, :5] / (totals[1, :5] + totals[2, :5]))
    with pytest.raises(KeyError):
        ev.compute(('mAP',))
    # the functions under mmseg's names, on lists of maps of different sizes
    results, gts = [pred[0], pred[1][:7]], [label[0], label[1][:7]]
    tot = ref.counts(results[0], gts[0], C) + ref.counts(results[1], gts[1], C)
    areas = evaluation.total_intersect_and_union(results, gts, C, 255)
    assert np.array_equal(torch.stack([areas[0], areas[2], areas[3]]).numpy(), tot)
    want = ref.metrics(tot, ('mIoU', 'mDice', 'mFscore'))
    _close(evaluation.mean_iou(results, gts, C, 255)['IoU'], want['IoU'])
    _close(evaluation.mean_dice(results, gts, C, 255)['Dice'], want['Dice'])
    _close(evaluation.mean_fscore(results, gts, C, 255)['Fscore'], want['Fscore'])
    _close(evaluation.eval_metrics(results, gts, C, 255, ['mIoU'])['aAcc'], want['aAcc'])
    pre = [evaluation.intersect_and_union(r, g, C, 255) for r, g in zip(results, gts)]
    _close(evaluation.pre_eval_to_metrics(pre, ['mIoU'])['IoU'], want['IoU'])
    _close(evaluation.total_area_to_metrics(*areas, 'mIoU')['Acc'], want['Acc'])


def test_updates_accumulate_and_reset():
    C = 19
    pred, label = _maps(5, C, shape=(4, 17, 29))
    whole, parts = SegEvaluator(C, reduce_zero_label=True, label_map={4: 9}), SegEvaluator(C, reduce_zero_label=True, label_map={4: 9})
    whole.update(pred, label)
    for i in range(4):
        parts.update(torch.from_numpy(pred[i]), torch.from_numpy(label[i:i + 1])[:, None] if i % 2 else label[i])
    assert torch.equal(whole.totals, parts.totals)
    assert np.array_equal(whole.totals.numpy(), ref.counts(pred, label, C, 255, True, {4: 9}))
    parts.reset()
    assert int(parts.totals.abs().sum()) == 0
    parts.update(pred[:1], label[:1])
    assert np.array_equal(parts.totals.numpy(), ref.counts(pred[:1], label[:1], C, 255, True, {4: 9}))
    assert int(SegEvaluator(C).totals.sum()) == 0           # before any update
    with pytest.raises(ValueError):
        whole.update(pred, label[:, :5])
    with pytest.raises(TypeError):
        whole.update('a.png', label)


def test_summary_keys_and_rounding():
    names = ('road', 'car', 'sky')
    ev = SegEvaluator(3, class_names=names)
    ev.totals.copy_(torch.tensor([[1, 2, 0], [3, 3, 0], [7, 2, 0]]))
    s = ev.summary(('mIoU', 'mFscore'))
    assert list(s) == ['aAcc', 'mIoU', 'mAcc', 'mFscore', 'mPrecision', 'mRecall'] + [
        '%s.%s' % (k, n) for k in ('IoU', 'Acc', 'Fscore', 'Precision', 'Recall') for n in names]
    iou = np.array([1 / 9, 2 / 3])
    assert s['aAcc'] == round(3 / 9 * 100, 2) / 100 == 33.33 / 100
    assert s['mIoU'] == round(float(iou.mean()) * 100, 2) / 100
    assert s['IoU.road'] == round(1 / 9 * 100, 2) / 100 == 11.11 / 100 and s['IoU.car'] == 66.67 / 100 and np.isnan(s['IoU.sky'])
    assert s['Acc.road'] == 14.29 / 100 and s['mAcc'] == round((1 / 7 + 1.0) / 2 * 100, 2) / 100
    assert list(SegEvaluator(2).summary()) == ['aAcc', 'mIoU', 'mAcc', 'IoU.0', 'IoU.1', 'Acc.0', 'Acc.1']
    with pytest.raises(ValueError):
        SegEvaluator(3, class_names=('a',))
    for name in ('SegEvaluator', 'intersect_and_union', 'total_intersect_and_union', 'total_area_to_metrics', 'pre_eval_to_metrics',
                 'eval_metrics', 'mean_iou', 'mean_dice', 'mean_fscore'):
        assert name in vitadapter.__all__ and getattr(vitadapter, name) is getattr(evaluation, name)


# ----------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.set_num_threads(1)
    for p in (ROOT, os.path.join(ROOT, 'vit-adapter_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    from vitadapter import SegEvaluator as Evaluator
    torch.distributed.init_process_group('gloo', rank=rank, world_size=world)
    pred, label = _maps(21, 19, shape=(4, 17, 29))
    ev = Evaluator(19, reduce_zero_label=True)
    ev.update(pred[rank::world], label[rank::world])
    ev.all_reduce()
    torch.save(ev.totals, os.path.join(out_dir, 'totals_rank%d.pt' % rank))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_all_reduce_over_two_gloo_ranks(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    pred, label = _maps(21, 19, shape=(4, 17, 29))
    ev = SegEvaluator(19, reduce_zero_label=True)
    ev.update(pred, label)
    ev.all_reduce()                                         # no process group here: nothing happens
    for rank in range(world):
        got = torch.load(os.path.join(tmp_path, 'totals_rank%d.pt' % rank), weights_only=True)
        assert got.dtype == torch.int64 and torch.equal(got, ev.totals), rank
