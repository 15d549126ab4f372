"""mIoU evaluation that stays on the device: label maps in, ``mIoU`` out, one host read at the end.

Every segmentation config of the reference ends in ``evaluation = dict(interval=..., metric='mIoU', save_best='mIoU')``; the
evaluator behind it is mmseg's (mmseg/core/evaluation/metrics.py and CustomDataset.evaluate of mmseg 0.20), which is not part
of the reference tree.  The public names, signatures and result keys below are mmseg's, restated from its published code;
parity with an installed mmseg is unpinned, as for vitadapter.heads (there is none to compare with here).

What differs is where the counting happens and in which type:
  * ``intersect_and_union`` counts with vitadapter.fused.seg_eval_update - on the GPU the kernels of
    include/vitadapter_hip_seg_eval.h, elsewhere masks and ``torch.bincount`` - and returns INT64 tensors on the inputs'
    device.  mmseg returns float32 ``torch.histc`` counts, which stop being exact at 2^24 pixels of a class.
  * ``label_map`` entries all apply to the original label (mmseg 0.20 applies them one after another in place, so a chain
    ``a -> b, b -> c`` sends ``a`` to ``c``; later mmseg versions map simultaneously, as here), and ``num_classes == 1``
    follows the general rule (mmseg's ``histc(min=0, max=0)`` counts everything).
  * The metrics are computed in float64 on the host from the int64 totals.
``SegEvaluator`` keeps the 3 x num_classes totals of a validation set on the device: ``update`` launches and returns,
``compute`` / ``summary`` are the single device-to-host copy.  File names as inputs (mmseg loads them) are not supported.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import fused

__all__ = ['f_score', 'intersect_and_union', 'total_intersect_and_union', 'mean_iou', 'mean_dice', 'mean_fscore', 'eval_metrics',
           'pre_eval_to_metrics', 'total_area_to_metrics', 'SegEvaluator']

_METRICS = ('mIoU', 'mDice', 'mFscore')


def f_score(precision, recall, beta=1):
    """mmseg's f_score: ``(1 + beta^2) * precision * recall / (beta^2 * precision + recall)``"""
    return (1 + beta ** 2) * (precision * recall) / ((beta ** 2 * precision) + recall)


def _as_map(x, name):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        raise TypeError('%s must be a tensor or an array, not %s (file names are not loaded here)' % (name, type(x).__name__))
    return x


def _batch(pred, label):
    """pred (H, W) or (N, H, W), label the same or (N, 1, H, W) -> both (N, H, W)"""
    pred, label = _as_map(pred, 'pred_label'), _as_map(label, 'label')
    if pred.dim() == 2:
        pred = pred[None]
    if label.dim() == 2:
        label = label[None]
    elif label.dim() == 4:
        label = label.squeeze(1)
    if pred.dim() != 3 or label.shape != pred.shape:
        raise ValueError('prediction %s and ground truth %s must be label maps of one shape' % (tuple(pred.shape), tuple(label.shape)))
    if label.device != pred.device:
        label = label.to(pred.device, non_blocking=True)
    return pred, label


def intersect_and_union(pred_label, label, num_classes, ignore_index, label_map=None, reduce_zero_label=False):
    """-> (area_intersect, area_union, area_pred_label, area_label), int64 tensors of ``num_classes`` entries on the inputs'
    device: the counts of mmseg's function of this name for one image, or for a batch (N, H, W) at once."""
    pred_label, label = _batch(pred_label, label)
    totals = torch.zeros((3, int(num_classes)), dtype=torch.int64, device=pred_label.device)
    fused.seg_eval_update(pred_label, label, totals, num_classes, ignore_index, reduce_zero_label, label_map)
    return totals[0], totals[1] + totals[2] - totals[0], totals[1], totals[2]


def total_intersect_and_union(results, gt_seg_maps, num_classes, ignore_index, label_map=None, reduce_zero_label=False):
    """The sums of ``intersect_and_union`` over pairs of maps (which may differ in size), in mmseg's order of results."""
    evaluator = SegEvaluator(num_classes, ignore_index, reduce_zero_label, label_map)
    for result, gt_seg_map in zip(results, gt_seg_maps):
        evaluator.update(result, gt_seg_map)
    t = evaluator.totals
    return t[0], t[1] + t[2] - t[0], t[1], t[2]


def _host(x):
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float64)


def total_area_to_metrics(total_area_intersect, total_area_union, total_area_pred_label, total_area_label, metrics=['mIoU'],
                          nan_to_num=None, beta=1):
    """mmseg's function of this name, in float64: an OrderedDict with 'aAcc' (a scalar) and per class, for 'mIoU' 'IoU' and
    'Acc', for 'mDice' 'Dice' and 'Acc', for 'mFscore' 'Fscore', 'Precision' and 'Recall'.  0 / 0 is NaN; ``nan_to_num``
    replaces it."""
    if isinstance(metrics, str):
        metrics = [metrics]
    if not set(metrics).issubset(set(_METRICS)):
        raise KeyError('metrics {} is not supported'.format(metrics))
    inter, union, pred, label = (_host(x) for x in (total_area_intersect, total_area_union, total_area_pred_label, total_area_label))
    with np.errstate(divide='ignore', invalid='ignore'):
        ret = OrderedDict({'aAcc': inter.sum() / label.sum()})
        for metric in metrics:
            if metric == 'mIoU':
                ret['IoU'] = inter / union
                ret['Acc'] = inter / label
            elif metric == 'mDice':
                ret['Dice'] = 2 * inter / (pred + label)
                ret['Acc'] = inter / label
            else:
                precision, recall = inter / pred, inter / label
                ret['Fscore'] = f_score(precision, recall, beta)
                ret['Precision'] = precision
                ret['Recall'] = recall
    if nan_to_num is not None:
        ret = OrderedDict((k, np.nan_to_num(v, nan=nan_to_num)) for k, v in ret.items())
    return ret


def pre_eval_to_metrics(pre_eval_results, metrics=['mIoU'], nan_to_num=None, beta=1):
    """mmseg's function of this name: ``pre_eval_results`` is a list of ``intersect_and_union`` tuples, one per image."""
    cols = tuple(zip(*pre_eval_results))
    if len(cols) != 4:
        raise ValueError('pre_eval_results holds tuples of four areas')
    sums = [sum(torch.as_tensor(x).to(torch.int64).cpu() for x in col) for col in cols]
    return total_area_to_metrics(*sums, metrics, nan_to_num, beta)


def eval_metrics(results, gt_seg_maps, num_classes, ignore_index, metrics=['mIoU'], nan_to_num=None, label_map=None,
                 reduce_zero_label=False, beta=1):
    """mmseg's function of this name: the totals of all pairs, then ``total_area_to_metrics``."""
    areas = total_intersect_and_union(results, gt_seg_maps, num_classes, ignore_index, label_map, reduce_zero_label)
    return total_area_to_metrics(*areas, metrics, nan_to_num, beta)


def mean_iou(results, gt_seg_maps, num_classes, ignore_index, nan_to_num=None, label_map=None, reduce_zero_label=False):
    """-> dict with 'aAcc', 'IoU', 'Acc'"""
    return eval_metrics(results, gt_seg_maps, num_classes, ignore_index, ['mIoU'], nan_to_num, label_map, reduce_zero_label)


def mean_dice(results, gt_seg_maps, num_classes, ignore_index, nan_to_num=None, label_map=None, reduce_zero_label=False):
    """-> dict with 'aAcc', 'Dice', 'Acc'"""
    return eval_metrics(results, gt_seg_maps, num_classes, ignore_index, ['mDice'], nan_to_num, label_map, reduce_zero_label)


def mean_fscore(results, gt_seg_maps, num_classes, ignore_index, nan_to_num=None, label_map=None, reduce_zero_label=False, beta=1):
    """-> dict with 'aAcc', 'Fscore', 'Precision', 'Recall'"""
    return eval_metrics(results, gt_seg_maps, num_classes, ignore_index, ['mFscore'], nan_to_num, label_map, reduce_zero_label,
                        beta)


class SegEvaluator:
    """The running totals of a validation set: ``update(pred, label)`` per batch, ``summary()`` at the end.

    ``totals`` is a (3, num_classes) int64 tensor - intersect, pred, label - created on the device of the first update and
    added to by fused.seg_eval_update.  ``update`` performs no host synchronisation on the kernel path; ``compute`` is the
    single device-to-host copy.  ``class_names`` name the per-class keys of ``summary`` (default: the class indices)."""

    def __init__(self, num_classes, ignore_index=255, reduce_zero_label=False, label_map=None, class_names=None):
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError('num_classes must be positive, not %r' % (num_classes,))
        self.ignore_index = int(ignore_index)
        self.reduce_zero_label = bool(reduce_zero_label)
        self.label_map = dict(label_map) if label_map else None
        if class_names is not None and len(class_names) != self.num_classes:
            raise ValueError('%d class names for %d classes' % (len(class_names), self.num_classes))
        self.class_names = tuple(class_names) if class_names is not None else tuple(str(i) for i in range(self.num_classes))
        self._totals = None

    def _zeros(self, device):
        return torch.zeros((3, self.num_classes), dtype=torch.int64, device=device)

    @property
    def totals(self):
        if self._totals is None:
            self._totals = self._zeros('cpu')
        return self._totals

    def reset(self):
        """Clear the totals (they stay on their device)."""
        if self._totals is not None:
            self._totals.zero_()

    def update(self, pred, label):
        """Add a batch: pred (N, H, W) or (H, W) predicted labels, label the same shape or (N, 1, H, W); tensors on any
        device, or arrays."""
        pred, label = _batch(pred, label)
        if self._totals is None:
            self._totals = self._zeros(pred.device)
        target = self._totals if self._totals.device == pred.device else self._zeros(pred.device)
        fused.seg_eval_update(pred, label, target, self.num_classes, self.ignore_index, self.reduce_zero_label, self.label_map)
        if target is not self._totals:
            self._totals += target.to(self._totals.device)

    def all_reduce(self, group=None):
        """Sum the totals over the ranks of ``group`` (every rank ends with the whole validation set's).  Without an
        initialised process group this does nothing."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.totals, op=dist.ReduceOp.SUM, group=group)

    def compute(self, metrics=('mIoU',), nan_to_num=None, beta=1):
        """-> ``total_area_to_metrics`` of the totals: 'aAcc' and the per-class arrays, float64.  The one host read."""
        t = self.totals.cpu()
        return total_area_to_metrics(t[0], t[1] + t[2] - t[0], t[1], t[2], list(metrics), nan_to_num, beta)

    def summary(self, metrics=('mIoU',), nan_to_num=None, beta=1):
        """The keys and rounding of mmseg's CustomDataset.evaluate: 'aAcc', 'mIoU', 'mAcc', ..., then 'IoU.<class>',
        'Acc.<class>', ..., each ``round(x * 100, 2) / 100`` with the means taken by nanmean before the rounding."""
        ret = self.compute(metrics, nan_to_num, beta)
        out = OrderedDict()
        with np.errstate(invalid='ignore'):
            for key, value in ret.items():
                mean = np.round(np.nanmean(value) * 100, 2) if np.isfinite(value).any() else np.float64('nan')
                out['aAcc' if key == 'aAcc' else 'm' + key] = float(mean) / 100.0
        for key, value in ret.items():
            if key != 'aAcc':
                for name, v in zip(self.class_names, np.round(value * 100, 2)):
                    out['%s.%s' % (key, name)] = float(v) / 100.0
        return out
