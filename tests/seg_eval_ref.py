"""numpy restatement of the counting rule of include/vitadapter_hip_seg_eval.h and of mmseg's metric formulas: what the
seg_eval tests compare with.  Written with masks, from the rule's text, step by step; `counts_loop` walks the pixels one by
one for the hand-counted case."""
import numpy as np


def mapped_labels(label, ignore_index=255, reduce_zero_label=False, label_map=None):
    """steps 1 - 3 of the rule -> int64 array"""
    g0 = np.asarray(label).astype(np.int64)
    g = g0.copy()
    if label_map:
        for old, new in label_map.items():          # every entry applies to the original value
            g[g0 == old] = new
    if reduce_zero_label:
        g = np.where((g == 0) | (g == 255), 255, g - 1)
    return g


def counts(pred, label, num_classes, ignore_index=255, reduce_zero_label=False, label_map=None):
    """-> int64 (3, C): intersect, pred, label"""
    C = int(num_classes)
    p = np.asarray(pred).astype(np.int64).reshape(-1)
    g = mapped_labels(label, ignore_index, reduce_zero_label, label_map).reshape(-1)
    keep = g != ignore_index
    p, g = p[keep], g[keep]
    p_in, g_in = (p >= 0) & (p < C), (g >= 0) & (g < C)
    out = np.zeros((3, C), dtype=np.int64)
    out[0] = np.bincount(p[p_in & (p == g)], minlength=C)
    out[1] = np.bincount(p[p_in], minlength=C)
    out[2] = np.bincount(g[g_in], minlength=C)
    return out


def counts_loop(pred, label, num_classes, ignore_index=255, reduce_zero_label=False, label_map=None):
    """the same, one pixel at a time"""
    C = int(num_classes)
    out = np.zeros((3, C), dtype=np.int64)
    for p, g in zip(np.asarray(pred).reshape(-1).tolist(), np.asarray(label).reshape(-1).tolist()):
        if label_map and g in label_map:
            g = label_map[g]
        if reduce_zero_label:
            g = 255 if g in (0, 255) else g - 1
        if g == ignore_index:
            continue
        if 0 <= p < C:
            out[1, p] += 1
        if 0 <= g < C:
            out[2, g] += 1
        if p == g and 0 <= p < C:
            out[0, p] += 1
    return out


def metrics(totals, names=('mIoU',), nan_to_num=None, beta=1):
    """float64 metrics from int64 (3, C) totals -> dict of 'aAcc' and the per-class arrays of mmseg's total_area_to_metrics"""
    inter, pred, label = (np.asarray(t, dtype=np.float64) for t in totals)
    union = pred + label - inter
    out = {}
    with np.errstate(divide='ignore', invalid='ignore'):
        out['aAcc'] = inter.sum() / label.sum()
        for name in names:
            if name == 'mIoU':
                out['IoU'], out['Acc'] = inter / union, inter / label
            elif name == 'mDice':
                out['Dice'], out['Acc'] = 2 * inter / (pred + label), inter / label
            elif name == 'mFscore':
                precision, recall = inter / pred, inter / label
                out['Fscore'] = (1 + beta ** 2) * precision * recall / (beta ** 2 * precision + recall)
                out['Precision'], out['Recall'] = precision, recall
            else:
                raise KeyError(name)
    if nan_to_num is not None:
        out = {k: np.nan_to_num(v, nan=nan_to_num) for k, v in out.items()}
    return out


def histc_counts(pred, label, num_classes, ignore_index=255, reduce_zero_label=False, label_map=None):
    """mmseg 0.20's formulation (three torch.histc calls on float copies of masked maps) on already mapped labels, for
    C >= 2 -> int64 (3, C)"""
    import torch
    C = int(num_classes)
    g = torch.from_numpy(mapped_labels(label, ignore_index, reduce_zero_label, label_map))
    p = torch.from_numpy(np.asarray(pred).astype(np.int64))
    mask = g != ignore_index
    p, g = p[mask], g[mask]
    inter = p[p == g]
    rows = [torch.histc(t.double(), bins=C, min=0, max=C - 1) for t in (inter, p, g)]
    return torch.stack(rows).to(torch.int64).numpy()


def blobs(rng, shape, num_classes, cell=8):
    """(N, H, W) piecewise-constant labels: nearest-neighbour upsampled low-resolution noise"""
    N, H, W = shape
    low = rng.integers(0, num_classes, size=(N, (H + cell - 1) // cell, (W + cell - 1) // cell))
    return np.repeat(np.repeat(low, cell, axis=1), cell, axis=2)[:, :H, :W].astype(np.int64)
