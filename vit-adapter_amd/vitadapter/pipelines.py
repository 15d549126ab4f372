"""Data-pipeline steps for loaders that stay on the CPU.

``ToMask`` is the step of that name of the reference's Mask2Former training pipelines
(segmentation/mmseg_custom/datasets/pipelines/formatting.py:52-82), on the same ``results`` dict of numpy arrays.  A training
loop that holds the label map on the device does not need it: ``EncoderDecoderMask2Former.forward_train`` derives the same
targets there (vitadapter.fused.seg_targets)."""
import numpy as np


class ToMask:
    """``results['gt_semantic_seg']`` -> ``results['gt_labels']`` (G,) int64, the distinct values of the map in ascending
    order without ``ignore_index``, and ``results['gt_masks']`` (G, H, W) int64, 1 where the map equals the label.  A map with
    nothing but ``ignore_index`` gives shapes (0,) and (0,) + ``results['pad_shape'][:-1]``."""

    def __init__(self, ignore_index=255):
        self.ignore_index = ignore_index

    def __call__(self, results):
        seg = results['gt_semantic_seg']
        labels = np.unique(seg)
        labels = labels[labels != self.ignore_index]
        if labels.size == 0:
            results['gt_labels'] = np.empty((0,), dtype=np.int64)
            results['gt_masks'] = np.empty((0,) + tuple(results['pad_shape'][:-1]), dtype=np.int64)
        else:
            results['gt_labels'] = labels.astype(np.int64)
            results['gt_masks'] = (seg[None] == labels.reshape((-1,) + (1,) * seg.ndim)).astype(np.int64)
        return results

    def __repr__(self):
        return '%s(ignore_index=%r)' % (type(self).__name__, self.ignore_index)
