"""EncoderDecoderMask2Former / EncoderDecoderMask2FormerAug: image in, label map out.

The two segmentors of the reference's segmentation/mmseg_custom/models/segmentors/encoder_decoder_mask2former.py and
encoder_decoder_mask2former_aug.py (cited by line below; the second file differs from the first in one place, the
un-padding of slide_inference, :193-196 there), with the reference's method names, signatures and results.  mmseg's
builders are not part of this project, so the constructor takes built modules instead of config dicts, and the two
Mask2Former classes have no auxiliary head (no ViT-Adapter Mask2Former config has one).  ``EncoderDecoder`` is mmseg's
segmentor of that name as the reference's ``upernet_*`` configs use it - a decode head and auxiliary heads that bring their own
losses (vitadapter.heads) - on the same inference tail.

What differs from the reference is which tensors exist, not what is computed.  Everything after
``decode_head.forward_test`` runs on the three entry points of include/vitadapter_hip_seg.h (vitadapter.fused.seg_resize_add,
seg_finish, seg_argmax; with ENABLED['seg_logits'] off, on the CPU or for another dtype than fp32 those evaluate the
reference's own expressions):
  * a window's logits are upsampled straight into their place in ``preds`` (no upsampled tensor, no padded tensor);
  * ``count_mat`` is kept as the two int32 vectors whose outer product it is (the windows are a grid product);
  * division, un-padding, rescale to ``ori_shape``, softmax and flip are one pass that adds into the probability sum of
    ``aug_test`` or - for ``simple_test``, which returns labels only - writes the labels and no probabilities at all.
The logit tail runs in fp32 with autocast disabled, as Mask2FormerHead.semantic_inference does.

``simple_test_labels`` / ``aug_test_labels`` are ``simple_test`` / ``aug_test`` without the copy to the host, and
``evaluate_batch`` hands their label map to a vitadapter.SegEvaluator (vitadapter/evaluation.py) on the device.
"""
import numpy as np
import torch
import torch.nn as nn

from . import fused

__all__ = ['EncoderDecoderMask2Former', 'EncoderDecoderMask2FormerAug', 'EncoderDecoder']


def _cfg(cfg, name, default=None):
    """test_cfg.name for a dict or an attribute object (mmcv's ConfigDict is both)"""
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(name, default)
    return getattr(cfg, name, default)


def window_grid(h_img, w_img, crop_size, stride):
    """The windows of slide_inference (:163-178) as ((y1, y2) per grid row, (x1, x2) per grid column): the reference's
    arithmetic, including the clamp that moves the last window back inside the image.  An image smaller than the crop
    gets one window, the image."""
    def axis(size, crop, step):
        grids = max(size - crop + step - 1, 0) // step + 1
        out = []
        for idx in range(grids):
            lo = idx * step
            hi = min(lo + crop, size)
            lo = max(hi - crop, 0)
            out.append((lo, hi))
        return out
    (h_crop, w_crop), (h_stride, w_stride) = crop_size, stride
    return axis(h_img, h_crop, h_stride), axis(w_img, w_crop, w_stride)


def _counts(spans, size):
    c = np.zeros(size, dtype=np.int32)
    for lo, hi in spans:
        c[lo:hi] += 1
    return c


class EncoderDecoderMask2Former(nn.Module):
    """``EncoderDecoderMask2Former(backbone, decode_head, neck=None, train_cfg=None, test_cfg=None)`` over built modules.
    ``decode_head`` has ``num_classes``, ``forward_train(x, img_metas, gt_semantic_seg, **kwargs)`` and
    ``forward_test(x, img_metas, test_cfg)`` (vitadapter.Mask2FormerHead); ``align_corners`` is the head's attribute, else the
    entry of its ``extra_cfg``, else False.  ``test_cfg``: ``mode`` ('slide' or 'whole'), ``crop_size``, ``stride``."""

    unpad = False       # the Aug class crops preds to img_shape before the rescale

    def __init__(self, backbone, decode_head, neck=None, train_cfg=None, test_cfg=None):
        super().__init__()
        if decode_head is None:
            raise ValueError('a decode head is required')           # :45 assert self.with_decode_head
        self.backbone = backbone
        if neck is not None:
            self.neck = neck
        self.decode_head = decode_head
        align = getattr(decode_head, 'align_corners', None)
        if align is None:
            align = (getattr(decode_head, 'extra_cfg', None) or {}).get('align_corners', False)
        self.align_corners = bool(align)
        self.num_classes = decode_head.num_classes
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self._count_cache = {}

    @property
    def with_neck(self):
        return getattr(self, 'neck', None) is not None

    @property
    def with_decode_head(self):
        return True

    @property
    def with_auxiliary_head(self):
        return False

    # ----------------------------------------------------------------------------------------------------------------
    def extract_feat(self, img):
        """:63-68"""
        x = self.backbone(img)
        if self.with_neck:
            x = self.neck(x)
        return x

    def _logits(self, img, img_metas):
        """:73-74: the head's semantic logits of ``img``, fp32 (fp64 stays: the CPU checks run the module in it)"""
        x = self.extract_feat(img)
        out = self.decode_head.forward_test(x, img_metas, self.test_cfg)
        return out if out.dtype in (torch.float32, torch.float64) else out.float()

    def encode_decode(self, img, img_metas):
        """:70-80: the logits resized to the size of ``img``"""
        out = self._logits(img, img_metas)
        with torch.autocast(img.device.type, enabled=False):
            dst = out.new_empty(out.shape[:2] + tuple(img.shape[2:]))
            return fused.seg_resize_add(out, dst, 0, 0, img.shape[2:], self.align_corners, accumulate=False)

    def forward_dummy(self, img):
        """:116-120"""
        return self.encode_decode(img, None)

    def forward_train(self, img, img_metas, gt_semantic_seg, **kwargs):
        """:122-153: the head's loss dict under the prefix ``decode.``.  A head with ``prepare_targets`` that is given the
        label map and neither ``gt_masks`` nor ``gt_targets`` has its targets started here, BEFORE the backbone: the scan of
        the label map and the copy of its counts to the host complete while the backbone's launches queue, and the head's
        ``finish()`` finds its event done."""
        head = self.decode_head
        if (hasattr(head, 'prepare_targets') and gt_semantic_seg is not None and kwargs.get('gt_masks') is None
                and kwargs.get('gt_targets') is None):
            kwargs = dict(kwargs, gt_targets=head.prepare_targets(gt_semantic_seg))
        x = self.extract_feat(img)
        loss_decode = self.decode_head.forward_train(x, img_metas, gt_semantic_seg, **kwargs)
        return {'decode.' + k: v for k, v in loss_decode.items()}

    # ----------------------------------------------------------------------------------------------------------------
    def _count_vectors(self, rows, cols, h_img, w_img, device):
        key = (tuple(rows), tuple(cols), h_img, w_img, str(device))
        if key not in self._count_cache:
            cy, cx = _counts(rows, h_img), _counts(cols, w_img)
            if (cy == 0).any() or (cx == 0).any():                  # :186 assert (count_mat == 0).sum() == 0
                raise ValueError('the windows (crop %s, stride %s) leave part of a %d x %d image uncovered'
                                 % (_cfg(self.test_cfg, 'crop_size'), _cfg(self.test_cfg, 'stride'), h_img, w_img))
            self._count_cache[key] = (torch.from_numpy(cy).to(device), torch.from_numpy(cx).to(device))
        return self._count_cache[key]

    def _slide_sum(self, img, img_meta):
        """:163-185 -> (sum of the windows' upsampled logits (N, C, h_img, w_img), (cy, cx)): count_mat = cy[:, None] * cx[None]"""
        batch_size, _, h_img, w_img = img.shape
        rows, cols = window_grid(h_img, w_img, _cfg(self.test_cfg, 'crop_size'), _cfg(self.test_cfg, 'stride'))
        counts = self._count_vectors(rows, cols, h_img, w_img, img.device)
        single = len(rows) * len(cols) == 1                          # one window covers the image: nothing to add up
        preds = None
        for y1, y2 in rows:
            for x1, x2 in cols:
                crop_img = img[:, :, y1:y2, x1:x2].contiguous()
                out = self._logits(crop_img, img_meta)
                with torch.autocast(img.device.type, enabled=False):
                    if preds is None:
                        shape = (batch_size, self.num_classes, h_img, w_img)
                        preds = out.new_empty(shape) if single else out.new_zeros(shape)
                    fused.seg_resize_add(out, preds, y1, x1, (y2 - y1, x2 - x1), self.align_corners, accumulate=not single)
        return preds, (None if single else counts)

    def _view_sum(self, img, img_meta):
        """One view up to the point where the two modes meet: -> (acc, counts, region) for fused.seg_finish"""
        mode = _cfg(self.test_cfg, 'mode')
        if mode not in ('slide', 'whole'):                            # :236
            raise ValueError("test_cfg.mode must be 'slide' or 'whole', not %r" % (mode,))
        ori_shape = img_meta[0]['ori_shape']
        if not all(tuple(m['ori_shape']) == tuple(ori_shape) for m in img_meta):      # :238
            raise ValueError('the images of a batch must share one ori_shape')
        if mode == 'slide':
            acc, counts = self._slide_sum(img, img_meta)
            region = tuple(img_meta[0]['img_shape'][:2]) if self.unpad else None
            return acc, counts, region
        return self.encode_decode(img, img_meta), None, None

    def _finish(self, img, img_meta, rescale, softmax, **kw):
        acc, counts, region = self._view_sum(img, img_meta)
        size = tuple(img_meta[0]['ori_shape'][:2]) if rescale else None
        with torch.autocast(img.device.type, enabled=False):
            if not softmax:
                return self._logit_view(acc, counts, region, size)
            flip = None
            if img_meta[0]['flip']:                                   # :244-251
                flip = img_meta[0]['flip_direction']
                if flip not in ('horizontal', 'vertical'):
                    raise ValueError("flip_direction must be 'horizontal' or 'vertical', not %r" % (flip,))
            return fused.seg_finish(acc, counts, region, size, self.align_corners, flip, **kw)

    def _logit_view(self, acc, counts, region, size):
        """:191-199, :204-218: the logits that slide_inference / whole_inference return (not on the path of inference)"""
        preds = acc
        if counts is not None:
            preds = preds / (counts[0][:, None] * counts[1][None, :]).to(preds.dtype)
        if region is not None:
            preds = preds[:, :, :region[0], :region[1]]
        if size is not None:
            dst = preds.new_empty(preds.shape[:2] + tuple(size))
            preds = fused.seg_resize_add(preds, dst, 0, 0, size, self.align_corners, accumulate=False)
        return preds

    def slide_inference(self, img, img_meta, rescale):
        """:156-199 (and :156-203 of the Aug file): logits of the sliding-window average"""
        acc, counts = self._slide_sum(img, img_meta)
        region = tuple(img_meta[0]['img_shape'][:2]) if self.unpad else None
        with torch.autocast(img.device.type, enabled=False):
            return self._logit_view(acc, counts, region, tuple(img_meta[0]['ori_shape'][:2]) if rescale else None)

    def whole_inference(self, img, img_meta, rescale):
        """:201-218"""
        seg_logit = self.encode_decode(img, img_meta)
        with torch.autocast(img.device.type, enabled=False):
            return self._logit_view(seg_logit, None, None, tuple(img_meta[0]['ori_shape'][:2]) if rescale else None)

    def inference(self, img, img_meta, rescale):
        """:220-253: the softmax output (N, C, H, W) with the flip undone"""
        return self._finish(img, img_meta, rescale, True)[0]

    def simple_test_labels(self, img, img_meta, rescale=True):
        """simple_test up to the label map: (N, H, W) int64 on the device; the probabilities are never formed"""
        return self._finish(img, img_meta, rescale, True, prob=False, labels=True)[1]

    def simple_test(self, img, img_meta, rescale=True):
        """:255-266: one (H, W) int64 array per image"""
        return list(self.simple_test_labels(img, img_meta, rescale).cpu().numpy())

    def aug_test_labels(self, imgs, img_metas, rescale=True):
        """aug_test up to the label map, (N, H, W) int64 on the device: the views' probabilities added into one sum, then
        argmax of sum / views"""
        if not rescale:                                                # :274
            raise ValueError('aug_test supports rescale=True only')
        total = None
        for img, meta in zip(imgs, img_metas):
            total = self._finish(img, meta, rescale, True, out=total, accumulate=total is not None)[0]
        with torch.autocast(total.device.type, enabled=False):
            return fused.seg_argmax(total, len(imgs))

    def aug_test(self, imgs, img_metas, rescale=True):
        """:268-285"""
        return list(self.aug_test_labels(imgs, img_metas, rescale).cpu().numpy())

    def evaluate_batch(self, img_or_imgs, img_metas, gt_semantic_seg, evaluator, rescale=True):
        """One step of a validation loop without leaving the device: the label map of ``simple_test_labels`` - or, for a
        list of views with their list of metas, of ``aug_test_labels`` - goes with ``gt_semantic_seg`` ((N, H, W) or
        (N, 1, H, W), uint8 or int64, a tensor on any device or an array) into ``evaluator`` (vitadapter.SegEvaluator).
        What mmseg's ``single_gpu_test(pre_eval=True)`` does per batch with a copy to the host and three ``histc`` calls.
        -> the (N, H, W) int64 label map, on the device.  A ground truth of another (H, W) than the prediction raises."""
        if isinstance(img_or_imgs, (list, tuple)):
            seg_pred = self.aug_test_labels(img_or_imgs, img_metas, rescale)
        else:
            seg_pred = self.simple_test_labels(img_or_imgs, img_metas, rescale)
        gt = gt_semantic_seg if torch.is_tensor(gt_semantic_seg) else torch.from_numpy(np.ascontiguousarray(gt_semantic_seg))
        if gt.dim() == 4 and gt.shape[1] == 1:
            gt = gt[:, 0]
        if gt.dim() != 3 or tuple(gt.shape) != tuple(seg_pred.shape):
            raise ValueError('ground truth %s for a prediction %s: evaluate against the map the prediction was rescaled to'
                             % (tuple(gt_semantic_seg.shape), tuple(seg_pred.shape)))
        evaluator.update(seg_pred, gt.to(seg_pred.device, non_blocking=True))
        return seg_pred


class EncoderDecoderMask2FormerAug(EncoderDecoderMask2Former):
    """encoder_decoder_mask2former_aug.py: slide_inference crops ``preds`` to ``img_meta[0]['img_shape'][:2]`` (the image
    before the test pipeline padded it) before the rescale (:193-196)."""

    unpad = True


class EncoderDecoder(EncoderDecoderMask2Former):
    """mmseg's ``EncoderDecoder(backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None, test_cfg=None)`` over
    built modules: the segmentor of the reference's UperNet configs (``UPerHead`` + auxiliary ``FCNHead``).  Inference -
    slide / whole, ``simple_test``, ``aug_test`` - is the parent's, unchanged; ``forward_train`` adds the auxiliary heads'
    loss dicts under mmseg's prefixes: ``aux.`` for one head, ``aux_0.``, ``aux_1.``, ... for a list."""

    def __init__(self, backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None, test_cfg=None):
        super().__init__(backbone, decode_head, neck=neck, train_cfg=train_cfg, test_cfg=test_cfg)
        if auxiliary_head is not None:
            self.auxiliary_head = nn.ModuleList(auxiliary_head) if isinstance(auxiliary_head, (list, tuple)) else auxiliary_head

    @property
    def with_auxiliary_head(self):
        return getattr(self, 'auxiliary_head', None) is not None

    def forward_train(self, img, img_metas, gt_semantic_seg, **kwargs):
        x = self.extract_feat(img)
        losses = {'decode.' + k: v for k, v in self.decode_head.forward_train(x, img_metas, gt_semantic_seg, self.train_cfg).items()}
        if self.with_auxiliary_head:
            if isinstance(self.auxiliary_head, nn.ModuleList):
                heads = [('aux_%d.' % i, head) for i, head in enumerate(self.auxiliary_head)]
            else:
                heads = [('aux.', self.auxiliary_head)]
            for prefix, head in heads:
                losses.update((prefix + k, v) for k, v in head.forward_train(x, img_metas, gt_semantic_seg, self.train_cfg).items())
        return losses
