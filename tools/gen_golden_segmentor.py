"""Segmentor golden from the reference's own two classes.  Container only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_segmentor.py [--check]

Imports /root/reference/segmentation/mmseg_custom/models/segmentors/encoder_decoder_mask2former.py and
encoder_decoder_mask2former_aug.py under in-memory stand-ins for mmseg: a bare ``BaseSegmentor`` (an nn.Module with the
``with_neck`` / ``with_decode_head`` / ``with_auxiliary_head`` properties), ``add_prefix``, a ``SEGMENTORS`` registry that
registers nothing, builders that return the object passed, and ``resize`` as F.interpolate.  mmseg is absent here, so the
stand-ins are NOT pinned against it; everything between ``forward_test`` and the label map - the window grid, the padding,
``count_mat``, the un-padding, the rescale, softmax, flips, the view sum, argmax, the ``decode.`` prefix - is the reference's
code.

Backbone and head are stubs: the backbone is ``avg_pool2d(img, 4)``, the head a 1 x 1 convolution from 3 channels to 5 classes
whose weight and bias (seeded, stored in the file) are its only parameters; its ``forward_train`` returns a fixed list of loss
names.  Images are cos(0.37 k + j) over the flat index k (not stored).

Case: a 1 x 3 x 40 x 52 image, test_cfg mode 'slide', crop 24, stride 16 (2 x 3 windows, the last column clamped back to 28),
ori_shape 31 x 45, img_shape 38 x 50 (read by the Aug class only).  The three views of aug_test: that image unflipped, a
1 x 3 x 48 x 60 image (img_shape 45 x 57) flipped horizontally, and the first size again (j = 2) flipped vertically.

Guard: the seeds of the head are walked in order until, for every label map stored, the relative gap (p1 - p2) / p1 between
the two largest probabilities is at least 1e-3 at every pixel, so that all labels compare.  ``meta`` holds the seed and the
smallest gap.

What the file holds, from an fp64 run, stored as fp32 (labels int64); prefix ``b_`` is EncoderDecoderMask2Former, ``a_``
EncoderDecoderMask2FormerAug:
  * ``head_weight``, ``head_bias``; ``meta`` (JSON): the case, the seed, the guard, the forward_train key list;
  * ``?_slide_rescale``, ``?_slide_raw``: slide_inference with and without rescale; ``b_whole``: whole_inference with rescale;
  * ``?_inference_none`` / ``_horizontal`` / ``_vertical``: inference of view 0 under each flip;
  * ``?_simple_test``, ``?_aug_test``: the label maps; ``b_whole_simple_test``: simple_test in mode 'whole'.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference/segmentation/mmseg_custom/models/segmentors'
OUT = os.path.join(ROOT, 'tests', 'golden', 'segmentor.npz')
CLASSES, CROP, STRIDE, ORI = 5, 24, 16, (31, 45, 3)
VIEWS = (dict(hw=(40, 52), img_shape=(38, 50, 3), j=0, flip=False, flip_direction='horizontal'),
         dict(hw=(48, 60), img_shape=(45, 57, 3), j=1, flip=True, flip_direction='horizontal'),
         dict(hw=(40, 52), img_shape=(38, 50, 3), j=2, flip=True, flip_direction='vertical'))
LOSS_KEYS = ['loss_cls', 'loss_mask', 'loss_dice', 'd0.loss_cls', 'd0.loss_mask', 'd0.loss_dice']
GAP = 1e-3


class AttrDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


def image(hw, j, dtype=torch.float64):
    n = 3 * hw[0] * hw[1]
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.37 + j).reshape(1, 3, *hw).to(dtype)


def metas(view, **over):
    m = dict(ori_shape=ORI, img_shape=view['img_shape'], flip=view['flip'], flip_direction=view['flip_direction'])
    m.update(over)
    return [m]


def head_params(seed):
    g = torch.Generator().manual_seed(seed)
    # drawn in fp32, so that the fp32 copies the file stores are the exact parameters of the fp64 run
    return 4.0 * torch.randn(CLASSES, 3, 1, 1, generator=g).double(), torch.randn(CLASSES, generator=g).double()


class StubBackbone(nn.Module):
    def forward(self, img):
        return F.avg_pool2d(img, 4)


class StubHead(nn.Module):
    align_corners = False
    num_classes = CLASSES

    def __init__(self, weight, bias):
        super().__init__()
        self.weight, self.bias = nn.Parameter(weight.clone()), nn.Parameter(bias.clone())

    def update(self, **kwargs):                 # the reference hands train_cfg / test_cfg to the head's config dict
        pass

    def forward_test(self, x, img_metas, test_cfg):
        return F.conv2d(x, self.weight, self.bias)

    def forward_train(self, x, img_metas, gt_semantic_seg, **kwargs):
        return {k: F.conv2d(x, self.weight, self.bias).mean() * (i + 1) for i, k in enumerate(LOSS_KEYS)}


def _install_stand_ins():
    class BaseSegmentor(nn.Module):
        def __init__(self, init_cfg=None):
            super().__init__()

        @property
        def with_neck(self):
            return hasattr(self, 'neck') and self.neck is not None

        @property
        def with_auxiliary_head(self):
            return hasattr(self, 'auxiliary_head') and self.auxiliary_head is not None

        @property
        def with_decode_head(self):
            return hasattr(self, 'decode_head') and self.decode_head is not None

    class Registry:
        def register_module(self):
            return lambda cls: cls

    def add_prefix(inputs, prefix):
        return {'%s.%s' % (prefix, k): v for k, v in inputs.items()}

    def resize(input, size=None, scale_factor=None, mode='nearest', align_corners=None, warning=True):
        return F.interpolate(input, size, scale_factor, mode, align_corners)

    builder = types.ModuleType('mmseg.models.builder')
    builder.SEGMENTORS = Registry()
    builder.build_backbone = builder.build_neck = builder.build_head = lambda obj: obj
    mods = {n: types.ModuleType(n) for n in ('mmseg', 'mmseg.core', 'mmseg.models', 'mmseg.models.segmentors',
                                             'mmseg.models.segmentors.base', 'mmseg.ops')}
    mods['mmseg.models.builder'] = builder
    mods['mmseg.core'].add_prefix = add_prefix
    mods['mmseg.models'].builder = builder
    mods['mmseg.models.segmentors.base'].BaseSegmentor = BaseSegmentor
    mods['mmseg.ops'].resize = resize
    sys.modules.update(mods)


def _load(fname, cls):
    spec = importlib.util.spec_from_file_location('ref_' + fname, os.path.join(REF, fname + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return getattr(mod, cls)


def min_gap(p):
    top = torch.sort(p, dim=1).values[:, -2:]
    return float(((top[:, 1] - top[:, 0]) / top[:, 1]).min())


def run(seed, classes):
    weight, bias = head_params(seed)
    out = dict(head_weight=weight.numpy(), head_bias=bias.numpy())
    gaps = []
    imgs = [image(v['hw'], v['j']) for v in VIEWS]
    for prefix, cls in classes.items():
        def build(mode):
            return cls(StubBackbone(), StubHead(weight, bias), test_cfg=AttrDict(mode=mode, crop_size=(CROP, CROP),
                                                                                stride=(STRIDE, STRIDE))).double().eval()
        with torch.no_grad():
            seg = build('slide')
            v0 = VIEWS[0]
            out[prefix + 'slide_rescale'] = seg.slide_inference(imgs[0], metas(v0), True).numpy()
            out[prefix + 'slide_raw'] = seg.slide_inference(imgs[0], metas(v0), False).numpy()
            for flip in ('none', 'horizontal', 'vertical'):
                m = metas(v0, flip=flip != 'none', flip_direction=flip if flip != 'none' else 'horizontal')
                out[prefix + 'inference_' + flip] = seg.inference(imgs[0], m, True).numpy()
            gaps.append(min_gap(seg.inference(imgs[0], metas(v0), True)))
            out[prefix + 'simple_test'] = np.stack(seg.simple_test(imgs[0], metas(v0)))
            total = sum(seg.inference(i, metas(v), True) for i, v in zip(imgs, VIEWS)) / len(VIEWS)
            gaps.append(min_gap(total))
            out[prefix + 'aug_test'] = np.stack(seg.aug_test(imgs, [metas(v) for v in VIEWS]))
            if prefix == 'b_':
                whole = build('whole')
                out['b_whole'] = whole.whole_inference(imgs[0], metas(v0), True).numpy()
                gaps.append(min_gap(whole.inference(imgs[0], metas(v0), True)))
                out['b_whole_simple_test'] = np.stack(whole.simple_test(imgs[0], metas(v0)))
        keys = list(seg.train().forward_train(imgs[0], metas(v0), None).keys())
    return out, min(gaps), keys


def main():
    _install_stand_ins()
    classes = {'b_': _load('encoder_decoder_mask2former', 'EncoderDecoderMask2Former'),
               'a_': _load('encoder_decoder_mask2former_aug', 'EncoderDecoderMask2FormerAug')}
    for seed in range(1000):
        out, gap, keys = run(seed, classes)
        if gap >= GAP:
            break
    else:
        raise SystemExit('no seed below 1000 passes the label guard')
    meta = dict(classes=CLASSES, crop=CROP, stride=STRIDE, ori_shape=ORI, views=VIEWS, seed=seed, guard=GAP, min_gap=gap,
                forward_train_keys=keys, loss_keys=LOSS_KEYS)
    arrays = {k: (v if v.dtype == np.int64 else v.astype(np.float32)) for k, v in out.items()}
    arrays['meta'] = np.array(json.dumps(meta))
    print('seed %d, smallest relative top-two gap %.3g, forward_train keys %s' % (seed, gap, keys))
    if '--check' in sys.argv:
        have = np.load(OUT)
        assert set(have.files) == set(arrays), sorted(set(have.files) ^ set(arrays))
        worst = max(float(np.abs(have[k].astype(np.float64) - arrays[k].astype(np.float64)).max()) for k in arrays if k != 'meta')
        assert str(have['meta']) == str(arrays['meta'])
        print('max diff against %s: %g' % (os.path.relpath(OUT, ROOT), worst))
        return
    np.savez_compressed(OUT, **arrays)
    print('wrote %s (%d bytes)' % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
