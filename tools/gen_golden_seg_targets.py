"""Mask2Former training targets golden from the reference's own pipeline steps.  Container only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_seg_targets.py

Runs the reference's ``ToMask`` and ``DefaultFormatBundle`` (segmentation/mmseg_custom/datasets/pipelines/formatting.py) and its
``MapillaryHack`` (pipelines/transform.py:310-346) under in-memory stand-ins for their imports: ``mmcv`` (an empty module),
``mmcv.parallel.DataContainer`` (keeps its data), ``mmseg.datasets.builder.PIPELINES`` (a registry whose decorator returns the
class) and ``mmseg.datasets.pipelines.formatting.to_tensor`` (torch.from_numpy).  Each image of each case of
tests/seg_targets_ref.py goes through the steps one at a time, as a loader does: ``MapillaryHack`` or mmseg's
``reduce_zero_label`` lines first where the case has a remap, then ``ToMask(ignore_index)``, then ``DefaultFormatBundle``.

Stored in tests/golden/seg_targets.npz: ``map_<name>`` the maps (uint8; the out-of-range one int64), per case ``<case>_labels``
(G,) int64, ``<case>_masks`` the (G, H, W) masks bit-packed with np.packbits over the flattened array, ``<case>_counts`` (N,);
``mapillary_table`` (256,) uint8: the reference's MapillaryHack applied to the values 0 .. 255 (its lists, as data);
``meta``: JSON with the cases (map, ignore_index, remap), the dtypes and shapes the bundle delivered, the empty-image shapes,
and the loss keys of the head of tests/golden/mask2former_loss.npz.
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import gen_golden as gg                                   # noqa: E402
import seg_targets_ref as ref                             # noqa: E402

PIPE = os.path.join(gg.REF, 'segmentation', 'mmseg_custom', 'datasets', 'pipelines')


class Registry:
    def register_module(self, *args, **kwargs):
        return lambda cls: cls


class DataContainer:
    def __init__(self, data, stack=False):
        self.data, self.stack = data, stack


def load_reference():
    """-> (formatting module, transform module) of the reference"""
    gg._mod('mmcv'), gg._mod('mmcv.parallel', DataContainer=DataContainer)
    gg._mod('mmseg'), gg._mod('mmseg.datasets'), gg._mod('mmseg.datasets.builder', PIPELINES=Registry())
    gg._mod('mmseg.datasets.pipelines'), gg._mod('mmseg.datasets.pipelines.formatting', to_tensor=torch.from_numpy)
    gg._mod('ref_pipe').__path__ = [PIPE]
    return importlib.import_module('ref_pipe.formatting'), importlib.import_module('ref_pipe.transform')


def reduce_zero_label(seg):
    """mmseg 0.20 LoadAnnotations.__call__, the reduce_zero_label lines"""
    seg = seg.copy()
    seg[seg == 0] = 255
    seg = seg - 1
    seg[seg == 254] = 255
    return seg


def run_image(fmt, seg, ignore_index, pre):
    results = dict(gt_semantic_seg=seg.copy(), pad_shape=seg.shape + (3,))
    if pre is not None:
        results = pre(results) if not isinstance(pre, str) else dict(results, gt_semantic_seg=reduce_zero_label(seg))
    results = fmt.ToMask(ignore_index)(results)
    return fmt.DefaultFormatBundle()(results)


def main():
    fmt, tr = load_reference()
    hack = tr.MapillaryHack()
    table = hack(dict(gt_semantic_seg=np.arange(256, dtype=np.uint8).reshape(16, 16)))['gt_semantic_seg'].reshape(-1)
    assert table.dtype == np.uint8
    maps = ref.case_maps()
    out = {'map_' + k: v for k, v in maps.items()}
    out['map_out_of_range'] = ref.OUT_OF_RANGE
    out['mapillary_table'] = table
    meta = dict(cases={}, bundle={}, loss_keys=json.loads(str(np.load(os.path.join(gg.GOLD, 'mask2former_loss.npz'))['meta']))['loss_keys'])
    cases = dict(ref.CASES, out_of_range=('out_of_range', 255, None))
    for name, (map_name, ignore, remap) in cases.items():
        m = out['map_' + map_name]
        pre = {None: None, 'mapillary': hack, 'reduce_zero': 'reduce_zero'}[remap]
        labels, masks, counts = [], [], []
        for n in range(m.shape[0]):
            r = run_image(fmt, m[n], ignore, pre)
            lab, msk, seg = r['gt_labels'].data, r['gt_masks'].data, r['gt_semantic_seg'].data
            assert lab.dtype == torch.int64 and msk.dtype == torch.int64 and seg.dtype == torch.int64
            assert tuple(seg.shape) == (1,) + m.shape[1:] and tuple(msk.shape) == (lab.numel(),) + m.shape[1:]
            meta['bundle'][name] = dict(gt_labels=str(lab.dtype), gt_masks=str(msk.dtype), gt_semantic_seg=str(seg.dtype),
                                        seg_shape=list(seg.shape))
            if lab.numel() == 0:
                meta.setdefault('empty', {})['%s/%d' % (name, n)] = dict(gt_labels=list(lab.shape), gt_masks=list(msk.shape))
            labels.append(lab.numpy())
            masks.append(msk.numpy())
            counts.append(int(lab.numel()))
        all_masks = np.concatenate(masks)
        assert set(np.unique(all_masks).tolist()) <= {0, 1}
        out[name + '_labels'] = np.concatenate(labels).astype(np.int64)
        out[name + '_masks'] = np.packbits(all_masks.astype(np.uint8).reshape(-1))
        out[name + '_counts'] = np.asarray(counts, dtype=np.int64)
        meta['cases'][name] = dict(map=map_name, ignore_index=ignore, remap=remap, shape=list(m.shape), targets=int(sum(counts)))
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(gg.GOLD, 'seg_targets.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes, cases %s' % (path, os.path.getsize(path), {k: v['targets'] for k, v in meta['cases'].items()}))


if __name__ == '__main__':
    main()
