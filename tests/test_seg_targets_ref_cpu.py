"""CPU: Mask2Former's targets from a label map against tests/golden/seg_targets.npz (the reference's own ToMask,
DefaultFormatBundle and MapillaryHack, see tools/gen_golden_seg_targets.py): the numpy rule of tests/seg_targets_ref.py, the torch
tier of fused.seg_targets, vitadapter.ToMask and seg_remap_table, then the head: ``loss`` fed a SegTargets against ``loss`` fed
the explicit lists, bit for bit, and ``forward_train`` from the label map alone.  Everything is an integer or a bitwise
comparison: no tolerance anywhere."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_targets_ref as ref  # noqa: E402
import test_mask2former_loss_cpu as loss_helpers  # noqa: E402

import vitadapter  # noqa: E402
from vitadapter import fused  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'seg_targets.npz')
ALL_CASES = sorted(ref.CASES) + ['out_of_range']


@pytest.fixture(scope='module')
def gold():
    g = np.load(GOLD)
    return g, json.loads(str(g['meta']))


def golden_case(g, meta, name):
    """-> (map, ignore_index, remap table or None, dict like seg_targets_ref.targets)"""
    c = meta['cases'][name]
    m = g['map_' + c['map']]
    N, H, W = m.shape
    labels, counts = g[name + '_labels'], g[name + '_counts'].tolist()
    G = int(sum(counts))
    masks = np.unpackbits(g[name + '_masks'])[:G * H * W].reshape(G, H, W)
    remap = {None: None, 'mapillary': g['mapillary_table'], 'reduce_zero': ref.reduce_zero_table()}[c['remap']]
    want = dict(masks=masks, labels=labels, counts=counts, offsets=[int(sum(counts[:n])) for n in range(N + 1)],
                image_of=np.repeat(np.arange(N, dtype=np.int32), counts))
    return m, c['ignore_index'], remap, want


def same(got, want):
    """a fused.SegTargets against the dict form, exactly"""
    assert got.masks.dtype == torch.uint8 and got.labels.dtype == torch.int64 and got.image_of.dtype == torch.int32
    assert got.offsets.dtype == torch.int32
    assert got.counts == want['counts'] and all(type(c) is int for c in got.counts)
    assert got.offsets.cpu().tolist() == want['offsets']
    assert np.array_equal(got.labels.cpu().numpy(), want['labels'])
    assert np.array_equal(got.image_of.cpu().numpy(), want['image_of'])
    assert tuple(got.masks.shape) == want['masks'].shape and np.array_equal(got.masks.cpu().numpy(), want['masks'])


def test_the_golden_holds_the_cases_of_the_ref_module(gold):
    g, meta = gold
    maps = ref.case_maps()
    assert set(meta['cases']) == set(ALL_CASES)
    for name, (map_name, ignore, remap) in ref.CASES.items():
        c = meta['cases'][name]
        assert (c['map'], c['ignore_index'], c['remap']) == (map_name, ignore, remap)
        assert g['map_' + map_name].dtype == np.uint8 and np.array_equal(g['map_' + map_name], maps[map_name])
    assert np.array_equal(g['map_out_of_range'], ref.OUT_OF_RANGE) and g['map_out_of_range'].dtype == np.int64
    assert {k: meta['cases'][k]['targets'] for k in ('all_values_255', 'all_values_0', 'all_values_neg', 'one_pixel', 'one_pixel_ignored')} \
        == dict(all_values_255=255, all_values_0=255, all_values_neg=256, one_pixel=1, one_pixel_ignored=0)
    assert set(np.unique(g['map_mapillary']).tolist()) == set(range(66))
    assert all(v == dict(gt_labels='torch.int64', gt_masks='torch.int64', gt_semantic_seg='torch.int64', seg_shape=v['seg_shape'])
               for v in meta['bundle'].values())


@pytest.mark.parametrize('name', ALL_CASES)
def test_ref_matches_golden(gold, name):
    g, meta = gold
    m, ignore, remap, want = golden_case(g, meta, name)
    if name == 'out_of_range':
        lab = np.unique(m[0])
        assert 300 in lab and -1 in lab and want['labels'].tolist()[:want['counts'][0]] == [-1, 0, 3, 300]
    got = ref.targets(m, ignore, remap)
    for k in ('masks', 'labels', 'image_of'):
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, k
    assert got['counts'] == want['counts'] and got['offsets'] == want['offsets']
    if name == 'odd':
        assert want['counts'][1] == 0 and want['offsets'][1] == want['offsets'][2]
        o = want['offsets']
        assert 9 in want['labels'][o[0]:o[1]] and 9 not in want['labels'][o[2]:o[3]] and 4 in want['labels'][o[2]:o[3]]
        assert int(want['masks'][o[2]:o[3]][want['labels'][o[2]:o[3]] == 4].sum()) == 1


@pytest.mark.parametrize('name,dtype', [(n, d) for n in ALL_CASES for d in (torch.uint8, torch.int64)
                                        if (n, d) != ('out_of_range', torch.uint8)])           # 300 and -1 have no uint8 form
def test_fused_seg_targets_on_cpu_tensors(gold, name, dtype):
    g, meta = gold
    m, ignore, remap, want = golden_case(g, meta, name)
    t = torch.from_numpy(m).to(dtype)
    table = None if remap is None else torch.from_numpy(remap)
    same(fused.seg_targets(t, ignore, table), want)
    same(fused.seg_targets(t[:, None], ignore, table), want)                 # (N, 1, H, W)
    handle = fused.seg_targets_begin(t, ignore, table)
    assert handle.finish() is handle.finish()
    with pytest.raises(ValueError, match='label map'):
        fused.seg_targets(t[0, 0], ignore)


def test_torch_tier_takes_other_remap_forms():
    m = torch.tensor([[[0, 1, 2, 7]]])
    got = fused.seg_targets(m, 255, torch.tensor([3, 3, 255]))      # a short int64 table: values past it stay
    assert got.labels.tolist() == [3, 7] and got.masks[0].tolist() == [[1, 1, 0, 0]]


@pytest.mark.parametrize('name', ALL_CASES)
def test_to_mask_matches_golden(gold, name):
    g, meta = gold
    m, ignore, remap, want = golden_case(g, meta, name)
    step = vitadapter.ToMask(ignore_index=ignore)
    assert 'ToMask' in vitadapter.__all__ and repr(step) == 'ToMask(ignore_index=%d)' % ignore
    src = m if remap is None else remap[m]
    o = want['offsets']
    for n in range(m.shape[0]):
        results = dict(gt_semantic_seg=src[n].copy(), pad_shape=src[n].shape + (3,), other='kept')
        out = step(results)
        assert out is results and sorted(out) == ['gt_labels', 'gt_masks', 'gt_semantic_seg', 'other', 'pad_shape']
        assert np.array_equal(out['gt_semantic_seg'], src[n])
        assert out['gt_labels'].dtype == np.int64 and out['gt_masks'].dtype == np.int64
        assert np.array_equal(out['gt_labels'], want['labels'][o[n]:o[n + 1]])
        assert out['gt_masks'].shape == (o[n + 1] - o[n],) + src[n].shape
        assert np.array_equal(out['gt_masks'], want['masks'][o[n]:o[n + 1]])
        key = '%s/%d' % (name, n)
        if key in meta.get('empty', {}):
            assert list(out['gt_labels'].shape) == meta['empty'][key]['gt_labels'] == [0]
            assert list(out['gt_masks'].shape) == meta['empty'][key]['gt_masks']
    assert 'odd/1' in meta['empty'] and 'one_pixel_ignored/0' in meta['empty']


def test_seg_remap_table():
    ident = fused.seg_remap_table()
    assert ident.dtype == torch.uint8 and ident.tolist() == list(range(256)) and ident.device.type == 'cpu'
    assert np.array_equal(fused.seg_remap_table(reduce_zero_label=True).numpy(), ref.reduce_zero_table())
    # label_map on the original value, all entries at once, then reduce_zero_label (the order of fused.seg_eval_update)
    got = fused.seg_remap_table(True, {1: 2, 2: 1, 7: 0})
    want = list(range(256))
    want[1], want[2], want[7] = 2, 1, 0
    want = [255 if v in (0, 255) else v - 1 for v in want]
    assert got.tolist() == want and got[7] == 255 and got[1] == 1 and got[2] == 0
    for bad in ({3: 256}, {3: -1}, {256: 1}, {-1: 0}):
        with pytest.raises(ValueError, match='8'):
            fused.seg_remap_table(False, bad)
    with pytest.raises(ValueError):
        fused.seg_remap_table(True, {3: 300})


def test_mapillary_table_is_the_references_lists(gold):
    g, _ = gold
    table = g['mapillary_table']
    assert table.dtype == np.uint8 and table.shape == (256,)
    assert sorted(set(table[:66].tolist())) == list(range(19)) + [255] and (table[66:] == 0).all()
    label_map = {v: int(table[v]) for v in range(256)}
    assert np.array_equal(fused.seg_remap_table(False, label_map).numpy(), table)


# ----------------------------------------------------------------------------------------------------------------------
# the head
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def loss_gold():
    g = np.load(loss_helpers.GOLD)
    return g, json.loads(str(g['meta']))


def label_map(meta, seed=5):
    """(N, 64, 96) int64: blocks of the head's classes, an ignored band, image 1 with two classes only"""
    rng = np.random.RandomState(seed)
    classes = meta['things'] + meta['stuff']
    m = rng.randint(0, classes, size=(meta['N'], 4, 6)).repeat(16, axis=1).repeat(16, axis=2)
    m[:, 10:20, 30:50] = 255
    m[1, :, :48] = 1
    m[1, :, 48:] = 3
    return torch.from_numpy(m.astype(np.int64))


def test_loss_fed_seg_targets_equals_loss_fed_lists(loss_gold):
    g, meta = loss_gold
    head = loss_helpers.build_head(meta, 'cpu')
    seg = label_map(meta)
    gt_labels, gt_masks = ref.lists(seg.numpy(), 255)
    assert [len(x) for x in gt_labels] == fused.seg_targets(seg).counts and min(len(x) for x in gt_labels) >= 2
    results = []
    for form in ('lists', 'targets'):
        masks, clss, _, _ = loss_helpers.inputs(g, meta, 'full', 'cpu')
        torch.manual_seed(11)
        if form == 'lists':
            losses = head.loss(clss, masks, [torch.from_numpy(x) for x in gt_labels], [torch.from_numpy(x) for x in gt_masks],
                               [None] * meta['N'])
        else:
            losses = head.loss(clss, masks, fused.seg_targets(seg), None, [None] * meta['N'])
        sum(losses.values()).backward()
        results.append((losses, [m.grad for m in masks], [c.grad for c in clss], head.last_assignment))
    (la, gma, gca, aa), (lb, gmb, gcb, ab) = results
    assert list(la) == list(lb) == meta['loss_keys']
    assert all(torch.equal(la[k], lb[k]) for k in la)
    assert all(torch.equal(x, y) for x, y in zip(gma + gca, gmb + gcb))
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for i in range(meta['L']) for x, y in zip(aa[i], ab[i]))


def test_forward_train_from_the_label_map_alone(loss_gold, gold):
    g, meta = loss_gold
    head = loss_helpers.build_head(meta, 'cpu')
    seg = label_map(meta)
    masks, clss, _, _ = loss_helpers.inputs(g, meta, 'full', 'cpu')
    seen = []
    keep = head.loss
    head.forward = lambda feats, metas=None: (clss, masks)          # the decoder is not what this test is about
    head.loss = lambda *a: (seen.append(a[2]), keep(*a))[1]
    losses = head.forward_train(None, [None] * meta['N'], seg[:, None])
    assert list(losses) == gold[1]['loss_keys'] == meta['loss_keys']
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert isinstance(seen[-1], fused.SegTargets)
    want = ref.targets(seg.numpy(), 255)
    assert np.array_equal(seen[-1].masks.numpy(), want['masks']) and seen[-1].counts == want['counts']
    # the other two ways: a handle or a finished SegTargets as gt_targets; explicit lists as before
    pending = head.prepare_targets(seg)
    head.forward_train(None, [None] * meta['N'], None, gt_targets=pending)
    assert seen[-1] is pending.finish()
    head.forward_train(None, [None] * meta['N'], None, gt_targets=pending.finish())
    assert seen[-1] is pending.finish()
    gt_labels, gt_masks = ref.lists(seg.numpy(), 255)
    head.forward_train(None, [None] * meta['N'], seg, [torch.from_numpy(x) for x in gt_labels], [torch.from_numpy(x) for x in gt_masks])
    assert isinstance(seen[-1], list)
    with pytest.raises(ValueError, match='gt_labels and gt_masks.*gt_targets.*gt_semantic_seg'):
        head.forward_train(None, [None] * meta['N'], None)


def test_segmentor_prepares_targets_before_the_backbone(loss_gold):
    from vitadapter import EncoderDecoderMask2Former
    g, meta = loss_gold
    order = []

    class Backbone(torch.nn.Module):
        def forward(self, img):
            order.append('backbone')
            return [img]

    class Head(torch.nn.Module):
        num_classes = 5

        def prepare_targets(self, gt):
            order.append('prepare')
            return 'handle'

        def forward_train(self, x, img_metas, gt_semantic_seg, **kwargs):
            order.append(sorted(kwargs.items()))
            return dict(loss=torch.zeros(()))

    class Stub(torch.nn.Module):
        num_classes = 5

        def forward_train(self, x, img_metas, gt_semantic_seg, **kwargs):
            order.append(sorted(kwargs))
            return dict(loss=torch.zeros(()))

    img, gt = torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8, dtype=torch.long)
    seg = EncoderDecoderMask2Former(Backbone(), Head())
    assert list(seg.forward_train(img, [None], gt)) == ['decode.loss']
    assert order == ['prepare', 'backbone', [('gt_targets', 'handle')]]
    for kwargs in (dict(gt_masks=[gt], gt_labels=[gt]), dict(gt_targets='mine')):
        del order[:]
        seg.forward_train(img, [None], gt, **kwargs)
        assert order == ['backbone', sorted(kwargs.items())]
    del order[:]
    seg.forward_train(img, [None], None)
    assert order == ['backbone', []]
    del order[:]
    EncoderDecoderMask2Former(Backbone(), Stub()).forward_train(img, [None], gt, extra=1)
    assert order == ['backbone', ['extra']]
