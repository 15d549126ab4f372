"""CPU: vitadapter.segmentor against tests/golden/segmentor.npz, the reference's two segmentor classes run in fp64 on stub
modules (tools/gen_golden_segmentor.py).  On the CPU the logit tail evaluates the reference's expressions, so what is held
here is the module's own part: the window grid, the count vectors, which region is read and resized, flips, the view sum,
the ValueErrors and the ``decode.`` prefix.  In fp64 the results agree with the golden (stored as fp32) to its rounding."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segmentor_case  # noqa: E402
from vitadapter import EncoderDecoderMask2Former, EncoderDecoderMask2FormerAug  # noqa: E402
from vitadapter import segmentor as seg_mod  # noqa: E402

CASE = segmentor_case.Case()
CLASSES = {'b_': EncoderDecoderMask2Former, 'a_': EncoderDecoderMask2FormerAug}
TOL = 2.0 ** -22          # the golden's fp32 storage (2^-24 relative, logits of magnitude up to ~16) with room


def _close(got, want):
    got = got.detach().double().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= TOL * max(1.0, np.abs(want).max()), err


@pytest.mark.parametrize('prefix', sorted(CLASSES))
def test_slide_inference_and_inference(prefix):
    seg = CASE.build(CLASSES[prefix])
    v0 = CASE.views[0]
    img = CASE.image(v0)
    with torch.no_grad():
        _close(seg.slide_inference(img, CASE.metas(v0), True), CASE.gold[prefix + 'slide_rescale'])
        _close(seg.slide_inference(img, CASE.metas(v0), False), CASE.gold[prefix + 'slide_raw'])
        for flip in ('none', 'horizontal', 'vertical'):
            m = CASE.metas(v0, flip=flip != 'none', flip_direction=flip if flip != 'none' else 'horizontal')
            out = seg.inference(img, m, True)
            _close(out, CASE.gold[prefix + 'inference_' + flip])
            assert out.shape == (1, CASE.meta['classes']) + CASE.ori[:2]
    raw = CASE.gold[prefix + 'slide_raw'].shape
    assert raw[2:] == (tuple(v0['img_shape'][:2]) if prefix == 'a_' else tuple(v0['hw']))


@pytest.mark.parametrize('as_dict', (False, True))
@pytest.mark.parametrize('prefix', sorted(CLASSES))
def test_simple_test_and_aug_test(prefix, as_dict):
    seg = CASE.build(CLASSES[prefix], as_dict=as_dict)
    imgs = [CASE.image(v) for v in CASE.views]
    metas = [CASE.metas(v) for v in CASE.views]
    with torch.no_grad():
        one = seg.simple_test(imgs[0], metas[0])
        aug = seg.aug_test(imgs, metas)
        prob = seg.inference(imgs[0], metas[0], True)
    for got, key in ((one, 'simple_test'), (aug, 'aug_test')):
        assert isinstance(got, list) and len(got) == 1
        assert isinstance(got[0], np.ndarray) and got[0].dtype == np.int64 and got[0].shape == CASE.ori[:2]
        assert np.array_equal(np.stack(got), CASE.gold[prefix + key])
    assert np.array_equal(one[0], prob.argmax(1)[0].numpy())                # simple_test == inference(...).argmax(1)
    assert not np.array_equal(one[0], aug[0])                               # the views do change something
    with torch.no_grad():                                                   # rescale=False: labels at the size of preds
        raw = seg.simple_test(imgs[0], metas[0], rescale=False)
    assert raw[0].shape == CASE.gold[prefix + 'slide_raw'].shape[2:]


def test_whole_mode():
    seg = CASE.build(EncoderDecoderMask2Former, mode='whole')
    v0 = CASE.views[0]
    with torch.no_grad():
        _close(seg.whole_inference(CASE.image(v0), CASE.metas(v0), True), CASE.gold['b_whole'])
        assert np.array_equal(np.stack(seg.simple_test(CASE.image(v0), CASE.metas(v0))), CASE.gold['b_whole_simple_test'])
        assert seg.whole_inference(CASE.image(v0), CASE.metas(v0), False).shape[2:] == tuple(v0['hw'])
        dummy = seg.forward_dummy(CASE.image(v0))
        assert dummy.shape == (1, CASE.meta['classes']) + tuple(v0['hw'])
        assert torch.equal(dummy, seg.encode_decode(CASE.image(v0), None))


def test_forward_train_prefixes_the_loss_dict():
    seg = CASE.build(EncoderDecoderMask2Former).train()
    v0 = CASE.views[0]
    losses = seg.forward_train(CASE.image(v0), CASE.metas(v0), None)
    assert list(losses) == CASE.meta['forward_train_keys']
    assert all(k.startswith('decode.') for k in losses)
    sum(losses.values()).backward()
    assert seg.decode_head.weight.grad is not None and bool(seg.decode_head.weight.grad.abs().sum() > 0)


def test_window_grid_is_the_references_arithmetic():
    grid = seg_mod.window_grid
    assert grid(40, 52, (24, 24), (16, 16)) == ([(0, 24), (16, 40)], [(0, 24), (16, 40), (28, 52)])       # the last column clamped back
    assert grid(896, 1195, (896, 896), (512, 512)) == ([(0, 896)], [(0, 896), (299, 1195)])               # the ADE20K view
    assert grid(20, 30, (24, 24), (16, 16)) == ([(0, 20)], [(0, 24), (6, 30)])                            # shorter than the crop
    assert grid(10, 12, (24, 24), (16, 16)) == ([(0, 10)], [(0, 12)])                                     # smaller: one window
    assert grid(24, 24, (24, 24), (16, 16)) == ([(0, 24)], [(0, 24)])
    assert grid(25, 24, (24, 24), (16, 16)) == ([(0, 24), (1, 25)], [(0, 24)])
    # the loop of encoder_decoder_mask2former.py:163-178, restated
    for h_img, w_img, crop, stride in ((40, 52, 24, 16), (100, 37, 32, 20), (33, 33, 32, 1)):
        rows, cols = grid(h_img, w_img, (crop, crop), (stride, stride))
        h_grids = max(h_img - crop + stride - 1, 0) // stride + 1
        w_grids = max(w_img - crop + stride - 1, 0) // stride + 1
        assert (len(rows), len(cols)) == (h_grids, w_grids)
        for idx, (y1, y2) in enumerate(rows):
            want2 = min(idx * stride + crop, h_img)
            assert (y1, y2) == (max(want2 - crop, 0), want2)


def test_an_image_smaller_than_the_crop_is_one_window():
    seg = CASE.build(EncoderDecoderMask2FormerAug)
    view = dict(hw=(20, 16), img_shape=(18, 15, 3), j=3, flip=False, flip_direction='horizontal')
    img = CASE.image(view)
    with torch.no_grad():
        got = seg.slide_inference(img, CASE.metas(view), False)
        want = seg.encode_decode(img, CASE.metas(view))[:, :, :18, :15]
        assert torch.equal(got, want)
        assert seg.simple_test(img, CASE.metas(view))[0].shape == CASE.ori[:2]


def test_the_references_asserts_are_value_errors():
    v0 = CASE.views[0]
    img = CASE.image(v0)
    seg = CASE.build(EncoderDecoderMask2Former, mode='tile')
    with pytest.raises(ValueError, match='mode'):
        seg.inference(img, CASE.metas(v0), True)
    seg = CASE.build(EncoderDecoderMask2Former)
    two = torch.cat([img, img])
    with pytest.raises(ValueError, match='ori_shape'):
        seg.inference(two, CASE.metas(v0) + CASE.metas(v0, ori_shape=(30, 45, 3)), True)
    with pytest.raises(ValueError, match='rescale'):
        seg.aug_test([img], [CASE.metas(v0)], rescale=False)
    with pytest.raises(ValueError, match='flip_direction'):
        seg.inference(img, CASE.metas(v0, flip=True, flip_direction='diagonal'), True)
    with torch.no_grad():
        assert seg.inference(two, CASE.metas(v0) + CASE.metas(v0), True).shape[0] == 2


def test_align_corners_comes_from_the_head():
    w, b, keys = CASE.gold['head_weight'], CASE.gold['head_bias'], CASE.meta['loss_keys']
    head = segmentor_case.StubHead(w, b, keys, align_corners=True)
    assert EncoderDecoderMask2Former(segmentor_case.StubBackbone(), head).align_corners is True
    head = segmentor_case.StubHead(w, b, keys)
    del head.align_corners
    assert EncoderDecoderMask2Former(segmentor_case.StubBackbone(), head).align_corners is False
    head.extra_cfg = dict(align_corners=True, in_index=[0, 1, 2, 3])
    seg = EncoderDecoderMask2Former(segmentor_case.StubBackbone(), head, test_cfg=CASE.test_cfg())
    assert seg.align_corners is True and seg.num_classes == 5
    with pytest.raises(ValueError):
        EncoderDecoderMask2Former(segmentor_case.StubBackbone(), None)
