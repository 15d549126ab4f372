"""GPU: vitadapter.segmentor with the logit tail on the kernels of csrc/seg_logits.hip.

Against tests/golden/segmentor.npz (the reference's classes in fp64 on stub modules), in fp32 on the GPU.  The stub's logits
carry their own fp32 error - an average of 16, a 3-term product sum and a bias: at most 32 u L with u = 2^-24 and L the largest
|logit| of the golden - on top of the tail's 16 u A (A <= L) of tests/seg_logits_ref.py.  So a logit may be off by
d = 48 u L (plus u L for the golden's fp32 storage), and by the budget of the probabilities there (p <= 1, |v - max v| <= 2 L) a
probability by 2 d + (2 L + C + 16) u.  The labels must be the golden's everywhere: its guard keeps every relative top-two gap
above 1e-3.

Also: kernels on against off on one case, one real composition (ViT-Adapter + Mask2FormerHead at the smallest size the
other tests build), and the tail of a simple_test captured into a graph and replayed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segmentor_case  # noqa: E402
import seg_logits_ref as ref  # noqa: E402
import test_mask2former_loss_cpu as loss_helpers  # noqa: E402
from oracle import backbone_cases  # noqa: E402
from vitadapter import EncoderDecoderMask2Former, EncoderDecoderMask2FormerAug, fused  # noqa: E402

pytestmark = pytest.mark.gpu

CASE = segmentor_case.Case()
CLASSES = {'b_': EncoderDecoderMask2Former, 'a_': EncoderDecoderMask2FormerAug}
U = 2.0 ** -24
L = float(max(np.abs(CASE.gold[k]).max() for k in ('b_slide_raw', 'a_slide_raw', 'b_whole')))
LOGIT_TOL = 49 * U * L
PROB_TOL = 2 * 48 * U * L + (2 * L + CASE.meta['classes'] + 16) * U


def dev():
    return torch.device('cuda:0')


class switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.keep = fused.ENABLED['seg_logits']
        fused.ENABLED['seg_logits'] = self.on

    def __exit__(self, *exc):
        fused.ENABLED['seg_logits'] = self.keep


def _err(got, want):
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max())


@pytest.mark.parametrize('prefix', sorted(CLASSES))
def test_golden_on_the_kernels(prefix):
    assert fused.ENABLED['seg_logits']
    seg = CASE.build(CLASSES[prefix], dtype=torch.float32, device=dev())
    imgs = [CASE.image(v, torch.float32, dev()) for v in CASE.views]
    metas = [CASE.metas(v) for v in CASE.views]
    v0 = CASE.views[0]
    _vah = fused._vah
    _vah.prof_enable(True, 'seg_')
    with torch.no_grad():
        e = [_err(seg.slide_inference(imgs[0], metas[0], True), CASE.gold[prefix + 'slide_rescale']),
             _err(seg.slide_inference(imgs[0], metas[0], False), CASE.gold[prefix + 'slide_raw'])]
        print('%s logits: worst error / tolerance %.3g' % (prefix, max(e) / LOGIT_TOL))
        assert max(e) <= LOGIT_TOL
        e = []
        for flip in ('none', 'horizontal', 'vertical'):
            m = CASE.metas(v0, flip=flip != 'none', flip_direction=flip if flip != 'none' else 'horizontal')
            e.append(_err(seg.inference(imgs[0], m, True), CASE.gold[prefix + 'inference_' + flip]))
        print('%s probabilities: worst error / tolerance %.3g' % (prefix, max(e) / PROB_TOL))
        assert max(e) <= PROB_TOL
        assert np.array_equal(np.stack(seg.simple_test(imgs[0], metas[0])), CASE.gold[prefix + 'simple_test'])
        assert np.array_equal(np.stack(seg.aug_test(imgs, metas)), CASE.gold[prefix + 'aug_test'])
    rows = _vah.prof_report()
    _vah.prof_enable(False)
    assert rows['seg_resize_add']['calls'] > 0 and rows['seg_finish']['calls'] > 0 and rows['seg_argmax']['calls'] > 0, rows


def test_whole_mode_on_the_kernels():
    seg = CASE.build(EncoderDecoderMask2Former, mode='whole', dtype=torch.float32, device=dev())
    v0 = CASE.views[0]
    img = CASE.image(v0, torch.float32, dev())
    with torch.no_grad():
        assert _err(seg.whole_inference(img, CASE.metas(v0), True), CASE.gold['b_whole']) <= LOGIT_TOL
        assert np.array_equal(np.stack(seg.simple_test(img, CASE.metas(v0))), CASE.gold['b_whole_simple_test'])


def test_kernels_on_against_off():
    seg = CASE.build(EncoderDecoderMask2FormerAug, dtype=torch.float32, device=dev())
    imgs = [CASE.image(v, torch.float32, dev()) for v in CASE.views]
    metas = [CASE.metas(v) for v in CASE.views]
    out = {}
    for on in (True, False):
        with switch(on), torch.no_grad():
            out[on] = (seg.inference(imgs[1], metas[1], True), seg.simple_test(imgs[1], metas[1]), seg.aug_test(imgs, metas))
    assert float((out[True][0] - out[False][0]).abs().max()) <= PROB_TOL
    assert np.array_equal(out[True][1][0], out[False][1][0]) and np.array_equal(out[True][2][0], out[False][2][0])


# ----------------------------------------------------------------------------------------------------------------------
def _real_segmentor():
    from vitadapter.backbones.vit_adapter import ViTAdapter
    g = np.load(loss_helpers.GOLD)
    meta = json.loads(str(g['meta']))
    torch.manual_seed(0)
    backbone = ViTAdapter(**backbone_cases.FULL_CASES['seg_glob_64']['cfg'])
    head = loss_helpers.build_head(meta, 'cpu')
    head.init_weights()
    cfg = dict(mode='slide', crop_size=(64, 64), stride=(32, 32))
    return EncoderDecoderMask2Former(backbone, head, test_cfg=cfg).to(dev()), meta


def test_real_composition_trains_and_segments():
    seg, meta = _real_segmentor()
    gen = torch.Generator().manual_seed(3)
    img = torch.randn(2, 3, 64, 64, generator=gen).to(dev())
    gt_masks = [(torch.rand(2, 64, 64, generator=gen) > 0.5).to(dev()), (torch.rand(1, 64, 64, generator=gen) > 0.5).to(dev())]
    gt_labels = [torch.tensor([0, 2], device=dev()), torch.tensor([1], device=dev())]
    seg.train()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        losses = seg.forward_train(img, [None, None], None, gt_labels=gt_labels, gt_masks=gt_masks)
    assert losses and all(k.startswith('decode.') for k in losses)
    assert [k[len('decode.'):] for k in losses] == meta['loss_keys']
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    grads = [p.grad for p in seg.parameters() if p.grad is not None]
    assert len(grads) > 50 and all(bool(torch.isfinite(g_).all()) for g_ in grads)

    seg.eval()
    img = torch.randn(2, 3, 64, 96, generator=gen).to(dev())               # 1 x 2 windows
    metas = [dict(ori_shape=(50, 75, 3), img_shape=(64, 96, 3), flip=False, flip_direction='horizontal') for _ in range(2)]
    with torch.no_grad():
        seg.simple_test(img, metas)                                        # first calls may time GEMM candidates
        with switch(True):
            on = seg.simple_test(img, metas)
        with switch(False):
            off = seg.simple_test(img, metas)
            prob = seg.inference(img, metas, True)
    assert len(on) == 2 and all(isinstance(a, np.ndarray) and a.dtype == np.int64 and a.shape == (50, 75) for a in on)
    _, gap = ref.argmax_gap(prob.cpu().double().numpy())
    sure = gap >= ref.BAND
    print('real composition: %.3g of the pixels inside the band' % (1 - sure.mean()))
    assert sure.mean() >= 0.99
    assert np.array_equal(np.stack(on)[sure], np.stack(off)[sure])


def test_simple_test_tail_captures_into_a_graph():
    N, C = 1, 19
    gen = torch.Generator().manual_seed(4)
    logits = [torch.randn(N, C, 16, 16, generator=gen).to(dev()) for _ in range(2)]
    cy = torch.ones(64, dtype=torch.int32, device=dev())
    cx = torch.ones(96, dtype=torch.int32, device=dev())
    cx[32:64] += 1
    preds = torch.empty(N, C, 64, 96, device=dev())

    def tail():
        preds.zero_()
        for out, x0 in zip(logits, (0, 32)):
            fused.seg_resize_add(out, preds, 0, x0, (64, 64), False, accumulate=True)
        return fused.seg_finish(preds, (cy, cx), (60, 90), (50, 75), False, 'horizontal', prob=False, labels=True)[1]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = tail().clone()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lab = tail()
    replays = []
    for _ in range(2):
        lab.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        replays.append(lab.clone())
    assert torch.equal(replays[0], replays[1]) and torch.equal(replays[0], eager)
    with switch(False):
        want = tail()
    _, gap = ref.argmax_gap(torch.softmax(torch.nn.functional.interpolate(
        (preds / (cy[:, None] * cx[None, :]))[:, :, :60, :90], size=(50, 75), mode='bilinear'), 1).flip(3).cpu().double().numpy())
    sure = torch.from_numpy(gap >= ref.BAND).to(dev())
    assert bool(sure.float().mean() >= 0.99) and torch.equal(replays[0][sure], want[sure])
