"""CPU: the training side of UPerHead / FCNHead (vitadapter/heads.py: losses, forward_train, forward_test) and the
EncoderDecoder segmentor (vitadapter/segmentor.py), on the torch path of vitadapter.fused.seg_cross_entropy, against the
expression of mmseg's BaseDecodeHead.losses written out by hand: resize, F.cross_entropy(reduction='none', ignore_index=255),
the mean over all pixels (or the valid ones), accuracy over all pixels.  tests/test_seg_ce_loss_module_gpu.py repeats the
checks on the kernels and imports the cases from here."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from vitadapter import EncoderDecoder, EncoderDecoderMask2Former, fused
from vitadapter.heads import FCNHead, UPerHead

CLASSES = 19


class StubBackbone(nn.Module):
    """four seeded maps of 64 channels at strides 4 - 32 of a 64 x 64 image, whatever the image holds"""

    def __init__(self, batch=2, seed=5):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        for i in range(4):
            self.register_buffer('f%d' % i, torch.randn(batch, 64, 16 >> i, 16 >> i, generator=g))

    def forward(self, img):
        return [getattr(self, 'f%d' % i).to(img.dtype) for i in range(4)]


def heads(aux=1, **loss):
    torch.manual_seed(3)
    loss_decode = dict(dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0), **loss)
    uper = UPerHead(in_channels=(64, 64, 64, 64), channels=64, num_classes=CLASSES, norm=nn.BatchNorm2d, loss_decode=loss_decode)
    fcn = [FCNHead(in_channels=64, in_index=2 + (i % 2), channels=64, num_classes=CLASSES, norm=nn.BatchNorm2d,
                   loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.4)) for i in range(aux)]
    for m in [uper] + fcn:
        with torch.no_grad():
            m.conv_seg.weight.normal_(0, 0.5)           # logits of size 1, not mmseg's 0.01
    return uper, fcn


def labels(batch=2, hw=(64, 64), seed=9, ignored=0.1):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, CLASSES, (batch, 1) + hw, generator=g)
    y[torch.rand((batch, 1) + hw, generator=g) < ignored] = 255
    return y


def by_hand(seg_logit, seg_label, align_corners=False, loss_weight=1.0, class_weight=None, avg_non_ignore=False):
    """mmseg's BaseDecodeHead.losses with the reference's CrossEntropyLoss, written out"""
    y = seg_label.squeeze(1)
    up = F.interpolate(seg_logit.float() if seg_logit.dtype != torch.float64 else seg_logit, size=y.shape[1:], mode='bilinear',
                       align_corners=align_corners)
    loss = F.cross_entropy(up, y, weight=class_weight, reduction='none', ignore_index=255)
    loss = loss.sum() / (y != 255).sum() if avg_non_ignore else loss.mean()
    acc = (up.argmax(dim=1) == y).sum() * (100.0 / y.numel())
    return loss_weight * loss, acc


def _f(t):
    return float(t.detach())


CASES = (dict(), dict(avg_non_ignore=True), dict(loss_weight=0.4),
         dict(loss_weight=0.4, avg_non_ignore=True, class_weight=[0.5 + 0.0625 * i for i in range(CLASSES)]))       # exact in fp32


@pytest.mark.parametrize('cfg', CASES)
@pytest.mark.parametrize('which', ('uper', 'fcn'))
def test_losses_are_the_hand_written_expression(which, cfg):
    if which == 'uper':
        head = heads(**cfg)[0].double()
    else:
        head = FCNHead(in_channels=64, in_index=2, channels=64, num_classes=CLASSES, norm=nn.BatchNorm2d,
                       loss_decode=dict(type='CrossEntropyLoss', **cfg)).double()
    y = labels()
    g = torch.Generator().manual_seed(1)
    logit = torch.randn(2, CLASSES, 16, 16, generator=g, dtype=torch.float64, requires_grad=True)
    out = head.losses(logit, y)
    assert sorted(out) == ['acc_seg', 'loss_ce']
    cw = None if 'class_weight' not in cfg else torch.tensor(cfg['class_weight'], dtype=torch.float64)
    want, acc = by_hand(logit, y, False, cfg.get('loss_weight', 1.0), cw, cfg.get('avg_non_ignore', False))
    assert abs(_f(out['loss_ce']) - _f(want)) <= 1e-12 * max(1.0, abs(_f(want)))
    assert abs(_f(out['acc_seg']) - _f(acc)) <= 1e-9 and 0 < _f(acc) < 100
    grad, = torch.autograd.grad(out['loss_ce'], logit)
    want_grad, = torch.autograd.grad(want, logit)
    assert float((grad - want_grad).abs().max()) <= 1e-15
    # the (N, H, W) form of the label map, and a loss name of one's own
    assert _f(head.losses(logit, y.squeeze(1))['loss_ce']) == _f(out['loss_ce'])
    named = FCNHead(in_channels=64, channels=8, num_classes=CLASSES, norm=nn.BatchNorm2d,
                    loss_decode=dict(type='CrossEntropyLoss', loss_name='loss_aux'))
    assert sorted(named.losses(logit.float(), y)) == ['acc_seg', 'loss_aux']


def test_all_ignored_is_zero_or_nan():
    uper, _ = heads()
    y = torch.full((2, 1, 64, 64), 255)
    logit = torch.randn(2, CLASSES, 16, 16)
    out = uper.losses(logit, y)
    assert float(out['loss_ce']) == 0.0 and float(out['acc_seg']) == 0.0
    uper, _ = heads(avg_non_ignore=True)
    assert torch.isnan(uper.losses(logit, y)['loss_ce'])                    # 0 / 0, as in the reference


def test_state_dict_and_forward_are_untouched():
    uper, (fcn,) = heads(class_weight=[1.0] * CLASSES)
    assert not any('class_weight' in k or 'loss' in k for k in list(uper.state_dict()) + list(fcn.state_dict()))
    assert uper.class_weight.dtype == torch.float32 and fcn.class_weight is None
    assert uper.ignore_index == 255 and uper.loss_weight == 1.0 and fcn.loss_weight == 0.4 and not uper.avg_non_ignore
    x = StubBackbone()(torch.zeros(2, 3, 64, 64))
    uper.eval()
    assert torch.equal(uper.forward_test(x, None, None), uper(x))


@pytest.mark.parametrize('kw', (dict(loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=True)),
                                dict(loss_decode=dict(type='CrossEntropyLoss', use_mask=True)),
                                dict(sampler=dict(type='OHEMPixelSampler', thresh=0.7))))
@pytest.mark.parametrize('cls', (UPerHead, FCNHead))
def test_unsupported_loss_options_raise(cls, kw):
    with pytest.raises(NotImplementedError):
        cls(in_channels=(64,) * 4 if cls is UPerHead else 64, channels=8, num_classes=CLASSES, norm=nn.BatchNorm2d, **kw)


def check_forward_train(dev, tol):
    """shared with the GPU test: the keys, the values against the hand-written expression on the head's own logits, and a
    gradient in every head parameter"""
    img = torch.zeros(2, 3, 64, 64, device=dev)
    y = labels().to(dev)
    uper, fcn = heads(aux=1)
    seg = EncoderDecoder(StubBackbone(), uper, auxiliary_head=fcn[0]).to(dev).train()
    assert seg.with_auxiliary_head and seg.with_decode_head
    for m in seg.modules():
        if isinstance(m, nn.Dropout2d):
            m.p = 0.0                                    # the hand-written side runs the head a second time
    out = seg.forward_train(img, None, y)
    assert sorted(out) == ['aux.acc_seg', 'aux.loss_ce', 'decode.acc_seg', 'decode.loss_ce']
    x = seg.extract_feat(img)
    for prefix, head, lw in (('decode.', seg.decode_head, 1.0), ('aux.', seg.auxiliary_head, 0.4)):
        want, acc = by_hand(head(x), y, loss_weight=lw)
        assert abs(_f(out[prefix + 'loss_ce']) - _f(want)) <= tol * _f(want), prefix
        assert abs(_f(out[prefix + 'acc_seg']) - _f(acc)) <= 100.0 * 8 / y.numel(), prefix
    sum(v for k, v in out.items() if 'loss' in k).backward()
    for name, p in list(seg.decode_head.named_parameters()) + list(seg.auxiliary_head.named_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    uper, fcn = heads(aux=2)
    seg = EncoderDecoder(StubBackbone(), uper, auxiliary_head=fcn).to(dev).train()
    out = seg.forward_train(img, None, y)
    assert sorted(out) == ['aux_0.acc_seg', 'aux_0.loss_ce', 'aux_1.acc_seg', 'aux_1.loss_ce', 'decode.acc_seg', 'decode.loss_ce']
    assert _f(out['aux_0.loss_ce']) != _f(out['aux_1.loss_ce'])
    seg = EncoderDecoder(StubBackbone(), uper).to(dev)
    assert not seg.with_auxiliary_head and sorted(seg.forward_train(img, None, y)) == ['decode.acc_seg', 'decode.loss_ce']


def test_forward_train_cpu():
    check_forward_train(torch.device('cpu'), 1e-5)


def test_switch_is_registered():
    assert fused.ENABLED['seg_ce_loss'] is True


class _FixedLogits(nn.Module):
    """a decode head for EncoderDecoderMask2Former that returns what it was given"""

    num_classes, align_corners = CLASSES, False

    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward_test(self, x, img_metas, test_cfg):
        return self.logits


@pytest.mark.parametrize('mode', ('whole', 'slide'))
def test_simple_test_is_the_mask2former_tail(mode):
    uper, _ = heads()
    uper.eval()
    cfg = dict(mode=mode, crop_size=(64, 64), stride=(48, 48))
    seg = EncoderDecoder(StubBackbone(batch=1), uper, test_cfg=cfg).eval()
    img = torch.zeros(1, 3, 64, 64)
    meta = [dict(ori_shape=(50, 70, 3), img_shape=(64, 64, 3), flip=False)]
    with torch.no_grad():
        logits = uper(seg.extract_feat(img))
        got = seg.simple_test(img, meta)
        want = EncoderDecoderMask2Former(StubBackbone(batch=1), _FixedLogits(logits), test_cfg=cfg).simple_test(img, meta)
    assert len(got) == 1 and got[0].shape == (50, 70) and (got[0] == want[0]).all()
    assert len(set(got[0].ravel().tolist())) > 3
