"""GPU: vitadapter.fused.seg_cross_entropy (autograd glue over csrc/seg_ce_loss.hip), the losses of UPerHead / FCNHead and
EncoderDecoder.forward_train on the kernels.

Switch on against switch off: both sides are held to the fp64 restatement of tests/seg_ce_loss_ref.py.  The kernel side gets
its budgets.  The torch side evaluates the same expression in fp32 with the same number of roundings in another order - the
blend, log_softmax's sum over C, the sum over the pixels, the scatter of the upsample's adjoint over the same K' summands -
so its own error is bounded by the same budgets, and it gets them twice: once for what the budgets allow the kernels, once
for itself."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_ce_loss_ref as ref  # noqa: E402
import test_heads_train_cpu as cases  # noqa: E402
from test_seg_ce_loss_fp64_gpu import chain, make  # noqa: E402
from vitadapter import fused  # noqa: E402
from vitadapter.heads import FCNHead, UPerHead  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


class switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = fused.ENABLED['seg_ce_loss']
        fused.ENABLED['seg_ce_loss'] = self.on

    def __exit__(self, *exc):
        fused.ENABLED['seg_ce_loss'] = self.old
        return False


def dev():
    return torch.device('cuda')


def run(logits, labels, weight, autocast, scale):
    """one forward + backward of scale * loss_sum -> what ref.compare takes (no lse: the glue keeps it to itself); the
    gradient arrives at the fp32 leaf through the cast that autocast's conv_seg would have made"""
    x = logits.to(dev()).float().requires_grad_(True)
    seg_logit = x if autocast is None else x.to(autocast)
    with torch.autocast('cuda', dtype=autocast or torch.bfloat16, enabled=autocast is not None):
        loss_sum, n_valid, n_correct = fused.seg_cross_entropy(seg_logit, labels.to(dev()), False, 255,
                                                               None if weight is None else weight.to(dev()))
    assert loss_sum.dtype == torch.float32 and n_valid.dtype == n_correct.dtype == torch.int64 and loss_sum.dim() == 0
    (scale * loss_sum).backward()
    return dict(loss_sum=float(loss_sum.detach()), n_valid=int(n_valid), n_correct=int(n_correct), dlogits=x.grad.cpu().numpy())


@pytest.mark.parametrize('autocast', (None, torch.float16, torch.bfloat16))
@pytest.mark.parametrize('C,hw,HW', ((19, (7, 5), (23, 18)), (150, (12, 12), (48, 48))))
def test_switch_on_against_off(C, hw, HW, autocast):
    name = 'float32' if autocast is None else str(autocast).replace('torch.', '')
    logits, labels, weight = make(C, hw, HW, N=2, seed=12, dtype=name)
    scale = 3.0 / labels.numel()
    want = ref.reference(logits.float().numpy(), labels.numpy(), False, 255, weight.numpy(), scale, name, K=chain(2, *HW))
    with switch(True):
        on = run(logits, labels.unsqueeze(1), weight, autocast, scale)
    with switch(False):
        off = run(logits, labels.unsqueeze(1), weight, autocast, scale)
    print('kernels', ref.compare(on, want))
    twice = dict(want, **{k: 2 * v for k, v in want.items() if k.startswith('b_')})
    print('torch  ', ref.compare(off, twice))


def test_two_runs_give_the_same_bits():
    logits, labels, weight = make(150, (32, 32), (128, 128), N=2, seed=13)
    a = run(logits, labels, weight, None, 0.5)
    b = run(logits, labels, weight, None, 0.5)
    assert a['loss_sum'] == b['loss_sum'] and a['n_valid'] == b['n_valid'] and a['n_correct'] == b['n_correct']
    assert np.array_equal(a['dlogits'], b['dlogits'])


def test_forward_and_backward_capture_into_a_graph():
    """one capture on one stream, replayed after logits and labels were overwritten in place: the eager result, bit for bit"""
    first, labels1, weight = make(19, (12, 10), (40, 36), N=2, seed=14)
    second, labels2, _ = make(19, (12, 10), (40, 36), N=2, seed=15)
    x = first.to(dev()).requires_grad_(True)
    y, cw = labels1.to(dev()), weight.to(dev())

    def step():
        loss_sum, n_valid, n_correct = fused.seg_cross_entropy(x, y, True, 255, cw)
        grad, = torch.autograd.grad(loss_sum / y.numel(), x)
        return loss_sum, n_valid, n_correct, grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        x.copy_(second.to(dev()))
        y.copy_(labels2.to(dev()))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    eager = step()
    for name, a, b in zip(('loss_sum', 'n_valid', 'n_correct', 'grad'), replayed, eager):
        assert torch.equal(a, b), name
    assert int(eager[1]) == int((labels2 != 255).sum()) != int((labels1 != 255).sum())


@pytest.mark.parametrize('cfg', cases.CASES)
@pytest.mark.parametrize('cls', (UPerHead, FCNHead))
def test_head_losses_follow_the_formulas(cls, cfg):
    """loss_ce = loss_weight * loss_sum / numel (or / n_valid), acc_seg = 100 * n_correct / numel, from the restatement's
    loss_sum and counts: loss_sum's budget scaled like the value, and 4 u for the division and the two products"""
    C = cases.CLASSES
    head = cls(in_channels=(64,) * 4 if cls is UPerHead else 64, channels=8, num_classes=C, norm=torch.nn.BatchNorm2d,
               loss_decode=dict(type='CrossEntropyLoss', **cfg)).to(dev())
    logits, labels, _ = make(C, (16, 16), (64, 64), N=2, seed=16)
    out = head.losses(logits.to(dev()), labels.unsqueeze(1).to(dev()))
    assert sorted(out) == ['acc_seg', 'loss_ce']
    want = ref.reference(logits.numpy(), labels.numpy(), False, 255, cfg.get('class_weight'), K=chain(2, 64, 64))
    factor = cfg.get('loss_weight', 1.0) / (want['n_valid'] if cfg.get('avg_non_ignore') else labels.numel())
    value = factor * want['loss_sum']
    assert abs(float(out['loss_ce'].detach()) - value) <= factor * want['b_loss_sum'] + 4 * U * abs(value)
    assert want['band'] <= ref.MAX_BAND
    lo, hi = (100.0 * n / labels.numel() for n in (want['n_correct_lo'], want['n_correct_hi']))
    assert lo * (1 - 2 * U) <= float(out['acc_seg']) <= hi * (1 + 2 * U) and lo > 0


def test_all_ignored_on_the_kernels():
    head = FCNHead(in_channels=64, channels=8, num_classes=19, norm=torch.nn.BatchNorm2d,
                   loss_decode=dict(type='CrossEntropyLoss', avg_non_ignore=True)).to(dev())
    logits = torch.randn(2, 19, 8, 8, device=dev(), requires_grad=True)
    out = head.losses(logits, torch.full((2, 1, 32, 32), 255, device=dev()))
    assert torch.isnan(out['loss_ce']) and float(out['acc_seg']) == 0.0      # 0 / 0, a device division


def test_encoder_decoder_forward_train():
    """the CPU test's checks with the loss on the kernels against the hand-written torch expression on the same device: two
    fp32 evaluations, each within (2 * 16 + C + 16 + 6 + K) u < 2e-6 of the exact mean relative to a loss of about 3"""
    assert fused.ENABLED['seg_ce_loss']
    cases.check_forward_train(dev(), 1e-5)
