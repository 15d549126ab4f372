"""GPU: vah_sce_forward / vah_sce_backward (csrc/seg_ce_loss.hip) through the C ABI against the fp64 restatement of
tests/seg_ce_loss_ref.py, within its budgets, with NaN-filled guard elements around every output that must come back
unchanged.

K, the longest chain of fp32 additions behind loss_sum, counted from the code: a thread contributes one value (no addition);
the workgroup's sum is wave_sum (6 additions) and the four waves in order (3); the merge launch's thread t adds the partials
t, t + 256, ... into 0 (ceil(P / 256) additions, P = N * ceil(H * W / 256) partials), then the same 6 + 3:
K = 18 + ceil(P / 256).  K' (the gather) is counted by the helper from the tap ranges.

The backward runs one of three instantiations, 16, 8 or 4 classes per workgroup, by the number of workgroups
N * tiles * ceil(C / R) against 1024 (tiles of 4 x 16 source pixels): the small cases all take 4, two cases below are sized to
take 8 and 16."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_ce_loss_ref as ref  # noqa: E402

import _vah  # noqa: E402

pytestmark = pytest.mark.gpu
lib = _vah.lib
DTYPES = {'float32': (torch.float32, 0), 'bfloat16': (torch.bfloat16, 1), 'float16': (torch.float16, 2)}
SIZES = (((5, 7), (20, 28)), ((3, 3), (48, 48)), ((7, 5), (23, 18)), ((9, 11), (9, 11)), ((12, 10), (5, 4)), ((1, 1), (6, 5)))
G = 64                  # guard elements on either side of a flat output
SENTINEL = -7


def chain(N, H, W):
    parts = N * ((H * W + 255) // 256)
    return 18 + (parts + 255) // 256


def run_of(N, C, h, w):
    """the backward's class run, restated from csrc/seg_ce_loss.hip"""
    tiles = ((h + 3) // 4) * ((w + 15) // 16)
    for R in (16, 8):
        if N * tiles * ((C + R - 1) // R) >= 1024:
            return R
    return 4


def make(C, hw, HW, N=2, seed=0, ignored=0.1, dtype='float32'):
    """seeded standard-normal logits rounded to ``dtype`` (the values the kernel reads), labels with ``ignored`` at 255,
    weights in [0.5, 1.5)"""
    g = torch.Generator().manual_seed(1000 * seed + 31 * C + hw[0] + HW[1])
    logits = torch.randn((N, C) + tuple(hw), generator=g).to(DTYPES[dtype][0])
    labels = torch.randint(0, C, (N,) + tuple(HW), generator=g)
    labels[torch.rand((N,) + tuple(HW), generator=g) < ignored] = 255
    weight = torch.rand((C,), generator=g) + 0.5
    return logits, labels, weight


def _guarded(n, dtype, fill, dev):
    buf = torch.full((n + 2 * G,), fill, dtype=dtype, device=dev)
    return buf, buf[G:G + n]


def _intact(buf, n, fill):
    edge = torch.cat([buf[:G], buf[G + n:]])
    return bool(torch.isnan(edge).all()) if fill != fill else bool((edge == fill).all())


def call(logits, labels, align=False, weight=None, scale=1.0, strided=False, ignore_index=255):
    """logits (N, C, h, w) in their storage dtype and labels (N, H, W) int64, CPU tensors -> dict(lse, loss_sum, n_valid,
    n_correct, dlogits) as NumPy arrays.  ``strided``: logits, labels and dlogits are windows of larger buffers."""
    dev = torch.device('cuda')
    N, C, h, w = logits.shape
    H, W = labels.shape[1:]
    code = {v[0]: v[1] for v in DTYPES.values()}[logits.dtype]
    nan = float('nan')
    if strided:
        big = torch.full((N, C + 1, h + 2, w + 3), 3.0, dtype=logits.dtype, device=dev)
        x = big[:, :C, 1:h + 1, 2:w + 2]
        x.copy_(logits)
        bigy = torch.full((N + 1, H + 1, W + 5), 1, dtype=torch.int64, device=dev)
        y = bigy[:N, 1:, 3:W + 3]
        y.copy_(labels)
        bigd = torch.full((N, C + 2, h + 1, w + 4), nan, dtype=logits.dtype, device=dev)
        d = bigd[:, 1:C + 1, :h, 3:w + 3]
    else:
        x, y = logits.to(dev), labels.to(dev)
        bigd, d = _guarded(N * C * h * w, logits.dtype, nan, dev)
        d = d.view(N, C, h, w)
    cw = None if weight is None else weight.to(dev).float().contiguous()
    lse_buf, lse = _guarded(N * H * W, torch.float32, nan, dev)
    sum_buf, loss_sum = _guarded(1, torch.float32, nan, dev)
    cnt_buf, counts = _guarded(2, torch.int64, SENTINEL, dev)
    scale_t = torch.tensor([scale], dtype=torch.float32, device=dev)
    nbytes = lib.vah_sce_ws_bytes(N, C, h, w, H, W)
    assert nbytes > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    head = (x.data_ptr(), code, x.stride(0), x.stride(1), x.stride(2), N, C, h, w, y.data_ptr(), y.stride(0), y.stride(1), H, W,
            1 if align else 0, ignore_index, None if cw is None else cw.data_ptr())
    stream = _vah.raw_stream(dev)
    _vah.check(lib.vah_sce_forward(*head, lse.data_ptr(), loss_sum.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, stream),
               'vah_sce_forward')
    ws.fill_(0xFF)                                       # the backward takes nothing from the forward's workspace
    _vah.check(lib.vah_sce_backward(*head, lse.data_ptr(), scale_t.data_ptr(), d.data_ptr(), d.stride(0), d.stride(1), d.stride(2),
                                    ws.data_ptr(), nbytes, stream), 'vah_sce_backward')
    torch.cuda.synchronize()
    assert _intact(lse_buf, N * H * W, nan) and _intact(sum_buf, 1, nan) and _intact(cnt_buf, 2, SENTINEL), 'a guard was written'
    if strided:
        mask = torch.ones(bigd.shape, dtype=torch.bool, device=dev)
        mask[:, 1:C + 1, :h, 3:w + 3] = False
        assert bool(torch.isnan(bigd[mask]).all()), 'dlogits was written outside its window'
        assert bool((big[:, C] == 3.0).all()) and bool((bigy[N] == 1).all())
    else:
        assert _intact(bigd, N * C * h * w, nan), 'a guard of dlogits was written'
    return dict(lse=lse.view(N, H, W).cpu().numpy(), loss_sum=float(loss_sum.cpu()[0]), n_valid=int(counts.cpu()[0]),
                n_correct=int(counts.cpu()[1]), dlogits=d.float().cpu().numpy().astype(np.float64))


def check(logits, labels, align=False, weight=None, scale=1.0, strided=False, informative=True):
    got = call(logits, labels, align, weight, scale, strided)
    N, C, h, w = logits.shape
    want = ref.reference(logits.float().numpy(), labels.numpy(), align, 255, None if weight is None else weight.numpy(), scale,
                         str(logits.dtype).replace('torch.', ''), K=chain(N, *labels.shape[1:]))
    worst = ref.compare(got, want, informative)
    print('C %d N %d %s -> %s %s%s: error / budget %s' % (C, N, (h, w), tuple(labels.shape[1:]), logits.dtype,
                                                        ' strided' if strided else '', worst))
    return got, want, worst


@pytest.mark.parametrize('align', (False, True))
@pytest.mark.parametrize('hw,HW', SIZES)
@pytest.mark.parametrize('C', (1, 3, 19, 150))
def test_against_fp64(C, hw, HW, align):
    """every dtype with (N 1, contiguous, no class weights) and (N 2, windows of larger buffers, class weights)"""
    for dtype in DTYPES:
        for N, strided, weighted, scale in ((1, False, False, 1.0), (2, True, True, 0.37 / (HW[0] * HW[1]))):
            logits, labels, weight = make(C, hw, HW, N=N, seed=int(align), dtype=dtype)
            check(logits, labels, align, weight if weighted else None, scale, strided)


def test_several_workgroups_are_merged():
    logits, labels, weight = make(150, (32, 32), (128, 128), N=2, seed=3)
    assert chain(2, 128, 128) == 19 and run_of(2, 150, 32, 32) == 4
    got, want, _ = check(logits, labels, False, weight, 1.0 / labels.numel())
    assert got['n_valid'] == int((labels != 255).sum())


@pytest.mark.parametrize('hw,HW,R', (((44, 256), (60, 300), 8), ((64, 256), (96, 300), 16)))
def test_the_wider_class_runs_of_the_backward(hw, HW, R):
    assert run_of(2, 19, *hw) == R
    for dtype in ('float32', 'float16'):
        logits, labels, weight = make(19, hw, HW, N=2, seed=4, dtype=dtype)
        check(logits, labels, False, weight, 2.0 / labels.numel())


def test_an_all_ignored_image():
    logits, labels, _ = make(19, (5, 7), (20, 28), N=2, seed=5)
    labels[0] = 255
    got, want, _ = check(logits, labels, informative=False)
    assert np.all(got['dlogits'][0] == 0) and np.abs(got['dlogits'][1]).max() > 0
    assert got['n_valid'] == int((labels[1] != 255).sum())
    labels[1] = 255
    got, _, _ = check(logits, labels, informative=False)
    assert got['loss_sum'] == 0.0 and got['n_valid'] == 0 and got['n_correct'] == 0 and np.all(got['dlogits'] == 0)
    assert np.isfinite(got['lse']).all()                 # lse is written for ignored pixels as well


def test_a_label_that_is_no_class_is_ignored():
    logits, labels, weight = make(150, (5, 7), (20, 28), N=2, seed=6)
    base = call(logits, labels, weight=weight)
    other = labels.clone()
    other[labels == 255] = 200                           # 150 <= 200, not ignore_index: the weights must not be read at 200
    other[0, 0, 0], other[1, 3, 4] = -1, 1 << 40
    labels[0, 0, 0] = labels[1, 3, 4] = 255
    got, want, _ = check(logits, other, weight=weight)
    same = call(logits, labels, weight=weight)
    assert got['loss_sum'] == same['loss_sum'] and got['n_valid'] == same['n_valid'] and got['n_correct'] == same['n_correct']
    assert np.array_equal(got['dlogits'], same['dlogits']) and got['n_valid'] <= base['n_valid']


def test_a_tie_goes_to_the_lower_index():
    logits, labels, _ = make(19, (7, 5), (23, 18), N=2, seed=7, ignored=0.0)
    logits[:, 4] = logits[:, 11] = logits.max() + 2.0    # two identical planes above all others
    labels[:] = 4
    got = call(logits, labels, align=True)
    assert got['n_valid'] == labels.numel() and got['n_correct'] == labels.numel()
    labels[:] = 11
    assert call(logits, labels, align=True)['n_correct'] == 0


@pytest.mark.parametrize('where', ('valid', 'ignored'))
@pytest.mark.parametrize('value', (float('nan'), float('inf'), float('-inf')))
def test_non_finite_logits(value, where):
    """one non-finite low-resolution logit (image 0, class 1, pixel (2, 3)), tapped by valid pixels only or by ignored pixels
    only; image 1 is ordinary.  The comparison requires NaN and inf in exactly the reference's places."""
    logits, labels, weight = make(3, (5, 7), (20, 28), N=2, seed=8, ignored=0.0)
    logits[0, 1, 2, 3] = value
    labels[0] = 255 if where == 'ignored' else 0
    got, want, _ = check(logits, labels, weight=weight, scale=0.01, informative=False)
    d = got['dlogits']
    assert np.isfinite(d[1]).all() and np.abs(d[1]).max() > 0
    if value == float('-inf'):                           # exp(-inf) = 0: a class that is never the label costs nothing
        assert np.isfinite(got['loss_sum']) and np.isfinite(d).all()
        assert np.all(d[0] == 0) == (where == 'ignored')
    else:
        assert np.isnan(got['loss_sum']) == (where == 'valid')
        assert np.isnan(d[0, :, 2, 3]).all() and np.isnan(d[0, :, 1:4, 2:5]).all() and np.isfinite(d[0, :, 0, 0]).all()
        assert np.isnan(got['lse'][0]).sum() == np.isnan(want['lse'][0]).sum() > 0
