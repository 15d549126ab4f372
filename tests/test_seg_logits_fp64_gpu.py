"""GPU: the segmentor's logit-tail kernels (csrc/seg_logits.hip, include/vitadapter_hip_seg.h) against the fp64 restatement
of tests/seg_logits_ref.py, called through the C ABI.

Budgets (tests/seg_logits_ref.py), u = 2^-24, A = sum |w| |v| of a logit's terms after the division:
    resize_add      16 u A + u |result|
    probabilities   p_c * (2 d + (|v_c - max v| + C + 16) u), d = 16 u max_c A_c;  + u |result| when accumulating
The taps are bit-identical to the restatement's (un-contracted fp32 operations), so nothing is allowed for them.  Each test
prints its worst error / budget ratio.

Labels are compared where the reference's relative top-two gap (p1 - p2) / p1 is at least 1e-4; there the reference's label
is required, and at most 1 % of a case's pixels may be left out.

Every output is pre-filled with NaN (labels: -7), or with a known prior value for `+=`, and sits between guard elements
that must stay bit-unchanged - as must the part of `dst` outside the window."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_logits_ref as ref  # noqa: E402
import _vah  # noqa: E402

pytestmark = pytest.mark.gpu

lib = _vah.lib
GUARD = 37                   # elements before and after a tensor: odd, so that nothing is 16-byte aligned by accident
CLASSES = (1, 3, 19, 150)
BATCHES = (1, 2)
HD, WD = 61, 67              # dst of resize_add
HA, WA = 50, 56              # acc buffer of finish; its read region (un-pad) is 48 x 52
REGION = (48, 52)


def dev():
    return torch.device('cuda:0')


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _guarded(shape, fill, dtype=torch.float32):
    """-> flat buffer with GUARD elements around a contiguous tensor of ``shape``; the tensor holds ``fill`` (a scalar or a
    CPU tensor), the guards NaN (int64: -7)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float('nan') if dtype.is_floating_point else -7, dtype=dtype, device=dev())
    t = buf[GUARD:GUARD + n].view(shape)
    if torch.is_tensor(fill):
        t.copy_(fill)
    else:
        t.fill_(fill)
    return buf, t


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _guards_unchanged(buf, what):
    g = _bits(buf)
    nan = _bits(torch.full((1,), float('nan') if buf.dtype.is_floating_point else -7, dtype=buf.dtype, device=buf.device))
    assert bool((g[:GUARD] == nan).all()) and bool((g[-GUARD:] == nan).all()), 'guard elements of %s were written' % what


def _pl(t):
    return t.data_ptr(), t.stride(0), t.stride(1), t.stride(2)


def _stream():
    return _vah.raw_stream(dev())


def _check_values(got, want, budget, what):
    """got (cuda fp32) against want (fp64) within budget; NaN exactly where the reference has NaN -> worst ratio"""
    got = got.detach().cpu().double().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), '%s: NaN pattern differs' % what
    ok = ~nan
    if not ok.any():
        return 0.0
    err, b = np.abs(got[ok] - want[ok]), budget[ok]
    assert (b >= 0).all()
    worst = float(np.max(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))))
    assert worst <= 1.0, '%s: worst error / budget %.3g' % (what, worst)
    return worst


def _check_labels(got, want, gap, what):
    got = got.cpu().numpy()
    sure = gap >= ref.BAND
    left_out = 1.0 - sure.mean()
    assert left_out <= 0.01, '%s: %.3g of the pixels inside the band' % (what, left_out)
    assert np.array_equal(got[sure], want[sure]), '%s: %d labels differ' % (what, int((got[sure] != want[sure]).sum()))
    assert got.min() >= 0
    return left_out


# ----------------------------------------------------------------------------------------------------------------------
def run_resize_add(src, prior, y0, x0, hw, align, accumulate):
    """src (N, C, hs, ws) CPU fp32; prior (N, C, Hd, Wd) CPU fp32 or None (NaN) -> dst as a cuda tensor"""
    N, C, hs, ws = src.shape
    s = src.to(dev())
    Hd, Wd = (HD, WD) if prior is None else prior.shape[2:]
    buf, dst = _guarded((N, C, Hd, Wd), float('nan') if prior is None else prior)
    before = _bits(dst).clone()
    _vah.check(lib.vah_seg_resize_add(*_pl(s), N, C, hs, ws, hw[0], hw[1], int(align), *_pl(dst), Hd, Wd, y0, x0, int(accumulate),
                                      _stream()), 'vah_seg_resize_add')
    torch.cuda.synchronize()
    _guards_unchanged(buf, 'dst')
    mask = torch.zeros(dst.shape, dtype=torch.bool)
    mask[:, :, y0:y0 + hw[0], x0:x0 + hw[1]] = True
    outside = ~mask.to(dev())
    assert torch.equal(_bits(dst)[outside], before[outside]), 'dst was written outside the window'
    return dst


@pytest.mark.parametrize('N', BATCHES)
@pytest.mark.parametrize('C', CLASSES)
def test_resize_add(C, N):
    src = _randn(N, C, 12, 13, seed=C * 10 + N)
    prior = _randn(N, C, HD, WD, seed=C * 10 + N + 5)
    worst = 0.0
    for (y0, x0) in ((0, 0), (5, 7)):
        for align in (False, True):
            for accumulate in (False, True):
                dst = run_resize_add(src, prior if accumulate else None, y0, x0, (48, 52), align, accumulate)
                base = prior.numpy() if accumulate else np.full((N, C, HD, WD), np.nan)
                want, budget, mask = ref.resize_add(src.numpy(), base, y0, x0, (48, 52), align, accumulate)
                got = dst.cpu().double().numpy()
                worst = max(worst, _check_values(dst[:, :, y0:y0 + 48, x0:x0 + 52], want[:, :, y0:y0 + 48, x0:x0 + 52],
                                                 budget[:, :, y0:y0 + 48, x0:x0 + 52], 'resize_add'))
                assert np.array_equal(np.isnan(got), ~mask) or accumulate
    print('resize_add C %d N %d: worst error / budget %.3g' % (C, N, worst))


@pytest.mark.parametrize('hw_in,hw_out', (((12, 13), (31, 45)), ((1, 13), (48, 52)), ((12, 1), (48, 52)), ((1, 1), (31, 45)),
                                          ((48, 52), (31, 45))))
def test_resize_add_ratios_and_thin_sources(hw_in, hw_out):
    N, C = 2, 3
    src = _randn(N, C, *hw_in, seed=77)
    prior = _randn(N, C, HD, WD, seed=78)
    worst = 0.0
    for align in (False, True):
        for accumulate in (False, True):
            y0, x0 = 5, 7
            dst = run_resize_add(src, prior if accumulate else None, y0, x0, hw_out, align, accumulate)
            base = prior.numpy() if accumulate else np.full((N, C, HD, WD), np.nan)
            want, budget, _ = ref.resize_add(src.numpy(), base, y0, x0, hw_out, align, accumulate)
            win = (slice(None), slice(None), slice(y0, y0 + hw_out[0]), slice(x0, x0 + hw_out[1]))
            worst = max(worst, _check_values(dst[win], want[win], budget[win], 'resize_add'))
    print('resize_add %s -> %s: worst error / budget %.3g' % (hw_in, hw_out, worst))


def test_resize_add_strided_source_and_non_finite():
    """the source is a channel slice of a wider tensor; 0 * inf = NaN reaches exactly the pixels that name the tap"""
    N, C = 2, 3
    wide = _randn(N, C + 2, 12, 16, seed=79)
    wide[1, 2, 4, 5] = float('inf')
    wide[0, 1, 11, 12] = float('nan')
    s = wide.to(dev())[:, 1:1 + C, :, :13]
    buf, dst = _guarded((N, C, HD, WD), float('nan'))
    _vah.check(lib.vah_seg_resize_add(*_pl(s), N, C, 12, 13, 48, 52, 0, *_pl(dst), HD, WD, 5, 7, 0, _stream()), 'vah_seg_resize_add')
    torch.cuda.synchronize()
    _guards_unchanged(buf, 'dst')
    want, budget, _ = ref.resize_add(wide[:, 1:1 + C, :, :13].numpy(), np.full((N, C, HD, WD), np.nan), 5, 7, (48, 52), False, False)
    got = dst.cpu().double().numpy()
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.isinf(want).any() and np.isnan(want[:, :, 5:53, 7:59]).any()
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert (np.abs(got[fin] - want[fin]) <= budget[fin]).all()


# ----------------------------------------------------------------------------------------------------------------------
def _count_vectors(h, w):
    cy, cx = np.ones(h, dtype=np.int32), np.ones(w, dtype=np.int32)
    cy[16:32] += 1           # two overlapping windows per axis: counts 1, 2 and 4
    cx[20:36] += 1
    return cy, cx


def run_finish(acc, counts, region, size, align, flip, prior, want_prob, want_labels):
    """acc (N, C, Ha, Wa) CPU fp32 -> (prob cuda or None, labels cuda or None)"""
    N, C, Ha, Wa = acc.shape
    a = acc.to(dev())
    Hs, Ws = (Ha, Wa) if region is None else region
    Ho, Wo = (Hs, Ws) if size is None else size
    cy = cx = None
    if counts is not None:
        cy, cx = torch.from_numpy(counts[0]).to(dev()), torch.from_numpy(counts[1]).to(dev())
    pbuf = prob = lbuf = lab = None
    if want_prob:
        pbuf, prob = _guarded((N, C, Ho, Wo), float('nan') if prior is None else prior)
    if want_labels:
        lbuf, lab = _guarded((N, Ho, Wo), -7, torch.int64)
    _vah.check(lib.vah_seg_finish(*_pl(a), N, C, Hs, Ws, None if cy is None else cy.data_ptr(), None if cx is None else cx.data_ptr(),
                                  0 if size is None else 1, Ho, Wo, int(align), flip,
                                  None if prob is None else prob.data_ptr(), C * Ho * Wo, Ho * Wo, Wo, 0 if prior is None else 1,
                                  None if lab is None else lab.data_ptr(), Ho * Wo, Wo, _stream()), 'vah_seg_finish')
    torch.cuda.synchronize()
    if want_prob:
        _guards_unchanged(pbuf, 'prob')
    if want_labels:
        _guards_unchanged(lbuf, 'labels')
    assert torch.equal(_bits(a.cpu()), _bits(acc)), 'acc was written'
    return prob, lab


#          size      flip  +=     prob   labels align  counts region
FINISH = ((None,     0,    False, True,  True,  False, True,  True),
          ((31, 45), 1,    True,  True,  True,  False, True,  True),
          ((31, 45), 2,    False, True,  False, True,  True,  True),
          ((70, 80), 0,    False, False, True,  False, False, False),
          ((70, 80), 1,    True,  True,  False, True,  True,  False),
          (None,     2,    True,  True,  True,  False, False, True),
          (None,     1,    False, False, True,  False, True,  True),
          ((31, 45), 0,    False, False, True,  False, True,  True))


@pytest.mark.parametrize('N', BATCHES)
@pytest.mark.parametrize('C', CLASSES)
def test_finish(C, N):
    acc = _randn(N, C, HA, WA, seed=C * 10 + N + 1)
    worst, left = 0.0, 0.0
    for size, flip, accumulate, want_prob, want_labels, align, with_counts, with_region in FINISH:
        region = REGION if with_region else None
        hs, ws = region or (HA, WA)
        counts = _count_vectors(hs, ws) if with_counts else None
        out_hw = size or (hs, ws)
        prior = _randn(N, C, *out_hw, seed=5).abs() if accumulate else None
        r = ref.finish(acc.numpy(), None if counts is None else counts[0], None if counts is None else counts[1], region, size,
                       align, flip, prior=None if prior is None else prior.numpy())
        prob, lab = run_finish(acc, counts, region, size, align, flip, prior, want_prob, want_labels)
        what = 'finish C %d N %d size %s flip %d' % (C, N, size, flip)
        if want_prob:
            worst = max(worst, _check_values(prob, r['prob'], r['budget'], what))
        if want_labels:
            left = max(left, _check_labels(lab, r['labels'], r['gap'], what))
    print('finish C %d N %d: worst error / budget %.3g, at most %.3g of the labels inside the band' % (C, N, worst, left))


@pytest.mark.parametrize('size', (None, (31, 45), (70, 80)))
def test_finish_tie_the_lower_index_wins(size):
    N, C = 2, 19
    acc = _randn(N, C, HA, WA, seed=31)
    acc[:, 11] = acc[:, 4] = acc[:, 4].abs() + 12.0              # bit-identical planes, the largest everywhere
    counts = _count_vectors(*REGION)
    _, lab = run_finish(acc, counts, REGION, size, False, 1, None, False, True)
    assert bool((lab == 4).all())
    prob, lab = run_finish(acc, None, None, size, True, 0, None, True, True)
    assert bool((lab == 4).all()) and torch.equal(prob[:, 4], prob[:, 11])


@pytest.mark.parametrize('size', (None, (31, 45), (40, 47)))
def test_finish_non_finite(size):
    N, C, H, W = 1, 3, 12, 13
    acc = _randn(N, C, H, W, seed=41)
    acc[0, 1, 3, 3] = float('nan')
    acc[0, 2, 8, 9] = float('inf')
    acc[0, :, 6, 2] = float('-inf')
    acc[0, 0, 10, 4] = float('-inf')
    r = ref.finish(acc.numpy(), size=size)
    prob, lab = run_finish(acc, None, None, size, False, 0, None, True, True)
    _check_values(prob, r['prob'], r['budget'], 'non-finite')             # NaN exactly where the reference has it
    got = lab.cpu().numpy()
    dead = np.isnan(r['p']).all(1)
    assert dead.any() and not dead.all() and np.array_equal(got[dead], r['labels'][dead]) and (got[dead] == 0).all()
    sure = r['gap'] >= ref.BAND
    assert np.array_equal(got[sure], r['labels'][sure])
    if size is None:
        assert float(prob[0, 0, 10, 4]) == 0.0 and bool(torch.isnan(prob[0, :, 6, 2]).all())


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', BATCHES)
@pytest.mark.parametrize('C', CLASSES)
def test_argmax(C, N):
    H, W = 31, 45
    total = torch.softmax(_randn(N, C, H, W, seed=C + N), 1) + torch.softmax(_randn(N, C, H, W, seed=C + N + 1), 1)
    t = total.to(dev())
    left = 0.0
    for divisor in (1, 3, 6):
        buf, lab = _guarded((N, H, W), -7, torch.int64)
        _vah.check(lib.vah_seg_argmax(*_pl(t), N, C, H, W, float(divisor), lab.data_ptr(), H * W, W, _stream()), 'vah_seg_argmax')
        torch.cuda.synchronize()
        _guards_unchanged(buf, 'labels')
        labels, gap = ref.argmax(total.numpy(), divisor)
        left = max(left, _check_labels(lab, labels, gap, 'argmax C %d N %d / %d' % (C, N, divisor)))
    print('argmax C %d N %d: at most %.3g of the labels inside the band' % (C, N, left))


def test_argmax_tie_and_nan():
    N, C, H, W = 2, 19, 31, 45
    total = _randn(N, C, H, W, seed=51).abs()
    total[:, 11] = total[:, 4] = total[:, 4] + 9.0
    total[1, 7, 2, 3] = float('nan')
    total[1, 15, 2, 3] = float('nan')
    total[0, 18, 30, 44] = float('inf')
    t = total.to(dev())
    for divisor in (1, 3, 6):
        buf, lab = _guarded((N, H, W), -7, torch.int64)
        _vah.check(lib.vah_seg_argmax(*_pl(t), N, C, H, W, float(divisor), lab.data_ptr(), H * W, W, _stream()), 'vah_seg_argmax')
        torch.cuda.synchronize()
        _guards_unchanged(buf, 'labels')
        want = torch.full((N, H, W), 4, dtype=torch.int64)
        want[1, 2, 3] = 7                # the first NaN
        want[0, 30, 44] = 18
        assert torch.equal(lab.cpu(), want)
        assert np.array_equal(ref.argmax(total.numpy(), divisor)[0], want.numpy())
