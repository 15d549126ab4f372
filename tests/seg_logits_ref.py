"""Restatement of the three entry points of include/vitadapter_hip_seg.h (csrc/seg_logits.hip) for the tests: the taps in
fp32 exactly as include/vitadapter_hip_resize.h states them (tests/resize_rows_ref.taps: NumPy float32 operations round one
by one, as the kernels' un-contracted ones do), everything else in fp64.  Not a conftest and not a test module.

The resize gathers its four taps and takes all four products, so a non-finite value spreads exactly as far as in torch
(0 * inf = NaN for a tap that is named with weight 0, nothing for a pixel that is not named).

Budgets, u = 2^-24, A_c = sum |w| * |v| over the terms of a logit (after the division):
    resize_add      16 u A + u |result|
    probabilities   p_c * (2 d + (|v_c - max v| + C + 16) u),  d = 16 u * max_c A_c;  + u |result| when accumulating
i.e. softmax's first-order sensitivity to the logits (|dp_c| <= p_c * 2 max|dv|), one rounding per summand of the
denominator and the exponent's argument scaling."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resize_rows_ref import taps  # noqa: E402

U = 2.0 ** -24
FLIPS = {0: None, 1: 3, 2: 2}          # flip code -> the axis of an (N, C, H, W) array it reverses
BAND = 1e-4                            # labels are compared where the reference's relative top-two gap is at least this


def resize(v, hw_out, align_corners):
    """v (N, C, H, W) -> y (N, C, Ho, Wo) fp64 and A = the same blend of |v|"""
    v = np.asarray(v, dtype=np.float64)
    H, W = v.shape[2:]
    Ho, Wo = hw_out
    i0, i1, ly0, ly1 = taps(H, Ho, align_corners)
    j0, j1, lx0, lx1 = taps(W, Wo, align_corners)
    ly0, ly1 = ly0.astype(np.float64)[:, None], ly1.astype(np.float64)[:, None]
    lx0, lx1 = lx0.astype(np.float64)[None, :], lx1.astype(np.float64)[None, :]

    def blend(a):
        v00, v01 = a[:, :, i0[:, None], j0[None, :]], a[:, :, i0[:, None], j1[None, :]]
        v10, v11 = a[:, :, i1[:, None], j0[None, :]], a[:, :, i1[:, None], j1[None, :]]
        with np.errstate(invalid='ignore'):
            return ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
    return blend(v), blend(np.abs(v))


def resize_add(src, dst, y0, x0, hw, align_corners, accumulate):
    """-> (dst after the call, fp64; budget, 0 outside the window; window mask)"""
    Hc, Wc = hw
    out = np.array(dst, dtype=np.float64)
    y, A = resize(src, hw, align_corners)
    win = (slice(None), slice(None), slice(y0, y0 + Hc), slice(x0, x0 + Wc))
    with np.errstate(invalid='ignore'):
        out[win] = out[win] + y if accumulate else y
    budget = np.zeros_like(out)
    with np.errstate(invalid='ignore'):
        budget[win] = 16 * U * A + U * np.abs(out[win])
    mask = np.zeros(out.shape, dtype=bool)
    mask[win] = True
    return out, budget, mask


def softmax(v):
    """over axis 1, with torch's non-finite results: NaN or +inf -> the pixel NaN, -inf -> 0, all -inf -> NaN"""
    with np.errstate(invalid='ignore', over='ignore'):
        m = np.max(v, axis=1, keepdims=True)            # NaN propagates
        e = np.exp(v - m)                               # inf - inf = NaN
        return e / e.sum(axis=1, keepdims=True)


def argmax_gap(p):
    """p (N, C, H, W) -> labels (first index of the largest, NaN counting as largest: np.argmax) and the relative gap
    (p1 - p2) / p1 between the two largest (1 where C == 1; NaN where a value is NaN)"""
    labels = np.argmax(p, axis=1)
    if p.shape[1] == 1:
        return labels, np.ones(labels.shape)
    top = np.sort(p, axis=1)[:, -2:]
    with np.errstate(invalid='ignore', divide='ignore'):
        gap = (top[:, 1] - top[:, 0]) / top[:, 1]
    return labels, gap


def finish(acc, cy=None, cx=None, region=None, size=None, align_corners=False, flip=0, prior=None):
    """-> dict(v, p, prob (p, or prior + p), budget (of prob), labels, gap): everything in output (flipped) position except
    v, the logits after divide / crop / resize"""
    t = np.asarray(acc, dtype=np.float64)
    if region is not None:                  # dividing before or after the crop is the same
        t = t[:, :, :region[0], :region[1]]
    if cy is not None:                      # cy, cx cover at least the read region
        cy, cx = np.asarray(cy, dtype=np.float64)[:t.shape[2]], np.asarray(cx, dtype=np.float64)[:t.shape[3]]
        t = t / (cy[:, None] * cx[None, :])
    if size is not None:
        v, A = resize(t, size, align_corners)
    else:
        v, A = t, np.abs(t)
    C = v.shape[1]
    p = softmax(v)
    with np.errstate(invalid='ignore'):
        d = 16 * U * np.max(np.where(np.isfinite(A), A, 0.0), axis=1, keepdims=True)     # a -inf logit carries no error
        budget = p * (2 * d + (np.abs(v - np.max(v, axis=1, keepdims=True)) + C + 16) * U)
        budget = np.where(p == 0, 0.0, budget)          # a -inf logit: exactly 0 is required (0 * inf above)
    ax = FLIPS[flip]
    if ax is not None:
        p, budget = np.flip(p, ax), np.flip(budget, ax)
    prob = p
    if prior is not None:
        prob = np.asarray(prior, dtype=np.float64) + p
        budget = budget + U * np.abs(prob)
    labels, gap = argmax_gap(p)
    return dict(v=v, p=p, prob=prob, budget=budget, labels=labels, gap=gap)


def argmax(total, divisor):
    """labels and relative top-two gap of total / divisor"""
    return argmax_gap(np.asarray(total, dtype=np.float64) / float(divisor))
