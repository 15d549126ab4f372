"""Restatement of the two entry points of include/vitadapter_hip_seg_loss.h (csrc/seg_ce_loss.hip) for the tests: the taps in
fp32 exactly as include/vitadapter_hip_resize.h states them (tests/seg_logits_ref.resize), everything else - lse, the
per-pixel loss, the sums, the counts and dlogits, the exact transpose of the blend - in fp64.  Not a conftest and not a
test module.

Non-finite rules (the header's): a pixel whose blended logits hold a NaN or +inf, or only -inf, has a NaN lse; a valid pixel
adds w * (lse - v_y) to loss_sum (NaN, or +inf for v_y = -inf), an ignored pixel adds 0; in the backward a valid pixel adds
scale * w * (exp(v_c - lse) - [c == y]) (NaN in every class for a NaN lse), an ignored pixel with a finite lse nothing, an
ignored pixel with a NaN lse NaN in every class - through every tap it NAMES, whatever the weight (0 * NaN = NaN).  A label
outside [0, C) that is not ignore_index is ignored.

n_correct lies between the valid pixels that are correct and outside the band - the relative gap of the two largest
probabilities is at least seg_logits_ref.BAND, or the two classes read identical taps (_same_taps) - and that number plus the
valid pixels inside the band.

Budgets, u = 2^-24, A_c = the blend of |v| for class c, d = 16 u max_c A_c (the blend's seven roundings and the 16-bit
headroom of seg_logits_ref), every lse and logit term by absolute value:
    lse        d + (C + 16) u + u |lse|
    loss l     w (2 d + (C + 16) u + u (|lse| + |v_y|)) + u |l|
    loss_sum   sum of the per-pixel budgets + K u sum |l|,  K = the longest chain of fp32 additions (the caller counts it)
    p_c        p_c (2 d + (|v_c - max v| + C + 16) u  +  (|lse| + ln C + 2) u)
               the first part is the form of seg_logits_ref (softmax's first-order sensitivity 2 max|dv|, one rounding per
               summand of the denominator, the exponent's argument).  The second part is added here and comes from how the
               backward forms p_c = expf(v_c - lse) from the STORED lse instead of exp(v_c - m) / s: the store rounds lse to
               fp32 (u |lse|, and p_c's sensitivity to lse is p_c), the subtraction v_c - lse rounds once
               (u |v_c - lse| <= u (|v_c - max v| + ln C), of which the first term is already counted), expf is good to 2 ulp.
    dlogits    sum over the tapping pixels of W |scale| w (budget(p_c) + u (p_c + 1))  +  K' u sum W |g|  +  e_out |dlogits|
               (+ 2^-25 for fp16, whose subnormals are 2^-24 apart), g = scale w (p_c - [c == y]), W = wy wx, e_out the
               output dtype's half-ulp (2^-24, 2^-8 bf16, 2^-11 fp16: 24, 8 and 11 significand bits).  K' = the additions of the gather, at most the number
               of tapping pixels, plus 6 for the roundings of the coefficient that the formula above does not name: l0 + l1 of
               a clamped tap on either axis (2), wy * wx (1), scale * w (1), their product (1) and the product with
               (p_c - [c == y]) (1).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resize_rows_ref import axis_matrix, taps  # noqa: E402
from seg_logits_ref import BAND, U, argmax_gap, resize, softmax  # noqa: E402

E_OUT = {'float32': 2.0 ** -24, 'bfloat16': 2.0 ** -8, 'float16': 2.0 ** -11}
MAX_BAND = 0.005            # a case whose band holds more of its pixels says nothing about n_correct


def _adjoint(my, mx, t):
    """t (N, C, H, W) -> (N, C, h, w): the transpose of the blend with the weight matrices my (H, h), mx (W, w)"""
    return np.einsum('oy,ncop,px->ncyx', my, t, mx, optimize=True)


def _same_taps(logits, p, arg, hw_out, align_corners):
    """per output pixel: do the two most probable classes read the same values through every tap of non-zero weight (all
    eight values being finite)?  A tap of weight 0 adds an exact 0, so the kernel's two logits are then the same bits - the
    same operations on the same operands - and its argmax is the lower index for certain, as ``arg`` is: such a tie,
    frequent between logits rounded to 16 bits, is outside the band although its gap is 0."""
    N, C, h, w = logits.shape
    if C == 1:
        return np.zeros(arg.shape, dtype=bool)
    rest = p.copy()
    np.put_along_axis(rest, arg[:, None], -np.inf, axis=1)
    second = np.argmax(rest, axis=1)
    i0, i1, ly0, ly1 = taps(h, hw_out[0], align_corners)
    j0, j1, lx0, lx1 = taps(w, hw_out[1], align_corners)
    n = np.arange(N)[:, None, None]
    same = np.ones(arg.shape, dtype=bool)
    for i, ly in ((i0, ly0), (i1, ly1)):
        for j, lx in ((j0, lx0), (j1, lx1)):
            a = logits[n, arg, i[None, :, None], j[None, None, :]]
            b = logits[n, second, i[None, :, None], j[None, None, :]]
            unused = (ly[None, :, None] == 0) | (lx[None, None, :] == 0)
            same &= np.isfinite(a) & np.isfinite(b) & ((a == b) | unused)
    return same


def reference(logits, labels, align_corners=False, ignore_index=255, class_weight=None, scale=1.0, out_dtype='float32', K=0):
    """logits (N, C, h, w): the values the kernel reads, upcast (fp32 / fp64 array); labels (N, H, W) int64.  ``K``: the
    forward's longest addition chain.  -> dict of the quantities and their budgets (``b_`` + name), fp64:
    lse, loss (per pixel), loss_sum, n_valid, n_correct_lo / n_correct_hi / band (fraction of the pixels), argmax and gap (per pixel), dlogits."""
    logits = np.asarray(logits, dtype=np.float64)
    labels = np.asarray(labels)
    N, C, h, w = logits.shape
    H, W = labels.shape[1:]
    cw = np.ones(C) if class_weight is None else np.asarray(class_weight, dtype=np.float64)
    v, A = resize(logits, (H, W), align_corners)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        bad = np.any(np.isnan(v) | (v == np.inf), axis=1) | np.all(v == -np.inf, axis=1)
        m = np.max(np.where(np.isfinite(v), v, -np.inf), axis=1)
        m = np.where(np.isfinite(m), m, 0.0)
        lse = np.where(bad, np.nan, m + np.log(np.sum(np.exp(np.where(np.isfinite(v), v, -np.inf) - m[:, None]), axis=1)))
        valid = (labels != ignore_index) & (labels >= 0) & (labels < C)
        y = np.where(valid, labels, 0)
        wy = np.where(valid, cw[y], 0.0)
        vy = np.take_along_axis(v, y[:, None], axis=1)[:, 0]
        loss = np.where(valid, wy * (lse - vy), 0.0)
        d = 16 * U * np.max(np.where(np.isfinite(A), A, 0.0), axis=1)
        b_lse = d + (C + 16) * U + U * np.abs(lse)
        b_loss = np.where(valid, wy * (2 * d + (C + 16) * U + U * (np.abs(lse) + np.abs(vy))) + U * np.abs(loss), 0.0)
        fin = np.isfinite(loss)
        loss_sum = loss.sum()
        b_loss_sum = b_loss[fin].sum() + K * U * np.abs(loss[fin]).sum()

        p = softmax(v)
        arg, gap = argmax_gap(p)
        out = (gap >= BAND) | _same_taps(logits, p, arg, (H, W), align_corners)     # False for a NaN gap
        n_lo = int((valid & out & (arg == labels)).sum())
        n_band = int((valid & ~out).sum())

        p = np.exp(v - lse[:, None])
        onehot = (np.arange(C)[None, :, None, None] == y[:, None]) & valid[:, None]
        g = scale * wy[:, None] * (p - onehot)
        nan_ignored = ~valid & ~np.isfinite(lse)
        g = np.where(nan_ignored[:, None], np.nan, g)   # a finite ignored pixel: wy = 0
        vmax = np.max(v, axis=1, keepdims=True)
        b_p = p * (2 * d[:, None] + (np.abs(v - vmax) + C + 16) * U + (np.abs(lse)[:, None] + np.log(C) + 2) * U)
        b_p = np.where(p == 0, 0.0, b_p)                # a -inf logit: exactly 0 is required (0 * inf above)
        b_g = abs(scale) * wy[:, None] * (b_p + U * (p + 1))
    (my, ny), (mx, nx) = axis_matrix(h, H, align_corners), axis_matrix(w, W, align_corners)
    Kp = int(ny.sum(0).max()) * int(nx.sum(0).max()) + 6
    gnan = ~np.isfinite(g)
    g0 = np.where(gnan, 0.0, g)
    dlogits = _adjoint(my, mx, g0)
    b_dlogits = (_adjoint(my, mx, np.where(gnan, 0.0, b_g)) + Kp * U * _adjoint(my, mx, np.abs(g0))
                 + E_OUT[out_dtype] * np.abs(dlogits) + (2.0 ** -25 if out_dtype == 'float16' else 0.0))
    named_nan = _adjoint(ny.astype(np.float64), nx.astype(np.float64), gnan.astype(np.float64)) > 0
    dlogits = np.where(named_nan, np.nan, dlogits)
    return dict(v=v, lse=lse, b_lse=b_lse, loss=loss, b_loss=b_loss, loss_sum=loss_sum, b_loss_sum=b_loss_sum,
                n_valid=int(valid.sum()), n_correct_lo=n_lo, n_correct_hi=n_lo + n_band, band=n_band / labels.size,
                dlogits=dlogits, b_dlogits=b_dlogits, Kp=Kp, argmax=arg, gap=gap)


def ratio(name, got, want, budget):
    """Worst |got - want| / budget over the finite elements of ``want``; AssertionError if it exceeds 1 or if the two differ
    in where they are NaN, +inf or -inf.  This is the comparison every GPU test goes through."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    budget = np.broadcast_to(np.asarray(budget, dtype=np.float64), want.shape)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s: NaN in different places (%d vs %d)' % (
        name, int(np.isnan(got).sum()), int(np.isnan(want).sum()))
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), '%s: inf in different places' % name
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    err, b = np.abs(got[fin] - want[fin]), budget[fin]
    assert np.all(np.isfinite(b)), name
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0, 0.0, err / b)
    worst = float(r.max())
    assert worst <= 1.0, '%s: error / budget %.3g (error %.3g)' % (name, worst, float(err[np.argmax(r)]))
    return worst


def compare(got, ref, informative=True):
    """got: dict(lse, loss_sum, n_valid, n_correct, dlogits) of the code under test; ref: reference(...).  -> the worst
    error / budget per quantity."""
    out = {k: ratio(k, got[k], ref[k], ref['b_' + k]) for k in ('lse', 'loss_sum', 'dlogits') if k in got}
    assert int(got['n_valid']) == ref['n_valid'], (int(got['n_valid']), ref['n_valid'])
    if informative:
        assert ref['band'] <= MAX_BAND, 'uninformative case: %.3g of the pixels inside the band' % ref['band']
    assert ref['n_correct_lo'] <= int(got['n_correct']) <= ref['n_correct_hi'], (ref['n_correct_lo'], int(got['n_correct']),
                                                                                 ref['n_correct_hi'])
    return out
