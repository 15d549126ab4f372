"""CPU: the restatement the resize kernels are held to (tests/resize_rows_ref.py) against torch's own operator.

Forward against F.interpolate(mode='bilinear', size=...) on CPU fp32 tensors, adjoint against autograd through it, every
shape of the GPU test and both align_corners values.  Bound per element, with A = sum |w| |v| of its terms:
    2 * 2^-23 * max(Hi, Wi) * A  +  16 * 2^-24 * A
The first term is one ulp of `src` on each axis for a library that may contract src's operations differently (src < max(Hi,
Wi), so an ulp of it is at most 2^-23 * max(Hi, Wi), and a fraction moved by d moves the blend by at most d * A per axis);
the second is the fp32 blend's rounding.  And the restated adjoint is the exact transpose of the restated forward."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_rows_ref as ref  # noqa: E402

N, C = 2, 8


def bound(a, hw_in):
    return (2.0 * 2.0 ** -23 * max(hw_in) + 16 * 2.0 ** -24) * a


def _maps(rows, hw):
    n, _, c = rows.shape
    return rows.reshape(n, hw[0], hw[1], c).permute(0, 3, 1, 2)


def _rows(maps):
    n, c, h, w = maps.shape
    return maps.permute(0, 2, 3, 1).reshape(n, h * w, c)


@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('hw_in,hw_out', ref.SHAPES)
def test_restatement_against_torch(hw_in, hw_out, align):
    gen = torch.Generator().manual_seed(hw_in[0] * 1000 + hw_out[1] * 10 + align)
    x = torch.randn(N, hw_in[0] * hw_in[1], C, generator=gen).requires_grad_(True)
    dy = torch.randn(N, hw_out[0] * hw_out[1], C, generator=gen)
    y = _rows(F.interpolate(_maps(x, hw_in), size=hw_out, mode='bilinear', align_corners=align))
    y.backward(dy)
    want, a = ref.forward(x.detach().numpy(), hw_in, hw_out, align)
    err = np.abs(y.detach().numpy().astype(np.float64) - want)
    assert (err <= bound(a, hw_in)).all(), float((err / np.maximum(bound(a, hw_in), 1e-300)).max())
    want, a, n = ref.adjoint(dy.numpy(), hw_in, hw_out, align)
    err = np.abs(x.grad.numpy().astype(np.float64) - want)
    b = bound(a, hw_in)
    assert (err <= b).all(), float((err / np.maximum(b, 1e-300)).max())
    assert (want[:, n == 0] == 0).all()


@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('hw_in,hw_out', ref.SHAPES)
def test_adjoint_is_the_exact_transpose(hw_in, hw_out, align):
    rng = np.random.default_rng(hw_in[1] * 100 + hw_out[0])
    x = rng.standard_normal((N, hw_in[0] * hw_in[1], C))
    g = rng.standard_normal((N, hw_out[0] * hw_out[1], C))
    y, _ = ref.forward(x, hw_in, hw_out, align)
    dx, _, _ = ref.adjoint(g, hw_in, hw_out, align)
    lhs, rhs = float((y * g).sum()), float((x * dx).sum())
    scale = float((np.abs(y) * np.abs(g)).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)


@pytest.mark.parametrize('align', [False, True])
def test_taps_are_monotone_in_range_and_sum_to_one(align):
    for n_in, n_out in [(16, 32), (16, 33), (1, 5), (3, 3), (7, 4), (9, 2), (6, 1), (2, 64), (100, 200), (168, 336), (5, 1000)]:
        i0, i1, l0, l1 = ref.taps(n_in, n_out, align)
        assert (np.diff(i0) >= 0).all() and (np.diff(i1) >= 0).all()
        assert i0.min() >= 0 and i1.max() <= n_in - 1 and ((i1 == i0) | (i1 == i0 + 1)).all()
        assert (l1 >= 0).all() and (l1 <= 1).all() and np.allclose(l0.astype(np.float64) + l1, 1, atol=2.0 ** -24)
