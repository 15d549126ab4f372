"""Restatement of the bilinear resize on channels-last rows and of its adjoint (include/vitadapter_hip_resize.h), for the
tests: the taps in fp32 exactly as the header states them (NumPy float32 operations round one by one, as the kernels'
un-contracted ones do), the blend and the adjoint's sums in fp64.  Not a conftest and not a test module.

Besides the result each function returns A, per element the sum of |weight| * |value| over the terms added into it -
the scale of the rounding error of any fp32 evaluation - and the adjoint returns n, the number of those terms."""
import numpy as np

SHAPES = [((16, 24), (32, 48)), ((16, 24), (33, 49)), ((1, 1), (5, 7)), ((3, 5), (3, 5)), ((7, 5), (4, 3)), ((9, 9), (2, 2)),
          ((6, 6), (1, 1)), ((2, 3), (64, 7))]


def taps(n_in, n_out, align_corners):
    """-> i0, i1 (int64), l0, l1 (float32) per output position of one axis"""
    f = np.float32
    dst = np.arange(n_out, dtype=np.float32)
    if align_corners:
        scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
        src = scale * dst
    else:
        scale = f(n_in) / f(n_out)
        src = np.maximum(scale * (dst + f(0.5)) - f(0.5), f(0))
    assert src.dtype == np.float32
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.minimum(np.maximum(src - i0.astype(np.float32), f(0)), f(1))
    l0 = f(1) - l1
    assert l0.dtype == l1.dtype == np.float32
    return i0, i1, l0, l1


def axis_matrix(n_in, n_out, align_corners):
    """(n_out, n_in) fp64: row o holds the weights with which output position o reads the input positions; and the
    same shape in bool: which input positions it names (a named position may carry weight 0)"""
    i0, i1, l0, l1 = taps(n_in, n_out, align_corners)
    m = np.zeros((n_out, n_in), dtype=np.float64)
    named = np.zeros((n_out, n_in), dtype=bool)
    o = np.arange(n_out)
    np.add.at(m, (o, i0), l0.astype(np.float64))
    np.add.at(m, (o, i1), l1.astype(np.float64))
    named[o, i0] = True
    named[o, i1] = True
    return m, named


def _apply(my, mx, v):
    """my (P, H), mx (Q, W), v (N, H, W, C) -> (N, P, Q, C): the two axes one after the other, in fp64"""
    t = np.tensordot(my, v, axes=([1], [1]))            # (P, N, W, C)
    t = np.tensordot(mx, t, axes=([1], [2]))            # (Q, P, N, C)
    return t.transpose(2, 1, 0, 3)


def forward(x, hw_in, hw_out, align_corners):
    """x (N, Hi * Wi, C) array -> y (N, Ho * Wo, C) fp64, A (same shape) = sum |w| |v|"""
    (Hi, Wi), (Ho, Wo) = hw_in, hw_out
    N, T, C = x.shape
    assert T == Hi * Wi
    my, _ = axis_matrix(Hi, Ho, align_corners)
    mx, _ = axis_matrix(Wi, Wo, align_corners)
    v = np.asarray(x, dtype=np.float64).reshape(N, Hi, Wi, C)
    return _apply(my, mx, v).reshape(N, Ho * Wo, C), _apply(my, mx, np.abs(v)).reshape(N, Ho * Wo, C)


def adjoint(dy, hw_in, hw_out, align_corners):
    """dy (N, Ho * Wo, C) array -> dx (N, Hi * Wi, C) fp64, A = sum |w| |dy|, n (Hi * Wi,) = terms per input pixel"""
    (Hi, Wi), (Ho, Wo) = hw_in, hw_out
    N, T, C = dy.shape
    assert T == Ho * Wo
    my, ny = axis_matrix(Hi, Ho, align_corners)
    mx, nx = axis_matrix(Wi, Wo, align_corners)
    g = np.asarray(dy, dtype=np.float64).reshape(N, Ho, Wo, C)
    n = np.outer(ny.sum(0), nx.sum(0)).reshape(Hi * Wi)
    return _apply(my.T, mx.T, g).reshape(N, Hi * Wi, C), _apply(my.T, mx.T, np.abs(g)).reshape(N, Hi * Wi, C), n


def rounding_unit(ref, dtype_name):
    """the spacing of ``dtype_name`` ('bf16' / 'fp16'; 'fp32' -> 0) numbers at |ref|, elementwise (fp64)"""
    if dtype_name == 'fp32':
        return np.zeros_like(ref)
    bits, emin = (8, -126) if dtype_name == 'bf16' else (11, -14)
    _, e = np.frexp(np.abs(ref))                           # |ref| = m * 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e - 1, emin) - (bits - 1))
