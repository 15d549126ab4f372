"""Micro-benchmark of the kernels that carry a Linear's bias-gradient partials (csrc/fused_ops.hip, the `_bsum` entry
points) against what they replace: the same backward kernel without the partials PLUS the column-sum launch over the
dY it wrote.  Through the C ABI, HIP-event timed, rotating over enough buffer sets that nothing is served from the
256 MB infinity cache.  Prints us per call; a `_bsum` kernel pays when it is faster than `parent + colsum`.

    python tools/bench_bias_partials.py            (8192 x 768 and 43008 x 768; GELU at 8192 x 3072)
"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'vit-adapter_amd'))
import _vah  # noqa: E402

L = _vah.lib


def timeit(fn, sets, iters=60):
    for s in sets:
        fn(s)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def rows_768(rows, C):
    d, B = 'cuda', 2
    rpb = rows // B
    st = torch.cuda.current_stream().cuda_stream
    nsets = max(2, int(600e6 / (rows * C * 18)) + 1)
    sets = [dict(t=torch.randn(rows, C, device=d), gh=torch.randn(rows, C, device=d).bfloat16(),
                 gt=torch.randn(rows, C, device=d), z=torch.randn(rows, C, device=d).bfloat16(),
                 dt=torch.empty(rows, C, device=d), dz=torch.empty(rows, C, device=d, dtype=torch.bfloat16),
                 mean=torch.zeros(rows, device=d), rstd=torch.ones(rows, device=d)) for _ in range(nsets)]
    w, gamma, sc = torch.ones(C, device=d), torch.ones(C, device=d), torch.tensor([1.0 / 0.7, 1.0 / 0.9], device=d)
    dw, db, dg = (torch.empty(C, device=d) for _ in range(3))
    ws = torch.empty(L.vah_reduce_ws_floats(3 * C), device=d)
    bpart = torch.empty(L.vah_reduce_ws_floats(C), device=d)
    n = ctypes.c_int64(0)
    p = lambda t: t.data_ptr()

    def ln(s, bsum):
        a = (p(s['t']), p(s['gh']), p(w), p(s['mean']), p(s['rstd']), p(s['gt']), p(s['z']), None, p(sc), B, rpb, C,
             p(s['dt']), p(s['dz']), None, p(dw), p(db), p(ws))
        _vah.check(L.vah_residual_layernorm_bwd_bsum(*a, p(bpart), ctypes.byref(n), st) if bsum
                   else L.vah_residual_layernorm_bwd(*a, st), 'ln')

    def sr(s, bsum, with_gamma):
        a = (p(s['gt']), p(s['z']), p(gamma) if with_gamma else None, p(sc), B, rpb, C, p(s['dz']),
             p(dg) if with_gamma else None, p(ws) if with_gamma else None)
        _vah.check(L.vah_scale_residual_bwd_bsum(*a, p(bpart), ctypes.byref(n), st) if bsum
                   else L.vah_scale_residual_bwd(*a, st), 'sr')

    def colsum(s):
        _vah.check(L.vah_colsum_bf16_partials(p(s['dz']), rows, C, p(bpart), ctypes.byref(n), st), 'colsum')

    cs = timeit(colsum, sets)
    print('%6d x %4d  colsum_bf16_partials                 %7.1f us' % (rows, C, cs))
    for name, fn in (('residual_layernorm_bwd (no gamma)', ln),
                     ('scale_residual_bwd (no gamma: scale_only)', lambda s, b: sr(s, b, False)),
                     ('scale_residual_bwd (gamma)', lambda s, b: sr(s, b, True))):
        a, b = timeit(lambda s: fn(s, False), sets), timeit(lambda s: fn(s, True), sets)
        print('%6d x %4d  %-42s parent %7.1f us  _bsum %7.1f us  (%+.1f; the column sum it removes: %.1f)'
              % (rows, C, name, a, b, b - a, cs))


def gelu(rows, C):
    d = 'cuda'
    st = torch.cuda.current_stream().cuda_stream
    nsets = max(2, int(600e6 / (rows * C * 6)) + 1)
    sets = [dict(da=torch.randn(rows, C, device=d).bfloat16(), h=torch.randn(rows, C, device=d).bfloat16(),
                 dh=torch.empty(rows, C, device=d, dtype=torch.bfloat16)) for _ in range(nsets)]
    bpart = torch.empty(L.vah_reduce_ws_floats(C), device=d)
    n = ctypes.c_int64(0)

    def ours(s):
        _vah.check(L.vah_gelu_bwd_bsum_bf16(s['da'].data_ptr(), s['h'].data_ptr(), rows, C, s['dh'].data_ptr(),
                                            bpart.data_ptr(), ctypes.byref(n), st), 'gelu')

    def torchs(s):
        torch.ops.aten.gelu_backward(s['da'], s['h'], approximate='none')

    def colsum(s):
        _vah.check(L.vah_colsum_bf16_partials(s['dh'].data_ptr(), rows, C, bpart.data_ptr(), ctypes.byref(n), st), 'colsum')

    a, c, b = timeit(torchs, sets), timeit(colsum, sets), timeit(ours, sets)
    print('%6d x %4d  gelu backward: torch %7.1f us + colsum %7.1f us  ->  gelu_bwd_bsum %7.1f us (%.2f TB/s on 6 B/element)'
          % (rows, C, a, c, b, rows * C * 6 / b / 1e6))


if __name__ == '__main__':
    for shape in ((8192, 768), (43008, 768)):
        rows_768(*shape)
    gelu(8192, 3072)
