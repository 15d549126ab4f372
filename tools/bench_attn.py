#!/usr/bin/env python
"""Micro-benchmark of the global attention kernels at the base_det shape (2 x 4096 tokens, 12 heads of 64)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'vit-adapter_amd'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)
import torch  # noqa: E402

import _vah  # noqa: E402
from bench_msda import timeit  # noqa: E402
from vitadapter import kernels  # noqa: E402

DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('dims', nargs='*', type=int, help='B N heads (default 2 4096 12)')
    ap.add_argument('--dtype', choices=('bf16', 'f16'), default='bf16', help='element type of q, k, v (default bf16)')
    args = ap.parse_args()
    B, N, H = args.dims[:3] if args.dims else (2, 4096, 12)
    dt = DTYPES[args.dtype]
    qkv = torch.randn(B, N, 3, H, 64, device='cuda').to(dt).requires_grad_(True)
    g = torch.randn(B, N, H, 64, device='cuda').to(dt)
    out = kernels.attention(qkv, 0.125)
    _vah.prof_enable(True, 'attn_')
    tf = timeit(lambda: kernels.attention(qkv, 0.125), iters=30)
    tb = timeit(lambda: torch.autograd.grad(out, qkv, g, retain_graph=True), iters=30)
    fl = 4 * B * H * N * N * 64
    print('attention %s %dx%d heads %d: fwd %.1f us (%.3f of 2.5 PF) | bwd %.1f us (%.3f)'
          % (args.dtype, B, N, H, tf * 1e6, fl / tf / 2.5e15, tb * 1e6, 2.5 * fl / tb / 2.5e15))
    for name, row in sorted(_vah.prof_report().items()):
        us = row['total_ms'] / row['calls'] * 1e3
        print('  %-24s %7.1f us  %.3f of MFMA peak' % (name, us, row['flops'] / row['calls'] / (us * 1e-6) / 2.5e15))


if __name__ == '__main__':
    main()
