#!/usr/bin/env python
"""What fused reference boxes buy: forward + backward of ops.modules.MSDeformAttn at one decoder-sized call
(N = 2, Lq = 900 queries, d_model 256 over 8 heads, P = 4, the four levels of an 800 x 1344 image at strides 8 - 64,
one set of boxes per image), under fp32, bf16 autocast and fp16 autocast:

    box fused | box with VAH_MSDA_FUSED=0 | point fused | point with VAH_MSDA_FUSED=0

in one process, alternating, device events around ITERS forward + backward passes per window, ROUNDS windows per
configuration after a warm-up of each.  Prints one line per (tier, configuration): median ms per pass and the spread
(min - max) over the windows, then the ratios.

    python tools/bench_msda_box.py [--iters 100] [--rounds 5] [--lq 900]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'vit-adapter_amd')]

import torch  # noqa: E402

LEVELS = ((100, 168), (50, 84), (25, 42), (13, 21))
N, C, HEADS, P = 2, 256, 8, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--lq', type=int, default=900)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU: there is no CPU path to time'
    import _vah
    from ops.functions import ms_deform_attn_fused as mf
    from ops.modules import MSDeformAttn
    dev = torch.device('cuda')
    S, L, Lq = sum(h * w for h, w in LEVELS), len(LEVELS), args.lq
    ws = mf.tile_ws_bytes(N, S, HEADS, C // HEADS, L, Lq, P)
    print('geometry N=%d Lq=%d S=%d levels=%s heads=%d x %d: vah_msda_tile_ws_bytes = %d' % (N, Lq, S, LEVELS, HEADS, C // HEADS, ws))
    assert ws >= 0, _vah.lib.vah_last_error().decode()

    torch.manual_seed(0)
    m = MSDeformAttn(d_model=C, n_levels=L, n_heads=HEADS, n_points=P).to(dev)
    with torch.no_grad():
        m.sampling_offsets.weight.normal_(0, 0.02)
        m.attention_weights.weight.normal_(0, 0.05)
    g = torch.Generator().manual_seed(1)
    query = torch.randn(N, Lq, C, generator=g).to(dev).requires_grad_(True)
    feat = torch.randn(N, S, C, generator=g).to(dev).requires_grad_(True)
    gout = torch.randn(N, Lq, C, generator=g).to(dev)
    centre = torch.rand(N, Lq, 1, 2, generator=g).expand(N, Lq, L, 2)
    boxes = torch.cat((centre, 0.05 + 0.3 * torch.rand(N, Lq, 1, 2, generator=g).expand(N, Lq, L, 2)), -1).contiguous().to(dev)
    points = centre.contiguous().to(dev)
    ss = torch.tensor(LEVELS, dtype=torch.long, device=dev)
    lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))

    def one(ref, dtype):
        with torch.autocast('cuda', dtype=dtype or torch.bfloat16, enabled=dtype is not None):
            out = m(query, ref, feat, ss, lsi)
        out.float().backward(gout)
        m.zero_grad(set_to_none=True)
        query.grad = feat.grad = None

    def window(ref, dtype, fused, iters):
        os.environ['VAH_MSDA_FUSED'] = fused
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            one(ref, dtype)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    configs = [('box fused', boxes, '1'), ('box unfused', boxes, '0'), ('point fused', points, '1'), ('point unfused', points, '0')]
    for tier, dtype in (('fp32', None), ('bf16', torch.bfloat16), ('fp16', torch.float16)):
        rows = {}
        for name, ref, fused in configs:          # which kernels serve the call, and the warm-up of every shape
            _vah.prof_enable(True, 'msda_')
            window(ref, dtype, fused, 3)
            _vah.prof_enable(False)
            rows[name] = sorted(_vah.prof_report())
            window(ref, dtype, fused, 10)
        times = {name: [] for name, _, _ in configs}
        for _ in range(args.rounds):
            for name, ref, fused in configs:
                times[name].append(window(ref, dtype, fused, args.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        for name, _, _ in configs:
            t = times[name]
            print('%-5s %-14s %8.4f ms per forward + backward (min %.4f max %.4f over %d windows of %d)  rows %s'
                  % (tier, name, med[name], min(t), max(t), len(t), args.iters, ','.join(rows[name])))
        print('%-5s box fused / point fused %.3f   box unfused / box fused %.3f   point unfused / point fused %.3f'
              % (tier, med['box fused'] / med['point fused'], med['box unfused'] / med['box fused'],
                 med['point unfused'] / med['point fused']))
    os.environ.pop('VAH_MSDA_FUSED', None)


if __name__ == '__main__':
    main()
