#!/usr/bin/env python
"""Micro-benchmark of the fused MSDA core (forward; backward through the tile pass and, for A/B, through
per-sample atomics) at the BASELINE call shapes, bf16 IO as under autocast.  HIP-event timed.

    bench_msda_fused.py [cfg ...]                 the core with the grid the batch shares (default: cfg3_inj cfg3_ext)
    bench_msda_fused.py --per-image [cfg ...]     the same calls with a shared grid AND with one grid per image
                                                  (reference points (N, Lq, L, 2): the grid times valid ratios)
    bench_msda_fused.py --encoder [--batch 2]     the pixel decoder's 6-layer deformable encoder, forward + backward under
                                                  bf16 autocast, at the shapes of the reference's 640 x 640 Mask2Former
                                                  configs (levels 20^2, 40^2, 80^2, 256 channels, 8 heads; samples_per_gpu=2:
                                                  mask2former_beit_adapter_large_640_160k_ade20k_ss.py:146) with a grid per image

`pixdec640` names that encoder's MSDA call (N = 2, 8 heads, Lq = S = 8400) for the first two forms."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'vit-adapter_amd'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)
import torch  # noqa: E402

from bench_msda import timeit  # noqa: E402
from oracle import cases  # noqa: E402

PIXDEC640 = [(20, 20), (40, 40), (80, 80)]          # low to high resolution, as the pixel decoder orders them


def _bench_inputs(cfg):
    if cfg == 'pixdec640':
        return 2, 8, 32, 4, sum(h * w for h, w in PIXDEC640), PIXDEC640, PIXDEC640
    return cases.bench_inputs(cfg)


def _valid_ratios(N, L, device):
    """(N, 1, L, 2): image 0 fills its maps, the others are padded on the right and at the bottom."""
    r = torch.ones(N, 1, L, 2, device=device)
    for n in range(1, N):
        r[n, 0, :, 0], r[n, 0, :, 1] = 1.0 - 0.25 * n / N, 1.0 - 0.4 * n / N
    return r


def core(cfgs, per_image):
    from ops.functions import MSDeformAttnFusedFunction
    dt = torch.bfloat16
    for cfg in cfgs:
        N, M, D, P, Lq, shapes, qshapes = _bench_inputs(cfg)
        L, S = len(shapes), sum(h * w for h, w in shapes)
        g = torch.Generator(device='cuda').manual_seed(0)
        value = torch.randn(N, S, M, D, device='cuda', generator=g).to(dt).requires_grad_(True)
        off = (cases.ring_offsets(M, L, P).cuda()[None, None] + float(os.environ.get("VAH_BENCH_NOISE", "1")) * torch.randn(N, Lq, M, L, P, 2, device="cuda", generator=g)).to(dt).requires_grad_(True)
        logit = torch.randn(N, Lq, M, L * P, device='cuda', generator=g).to(dt).requires_grad_(True)
        shared = cases.reference_grid(qshapes).cuda()
        grids = [('', shared)]
        if per_image:
            # L == 1: both through the 8-lane forward (the window forward takes a shared grid only)
            os.environ['VAH_MSDA_FWD_WIN'] = '0'
            grids = [(' grid=shared   ', shared),
                     (' grid=per-image', (shared.expand(N, Lq, -1, 2) * _valid_ratios(N, shared.shape[2], 'cuda')).contiguous())]
        hw = torch.as_tensor(shapes, dtype=torch.long, device='cuda')
        lsi = cases.level_start_index(shapes).cuda()
        gout = torch.randn(N, Lq, M * D, device='cuda', generator=g).to(dt)
        mb_f = 2 * (N * S * M * D + N * Lq * M * D) + 2 * 3 * N * Lq * M * L * P          # bytes moved with bf16 IO
        mb_b = 2 * (2 * N * S * M * D + N * Lq * M * D) + 2 * 6 * N * Lq * M * L * P
        for tiled in ('1', '0'):
            os.environ['VAH_MSDA_TILED'] = tiled
            for tag, ref in grids:
                out = MSDeformAttnFusedFunction.apply(value, hw, lsi, off, logit, ref)
                tf = timeit(lambda: MSDeformAttnFusedFunction.apply(value, hw, lsi, off, logit, ref))

                def bwd():
                    torch.autograd.grad(out, [value, off, logit], gout, retain_graph=True)
                tb = timeit(bwd)
                print('%-9s tiled=%s%s fwd %7.1f us (%.3f of 8 TB/s on moved bytes) | bwd %8.1f us (%.3f)'
                      % (cfg, tiled, tag, tf * 1e6, mb_f / tf / 8e12, tb * 1e6, mb_b / tb / 8e12), flush=True)


def encoder(batch, iters):
    """One line: median HIP-event time of forward + backward of the 6-layer encoder under bf16 autocast - the eager step
    and the replay of one step captured into a HIP graph - and the msda_* rows of one profiled step (which kernels ran)."""
    import _vah
    from vitadapter.pixel_decoder import MSDeformAttnEncoder, encoder_inputs
    torch.manual_seed(0)
    m = MSDeformAttnEncoder().cuda()
    with torch.no_grad():                       # away from the all-zero initial offsets / weights
        for layer in m.layers:
            layer.attentions[0].sampling_offsets.weight.normal_(0, 0.02)
            layer.attentions[0].attention_weights.weight.normal_(0, 0.1)
    query, pos, ref, ss, lsi = encoder_inputs(PIXDEC640, batch, 256, 'cuda', seed=0)
    ref = (ref * _valid_ratios(batch, len(PIXDEC640), 'cuda')).contiguous()
    query.requires_grad_(True)
    gout = torch.randn_like(query)

    def step():
        m.zero_grad(set_to_none=True)
        query.grad = None
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = m(query=query, query_pos=pos, spatial_shapes=ss, reference_points=ref, level_start_index=lsi)
        out.float().backward(gout)
    t = timeit(step, iters=iters, warm=5)
    # the eager step is bound by the host's enqueue at these sizes (batch 1 and batch 2 take the same time): the device's
    # share is what one captured step takes to replay
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=True)
    query.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    tg = timeit(graph.replay, iters=iters, warm=5)
    del graph
    _vah.prof_enable(True, 'msda_')
    try:
        step()
        torch.cuda.synchronize()
    finally:
        _vah.prof_enable(False)
    rows = ' '.join('%s x%d %.1f us/call' % (k, r['calls'], 1e3 * r['total_ms'] / r['calls']) for k, r in sorted(_vah.prof_report().items()))
    print('encoder640 batch=%d ref=%s fwd+bwd bf16 eager %7.3f ms, captured step replayed %7.3f ms | %s'
          % (batch, tuple(ref.shape), t * 1e3, tg * 1e3, rows), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('cfgs', nargs='*')
    ap.add_argument('--per-image', action='store_true')
    ap.add_argument('--encoder', action='store_true')
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    if a.encoder:
        encoder(a.batch, a.iters)
    else:
        core(a.cfgs or ['cfg3_inj', 'cfg3_ext'], a.per_image)


if __name__ == '__main__':
    main()
