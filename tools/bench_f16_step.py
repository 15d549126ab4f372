#!/usr/bin/env python
"""fp16-autocast training step of a ViT-Adapter preset (the reference's AMP mode: GradScaler(init_scale=512)), eager:
forward + backward + unscale per step, HIP-event timed.  bench.py has no fp16 mode; this is the A/B tool for the fp16
row kernels, the fp16 SpatialPriorModule kernels, the fp16 output tail, the fp16 deformable attention and the fp16 Linears:

    python tools/bench_f16_step.py                                   # fused fp16 rows (default)
    VAH_FUSED_DISABLE=fp16_rows python tools/bench_f16_step.py       # torch's expressions: the behaviour before them
    VAH_FUSED_DISABLE=fp16_spm python tools/bench_f16_step.py        # the SpatialPriorModule as torch's NCHW module
    VAH_FUSED_DISABLE=fp16_tail python tools/bench_f16_step.py       # the output tail as torch's separate ops
    VAH_FUSED_DISABLE=fp16_msda python tools/bench_f16_step.py       # MSDA as the reference's op sequence on the fp32 kernels
    VAH_FUSED_DISABLE=fp16_linear python tools/bench_f16_step.py     # the Linear layers as torch's fp16 library GEMMs
    python tools/bench_f16_step.py --autocast bfloat16               # the same step under bf16, for the rows side by side

Prints ms per step (median and mean of the timed steps) and, from one more profiled step, the GPU time of every
profiler row of the row-kernel, conv_, spm_, output-tail, msda_ and Linear (gemm_, gelu_bwd, colsum) families (none with the switches off: torch's kernels are not timed by this library).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'vit-adapter_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402

FAMILIES = 'layernorm,residual_layernorm,scale_residual,dwconv_tokens,conv_,spm_,bn_tail,transpose_tokens,pixel_shuffle2,maxpool,msda_,gemm_,gelu_bwd,colsum'


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--preset', default='base_det')
    ap.add_argument('--size', type=int, nargs=2, default=[1024, 1024], metavar=('H', 'W'))
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--autocast', default='float16', choices=['float16', 'bfloat16'])
    args = ap.parse_args()
    import _vah
    from vitadapter import fused
    from vitadapter.backbones.vit_adapter import build_preset
    torch.manual_seed(0)
    model = build_preset(args.preset).cuda().train()
    opt = torch.optim.SGD(model.parameters(), lr=0.)
    dtype = getattr(torch, args.autocast)
    scaler = torch.amp.GradScaler('cuda', init_scale=512., enabled=dtype == torch.float16)
    x = torch.randn(args.batch, 3, *args.size, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1234))

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=dtype):
            feats = model(x)
        scaler.scale(sum(f.float().mean() for f in feats)).backward()
        scaler.unscale_(opt)
        scaler.update()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for e0, e1 in ev:
        e0.record()
        step()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    _vah.prof_enable(True, FAMILIES)
    step()
    torch.cuda.synchronize()
    _vah.prof_enable(False)
    rows = {k: round(r['total_ms'], 4) for k, r in sorted(_vah.prof_report().items())}
    finite = all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    print(json.dumps({'preset': args.preset, 'size': args.size, 'batch': args.batch, 'autocast': args.autocast,
                      'fp16_rows': fused.ENABLED['fp16_rows'], 'fp16_spm': fused.ENABLED['fp16_spm'], 'fp16_tail': fused.ENABLED['fp16_tail'],
                      'fp16_msda': fused.ENABLED['fp16_msda'], 'fp16_linear': fused.ENABLED['fp16_linear'],
                      'ms_per_step_median': round(ms[len(ms) // 2], 3), 'ms_per_step_mean': round(sum(ms) / len(ms), 3),
                      'ms_min': round(ms[0], 3), 'ms_max': round(ms[-1], 3), 'steps': args.steps, 'grads_finite': finite,
                      'row_ms_one_step': rows, 'row_ms_total': round(sum(rows.values()), 3)}))


if __name__ == '__main__':
    main()
