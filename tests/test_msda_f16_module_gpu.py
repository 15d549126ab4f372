"""GPU: MSDeformAttn under fp16 autocast on the fp16 instantiation of the fused MSDA kernels, against the same module with
ENABLED['fp16_msda'] off - the reference's op sequence: fp16 softmax / location arithmetic, three casts to fp32, the
unfused fp32 kernels - which rounds where the reference rounds.

MSDeformAttn(d_model=192, n_levels=L, n_heads=6), L = 1 (window forward for a shared grid) and L = 3, N = 2, a grid shared
by the batch and one grid per image; 185 / 143 queries (no multiple of a wave).

The maps are powers of two on purpose.  The reference sequence rounds offsets / (W, H) to fp16 before it adds the fp32
reference point; the fused kernels divide in fp32.  For a power-of-two map that quotient is exact in fp16 and both paths
sample at the same locations; for any other size they are up to 2^-11 |offset| px apart, a few samples fall on the other
side of an integer pixel coordinate - where d(out)/d(location) jumps - and parameter gradients, which cannot be masked
sample by sample, would compare two different derivatives there.  Ragged maps are held to fp64, with the mask, by
tests/test_msda_f16_fp64_gpu.py.

Bounds: outputs within 2 fp16 ulps of max|out|; parameter and input gradients within relative L2 1e-2.  The disabled
path against itself with float atomics (VAH_MSDA_TILED=0) spreads by at most 2.8e-5 on these inputs (DESIGN.md section
4.2b); 4x that is below 1e-2, so 1e-2 stands."""
import math

import pytest
import torch

from oracle import cases

pytestmark = pytest.mark.gpu

GEOM = {1: dict(levels=[(16, 16)], qgrids=[(13, 11), (7, 6)]),
        3: dict(levels=[(32, 32), (16, 16), (8, 8)], qgrids=[(13, 11)])}
N, C, M = 2, 192, 6


def _module(L):
    from ops.modules import MSDeformAttn
    torch.manual_seed(L)
    mod = MSDeformAttn(d_model=C, n_levels=L, n_heads=M)
    with torch.no_grad():           # the initial offsets / weights matrices are zero: give every query its own samples
        mod.sampling_offsets.weight.normal_(0., 0.02)
        mod.attention_weights.weight.normal_(0., 0.05)
        mod.attention_weights.bias.normal_(0., 0.5)
    return mod.cuda().train()


def _inputs(L, per_image):
    g = GEOM[L]
    S = sum(h * w for h, w in g['levels'])
    ref = cases.reference_grid(g['qgrids'])[0]                   # (Lq, 1, 2)
    Lq = ref.shape[0]
    ref = ref[None].repeat(1, 1, L, 1)                           # (1, Lq, L, 2)
    if per_image:                                                # the pixel decoder's grid times valid ratios
        ratios = torch.tensor([[1.0, 1.0], [0.875, 0.75]])
        ref = ref * ratios[:, None, None, :]
    gen = torch.Generator().manual_seed(17 + L)
    q = torch.randn(N, Lq, C, generator=gen)
    x = torch.randn(N, S, C, generator=gen)
    gout = torch.randn(N, Lq, C, generator=gen)
    shapes = torch.tensor(g['levels'], dtype=torch.long)
    lsi = cases.level_start_index(g['levels'])
    return [t.cuda() for t in (q, ref.contiguous(), x, shapes, lsi, gout)]


def _run(mod, q, ref, x, shapes, lsi, gout, fused_on, profile=False):
    """One forward + backward under fp16 autocast -> (out fp32, {name: gradient fp64}, profiler rows)."""
    import _vah
    from vitadapter import fused
    q, x = q.clone().requires_grad_(True), x.clone().requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    was = fused.ENABLED['fp16_msda']
    fused.ENABLED['fp16_msda'] = fused_on
    rows = {}
    try:
        if profile:
            _vah.prof_enable(True, 'msda_')
        with torch.autocast('cuda', dtype=torch.float16):
            out = mod(q, ref, x, shapes, lsi)
        assert out.dtype == torch.float16
        (out.float() * gout).sum().backward()
        torch.cuda.synchronize()
        if profile:
            _vah.prof_enable(False)
            rows = _vah.prof_report()
    finally:
        _vah.prof_enable(False)
        fused.ENABLED['fp16_msda'] = was
    grads = {k: p.grad.detach().double().clone() for k, p in mod.named_parameters()}
    grads['query'], grads['input_flatten'] = q.grad.double(), x.grad.double()
    return out.detach().float(), grads, rows


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize('per_image', [False, True], ids=['shared_grid', 'grid_per_image'])
@pytest.mark.parametrize('L', [1, 3])
def test_module_fp16_autocast(L, per_image):
    mod = _module(L)
    args = _inputs(L, per_image)
    out, grads, rows = _run(mod, *args, fused_on=True, profile=True)
    want, gwant, rows_off = _run(mod, *args, fused_on=False, profile=True)

    assert rows.get('msda_fused_fwd_f16', {}).get('calls', 0) == 1, sorted(rows)
    assert rows.get('msda_fused_bwd_f16', {}).get('calls', 0) == 1, sorted(rows)
    assert 'msda_fwd_f32' not in rows and 'msda_bwd_f32' not in rows, sorted(rows)
    assert not any(r.endswith('_bf16') for r in rows), sorted(rows)
    # the switch gives the reference's sequence back
    assert 'msda_fwd_f32' in rows_off and 'msda_bwd_f32' in rows_off and 'msda_fused_fwd_f16' not in rows_off, sorted(rows_off)

    assert torch.isfinite(out).all()
    top = float(want.abs().max())
    ulp = 2.0 ** (math.floor(math.log2(top)) - 10)
    err = float((out - want).abs().max())
    print('FIGURE L=%d %s out: max err %.3e = %.2f fp16 ulps of max|out| %.3e' % (L, 'per image' if per_image else 'shared', err, err / ulp, top))
    figs = {k: rel_l2(grads[k], gwant[k]) for k in gwant}
    for k in sorted(figs):
        print('FIGURE L=%d %s grad %s: relative L2 %.3e' % (L, 'per image' if per_image else 'shared', k, figs[k]))
    assert err <= 2 * ulp, (err, ulp)
    assert set(grads) == set(gwant)
    for k, g in grads.items():
        assert torch.isfinite(g).all(), k
    bad = {k: f for k, f in figs.items() if not f <= 1e-2}
    assert not bad, bad
