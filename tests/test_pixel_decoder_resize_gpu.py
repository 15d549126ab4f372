"""MSDeformAttnPixelDecoder with the FPN tail's upsample on csrc/resize_rows.hip (fused.resize_bilinear_rows,
ENABLED['bilinear_rows']), on the golden of tests/test_pixel_decoder_module.py (tests/golden/pixel_decoder.npz; model and
input construction restated here).

  * the kernels run: exactly one resize_rows_fwd / resize_rows_bwd launch per step in fp32, bf16 and fp16 autocast;
  * fp32 meets the golden within that file's 2e-4 / 2e-4 / 3e-4;
  * under either autocast, outputs and gradients with the switch on stay within 2 x the error of the switch-off run
    (torch's fp32 NCHW upsample, then the cast), both against the module's fp32 run;
  * in the ragged 33 x 49 case under bf16 autocast two runs agree bit for bit on the last encoder layer's norms.1 gradients,
    which sit behind the upsample's adjoint and in front of the MSDA tile pass: with torch's adjoint (float atomics) they
    differ from run to run;
  * fused.resize_bilinear_rows on CPU tensors, and on the GPU with the switch off, is F.interpolate on the permuted view."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pixel_decoder.npz')
CASES = ('base', 'odd')


@pytest.fixture(scope='module')
def gold():
    g = np.load(GOLD)
    return g, json.loads(str(g['meta']))


def _grid(g, key):
    return torch.from_numpy(g[key + '_q'].astype(np.float32)) * float(g[key + '_scale'])


def _model(g, meta, dev):
    from vitadapter.pixel_decoder import MSDeformAttnPixelDecoder
    m = MSDeformAttnPixelDecoder(**meta['config'])
    sd = {}
    for k, shape in meta['state_dict'].items():
        v = _grid(g, 'w_' + k)
        sd[k] = 1.0 + v if (v.dim() == 1 and not k.endswith('bias')) else v
        assert list(v.shape) == shape
    m.load_state_dict(sd)
    return m.to(dev)


def _io(g, case, dev):
    feats = [_grid(g, '%s_feat%d' % (case if i == 0 else 'base', i)).to(dev).requires_grad_(True) for i in range(4)]
    gouts = [_grid(g, '%s_gout%d' % (case if j == 0 else 'base', j)).to(dev) for j in range(4)]
    return feats, gouts


def _run(m, feats, gouts, autocast=None):
    m.zero_grad(set_to_none=True)
    for f in feats:
        f.grad = None
    if autocast is None:
        mf, ms = m(feats)
    else:
        with torch.autocast('cuda', dtype=autocast):
            mf, ms = m(feats)
    outs = [mf] + list(ms)
    sum((o.float() * go).sum() for o, go in zip(outs, gouts)).backward()
    return [o.detach().float() for o in outs], [f.grad.detach().float() for f in feats], {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _digest(t):
    a = t.detach().to(torch.float64).flatten().cpu().numpy()
    return np.array([a.sum(), (a * np.cos(np.arange(a.size, dtype=np.float64) * 0.61803398875)).sum()], dtype=np.float64)


def _check_digest(what, t, want, tol):
    got = _digest(t)
    bound = tol * max(1.0, want[3])
    assert np.abs(got - want[:2]).max() <= bound, (what, got, want, bound)
    assert abs(float(t.detach().abs().max()) - want[2]) <= tol * max(1.0, want[2]), (what, float(t.detach().abs().max()), want[2])
    assert abs(float(t.detach().double().abs().sum()) - want[3]) <= bound, (what, float(t.detach().double().abs().sum()), want[3])


def _check_against_golden(g, meta, case, outs, gfeats, gparams, tol_out, tol_g, tol_gp):
    want = [g[case + '_mask_feature']] + [g['base_ms%d' % j] for j in range(3)]
    for j, (o, w) in enumerate(zip(outs, want)):
        assert tuple(o.shape) == w.shape, (j, o.shape, w.shape)
        assert np.abs(o.cpu().numpy() - w).max() <= tol_out, (case, j, np.abs(o.cpu().numpy() - w).max())
    step = meta['step']
    for i, gf in enumerate(gfeats):
        w = g['%s_gfeat%d_sample' % (case, i)]
        got = gf.cpu().flatten()[::step].numpy()
        assert np.abs(got - w).max() <= tol_g * max(1.0, np.abs(w).max()), (case, i, np.abs(got - w).max())
        _check_digest((case, 'gfeat', i), gf, g['%s_gfeat%d_digest' % (case, i)], tol_g)
    for k, gr in gparams.items():
        _check_digest((case, k), gr, g['%s_gp_%s' % (case, k)], tol_gp)
    assert len(gparams) == len(meta['state_dict'])


def _counted(fn):
    """fn() with the resize rows of the launch profile counted -> fn's result, {row: calls}"""
    import _vah
    _vah.prof_enable(True, 'resize_rows')
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        _vah.prof_enable(False)
    return res, {k: r['calls'] for k, r in _vah.prof_report().items()}


def _switch_off():
    from vitadapter import fused

    class _Off:
        def __enter__(self):
            assert fused.ENABLED['bilinear_rows']
            fused.ENABLED['bilinear_rows'] = False

        def __exit__(self, *exc):
            fused.ENABLED['bilinear_rows'] = True
            return False
    return _Off()


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_gpu_fp32_on_the_resize_kernels_matches_golden(gold, case):
    g, meta = gold
    m = _model(g, meta, 'cuda')
    feats, gouts = _io(g, case, 'cuda')
    (outs, gfeats, gparams), calls = _counted(lambda: _run(m, feats, gouts))
    assert calls == {'resize_rows_fwd': 1, 'resize_rows_bwd': 1}, calls
    _check_against_golden(g, meta, case, outs, gfeats, gparams, 2e-4, 2e-4, 3e-4)
    with _switch_off():
        (outs, gfeats, gparams), calls = _counted(lambda: _run(m, feats, gouts))
    assert calls == {}, calls
    _check_against_golden(g, meta, case, outs, gfeats, gparams, 2e-4, 2e-4, 3e-4)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_gpu_autocast_switch_on_against_switch_off(gold, dtype):
    g, meta = gold
    m = _model(g, meta, 'cuda')
    sfx = '_f16' if dtype == torch.float16 else ''
    for case in CASES:
        feats, gouts = _io(g, case, 'cuda')
        outs32, gf32, gp32 = _run(m, feats, gouts)
        sides = {}
        for side in ('on', 'off'):
            if side == 'on':
                (outs, gf, gp), calls = _counted(lambda: _run(m, feats, gouts, autocast=dtype))
                assert calls == {'resize_rows_fwd' + sfx: 1, 'resize_rows_bwd' + sfx: 1}, calls
            else:
                with _switch_off():
                    (outs, gf, gp), calls = _counted(lambda: _run(m, feats, gouts, autocast=dtype))
                assert calls == {}, calls
            assert all(bool(torch.isfinite(o).all()) for o in outs)
            rel_p = sorted(_rel(gp[k], gp32[k]) for k in gp32 if float(gp32[k].norm()) > 0)
            sides[side] = dict(out=max(_rel(o, w) for o, w in zip(outs, outs32)), gfeat=max(_rel(a, b) for a, b in zip(gf, gf32)),
                               gp_median=rel_p[len(rel_p) // 2], gp_worst=rel_p[-1])
        print('pixel decoder %s autocast, case %s, bilinear_rows: %s' % (dtype, case, sides))
        for q, v in sides['on'].items():
            assert v <= 2.0 * sides['off'][q], (case, q, v, sides['off'][q])


@pytest.mark.gpu
def test_gpu_gradients_behind_the_upsample_adjoint_keep_their_bits(gold):
    g, meta = gold
    m = _model(g, meta, 'cuda')
    feats, gouts = _io(g, 'odd', 'cuda')
    names = [k for k, _ in m.named_parameters() if re.fullmatch(r'encoder\.layers\.\d+\.norms\.1\.(weight|bias)', k)]
    last = max(int(k.split('.')[2]) for k in names)
    keys = ['encoder.layers.%d.norms.1.%s' % (last, s) for s in ('weight', 'bias')]
    assert set(keys) <= set(names)
    _run(m, feats, gouts, autocast=torch.bfloat16)                  # the first run chooses GEMM algorithms
    runs = [_run(m, feats, gouts, autocast=torch.bfloat16)[2] for _ in range(3)]
    for k in keys:
        assert float(runs[0][k].abs().max()) > 0
        for other in runs[1:]:
            assert torch.equal(runs[0][k], other[k]), k


def _interp_rows(x, hw_in, hw_out, align):
    n, _, c = x.shape
    y = F.interpolate(x.permute(0, 2, 1).reshape(n, c, *hw_in), size=hw_out, mode='bilinear', align_corners=align)
    return y.permute(0, 2, 3, 1).reshape(n, hw_out[0] * hw_out[1], c)


@pytest.mark.parametrize('align', [False, True])
def test_api_on_cpu_tensors_is_interpolate(align):
    from vitadapter import fused
    hw_in, hw_out = (5, 7), (9, 10)
    x = torch.randn(2, 35, 16, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    y = fused.resize_bilinear_rows(x, hw_in, hw_out, align_corners=align)
    want = _interp_rows(x, hw_in, hw_out, align)
    assert y.shape == (2, 90, 16) and y.dtype == torch.float32 and y.is_contiguous() and torch.equal(y, want)
    gy = torch.randn(2, 90, 16, generator=torch.Generator().manual_seed(1))
    (gx,) = torch.autograd.grad(y, x, gy)
    (gw,) = torch.autograd.grad(want, x, gy)
    assert torch.equal(gx, gw)
    y16 = fused.resize_bilinear_rows(x.detach(), hw_in, hw_out, align_corners=align, out_dtype=torch.bfloat16)
    assert y16.dtype == torch.bfloat16 and torch.equal(y16, want.detach().to(torch.bfloat16))


@pytest.mark.gpu
def test_api_on_the_gpu():
    from vitadapter import fused
    hw_in, hw_out = (5, 7), (9, 10)
    buf = torch.randn(35 + 11, 2, 16, device='cuda', generator=torch.Generator('cuda').manual_seed(0))
    x = buf[11:].permute(1, 0, 2).requires_grad_(True)              # a level's rows of an (Lq, N, C) buffer, in place
    want = _interp_rows(x, hw_in, hw_out, False)
    with _switch_off():
        y, calls = _counted(lambda: fused.resize_bilinear_rows(x, hw_in, hw_out))
        assert calls == {} and torch.equal(y, want) and y.is_contiguous()
        y16 = fused.resize_bilinear_rows(x, hw_in, hw_out, out_dtype=torch.float16)
        assert y16.dtype == torch.float16 and torch.equal(y16, want.to(torch.float16))
    y, calls = _counted(lambda: fused.resize_bilinear_rows(x, hw_in, hw_out))
    assert calls == {'resize_rows_fwd': 1} and y.is_contiguous() and y.dtype == torch.float32
    assert float((y - want).detach().abs().max()) <= 1e-5
    gy = torch.randn_like(y)
    (gx,), calls = _counted(lambda: torch.autograd.grad(y, x, gy))
    (gw,) = torch.autograd.grad(want, x, gy)
    assert calls == {'resize_rows_bwd': 1} and gx.dtype == x.dtype and float((gx - gw).abs().max()) <= 1e-5
    # C not a multiple of 8, and a change from one 16-bit type to the other: torch's expression, not an error
    x12 = torch.randn(1, 35, 12, device='cuda')
    y12, calls = _counted(lambda: fused.resize_bilinear_rows(x12, hw_in, hw_out))
    assert calls == {} and torch.equal(y12, _interp_rows(x12, hw_in, hw_out, False))
    xb = torch.randn(1, 35, 16, device='cuda').bfloat16()
    yb, calls = _counted(lambda: fused.resize_bilinear_rows(xb, hw_in, hw_out, out_dtype=torch.float16))
    assert calls == {} and yb.dtype == torch.float16
    yb, calls = _counted(lambda: fused.resize_bilinear_rows(xb, hw_in, hw_out))
    assert calls == {'resize_rows_fwd': 1} and yb.dtype == torch.bfloat16
