"""GPU: the fp16 instantiations of the SpatialPriorModule kernels (csrc/conv.hip, csrc/spm_nhwc.hip: the `_f16` entry
points, what fp16 autocast runs) held to fp64 (oracle/spm.py, which upcasts whatever 16-bit operands it is given) - the
fp16 counterpart of tests/test_spm_fp64_gpu.py, whose cases, launch-geometry mirror and discipline it imports: NaN-filled
outputs and workspaces inside guard bands that must come back intact, every call twice with the same bits, and the
spm_nhwc autograd classes returning the direct calls' bits.

Budget.  Operands are fp16, every sum is fp32, each fp16 output is rounded once at its store; dW, the BatchNorm sums,
mean and rstd stay fp32.  Per element

    |got - ref| <= 256 * 2^-24 * A + 2^-11 |ref| + 2^-25      (fp16 outputs; the first term alone for fp32 outputs)

A = the sum of |terms| from oracle/spm.py, composed here from spm.bound(ref, A).  2^-11 is fp16's round-to-nearest
bound (11 significant bits), 2^-25 half the spacing of its subnormals (2^-24): both follow from the format, none from
what the kernels return.  fp16 outputs therefore sit near 1.0 - the rounding bound itself; the "(acc)" rows show the
part beyond half an fp16 ulp of the reference over the accumulation term alone.

Cases: the five distinct conv layers of BASELINE configs[1]-[4] at production size (forward, input gradient, weight
gradient), one walk-boundary case per kernel instantiation (WALK_CASES of the bf16 file, geometry asserted the same
way), the tiny maps, BatchNorm at the production rows x C and the 512-part cap, max-pool values and window index (exact),
the NHWC16 layout (exact, against x.to(float16)).  In addition:
  * loss-scaled gradients: dgrad, wgrad, bn_bwd_stats and bn_bwd_apply with dy drawn at scale 2^-18, where more than
    half (about 99.4 %) of the fp16 dy are subnormal and non-zero - A / B operands of v_mfma_f32_32x32x16_f16 in the two
    convolution gradients - held to the budget above with no extra term: a flushed operand is an error of the size of
    the element itself;
  * the fp32 -> fp16 conversion of the conv_taps and bn_apply stores, bit for bit against torch's .to(float16) of the
    fp32 value (round to nearest even, overflow to inf, subnormals kept), on inputs whose fp32 result is exact and that
    reach the subnormal range, exact ties and overflow;
  * ReLU edge: elements whose pre-activation the oracle marks as `edge` are left out of dx, as in the bf16 file; their
    share must stay below 1e-4 (asserted per case).

Run with -s for one RATIO line per checked output and the worst ratio per family at the end."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import spm
from test_spm_fp64_gpu import (BN_CAP_CASES, BN_CASES, C_FIN, CONFIGS, CONV_CASES, EPS, MOMENTUM, POOL_CASES, TINY_CASES,
                               WALK_CASES, _ck, _equal, _Guarded, _same_bits, _st, _taps_walk, _twice, _vah, _wgrad_walk)

pytestmark = pytest.mark.gpu

F16 = torch.float16
F16_U = 2.0 ** -11            # round to nearest with 11 significant bits
F16_SUB = 2.0 ** -25          # half the spacing of fp16's subnormals
F16_MIN_NORMAL = 2.0 ** -14
SCALED = 2.0 ** -18           # a loss-scaled output gradient: fp16 subnormals

# one walk-boundary case per instantiation: the "just above" ones (a few workgroups walk a second, ragged tile)
F16_WALK_CASES = [c for c in WALK_CASES if c[0].endswith('_above')]

WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for key in sorted(WORST):
        r, case = WORST[key]
        print('WORST f16 %-16s %.3f (%s)' % (key, r, case))


def _record(family, case, r):
    print('RATIO f16 %s %s %.4f' % (family, case, r))
    prev = WORST.get(family)
    if prev is None or r > prev[0]:
        WORST[family] = (r, case)


def _bound16(ref, A):
    return spm.bound(ref, A) + F16_U * ref.to(torch.float64).abs() + F16_SUB


def _worst(num, den):
    if num.numel() == 0:
        return 0.0
    return float(torch.where(num == 0, torch.zeros_like(num), num / den).nan_to_num(float('inf')).max())


def _check16(family, case, what, got, ref, A, mask=None):
    """an fp16 output: every element within its budget; records the worst ratio, and the accumulation part alone: what
    lies beyond half an fp16 ulp of ref (2^-25 in the subnormal range), over 256 * 2^-24 * A"""
    assert got.dtype == F16
    r64 = ref.to(torch.float64)
    err = (got.to(torch.float64) - r64).abs()
    b = _bound16(ref, A)
    e = torch.floor(torch.log2(r64.abs().clamp_min(F16_MIN_NORMAL)))
    ex = (err - torch.exp2(e - 11)).clamp_min(0.)
    acc = spm.bound(ref, A)
    bad = ~(err <= b)
    if mask is not None:
        bad &= mask
        err, b, ex, acc = err[mask], b[mask], ex[mask], acc[mask]
    r = _worst(err, b)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError('%s %s: %d of %d elements over budget; first at flat %d: got %r ref %r budget %.3e (worst err / '
                             'budget %.3g)' % (case, what, int(bad.sum()), bad.numel(), i, got.reshape(-1)[i].item(),
                                               r64.reshape(-1)[i].item(), _bound16(ref, A).reshape(-1)[i].item(), r))
    assert r <= 1.0, (case, what, r)
    _record(family, case, r)
    _record(family + ' (acc)', case, _worst(ex, acc))


def _sym(name):
    return getattr(_vah().lib, _vah().SPM_F16_TWINS[name])


def _subnormal_share(t):
    a = t.float().abs()
    return float(((a > 0) & (a < F16_MIN_NORMAL)).double().mean())


def _image16(x):
    y = torch.zeros((x.shape[0], x.shape[2], x.shape[3], 16), dtype=F16, device=x.device)
    y[..., :3] = x.permute(0, 2, 3, 1).to(F16)
    return y


# ---------------------------------------------------------------- direct calls
def _fwd(x, w9, S, out):
    N, H, W, Cin = x.shape
    OH, OW = out.shape[1:3]
    ty = (ctypes.c_int * 9)(*[t // 3 - 1 for t in range(9)])
    tx = (ctypes.c_int * 9)(*[t % 3 - 1 for t in range(9)])
    _ck(_sym('vah_conv_taps_nhwc_bf16')(x.data_ptr(), N, H, W, Cin, w9.data_ptr(), w9.shape[0], 9, ty, tx, S, out.data_ptr(), OH, OW,
                                       OH, OW, 1, 0, 0, _st()), 'conv_taps_f16')


def _dgrad(gy, wt9, S, gx):
    N, OH, OW, Cout = gy.shape
    _, H, W, Cin = gx.shape
    _ck(_sym('vah_conv3x3_dgrad_nhwc_bf16')(gy.data_ptr(), N, OH, OW, Cout, wt9.data_ptr(), Cin, S, gx.data_ptr(), H, W, _st()),
        'conv_dgrad_f16')


def _wgrad(x, gy, S, ws, dw):
    N, H, W, Cin = x.shape
    _, OH, OW, Cout = gy.shape
    _ck(_sym('vah_conv3x3_wgrad_nhwc_bf16')(x.data_ptr(), N, H, W, Cin, gy.data_ptr(), OH, OW, Cout, S, ws.data_ptr(), ws.numel(),
                                           dw.data_ptr(), _st()), 'conv_wgrad_f16')


def _conv_operands(N, H, W, Cin, Cout, S, wcin, seed, gscale):
    g = torch.Generator(device='cuda').manual_seed(seed)
    if Cin == 16:                                     # the stem reads the fp16 NHWC16 image
        x = _image16(torch.randn(N, 3, H, W, device='cuda', generator=g))
    else:                                             # post-ReLU activations: about half zeros
        x = torch.randn(N, H, W, Cin, device='cuda', generator=g).clamp_min(0).to(F16)
    w32 = torch.randn(Cout, wcin, 3, 3, device='cuda', generator=g) * (9 * wcin) ** -0.5
    OH, OW = (H - 1) // S + 1, (W - 1) // S + 1
    gy = (torch.randn(N, OH, OW, Cout, device='cuda', generator=g) * gscale).to(F16)
    return x, w32, gy


def _run_conv(case, N, H, W, Cin, Cout, S, wcin, kinds, seed, wrapper=False, gscale=1.0):
    from vitadapter import conv
    x, w32, gy = _conv_operands(N, H, W, Cin, Cout, S, wcin, seed, gscale)
    if gscale != 1.0:
        share = _subnormal_share(gy)
        print('SUBNORMAL dy share %s %.4f' % (case, share))
        assert share > 0.5, (case, share)
    wb = F.pad(w32, (0, 0, 0, 0, 0, Cin - wcin)).to(F16)
    w9, wt9 = conv.forward_weight(wb, F16), conv.dgrad_weight(wb, F16)
    assert w9.dtype == wt9.dtype == F16
    OH, OW = gy.shape[1:3]
    sfx = '' if gscale == 1.0 else ' scaled'
    res = {}
    if 'fwd' in kinds:
        out = _Guarded((N, OH, OW, Cout), F16, OW * Cout)
        got, = _twice(lambda: _fwd(x, w9, S, out.t), [out], case + ' forward')
        ref, A = spm.conv_forward(x, w9, S)
        _check16('conv fwd', case, 'forward', got, ref, A)
        res['fwd'] = got
        del ref, A
    if 'dgrad' in kinds and Cin != 16:
        gx = _Guarded((N, H, W, Cin), F16, W * Cin)
        got, = _twice(lambda: _dgrad(gy, wt9, S, gx.t), [gx], case + ' input grad')
        ref, A = spm.conv_input_grad(gy, wt9, S, H, W)
        _check16('conv dgrad' + sfx, case, 'input grad', got, ref, A)
        res['dgrad'] = got
        del ref, A
    if 'wgrad' in kinds:
        ws = _Guarded((_vah().lib.vah_conv3x3_wgrad_ws_floats(Cin, Cout),), torch.float32, 0)
        dw = _Guarded((Cout, 9, Cin), torch.float32, 9 * Cin)
        _, got = _twice(lambda: _wgrad(x, gy, S, ws.t, dw.t), [ws, dw], case + ' weight grad')
        ref, A = spm.conv_weight_grad(x, gy, S)
        _record('conv wgrad' + sfx, case, spm.check(case + ' weight grad', got, ref, A))
        if wcin < Cin:
            assert (got[..., wcin:] == 0).all()
        res['wgrad'] = got
        del ref, A
    if wrapper:
        from vitadapter import spm_nhwc
        xr = x.clone().requires_grad_(Cin != 16)
        wr = w32.clone().requires_grad_(True)
        y = spm_nhwc._Conv3x3.apply(xr, wr, S)
        assert y.dtype == F16
        y.backward(gy)
        torch.cuda.synchronize()
        _same_bits(y.detach(), res['fwd'], case + ' _Conv3x3 forward')
        if Cin != 16:
            assert xr.grad.dtype == F16
            _same_bits(xr.grad, res['dgrad'], case + ' _Conv3x3 input grad')
        else:
            assert xr.grad is None
        assert wr.grad.dtype == torch.float32
        _same_bits(wr.grad, res['wgrad'].view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)[:, :wcin].contiguous(), case + ' _Conv3x3 weight grad')


@pytest.mark.parametrize('cfg,layer,H,W,Cin,Cout,S,wcin', CONV_CASES, ids=['%s_%s' % c[:2] for c in CONV_CASES])
def test_conv_production(cfg, layer, H, W, Cin, Cout, S, wcin):
    N = CONFIGS[cfg][2]
    _run_conv('%s_%s' % (cfg, layer), N, H, W, Cin, Cout, S, wcin, ('fwd', 'dgrad', 'wgrad'), seed=H + W + Cin + Cout, wrapper=True)


def test_walk_cases_cover_every_instantiation():
    assert {c[8] for c in F16_WALK_CASES} == {c[8] for c in WALK_CASES} and len(F16_WALK_CASES) == 9


@pytest.mark.parametrize('case', F16_WALK_CASES, ids=[c[0] for c in F16_WALK_CASES])
def test_conv_walk_boundary(case):
    name, kind, N, H, W, Cin, Cout, S, inst, slots, most, fewest = case
    geo = _wgrad_walk(N, H, W, Cin, Cout, S) if kind == 'wgrad' else _taps_walk(kind, N, H, W, Cin, Cout, S)
    assert geo == (inst, slots, most, fewest), (name, geo)
    _run_conv(name, N, H, W, Cin, Cout, S, 3 if Cin == 16 else Cin, (kind,), seed=len(name) * 7 + N)


@pytest.mark.parametrize('shape', TINY_CASES, ids=['x'.join(map(str, c)) for c in TINY_CASES])
def test_conv_tiny(shape):
    N, H, W, Cin, Cout, S = shape
    _run_conv('tiny_' + 'x'.join(map(str, shape)), N, H, W, Cin, Cout, S, 3 if Cin == 16 else Cin, ('fwd', 'dgrad', 'wgrad'),
              seed=H * 100 + W)


# loss-scaled output gradients (fp16 subnormals as MFMA operands): configs[1] layers of every gradient instantiation
SCALED_CONV_CASES = [c for c in CONV_CASES if c[0] == 'c1']


@pytest.mark.parametrize('cfg,layer,H,W,Cin,Cout,S,wcin', SCALED_CONV_CASES, ids=['%s_%s' % c[:2] for c in SCALED_CONV_CASES])
def test_conv_gradients_of_subnormal_dy(cfg, layer, H, W, Cin, Cout, S, wcin):
    N = CONFIGS[cfg][2]
    _run_conv('%s_%s_scaled' % (cfg, layer), N, H, W, Cin, Cout, S, wcin, ('dgrad', 'wgrad'), seed=H + W + Cin + Cout + 1,
              gscale=SCALED)


# ---------------------------------------------------------------- BatchNorm
def _run_bn(case, rows, C, seed, gscale=1.0):
    lib = _vah().lib
    g = torch.Generator(device='cuda').manual_seed(seed)
    sig = torch.rand(C, device='cuda', generator=g) * 1.5 + 0.5
    off = 3.0 * sig * torch.sign(torch.randn(C, device='cuda', generator=g))          # a mean offset of 3 sigma
    x = (torch.randn(rows, C, device='cuda', generator=g) * sig + off).to(F16)
    dy = (torch.randn(rows, C, device='cuda', generator=g) * gscale).to(F16)
    if gscale != 1.0:
        share = _subnormal_share(dy)
        print('SUBNORMAL dy share %s %.4f' % (case, share))
        assert share > 0.5, (case, share)
    sfx = '' if gscale == 1.0 else ' scaled'
    w = torch.randn(C, device='cuda', generator=g) * 0.3 + 1.0
    b = torch.randn(C, device='cuda', generator=g) * 0.3
    rm0 = torch.randn(C, device='cuda', generator=g) * 0.1
    rv0 = torch.rand(C, device='cuda', generator=g) + 0.5
    nws = lib.vah_bn_nhwc_ws_floats(C)
    ws, sums, sums2 = _Guarded((nws,), torch.float32, 0), _Guarded((2 * C + 1,), torch.float32, 0), _Guarded((2 * C,), torch.float32, 0)
    mean, rstd = _Guarded((C,), torch.float32, 0), _Guarded((C,), torch.float32, 0)
    y, ye, dx = (_Guarded((rows, C), F16, C) for _ in range(3))
    st = _st()
    stats, apply, bwd_stats, bwd_apply = (_sym(n) for n in ('vah_bn_nhwc_stats', 'vah_bn_nhwc_apply', 'vah_bn_nhwc_bwd_stats',
                                                            'vah_bn_nhwc_bwd_apply'))

    def run():
        ws.reset()
        _ck(stats(x.data_ptr(), rows, C, sums.t.data_ptr(), ws.t.data_ptr(), st), 'bn_nhwc_stats_f16')
        sums.t[2 * C:].fill_(float(rows))
        rm, rv = rm0.clone(), rv0.clone()
        _ck(lib.vah_bn_finalize_stats(sums.t.data_ptr(), C, EPS, MOMENTUM, rm.data_ptr(), rv.data_ptr(), mean.t.data_ptr(),
                                      rstd.t.data_ptr(), st), 'bn_finalize_stats')
        _ck(apply(x.data_ptr(), rows, C, mean.t.data_ptr(), rstd.t.data_ptr(), w.data_ptr(), b.data_ptr(), 1, y.t.data_ptr(), st),
            'bn_nhwc_apply_f16')
        ws.reset()
        _ck(bwd_stats(x.data_ptr(), dy.data_ptr(), rows, C, mean.t.data_ptr(), rstd.t.data_ptr(), w.data_ptr(), b.data_ptr(), 1,
                      sums2.t.data_ptr(), ws.t.data_ptr(), st), 'bn_nhwc_bwd_stats_f16')
        means = sums2.t / sums.t[2 * C:]
        _ck(bwd_apply(x.data_ptr(), dy.data_ptr(), rows, C, mean.t.data_ptr(), rstd.t.data_ptr(), w.data_ptr(), b.data_ptr(), 1,
                      means[:C].data_ptr(), means[C:].data_ptr(), dx.t.data_ptr(), st), 'bn_nhwc_bwd_apply_f16')
        rse = torch.rsqrt(rv + EPS)                                 # eval mode: the running statistics, as _BNRelu forms them
        _ck(apply(x.data_ptr(), rows, C, rm.data_ptr(), rse.data_ptr(), w.data_ptr(), b.data_ptr(), 1, ye.t.data_ptr(), st),
            'bn_nhwc_apply_f16 eval')
        torch.cuda.synchronize()
        return [t.t.clone() for t in (sums, mean, rstd, y, sums2, dx, ye)] + [rm, rv, means, rse]

    outs = [sums, sums2, mean, rstd, y, ye, dx]
    for o in outs:
        o.reset()
    first = run()
    for o in outs:
        o.assert_intact(case + ' BatchNorm')
    for o in outs:
        o.reset()
    for a, c in zip(first, run()):
        _same_bits(a, c, case + ' BatchNorm: repeated call')
    s_k, mu_k, rs_k, y_k, s2_k, dx_k, ye_k, rm, rv, means, rse = first

    if gscale == 1.0:
        ref, A = spm.bn_stats(x)
        _record('bn stats', case, spm.check(case + ' stats', s_k[:2 * C], ref, A))
        fin = spm.finalize_stats(s_k, C, EPS, MOMENTUM, rm0, rv0)
        r = 0.
        for k, got in (('mean', mu_k), ('rstd', rs_k), ('running_mean', rm), ('running_var', rv)):
            r = max(r, spm.check(case + ' finalize ' + k, got, fin[k][0], fin[k][1], c_acc=C_FIN))
        _record('bn finalize', case, r)
        yr, Ay = spm.bn_apply(x, mu_k, rs_k, w, b, True)
        _check16('bn apply', case, 'apply', y_k, yr, Ay)
        yr, Ay = spm.bn_apply(x, rm, rse, w, b, True)
        _check16('bn apply eval', case, 'eval apply', ye_k, yr, Ay)
        del yr, Ay
    ref, A, edge = spm.bn_bwd_stats(x, dy, mu_k, rs_k, w, b, True)
    assert float(edge.double().mean()) < 1e-4, (case, int(edge.sum()))
    _record('bn bwd stats' + sfx, case, spm.check(case + ' bwd stats', s2_k, ref, A))
    dxr, Adx = spm.bn_bwd_apply(x, dy, mu_k, rs_k, w, b, True, means[:C], means[C:])
    assert torch.isfinite(dx_k).all()
    _check16('bn bwd apply' + sfx, case, 'bwd apply', dx_k, dxr, Adx, mask=~edge)
    del dxr, Adx, edge
    return x, dy, w, b, rm0, rv0, first


@pytest.mark.parametrize('case,rows,C', BN_CASES, ids=[c[0] for c in BN_CASES])
def test_bn_production(case, rows, C):
    from vitadapter import spm_nhwc
    x, dy, w, b, rm0, rv0, (s_k, mu_k, rs_k, y_k, s2_k, dx_k, ye_k, rm, rv, means, rse) = _run_bn(case, rows, C, seed=rows % 997 + C)
    norm = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM).cuda().train()
    with torch.no_grad():
        norm.weight.copy_(w), norm.bias.copy_(b), norm.running_mean.copy_(rm0), norm.running_var.copy_(rv0)
    xr = x.clone().requires_grad_(True)
    yw = spm_nhwc._BNRelu.apply(xr, norm.weight, norm.bias, norm, True)
    assert yw.dtype == F16
    yw.backward(dy)
    torch.cuda.synchronize()
    _same_bits(yw.detach(), y_k, case + ' _BNRelu forward')
    assert xr.grad.dtype == F16
    _same_bits(xr.grad, dx_k, case + ' _BNRelu input grad')
    _same_bits(norm.bias.grad, s2_k[:C], case + ' _BNRelu dbias')
    _same_bits(norm.weight.grad, s2_k[C:], case + ' _BNRelu dweight')
    _same_bits(norm.running_mean, rm, case + ' running mean')
    _same_bits(norm.running_var, rv, case + ' running var')
    norm.eval()
    with torch.no_grad():
        _same_bits(spm_nhwc._BNRelu.apply(x, norm.weight, norm.bias, norm, True), ye_k, case + ' _BNRelu eval')


@pytest.mark.parametrize('case,rows,C', BN_CAP_CASES, ids=[c[0] for c in BN_CAP_CASES])
def test_bn_stats_cap(case, rows, C):
    _run_bn(case, rows, C, seed=rows)


# the stem of configs[1] and the widest production matrix, with loss-scaled dy
SCALED_BN_CASES = [('scaled_131072x64', 131072, 64), ('scaled_32768x256', 32768, 256)]


@pytest.mark.parametrize('case,rows,C', SCALED_BN_CASES, ids=[c[0] for c in SCALED_BN_CASES])
def test_bn_backward_of_subnormal_dy(case, rows, C):
    _run_bn(case, rows, C, seed=rows % 997 + C + 1, gscale=SCALED)


# ---------------------------------------------------------------- max-pool, image layout
@pytest.mark.parametrize('case,N,H,W,kind', POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_maxpool(case, N, H, W, kind):
    from vitadapter import spm_nhwc
    C = 64
    g = torch.Generator(device='cuda').manual_seed(H + W)
    if kind == 'relu':                  # post-ReLU: ties among zeros are the common case
        x = torch.randn(N, H, W, C, device='cuda', generator=g).clamp_min(0).to(F16)
    else:                               # a handful of distinct values: ties between non-zero values
        vals = torch.tensor([-1.0, 0.375, 1.25, 2.5, 2.5], device='cuda')
        x = vals[torch.randint(0, 5, (N, H, W, C), device='cuda', generator=g)].to(F16)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(N, OH, OW, C, device='cuda', generator=g).to(F16)
    y, idx = _Guarded((N, OH, OW, C), F16, OW * C), _Guarded((N, OH, OW, C), torch.uint8, OW * C)
    gx = _Guarded((N, H, W, C), F16, W * C)
    st = _st()

    def fwd():
        _ck(_sym('vah_maxpool3s2_nhwc_fwd_bf16')(x.data_ptr(), N, H, W, C, y.t.data_ptr(), idx.t.data_ptr(), st), 'maxpool fwd f16')

    y_k, i_k = _twice(fwd, [y, idx], case + ' max-pool')
    yr, ir = spm.maxpool_forward(x)
    _equal(y_k.double(), yr, case + ' max-pool output')
    _equal(i_k, ir, case + ' max-pool window index')
    idx.t.copy_(i_k)

    def bwd():
        _ck(_sym('vah_maxpool3s2_nhwc_bwd_bf16')(gy.data_ptr(), idx.t.data_ptr(), N, H, W, C, gx.t.data_ptr(), st), 'maxpool bwd f16')

    gx_k, = _twice(bwd, [gx], case + ' max-pool backward')
    gr, A = spm.maxpool_backward(gy, ir, H, W)
    _check16('maxpool bwd', case, 'max-pool backward', gx_k, gr, A)
    xr = x.clone().requires_grad_(True)
    yw = spm_nhwc._MaxPool.apply(xr)
    assert yw.dtype == F16
    yw.backward(gy)
    torch.cuda.synchronize()
    _same_bits(yw.detach(), y_k, case + ' _MaxPool forward')
    assert xr.grad.dtype == F16
    _same_bits(xr.grad, gx_k, case + ' _MaxPool backward')


@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_image_to_nhwc16(cfg):
    from vitadapter import spm_nhwc
    H, W, N = CONFIGS[cfg]
    x = torch.randn(N, 3, H, W, device='cuda') * 3
    x[0, :, 0, :8] = torch.tensor([70000., -1e6, 65519.9, 65520., 3e-6, -2.0 ** -25, 2.0 ** -25 * 1.0001, 1e-9], device='cuda')
    y = _Guarded((N, H, W, 16), F16, W * 16)

    def run():
        _ck(_sym('vah_image_to_nhwc16_bf16')(x.data_ptr(), N, H, W, y.t.data_ptr(), _st()), 'image_to_nhwc16_f16')

    got, = _twice(run, [y], cfg + ' image_to_nhwc16')
    _same_bits(got, _image16(x), cfg + ' image_to_nhwc16')
    assert torch.isinf(got[0, 0, 0, :3]).all() and float(got[0, 0, 2, 0]) == 65504. and torch.isinf(got[0, 0, 3, 0])
    assert (got[..., 3:].view(torch.int16) == 0).all()
    _same_bits(spm_nhwc.image_to_nhwc16(x, F16), got, cfg + ' spm_nhwc.image_to_nhwc16')


# ---------------------------------------------------------------- the fp32 -> fp16 conversion of the stores
def _classes(p32):
    """of fp32 values: how many round to fp16 subnormals (non-zero), overflow to inf, and lie exactly half way between
    two fp16 values"""
    q = p32.double().abs()
    sub = (q >= 2.0 ** -25) & (q < F16_MIN_NORMAL)
    over = q >= 65520.
    spacing = torch.exp2(torch.floor(torch.log2(q.clamp_min(F16_MIN_NORMAL))) - 10)
    frac = q / spacing - torch.floor(q / spacing)
    tie = (frac == 0.5) & ~over
    return int(sub.sum()), int(over.sum()), int(tie.sum()), int((tie & (q < F16_MIN_NORMAL)).sum())


def _conversion_values(n, g):
    """n non-zero normal fp16 values: random signs and magnitudes over fp16's normal range, odd and even significands"""
    e = torch.randint(-13, 15, (n,), device='cuda', generator=g).float()
    m = torch.randint(1024, 2048, (n,), device='cuda', generator=g).float() / 1024.
    s = torch.where(torch.rand(n, device='cuda', generator=g) < 0.5, -1.0, 1.0)
    v = (s * m * torch.exp2(e)).to(F16)
    assert bool((v.float().abs() >= F16_MIN_NORMAL).all()) and bool(torch.isfinite(v).all())
    return v


def test_f16_conversion_is_torchs():
    """The stores of conv_taps and bn_apply against torch's .to(float16) of the fp32 value, bit for bit.  conv_taps: one
    non-zero channel per pixel (a_i) meets one non-zero weight of the centre tap per output channel (b_co), both normal
    fp16: the accumulator holds a_i * b_co, exact in fp32 (11 x 11 significant bits).  bn_apply: mean 0, rstd 1, bias 0,
    no ReLU: y = fp16(x * w), the product rounded once to fp32 by the kernel's fma as by torch's multiplication; powers
    of two and 1.5 among the w put results exactly half way between fp16 values."""
    g = torch.Generator(device='cuda').manual_seed(2024)
    W, C = 512, 64
    a = _conversion_values(W, g)
    b = _conversion_values(C, g)
    a[:6] = torch.tensor([65504., 1.0 + 2.0 ** -10, 3 * 2.0 ** -13, 256., -(1.0 + 2.0 ** -10), 2047 * 2.0 ** -13], device='cuda').to(F16)
    b[:6] = torch.tensor([1.0 + 2.0 ** -10, 1.5, 2.0 ** -12, 300., -2.0 ** -14, 2.0 ** -13], device='cuda').to(F16)
    # 1.5 x and 1 x powers of two: an odd significand of a_i lands exactly half way, in the normal and the subnormal range
    b[6:16] = torch.tensor([1.5 * 2.0 ** k for k in (-3, 0, 2, -10, -12, -13)] + [2.0 ** k for k in (-11, -12, -13, -14)], device='cuda').to(F16)
    x = torch.zeros(1, 1, W, C, dtype=F16, device='cuda')
    x[0, 0, :, 0] = a
    w9 = torch.zeros(C, 9, C, dtype=F16, device='cuda')
    w9[:, 4, 0] = b
    out = _Guarded((1, 1, W, C), F16, W * C)
    got, = _twice(lambda: _fwd(x, w9, 1, out.t), [out], 'conversion conv_taps')
    p = a.float()[:, None] * b.float()[None, :]
    assert bool((p != 0).all())
    n_sub, n_over, n_tie, n_subtie = _classes(p)
    print('CONVERSION conv_taps: %d values, %d subnormal, %d overflow, %d ties (%d subnormal)' % (p.numel(), n_sub, n_over, n_tie, n_subtie))
    assert n_sub > 100 and n_over > 100 and n_tie > 10 and n_subtie > 0
    _same_bits(got.view(W, C), p.to(F16), 'conv_taps_f16 store vs torch .to(float16)')
    assert int(torch.isinf(got).sum()) == n_over

    rows = 1024
    xs = _conversion_values(rows * C, g).view(rows, C)
    wv = torch.exp2(((torch.arange(C, device='cuda') // 4) % 16 - 12).float())      # 2^-12 .. 2^3 in each of the four kinds below
    wv[1::4] *= 1.5
    wv[2::4] *= torch.rand(C // 4, device='cuda', generator=g) + 1.0        # full 24-bit significands
    wv[3::8] *= -1.0
    zero, one = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    y = _Guarded((rows, C), F16, C)
    got, = _twice(lambda: _ck(_sym('vah_bn_nhwc_apply')(xs.data_ptr(), rows, C, zero.data_ptr(), one.data_ptr(), wv.data_ptr(),
                                                       zero.data_ptr(), 0, y.t.data_ptr(), _st()), 'bn_nhwc_apply_f16'),
                  [y], 'conversion bn_apply')
    p = xs.float() * wv[None, :]
    n_sub, n_over, n_tie, n_subtie = _classes(p)
    print('CONVERSION bn_apply: %d values, %d subnormal, %d overflow, %d ties (%d subnormal)' % (p.numel(), n_sub, n_over, n_tie, n_subtie))
    assert n_sub > 100 and n_over > 100 and n_tie > 10 and n_subtie > 0
    _same_bits(got, p.to(F16), 'bn_nhwc_apply_f16 store vs torch .to(float16)')
    assert int(torch.isinf(got).sum()) == n_over
