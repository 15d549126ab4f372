"""GPU: the fp16 Linear path held to fp64 - vah_gemm_f16 / vah_gemm_f16_fin (csrc/gemm.hip) through vitadapter.fused, and
the fp16 twins of the column-sum, GELU-backward and `_bsum` residual kernels (csrc/fused_ops.hip).

Budgets.  A product or column sum accumulated in fp32: 64 * 2^-24 * sum|terms| per element, the project's fp32-sum
budget (tests/test_reductions_fullsize_gpu.py); a bias adds |bias| * 2^-24.  An fp16 result adds its one rounding,
2^-11 |ref| + 2^-25 (half a subnormal step: subnormal results are kept).  Every output is NaN-filled before the call.

Nothing here tunes live (a module fixture puts the dispatcher into mode 0: hipBLASLt's first heuristic answer, no timing,
no candidate runs) except the one split-K case, which exists only in mode 1."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

BUDGET = 64 * 2.0 ** -24
F16 = torch.float16
NAN = float('nan')


def _lib():
    import _vah
    return _vah


def _env_tuning():
    spec = os.environ.get('VAH_GEMM_TUNING')
    if spec:
        parts = [int(t) for t in spec.split(',')]
        return parts[0], parts[1] if len(parts) > 1 else 32
    return 1, 32


@pytest.fixture(scope='module', autouse=True)
def _no_live_tuning():
    v = _lib()
    v.check(v.lib.vah_gemm_set_tuning(0, 32), 'gemm_set_tuning')
    yield
    v.check(v.lib.vah_gemm_set_tuning(*_env_tuning()), 'gemm_set_tuning')


def _p(t):
    return t.data_ptr() if t is not None else None


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device='cuda')


def _stream():
    return _lib().raw_stream(torch.device('cuda', torch.cuda.current_device()))


def _within(got, ref, mag, what, f16_out=False, extra=None):
    """|got - ref| <= BUDGET * mag (+ extra) (+ the fp16 rounding of ref), element by element; prints the worst ratio"""
    got = got.double()
    assert bool(torch.isfinite(got).all()), what + ': not finite (an element was not written?)'
    bound = BUDGET * mag
    if extra is not None:
        bound = bound + extra
    if f16_out:
        bound = bound + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print('%s: worst error / budget %.3f' % (what, worst))
    assert bool((err <= bound).all()), (what, worst)


# ---------------------------------------------------------------------------------------
# vah_gemm_f16
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('bias_kind', ['none', 'f32', 'f16'])
@pytest.mark.parametrize('out_dtype', [F16, torch.float32], ids=['out_f16', 'out_f32'])
@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 0), (1, 1)], ids=['nn', 'nt', 'tn', 'tt'])
@pytest.mark.parametrize('M,N,K', [(200, 72, 96), (64, 256, 128)])
def test_gemm_f16(M, N, K, ta, tb, out_dtype, bias_kind):
    from vitadapter import fused
    gen = torch.Generator(device='cuda').manual_seed(M + 2 * ta + tb)
    a = torch.randn((K, M) if ta else (M, K), device='cuda', generator=gen).to(F16)
    b = torch.randn((N, K) if tb else (K, N), device='cuda', generator=gen).to(F16)
    bias = None
    if bias_kind != 'none':
        bias = (torch.randn(N, device='cuda', generator=gen) * 3).to(F16 if bias_kind == 'f16' else torch.float32)
    outs = []
    for _ in range(2):
        d = _nan(M, N, dtype=out_dtype)
        assert fused.gemm_16(a, b, trans_a=bool(ta), trans_b=bool(tb), bias=bias, out=d) is d
        torch.cuda.synchronize()
        outs.append(d)
    assert torch.equal(outs[0], outs[1]), 'two calls differ'
    ad = a.double().t() if ta else a.double()
    bd = b.double().t() if tb else b.double()
    ref, mag = ad @ bd, ad.abs() @ bd.abs()
    extra = None
    if bias is not None:
        ref = ref + bias.double()
        extra = bias.double().abs().expand(M, N) * 2.0 ** -24
    _within(outs[0], ref, mag, 'gemm_f16 %dx%dx%d ta%d tb%d %s bias %s' % (M, N, K, ta, tb, out_dtype, bias_kind),
            f16_out=out_dtype == F16, extra=extra)


def test_gemm_f16_overflows_to_inf():
    """Every |ref| >= 2 * 65504: the fp16 result is inf with ref's sign (GradScaler has to see it; no saturation), the fp32
    result of the same product is finite and within budget."""
    from vitadapter import fused
    M, N, K = 64, 72, 96
    gen = torch.Generator(device='cuda').manual_seed(1)
    sign = torch.where(torch.rand(M, 1, device='cuda', generator=gen) < 0.5, -1.0, 1.0)
    a = (sign * (1.0 + torch.rand(M, K, device='cuda', generator=gen)) * 40.0).to(F16)
    b = ((1.0 + torch.rand(K, N, device='cuda', generator=gen)) * 40.0).to(F16)
    ref, mag = a.double() @ b.double(), a.double().abs() @ b.double().abs()
    assert float(ref.abs().min()) >= 2 * 65504.0 and bool((ref < 0).any()) and bool((ref > 0).any())
    d16, d32 = _nan(M, N, dtype=F16), _nan(M, N)
    fused.gemm_16(a, b, out=d16)
    fused.gemm_16(a, b, out=d32)
    torch.cuda.synchronize()
    assert bool(torch.isinf(d16).all()), 'saturated or unwritten'
    assert torch.equal(torch.sign(d16.float()), torch.sign(ref).float())
    _within(d32, ref, mag, 'overflow case, fp32 output')


def test_gemm_f16_keeps_subnormal_results():
    """Products near 2^-20, 8 of them per element: every result lies below fp16's smallest normal (2^-14) and is kept,
    not flushed - within the budget and half a subnormal step."""
    from vitadapter import fused
    M, N, K = 64, 72, 8
    gen = torch.Generator(device='cuda').manual_seed(2)
    a = ((1.0 + torch.rand(M, K, device='cuda', generator=gen)) * 2.0 ** -10).to(F16)
    b = ((1.0 + torch.rand(K, N, device='cuda', generator=gen)) * 2.0 ** -10).to(F16)
    ref = a.double() @ b.double()
    assert 2.0 ** -18 < float(ref.min()) and float(ref.max()) < 2.0 ** -14
    d = _nan(M, N, dtype=F16)
    fused.gemm_16(a, b, out=d)
    torch.cuda.synchronize()
    assert bool((d.float() > 0).all()), 'flushed to zero'
    _within(d, ref, ref, 'subnormal results', f16_out=True)


# ---------------------------------------------------------------------------------------
# GELU backward
# ---------------------------------------------------------------------------------------
def _run_gelu(da, h):
    v = _lib()
    rows, C = h.shape
    dh = _nan(rows, C, dtype=F16)
    bpart, n = _nan(v.lib.vah_reduce_ws_floats(C)), ctypes.c_int64(-1)
    v.check(v.lib.vah_gelu_bwd_bsum_f16(_p(da), _p(h), rows, C, _p(dh), _p(bpart), ctypes.byref(n), _stream()), 'gelu_bwd_bsum_f16')
    torch.cuda.synchronize()
    return dh, bpart, n.value


def _ordered(t):
    """fp16 -> integers in which neighbouring values differ by 1 (and +0 == -0)"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i >= 0, i, -(i & 0x7fff))


def _torch_gelu_bwd(da, h):
    hh = h.clone().requires_grad_(True)
    torch.nn.functional.gelu(hh).backward(da)
    return hh.grad


def _gelu_ref64(da, h):
    x, d = h.double(), da.double()
    cdf = 0.5 * (1.0 + torch.erf(x * 0.5 ** 0.5))
    pdf = torch.exp(-0.5 * x * x) / (2.0 * torch.pi) ** 0.5
    return d * (cdf + x * pdf)


def _check_partials(bpart, nparts, dz, C, what):
    """rows [0, nparts) finite, and their sum within the budget of the fp64 column sum of the fp16 dz"""
    assert 1 <= nparts <= 512, (what, nparts)
    rows = bpart[:nparts * C].view(nparts, C)
    assert bool(torch.isfinite(rows).all()), what
    d = dz.reshape(-1, C).double()
    _within(rows.double().sum(0), d.sum(0), d.abs().sum(0), what + ' partial rows (%d)' % nparts)


@pytest.mark.parametrize('lo,hi', [(0.0, 0.0), (0.0, 2.0 ** -6), (2.0 ** -6, 0.5), (0.5, 2.0), (2.0, 4.0), (4.0, 6.0), (6.0, 8.0)])
def test_gelu_bwd_f16_values(lo, hi):
    """The value bands of tests/test_bias_partials_gpu.py::test_gelu_bwd_values on fp16 operands: against fp64 the fp16
    rounding of the result, 2^-11 |ref| + 2^-25, plus the fp32 evaluation, 2^-20 |da|; against torch's GeluBackward on
    the same fp16 tensors at most one fp16 ulp."""
    rows, C = 64, 264
    gen = torch.Generator(device='cuda').manual_seed(int(hi * 1024) + 1)
    mag = lo + (hi - lo) * torch.rand(rows, C, device='cuda', generator=gen)
    sign = torch.where(torch.rand(rows, C, device='cuda', generator=gen) < 0.5, -1.0, 1.0)
    h = (mag * sign).to(F16)
    if hi == 8.0:
        h[0, :8] = torch.tensor([8.0, -8.0] * 4, device='cuda').to(F16)
        assert float(h.float().abs().max()) == 8.0
    if hi == 0.0:
        assert bool((h.view(torch.int16) < 0).any()) and bool((h.view(torch.int16) == 0).any()), 'both zeros'
    da = (torch.randn(rows, C, device='cuda', generator=gen) * 3).to(F16)
    dh, bpart, n = _run_gelu(da, h)
    ref = _gelu_ref64(da, h)
    err = (dh.double() - ref).abs()
    bound = 2.0 ** -11 * ref.abs() + 2.0 ** -20 * da.double().abs() + 2.0 ** -25
    steps = (_ordered(dh) - _ordered(_torch_gelu_bwd(da, h))).abs()
    print('|h| in [%g, %g]: worst error / budget %.3f; differs from torch in %d of %d elements (max %d ulp)'
          % (lo, hi, float((err / bound).max()), int((steps > 0).sum()), steps.numel(), int(steps.max())))
    assert bool(torch.isfinite(dh.float()).all())
    assert bool((err <= bound).all())
    assert int(steps.max()) <= 1
    _check_partials(bpart, n, dh, C, 'gelu values')


@pytest.mark.parametrize('C', [8, 264, 3072])
@pytest.mark.parametrize('rows', [1, 37, 4101])
def test_gelu_bwd_f16_partial_rows(rows, C):
    gen = torch.Generator(device='cuda').manual_seed(rows + C)
    h = (torch.randn(rows, C, device='cuda', generator=gen) * 1.5).to(F16)
    da = torch.randn(rows, C, device='cuda', generator=gen).to(F16)
    dh1, bp1, n1 = _run_gelu(da, h)
    dh2, bp2, n2 = _run_gelu(da, h)
    assert torch.equal(dh1, dh2) and n1 == n2 and torch.equal(bp1[:n1 * C], bp2[:n2 * C])
    ref = _gelu_ref64(da, h)
    assert bool(((dh1.double() - ref).abs() <= 2.0 ** -11 * ref.abs() + 2.0 ** -20 * da.double().abs() + 2.0 ** -25).all())
    _check_partials(bp1, n1, dh1, C, 'gelu_bwd_bsum_f16 %dx%d' % (rows, C))


# ---------------------------------------------------------------------------------------
# _wgrad_bgrad on fp16
# ---------------------------------------------------------------------------------------
def _wgrad_direct(g2, x2, partials, split):
    """fused._wgrad_bgrad's calls with every buffer it hands over poisoned: column-sum partial rows (unless a producer
    left them), outputs, and the split-K partial products at the front of the GEMM workspace."""
    from vitadapter import fused
    v = _lib()
    R, N = g2.shape
    K = x2.shape[1]
    ws_bytes = fused._GEMM_WS_BYTES + (min(64 * N * K * 4, 160 << 20) if R >= 4096 else 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    if split > 1:
        ws[:split * N * K * 4].view(torch.float32).fill_(NAN)
    gw, gb = _nan(N, K), _nan(N)
    st = _stream()
    if partials is None:
        cws, nparts = _nan(v.lib.vah_reduce_ws_floats(N)), ctypes.c_int64(0)
        v.check(v.lib.vah_colsum_f16_partials(_p(g2), R, N, _p(cws), ctypes.byref(nparts), st), 'colsum_f16_partials')
        nparts = nparts.value
    else:
        cws, nparts = partials
    v.check(v.lib.vah_gemm_f16_fin(1, 0, N, K, R, _p(g2), N, _p(x2), K, _p(gw), K, 1, _p(ws), ws_bytes, _p(cws), nparts, N,
                                   _p(gb), st), 'gemm_f16_fin')
    torch.cuda.synchronize()
    return gw, gb


def _split_of(N, K, R):
    key = 'f16 1 0 1 0 0 %d %d %d %d %d %d ' % (N, K, R, N, K, K)
    lines = [ln for ln in _lib().gemm_table_dump().splitlines() if ln.startswith(key)]
    assert len(lines) == 1, (key, lines)
    return int(lines[0].split()[13])


@pytest.mark.parametrize('from_gelu', [False, True], ids=['colsum', 'gelu_partials'])
@pytest.mark.parametrize('R,N,K', [(13, 72, 40), (1367, 264, 96), (4096, 64, 64)])
def test_wgrad_bgrad_f16(R, N, K, from_gelu):
    """(dW, db) = (g2^T x2, column sums of g2) in fp32 from fp16 operands, per element within the budget of the fp64
    values.  With ``from_gelu`` g2 is what vah_gelu_bwd_bsum_f16 wrote and the partial rows are the ones it left.
    (4096, 64, 64) is the one case that tunes live (mode 1): split-K exists only there; the split the tuner took is
    printed and the result is held to the same budget whatever it was."""
    from vitadapter import fused
    v = _lib()
    gen = torch.Generator(device='cuda').manual_seed(R + N)
    x2 = torch.randn(R, K, device='cuda', generator=gen).to(F16)
    partials = None
    if from_gelu:
        h = (torch.randn(R, N, device='cuda', generator=gen) * 1.5).to(F16)
        da = torch.randn(R, N, device='cuda', generator=gen).to(F16)
        g2, bpart, n = _run_gelu(da, h)
        partials = (bpart, n)
    else:
        g2 = torch.randn(R, N, device='cuda', generator=gen).to(F16)
    live = R == 4096
    if live:
        v.check(v.lib.vah_gemm_set_tuning(1, 32), 'gemm_set_tuning')
    try:
        ew, eb = fused._wgrad_bgrad(g2, x2, partials)
        torch.cuda.synchronize()
    finally:
        if live:
            v.check(v.lib.vah_gemm_set_tuning(0, 32), 'gemm_set_tuning')
    split = _split_of(N, K, R)
    print('wgrad %dx%dx%d: split %d' % (N, K, R, split))
    assert split == 1 or live
    assert ew.dtype == eb.dtype == torch.float32
    gw1, gb1 = _wgrad_direct(g2, x2, partials, split)
    gw2, gb2 = _wgrad_direct(g2, x2, partials, split)
    assert torch.equal(gw1, gw2) and torch.equal(gb1, gb2), 'two calls differ'
    assert torch.equal(ew, gw1) and torch.equal(eb, gb1), 'fused._wgrad_bgrad differs from the direct call'
    gd, xd = g2.double(), x2.double()
    _within(gw1, gd.t() @ xd, gd.abs().t() @ xd.abs(), 'dW %dx%dx%d' % (N, K, R))
    _within(gb1, gd.sum(0), gd.abs().sum(0), 'db %dx%dx%d' % (N, K, R))


# ---------------------------------------------------------------------------------------
# the `_bsum` forms of the residual backward kernels
# ---------------------------------------------------------------------------------------
def _ln_inputs(batch, rpb, C, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    rows = batch * rpb
    t = torch.randn(rows, C, device='cuda', generator=g) * 1.5 + 0.3
    gh = torch.randn(rows, C, device='cuda', generator=g).to(F16)
    gt = torch.randn(rows, C, device='cuda', generator=g) * 0.5
    z = torch.randn(rows, C, device='cuda', generator=g).to(F16)
    w = torch.randn(C, device='cuda', generator=g) * 0.2 + 1.0
    sc = torch.tensor([1.0 / 0.7, 0.0, 1.0 / 0.9][:batch], device='cuda') if batch > 1 else torch.tensor([1.25], device='cuda')
    mean = t.mean(1)
    rstd = torch.rsqrt(t.var(1, unbiased=False) + 1e-6)
    return t, gh, w, mean.contiguous(), rstd.contiguous(), gt, z, sc


def _run_ln(entry, ins, batch, rpb, C, bsum):
    v = _lib()
    t, gh, w, mean, rstd, gt, z, sc = ins
    rows = batch * rpb
    dt, dz = _nan(rows, C), _nan(rows, C, dtype=F16)
    dw, db = _nan(C), _nan(C)
    ws = _nan(v.lib.vah_reduce_ws_floats(3 * C))
    args = [_p(t), _p(gh), _p(w), _p(mean), _p(rstd), _p(gt), _p(z), None, _p(sc), batch, rpb, C, _p(dt), _p(dz), None,
            _p(dw), _p(db), _p(ws)]
    bpart, n = None, ctypes.c_int64(-1)
    if bsum:
        bpart = _nan(v.lib.vah_reduce_ws_floats(C))
        args += [_p(bpart), ctypes.byref(n)]
    v.check(getattr(v.lib, entry)(*args, _stream()), entry)
    torch.cuda.synchronize()
    return dict(dt=dt, dz=dz, dw=dw, db=db), bpart, n.value


SHAPES = pytest.mark.parametrize('batch,rpb', [(1, 13), (3, 1367)], ids=['rows13', 'rows4101'])


@pytest.mark.parametrize('C', [200, 768])
@SHAPES
def test_residual_layernorm_bwd_f16_bsum(batch, rpb, C):
    ins = _ln_inputs(batch, rpb, C, 11 + C + rpb)
    want, _, _ = _run_ln('vah_residual_layernorm_bwd_f16', ins, batch, rpb, C, False)
    got1, bp1, n1 = _run_ln('vah_residual_layernorm_bwd_f16_bsum', ins, batch, rpb, C, True)
    got2, bp2, n2 = _run_ln('vah_residual_layernorm_bwd_f16_bsum', ins, batch, rpb, C, True)
    for k in want:
        assert bool(torch.isfinite(want[k].float()).all()), k
        assert torch.equal(got1[k], want[k]) and torch.equal(got2[k], want[k]), k
    assert n1 == n2 and torch.equal(bp1[:n1 * C], bp2[:n2 * C])
    _check_partials(bp1, n1, got1['dz'], C, 'residual_layernorm_bwd_f16_bsum %dx%d' % (batch * rpb, C))


def _run_sr(entry, g, z, gamma, s, batch, rpb, C, bsum):
    v = _lib()
    dz = _nan(batch * rpb, C, dtype=F16)
    dgamma = _nan(C) if gamma is not None else None
    ws = _nan(v.lib.vah_reduce_ws_floats(C)) if gamma is not None else None
    args = [_p(g), _p(z), _p(gamma), _p(s), batch, rpb, C, _p(dz), _p(dgamma), _p(ws)]
    bpart, n = None, ctypes.c_int64(-1)
    if bsum:
        bpart = _nan(v.lib.vah_reduce_ws_floats(C))
        args += [_p(bpart), ctypes.byref(n)]
    v.check(getattr(v.lib, entry)(*args, _stream()), entry)
    torch.cuda.synchronize()
    out = dict(dz=dz)
    if dgamma is not None:
        out['dgamma'] = dgamma
    return out, bpart, n.value


@pytest.mark.parametrize('C', [200, 768])
@SHAPES
@pytest.mark.parametrize('form', ['plain', 'gamma'])
def test_scale_residual_bwd_f16_bsum(form, batch, rpb, C):
    """plain: the column-tiled kernel (no layer scale); gamma: the row-strip kernel with its second accumulator"""
    rows = batch * rpb
    gen = torch.Generator(device='cuda').manual_seed(3 * rows + C)
    g = torch.randn(rows, C, device='cuda', generator=gen)
    z = torch.randn(rows, C, device='cuda', generator=gen).to(F16)
    gamma = (torch.randn(C, device='cuda', generator=gen) * 0.3 + 1.0) if form == 'gamma' else None
    s = torch.tensor([1.0 / 0.7, 0.0, 1.0 / 0.9][:batch], device='cuda')
    want, _, _ = _run_sr('vah_scale_residual_bwd_f16', g, z, gamma, s, batch, rpb, C, False)
    got1, bp1, n1 = _run_sr('vah_scale_residual_bwd_f16_bsum', g, z, gamma, s, batch, rpb, C, True)
    got2, bp2, n2 = _run_sr('vah_scale_residual_bwd_f16_bsum', g, z, gamma, s, batch, rpb, C, True)
    assert sorted(want) == sorted(got1)
    for k in want:
        assert bool(torch.isfinite(want[k].float()).all()), k
        assert torch.equal(got1[k], want[k]) and torch.equal(got2[k], want[k]), k
    assert n1 == n2 and torch.equal(bp1[:n1 * C], bp2[:n2 * C])
    _check_partials(bp1, n1, got1['dz'], C, 'scale_residual_bwd_f16_bsum %s %dx%d' % (form, rows, C))


def test_bsum_f16_entries_refuse_what_the_bf16_entries_refuse():
    """On live buffers: the same codes and messages (the name changed), and nothing is launched."""
    v = _lib()
    C, batch, rpb = 200, 1, 13
    t, gh, w, mean, rstd, gt, z, sc = _ln_inputs(batch, rpb, C, 5)
    gamma, dgamma = torch.ones(C, device='cuda'), _nan(C)
    dt, dz = _nan(rpb, C), _nan(rpb, C, dtype=F16)
    dw, db, ws = _nan(C), _nan(C), _nan(v.lib.vah_reduce_ws_floats(3 * C))
    bpart, n = _nan(v.lib.vah_reduce_ws_floats(C)), ctypes.c_int64(-1)

    def ln_args(**kw):
        a = dict(z=_p(z), gamma=None, dgamma=None, dz=_p(dz), bpart=_p(bpart), n=ctypes.byref(n))
        a.update(kw)
        return (_p(t), _p(gh), _p(w), _p(mean), _p(rstd), _p(gt), a['z'], a['gamma'], _p(sc), batch, rpb, C, _p(dt), a['dz'],
                a['dgamma'], _p(dw), _p(db), _p(ws), a['bpart'], a['n'], _stream())

    def sr_args(**kw):
        a = dict(g=_p(gt), z=_p(z), dz=_p(dz), bpart=_p(bpart), n=ctypes.byref(n))
        a.update(kw)
        return (a['g'], a['z'], None, None, batch, rpb, C, a['dz'], None, None, a['bpart'], a['n'], _stream())

    cases = [('vah_residual_layernorm_bwd_bsum', ln_args, [
                  (dict(gamma=_p(gamma), dgamma=_p(dgamma)), -2), (dict(bpart=None), -1), (dict(n=None), -1),
                  (dict(bpart=_p(bpart) + 4), -4), (dict(dz=_p(dz) + 2), -4), (dict(z=None), -1)]),
             ('vah_scale_residual_bwd_bsum', sr_args, [
                  (dict(g=_p(gt) + 8), -4), (dict(dz=_p(dz) + 4), -4), (dict(z=None), -1), (dict(dz=None), -1),
                  (dict(bpart=None), -1), (dict(n=None), -1), (dict(bpart=_p(bpart) + 8), -4)])]
    for name, build, bad in cases:
        f16 = v.LINEAR_F16_TWINS[name]
        for kw, code in bad:
            rcb = getattr(v.lib, name)(*build(**kw))
            msgb = v.lib.vah_last_error().decode()
            rc16 = getattr(v.lib, f16)(*build(**kw))
            msg16 = v.lib.vah_last_error().decode()
            assert rcb == rc16 == code, (name, kw, rcb, rc16)
            assert msg16 == msgb.replace(name, f16) and msg16.startswith(f16 + ':'), (msgb, msg16)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz.float()).all()) and bool(torch.isnan(bpart).all()), 'nothing was launched'
