"""GPU: the fp16 instantiations of the row-streaming kernels (csrc/fused_ops.hip, the `_f16` entry points) held to
fp64 at the production shapes of tests/test_reductions_fullsize_gpu.py, whose fp64 references are used here as they
are (they take the kernel's own operands: fp16 inputs upcast, a backward uses the kernel's fp32 mean / rstd).

Budget per element:

    |got - ref| <= C_ACC * 2^-24 * A   +   (fp16 outputs only)  2^-11 * |ref| + 2^-25

A = the sum of |terms| of the element, C_ACC = 64 as in that file: its chain-length argument is about the fp32 part of
the kernels, which does not depend on the 16-bit type.  2^-11 |ref| is fp16's round-to-nearest bound and 2^-25 half the
spacing of its subnormals: both derived from the format, not measured.

Every output and workspace is NaN-filled before the call and sits between two guard bands of a sentinel that must be
untouched afterwards; every case runs twice and must give the same bits; every fused.* entry point under
torch.autocast(float16) must give the bits of the direct C call.  The fp32 -> fp16 conversion itself is checked by bits
(test_f16_conversion_is_torchs): round to nearest even, overflow to inf, subnormals kept.

Measured on an MI355X (worst err / budget): fp32 outputs <= 0.047 (dx of the dual LayerNorm; mean / rstd 0.02, parameter
gradients <= 0.007), where the bf16 file has them; fp16 outputs (y, h, ya, yb, dz, DWConv y / dx) 0.988 - 0.996, the
rounding bound itself."""
import math

import pytest
import torch

from test_reductions_fullsize_gpu import (C_ACC, DUAL_SHAPES, EPS, LN_CAP_768, LN_SHAPES, NAN, RES_CAP_1024, U, _dwconv_ref,
                                          _ln_bwd_ref, _ln_data, _ln_fwd_ref)

pytestmark = pytest.mark.gpu

F16 = torch.float16
G = 64                 # guard band, elements (128 B of fp16, 256 B of fp32: the 16-byte alignment of the views is kept)
SENTINEL = 1232.0      # exact in bf16, fp16 and fp32 (tests/test_fused_widths_fp64_gpu.py guards bf16 outputs with it)
FAMILIES = 'layernorm,residual_layernorm,scale_residual,dwconv_tokens'


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    import _vah
    return _vah


class _Guarded:
    """NaN-filled output buffers between two guard bands."""

    def __init__(self):
        self.bufs = []

    def nan(self, *shape, dtype=torch.float32):
        n = math.prod(shape)
        buf = torch.full((n + 2 * G,), SENTINEL, dtype=dtype, device='cuda')
        buf[G:G + n] = NAN
        self.bufs.append((buf, n))
        return buf[G:G + n].view(shape)

    def check(self, what):
        for k, (buf, n) in enumerate(self.bufs):
            assert bool((buf[:G] == SENTINEL).all()) and bool((buf[G + n:] == SENTINEL).all()), \
                '%s: guard band of buffer %d (%d elements, %s) was written' % (what, k, n, buf.dtype)


def _within(got, ref, A, what, f16=False):
    """Per-element budget C_ACC * 2^-24 * A (+ 2^-11 |ref| + 2^-25 for fp16 outputs); NaN (an unwritten element) fails.
    Prints the worst err / budget ratio before it asserts."""
    got = got.double().reshape(-1)
    ref = ref.double().reshape(-1)
    bound = C_ACC * U * A.double().reshape(-1)
    if f16:
        bound = bound + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    err = (got - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).nan_to_num(float('inf')).max().item()
    print('RATIO %-28s %s worst err / budget %.4g' % (what, 'f16' if f16 else 'f32', ratio))
    bad = ~(err <= bound)
    nbad = int(bad.sum())
    if nbad:
        i = int(torch.nonzero(bad)[0])
        raise AssertionError('%s: %d of %d elements over budget; first at %d: got %r ref %r budget %.3e '
                             '(worst err / budget %.3g)' % (what, nbad, got.numel(), i, got[i].item(), ref[i].item(),
                                                            bound[i].item(), ratio))


def _equal(a, b, what):
    assert torch.equal(a, b), '%s: two identical calls differ (%d elements)' % (what, int((a != b).sum()))


def _check_ln_fwd(y, mean, rstd, x, w, b, C, what):
    yr, A_y, mu, ma, rs = _ln_fwd_ref(x, w, b, C)
    _within(mean, mu, ma, what + ' mean')
    _within(rstd, rs, rs * (1.0 + ma * rs), what + ' rstd')
    _within(y, yr, A_y, what + ' y', f16=True)


def _norm(C, w, b):
    ln = torch.nn.LayerNorm(C, eps=EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(w)
        ln.bias.copy_(b)
    return ln


class _Drop:
    drop_prob, training = 0.3, True


class _fixed_drop:
    """fused.DROP_POOL.take answers with the given per-image scales (stands in for the pooled drop-path draw)."""

    def __init__(self, sc):
        self.sc = sc

    def __enter__(self):
        from vitadapter import fused
        self.take = fused.DROP_POOL.take
        fused.DROP_POOL.take = lambda x_, keep: self.sc

    def __exit__(self, *exc):
        from vitadapter import fused
        fused.DROP_POOL.take = self.take
        return False


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows,C', LN_SHAPES + LN_CAP_768)
def test_layer_norm_f16(rows, C):
    """Forward, backward without and with the residual-branch gradient gres."""
    from vitadapter import fused
    v = _lib()
    x, w, b = _ln_data(rows, C, 100 + rows % 97)
    g = torch.randn(rows, C, device='cuda').to(F16)
    gres = torch.randn(rows, C, device='cuda')
    st = _stream()
    outs = []
    for _ in range(2):
        gd = _Guarded()
        y, mean, rstd = gd.nan(rows, C, dtype=F16), gd.nan(rows), gd.nan(rows)
        v.check(v.lib.vah_layernorm_fwd_f32_f16(x.data_ptr(), w.data_ptr(), b.data_ptr(), rows, C, EPS, y.data_ptr(),
                                                mean.data_ptr(), rstd.data_ptr(), st), 'layernorm_fwd_f16')
        res = [y, mean, rstd]
        for gr in (None, gres):
            dx, dw, db = gd.nan(rows, C), gd.nan(C), gd.nan(C)
            ws = gd.nan(v.lib.vah_reduce_ws_floats(2 * C))
            v.check(v.lib.vah_layernorm_bwd_f32_f16(x.data_ptr(), g.data_ptr(), w.data_ptr(), mean.data_ptr(),
                                                    rstd.data_ptr(), gr.data_ptr() if gr is not None else None, rows, C,
                                                    dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st),
                    'layernorm_bwd_f16')
            res += [dx, dw, db]
        torch.cuda.synchronize()
        gd.check('layer_norm_f16')
        outs.append(res)
    names = ('y', 'mean', 'rstd', 'dx', 'dw', 'db', 'dx+gres', 'dw (gres)', 'db (gres)')
    for a, c, nm in zip(outs[0], outs[1], names):
        _equal(a, c, nm)
    y, mean, rstd, dx, dw, db, dxr, dwr, dbr = outs[0]
    # the entry points: same kernels, same bits
    ln = _norm(C, w, b)
    xe = x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=F16):
        ye = fused.layer_norm(ln, xe)
    assert type(ye.grad_fn).__name__ == '_LayerNormBF16Backward' and ye.dtype == F16
    ye.backward(g)
    for a, c, nm in ((ye, y, 'y'), (xe.grad, dx, 'dx'), (ln.weight.grad, dw, 'dw'), (ln.bias.grad, db, 'db')):
        assert torch.equal(a, c), 'fused.layer_norm %s differs from the direct call' % nm
    ln.zero_grad(set_to_none=True)
    xe = x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=F16):
        xk, ye = fused.layer_norm_keep(ln, xe * 1.0)
    torch.autograd.backward([xk, ye], [gres, g])
    for a, c, nm in ((ye, y, 'y'), (xe.grad, dxr, 'dx'), (ln.weight.grad, dwr, 'dw'), (ln.bias.grad, dbr, 'db')):
        assert torch.equal(a, c), 'fused.layer_norm_keep %s differs from the direct call' % nm
    del xe, xk, ye, ln
    _check_ln_fwd(y, mean, rstd, x, w, b, C, 'layer_norm')
    for gr, (a, bw, bb), tag in ((None, (dx, dw, db), ''), (gres, (dxr, dwr, dbr), ' +gres')):
        rdx, A_dx, rdw, A_dw, rdb, A_db = _ln_bwd_ref(x, g, w, mean, rstd, gr)
        _within(a, rdx, A_dx, 'layer_norm dx' + tag)
        _within(bw, rdw, A_dw, 'layer_norm dgamma' + tag)
        _within(bb, rdb, A_db, 'layer_norm dbeta' + tag)


def test_layer_norm_f16_keeps_subnormal_outputs():
    """Rows scaled so that |y| is about 2^-16 ... 2^-20, fp16's subnormal range: the store must round them, not flush
    them (a flush misses the 2^-25 term of the budget by up to 2^-16)."""
    v = _lib()
    rows, C = 2048, 768
    x, _, _ = _ln_data(rows, C, 77)
    w = torch.pow(2.0, -16.0 - 4.0 * torch.rand(C, device='cuda')) * torch.where(torch.rand(C, device='cuda') < 0.5, -1.0, 1.0)
    b = torch.randn(C, device='cuda') * 2.0 ** -19
    gd = _Guarded()
    y, mean, rstd = gd.nan(rows, C, dtype=F16), gd.nan(rows), gd.nan(rows)
    v.check(v.lib.vah_layernorm_fwd_f32_f16(x.data_ptr(), w.data_ptr(), b.data_ptr(), rows, C, EPS, y.data_ptr(),
                                            mean.data_ptr(), rstd.data_ptr(), _stream()), 'layernorm_fwd_f16')
    torch.cuda.synchronize()
    gd.check('subnormal rows')
    yr, A_y, _, _, _ = _ln_fwd_ref(x, w, b, C)
    sub = (y != 0) & (y.abs().float() < 2.0 ** -14)
    assert float(sub.float().mean()) > 0.5, 'the case does not produce subnormal outputs'
    _within(y, yr, A_y, 'subnormal y', f16=True)
    # the rounding itself: where the fp32 math is far inside the budget the stored value is the fp16 nearest to the reference
    assert float((y == yr.float().half()).float().mean()) > 0.95


# ---------------------------------------------------------------------------------------------------------------
# residual + LayerNorm: t = x + sc[b] * gamma * z, h = LayerNorm(t)
# ---------------------------------------------------------------------------------------------------------------

RES_VARIANTS = [(r, c, True, True) for r, c in LN_SHAPES + LN_CAP_768 + RES_CAP_1024] + [
    (8192, 768, False, True), (8192, 768, True, False), (43008, 768, False, False), (3200, 1024, False, False)]


@pytest.mark.parametrize('rows,C,with_gamma,with_sc', RES_VARIANTS)
def test_residual_ln_f16(rows, C, with_gamma, with_sc):
    """With / without gamma and the DropPath scales (batch 2 where the rows split evenly, the two images with different
    scales so a wrong batch index shows); the backward with and without the stream gradient gt."""
    from vitadapter import fused
    v = _lib()
    x, w, b = _ln_data(rows, C, 200 + rows % 89)
    batch = 2 if rows % 2 == 0 else 1
    rpb = rows // batch
    z = torch.randn(rows, C, device='cuda').to(F16)
    gamma = torch.randn(C, device='cuda') * 0.5 if with_gamma else None
    sc = torch.tensor([1.0 / 0.7, 0.45][:batch], device='cuda') if with_sc else None
    gh = torch.randn(rows, C, device='cuda').to(F16)
    gt = torch.randn(rows, C, device='cuda')
    gp, sp = (gamma.data_ptr() if with_gamma else None), (sc.data_ptr() if with_sc else None)
    st = _stream()
    outs = []
    for _ in range(2):
        gd = _Guarded()
        t, h, mean, rstd = gd.nan(rows, C), gd.nan(rows, C, dtype=F16), gd.nan(rows), gd.nan(rows)
        v.check(v.lib.vah_residual_layernorm_fwd_f16(x.data_ptr(), z.data_ptr(), gp, sp, batch, rpb, C, w.data_ptr(),
                                                     b.data_ptr(), EPS, t.data_ptr(), h.data_ptr(), mean.data_ptr(),
                                                     rstd.data_ptr(), st), 'residual_layernorm_fwd_f16')
        res = [t, h, mean, rstd]
        for gtt in (gt, None):
            dt, dz = gd.nan(rows, C), gd.nan(rows, C, dtype=F16)
            dgm, dw, db = gd.nan(C), gd.nan(C), gd.nan(C)
            ws = gd.nan(v.lib.vah_reduce_ws_floats(3 * C))
            v.check(v.lib.vah_residual_layernorm_bwd_f16(
                t.data_ptr(), gh.data_ptr(), w.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                gtt.data_ptr() if gtt is not None else None, z.data_ptr(), gp, sp, batch, rpb, C, dt.data_ptr(), dz.data_ptr(),
                dgm.data_ptr() if with_gamma else None, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st),
                'residual_layernorm_bwd_f16')
            res += [dt, dz, dgm, dw, db]
        torch.cuda.synchronize()
        gd.check('residual_ln_f16')
        outs.append(res)
    for k, (a, c) in enumerate(zip(outs[0], outs[1])):
        if not with_gamma and k in (6, 11):       # dgamma is not written without gamma
            assert bool(torch.isnan(a).all())
            continue
        _equal(a, c, 'output %d' % k)
    t, h, mean, rstd, dt, dz, dgm, dw, db, dt0, dz0, dgm0, dw0, db0 = outs[0]
    # the entry point
    ln = _norm(C, w, b)
    xe = x.view(batch, rpb, C).clone().requires_grad_(True)
    ze = z.view(batch, rpb, C).clone().requires_grad_(True)
    ge = gamma.clone().requires_grad_(True) if with_gamma else None
    with _fixed_drop(sc), torch.autocast('cuda', dtype=F16):
        te, he = fused.residual_ln(xe, ze, ge, _Drop() if with_sc else None, ln)
    assert type(he.grad_fn).__name__ == '_ResidualLNBackward' and he.dtype == F16 and te.dtype == torch.float32
    torch.autograd.backward([te, he], [gt.view(batch, rpb, C), gh.view(batch, rpb, C)])
    pairs = [(te, t, 't'), (he, h, 'h'), (xe.grad, dt, 'dx'), (ze.grad, dz, 'dz'), (ln.weight.grad, dw, 'dw'),
             (ln.bias.grad, db, 'db')] + ([(ge.grad, dgm, 'dgamma')] if with_gamma else [])
    for a, c, nm in pairs:
        assert torch.equal(a.reshape(c.shape), c), 'fused.residual_ln %s differs from the direct call' % nm
    del xe, ze, te, he, ln
    scr = sc.double().repeat_interleave(rpb).view(-1, 1) if with_sc else torch.ones(rows, 1, dtype=torch.float64, device='cuda')
    gmd = gamma.double() if with_gamma else torch.ones(C, dtype=torch.float64, device='cuda')
    sgz = scr * gmd * z.double()
    _within(t, x.double() + sgz, x.double().abs() + sgz.abs(), 'residual_ln t')
    _check_ln_fwd(h, mean, rstd, t, w, b, C, 'residual_ln')
    sgd = scr * gmd
    for gtt, (a_dt, a_dz, a_dgm, a_dw, a_db), tag in ((gt, (dt, dz, dgm, dw, db), ''), (None, (dt0, dz0, dgm0, dw0, db0), ' gt=0')):
        rdt, A_dt, rdw, A_dw, rdb, A_db = _ln_bwd_ref(t, gh, w, mean, rstd, gtt)
        _within(a_dt, rdt, A_dt, 'residual_ln dt' + tag)
        _within(a_dz, sgd * rdt, sgd.abs() * A_dt, 'residual_ln dz' + tag, f16=True)
        if with_gamma:       # dgamma = sum sc * dt * z: held to the kernel's own dt (checked above) as the operand
            szd = scr * a_dt.double() * z.double()
            _within(a_dgm, szd.sum(0), szd.abs().sum(0), 'residual_ln dgamma' + tag)
        _within(a_dw, rdw, A_dw, 'residual_ln dw' + tag)
        _within(a_db, rdb, A_db, 'residual_ln db' + tag)


@pytest.mark.parametrize('with_gamma', [True, False])
def test_residual_ln_f16_unused_norm_branch(with_gamma):
    """`gh is None`: the normalised copy is not used, _ResidualLN's backward is the plain scale-residual backward
    (vah_scale_residual_bwd_f16; without gamma its flat scale-only kernel)."""
    from vitadapter import fused
    v = _lib()
    rows, C, batch = 8192, 768, 2
    rpb = rows // batch
    x, w, b = _ln_data(rows, C, 31)
    z = torch.randn(rows, C, device='cuda').to(F16)
    gamma = torch.randn(C, device='cuda') * 0.5 if with_gamma else None
    sc = torch.tensor([1.0 / 0.7, 0.45], device='cuda')
    gt = torch.randn(rows, C, device='cuda')
    gd = _Guarded()
    dz, dgm, ws = gd.nan(rows, C, dtype=F16), gd.nan(C), gd.nan(v.lib.vah_reduce_ws_floats(C))
    v.check(v.lib.vah_scale_residual_bwd_f16(gt.data_ptr(), z.data_ptr(), gamma.data_ptr() if with_gamma else None, sc.data_ptr(),
                                             batch, rpb, C, dz.data_ptr(), dgm.data_ptr() if with_gamma else None,
                                             ws.data_ptr() if with_gamma else None, _stream()), 'scale_residual_bwd_f16')
    torch.cuda.synchronize()
    gd.check('unused norm branch')
    ln = _norm(C, w, b)
    xe = x.view(batch, rpb, C).clone().requires_grad_(True)
    ze = z.view(batch, rpb, C).clone().requires_grad_(True)
    ge = gamma.clone().requires_grad_(True) if with_gamma else None
    with _fixed_drop(sc), torch.autocast('cuda', dtype=F16):
        te, he = fused.residual_ln(xe, ze, ge, _Drop(), ln)
    assert type(te.grad_fn).__name__ == '_ResidualLNBackward'
    te.backward(gt.view(batch, rpb, C))
    assert torch.equal(xe.grad.view(rows, C), gt) and torch.equal(ze.grad.view(rows, C), dz)
    assert ln.weight.grad is None and ln.bias.grad is None
    scr = sc.double().repeat_interleave(rpb).view(-1, 1)
    sg = scr * (gamma.double() if with_gamma else 1.0) * gt.double()
    _within(dz, sg, sg.abs(), 'unused-norm dz', f16=True)
    if with_gamma:
        assert torch.equal(ge.grad, dgm)
        sgz = scr * gt.double() * z.double()
        _within(dgm, sgz.sum(0), sgz.abs().sum(0), 'unused-norm dgamma')


# ---------------------------------------------------------------------------------------------------------------
# two LayerNorms of the same rows
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows,C,drop', [(r, c, None) for r, c in DUAL_SHAPES] + [(8192, 768, 'gb'), (8192, 768, 'gres')])
def test_layer_norm_dual_f16(rows, C, drop):
    from vitadapter import fused
    v = _lib()
    x, wa, ba = _ln_data(rows, C, 300 + rows % 83)
    wb = torch.randn(C, device='cuda') * 0.3 + 1.0
    bb = torch.randn(C, device='cuda') * 0.3
    ga = torch.randn(rows, C, device='cuda').to(F16)
    gb = torch.randn(rows, C, device='cuda').to(F16) if drop != 'gb' else None
    gres = torch.randn(rows, C, device='cuda') if drop != 'gres' else None
    st = _stream()
    outs = []
    for _ in range(2):
        gd = _Guarded()
        ya, yb = gd.nan(rows, C, dtype=F16), gd.nan(rows, C, dtype=F16)
        mean, rstd = gd.nan(rows), gd.nan(rows)
        v.check(v.lib.vah_layernorm_dual_fwd_f16(x.data_ptr(), wa.data_ptr(), ba.data_ptr(), wb.data_ptr(), bb.data_ptr(),
                                                 rows, C, EPS, ya.data_ptr(), yb.data_ptr(), mean.data_ptr(),
                                                 rstd.data_ptr(), st), 'layernorm_dual_fwd_f16')
        dx, dp = gd.nan(rows, C), gd.nan(4, C)
        ws = gd.nan(v.lib.vah_reduce_ws_floats(2 * C))
        v.check(v.lib.vah_layernorm_dual_bwd_f16(x.data_ptr(), ga.data_ptr(), gb.data_ptr() if gb is not None else None,
                                                 wa.data_ptr(), wb.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                                 gres.data_ptr() if gres is not None else None, rows, C, dx.data_ptr(),
                                                 dp.data_ptr(), ws.data_ptr(), st), 'layernorm_dual_bwd_f16')
        torch.cuda.synchronize()
        gd.check('layer_norm_dual_f16')
        outs.append((ya, yb, mean, rstd, dx, dp))
    for a, c, nm in zip(outs[0], outs[1], ('ya', 'yb', 'mean', 'rstd', 'dx', 'dparams')):
        _equal(a, c, nm)
    ya, yb, mean, rstd, dx, dp = outs[0]
    na, nb = _norm(C, wa, ba), _norm(C, wb, bb)
    xe = x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=F16):
        xk, yae, ybe = fused.layer_norm_dual_keep(na, nb, xe * 1.0)
    assert type(yae.grad_fn).__name__ == '_LayerNormDualBF16Backward' and yae.dtype == F16 and ybe.dtype == F16
    heads = [(t_, g_) for t_, g_ in ((xk, gres), (yae, ga), (ybe, gb)) if g_ is not None]
    torch.autograd.backward([h_[0] for h_ in heads], [h_[1] for h_ in heads])
    for a, c, nm in ((yae, ya, 'ya'), (ybe, yb, 'yb'), (xe.grad, dx, 'dx'), (na.weight.grad, dp[0], 'dwa'),
                     (na.bias.grad, dp[1], 'dba'), (nb.weight.grad, dp[2], 'dwb'), (nb.bias.grad, dp[3], 'dbb')):
        assert torch.equal(a, c), 'fused.layer_norm_dual_keep %s differs from the direct call' % nm
    del xe, xk, yae, ybe
    _check_ln_fwd(ya, mean, rstd, x, wa, ba, C, 'dual a')
    _check_ln_fwd(yb, mean, rstd, x, wb, bb, C, 'dual b')
    gbz = gb if gb is not None else torch.zeros(rows, C, dtype=F16, device='cuda')
    dxa, A_a, dwa, A_wa, dba, A_ba = _ln_bwd_ref(x, ga, wa, mean, rstd, gres)
    dxb, A_b, dwb, A_wb, dbb, A_bb = _ln_bwd_ref(x, gbz, wb, mean, rstd, None)
    _within(dx, dxa + dxb, A_a + A_b, 'dual dx')
    for got, ref, A, nm in ((dp[0], dwa, A_wa, 'dwa'), (dp[1], dba, A_ba, 'dba'), (dp[2], dwb, A_wb, 'dwb'),
                            (dp[3], dbb, A_bb, 'dbb')):
        _within(got, ref, A, 'dual ' + nm)


# ---------------------------------------------------------------------------------------------------------------
# scale_residual: y = x + sc[b] * gamma * z; backward dz = sc * gamma * g, dgamma = sum sc * g * z
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows,C,with_gamma', [(43008, 768, True), (16800, 1024, True), (43008, 768, False)])
def test_scale_residual_f16(rows, C, with_gamma):
    from vitadapter import fused
    v = _lib()
    torch.manual_seed(400 + C)
    batch, rpb = 2, rows // 2
    x = torch.randn(rows, C, device='cuda')
    z = torch.randn(rows, C, device='cuda').to(F16)
    gamma = torch.randn(C, device='cuda') * 0.5 if with_gamma else None
    gp = gamma.data_ptr() if with_gamma else None
    sc = torch.tensor([1.0 / 0.7, 0.45], device='cuda')
    g = torch.randn(rows, C, device='cuda')
    st = _stream()
    outs = []
    for _ in range(2):
        gd = _Guarded()
        y = gd.nan(rows, C)
        v.check(v.lib.vah_scale_residual_fwd_f16(x.data_ptr(), z.data_ptr(), gp, sc.data_ptr(), batch, rpb, C,
                                                 y.data_ptr(), st), 'scale_residual_fwd_f16')
        dz, dgm = gd.nan(rows, C, dtype=F16), gd.nan(C)
        ws = gd.nan(v.lib.vah_reduce_ws_floats(C))
        v.check(v.lib.vah_scale_residual_bwd_f16(g.data_ptr(), z.data_ptr(), gp, sc.data_ptr(), batch, rpb, C, dz.data_ptr(),
                                                 dgm.data_ptr() if with_gamma else None, ws.data_ptr() if with_gamma else None,
                                                 st), 'scale_residual_bwd_f16')
        torch.cuda.synchronize()
        gd.check('scale_residual_f16')
        outs.append((y, dz, dgm))
    _equal(outs[0][0], outs[1][0], 'y')
    _equal(outs[0][1], outs[1][1], 'dz')
    if with_gamma:
        _equal(outs[0][2], outs[1][2], 'dgamma')
    y, dz, dgm = outs[0]
    xe = x.view(batch, rpb, C).clone().requires_grad_(True)
    ze = z.view(batch, rpb, C).clone().requires_grad_(True)
    ge = gamma.clone().requires_grad_(True) if with_gamma else None
    with _fixed_drop(sc), torch.autocast('cuda', dtype=F16):
        ye = fused.residual(xe, ze, ge, _Drop())
    assert type(ye.grad_fn).__name__ == '_ScaleResidualBackward'
    ye.backward(g.view(batch, rpb, C))
    for a, c, nm in [(ye, y, 'y'), (ze.grad, dz, 'dz')] + ([(ge.grad, dgm, 'dgamma')] if with_gamma else []):
        assert torch.equal(a.reshape(c.shape), c), 'fused.residual %s differs from the direct call' % nm
    del xe, ze, ye
    scr = sc.double().repeat_interleave(rpb).view(-1, 1)
    gmd = gamma.double() if with_gamma else 1.0
    sgz = scr * gmd * z.double()
    _within(y, x.double() + sgz, x.double().abs() + sgz.abs(), 'scale_residual y')
    sg = scr * gmd * g.double()
    _within(dz, sg, sg.abs(), 'scale_residual dz', f16=True)
    if with_gamma:
        sgz = scr * g.double() * z.double()
        _within(dgm, sgz.sum(0), sgz.abs().sum(0), 'scale_residual dgamma')


def _conversion_operands(n):
    """fp32 values whose conversion to fp16 tells the rounding rules apart: (a) fp16's subnormal range and below,
    (b) beyond 65504 in both signs next to ordinary values, (c) exact ties between two fp16 neighbours, normal and
    subnormal, (d) random normals."""
    dev = 'cuda'
    k = n // 4
    sign = lambda m: torch.where(torch.rand(m, device=dev) < 0.5, -1.0, 1.0)
    a = sign(k) * (1.0 + torch.rand(k, device=dev)) * torch.pow(2.0, torch.randint(-27, -14, (k,), device=dev).float())
    big = torch.tensor([65504.0, 65519.0, 65519.996, 65520.0, 65521.0, 65536.0, 7.0e4, 1.0e5, 3.0e38, float('inf')], device=dev)
    b = torch.randn(k, device=dev)
    idx = torch.arange(0, k, 3, device=dev)
    b[idx] = (big[torch.arange(idx.numel(), device=dev) % big.numel()]) * sign(idx.numel())
    # ties: the midpoint of an fp16 value and its successor is exact in fp32 (12 significant bits at most)
    h = (torch.randn(k // 2, device=dev) * 8.0).half()
    hn = (h.view(torch.int16) + 1).view(F16)              # next fp16 away from zero (same sign)
    ok = torch.isfinite(hn)
    c1 = torch.where(ok, (h.float() + hn.float()) * 0.5, h.float())
    ks = torch.randint(0, 1024, (k - k // 2,), device=dev).float()
    c2 = sign(k - k // 2) * (ks * 2.0 ** -24 + 2.0 ** -25)
    d = torch.randn(n - 3 * k, device=dev) * 3.0
    return torch.cat([a, b, c1, c2, d])


@pytest.mark.parametrize('kernel', ['scale_only', 'scale_residual'])
def test_f16_conversion_is_torchs(kernel):
    """dz = s * gamma * g with s absent and gamma absent (scale_only_bwd_kernel) or all ones (scale_residual_bwd_kernel)
    is the conversion of the fp32 g and nothing else: it must equal g.to(float16) bit for bit - round to nearest even,
    overflow to +-inf (not 65504), subnormals kept (not flushed), no NaN."""
    v = _lib()
    torch.manual_seed(9)
    batch, rpb, C = 2, 2048, 768
    rows = batch * rpb
    g = _conversion_operands(rows * C)
    g = g[torch.randperm(g.numel(), device='cuda')].view(rows, C).contiguous()
    z = torch.randn(rows, C, device='cuda').to(F16)
    gamma = torch.ones(C, device='cuda') if kernel == 'scale_residual' else None
    want = g.to(F16)
    assert bool(torch.isinf(want).any()) and bool(((want != 0) & (want.abs().float() < 2.0 ** -14)).any())
    assert not bool(torch.isnan(want).any())
    gd = _Guarded()
    dz, dgm, ws = gd.nan(rows, C, dtype=F16), gd.nan(C), gd.nan(v.lib.vah_reduce_ws_floats(C))
    v.check(v.lib.vah_scale_residual_bwd_f16(g.data_ptr(), z.data_ptr(), gamma.data_ptr() if gamma is not None else None, None,
                                             batch, rpb, C, dz.data_ptr(), dgm.data_ptr() if gamma is not None else None,
                                             ws.data_ptr() if gamma is not None else None, _stream()), 'scale_residual_bwd_f16')
    torch.cuda.synchronize()
    gd.check('conversion')
    diff = dz.view(torch.int16) != want.view(torch.int16)
    if bool(diff.any()):
        i = int(torch.nonzero(diff.reshape(-1))[0])
        raise AssertionError('%d of %d conversions differ from torch; first: g %r -> %r, torch %r' % (
            int(diff.sum()), diff.numel(), g.reshape(-1)[i].item(), dz.reshape(-1)[i].item(), want.reshape(-1)[i].item()))
    assert torch.equal(dz.view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------
# DWConv 3x3 on the concatenated token maps
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,H,W,C', [(2, 32, 32, 48), (2, 64, 64, 192), (2, 40, 40, 256), (1, 50, 84, 256)])
def test_dwconv_tokens_f16(B, H, W, C):
    from vitadapter import fused
    v = _lib()
    torch.manual_seed(500 + C + H)
    N = 21 * (H // 2) * (W // 2)
    x = torch.randn(B, N, C, device='cuda').to(F16)
    g = torch.randn(B, N, C, device='cuda').to(F16)
    w9 = torch.randn(C, 9, device='cuda') * 0.3
    bias = torch.randn(C, device='cuda') * 0.3
    st = _stream()
    outs = []
    for _ in range(2):
        gd = _Guarded()
        y, dx = gd.nan(B, N, C, dtype=F16), gd.nan(B, N, C, dtype=F16)
        v.check(v.lib.vah_dwconv3x3_tokens_f16(x.data_ptr(), w9.data_ptr(), bias.data_ptr(), B, H, W, C, 0, y.data_ptr(), st),
                'dwconv_fwd_f16')
        v.check(v.lib.vah_dwconv3x3_tokens_f16(g.data_ptr(), w9.data_ptr(), None, B, H, W, C, 1, dx.data_ptr(), st),
                'dwconv_dgrad_f16')
        dw, db = gd.nan(C * 9), gd.nan(C)
        ws = gd.nan(v.lib.vah_reduce_ws_floats(10 * C))
        v.check(v.lib.vah_dwconv3x3_tokens_wgrad_f16(x.data_ptr(), g.data_ptr(), B, H, W, C, dw.data_ptr(), db.data_ptr(),
                                                     ws.data_ptr(), st), 'dwconv_wgrad_f16')
        torch.cuda.synchronize()
        gd.check('dwconv_tokens_f16')
        outs.append((y, dx, dw, db))
    for a, c, nm in zip(outs[0], outs[1], ('y', 'dx', 'dw', 'db')):
        _equal(a, c, nm)
    y, dx, dw, db = outs[0]
    conv = torch.nn.Conv2d(C, C, 3, padding=1, groups=C).cuda()
    with torch.no_grad():
        conv.weight.copy_(w9.view(C, 1, 3, 3))
        conv.bias.copy_(bias)
    xe = x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=F16):
        ye = fused.dwconv_tokens(conv, xe, H, W)
    assert ye is not None and type(ye.grad_fn).__name__ == '_DWConvTokensBackward' and ye.dtype == F16
    ye.backward(g)
    for a, c, nm in ((ye, y, 'y'), (xe.grad, dx, 'dx'), (conv.weight.grad.reshape(-1), dw, 'dw'),
                     (conv.bias.grad, db, 'db')):
        assert torch.equal(a, c), 'fused.dwconv_tokens %s differs from the direct call' % nm
    del xe, ye, conv
    ry, Ay, rdx, Adx, rdw, Adw, rdb, Adb = _dwconv_ref(x, g, w9, bias, H, W)
    _within(y, ry, Ay, 'dwconv y', f16=True)
    _within(dx, rdx, Adx, 'dwconv dx', f16=True)
    _within(dw, rdw, Adw, 'dwconv dw')
    _within(db, rdb, Adb, 'dwconv db')


# ---------------------------------------------------------------------------------------------------------------
# host gates
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('z_dtype,ac_dtype', [(torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)])
def test_residual_ln_type_mismatch_takes_torch(z_dtype, ac_dtype):
    """A branch output in the other 16-bit type than the active autocast: fused.residual_ln returns the torch
    expression's result and launches none of the fused row kernels."""
    from vitadapter import fused
    v = _lib()
    torch.manual_seed(3)
    B, T, C = 2, 320, 768
    x = torch.randn(B, T, C, device='cuda', requires_grad=True)
    z = torch.randn(B, T, C, device='cuda').to(z_dtype).requires_grad_(True)
    gamma = (torch.randn(C, device='cuda') * 0.5).requires_grad_(True)
    ln = torch.nn.LayerNorm(C, eps=EPS).cuda()
    v.prof_enable(True, FAMILIES)
    try:
        with torch.autocast('cuda', dtype=ac_dtype):
            t, h = fused.residual_ln(x, z, gamma, None, ln)
            (t.sum() + h.float().sum()).backward()
        torch.cuda.synchronize()
    finally:
        v.prof_enable(False)
    assert v.prof_report() == {}
    got = [t.detach(), h.detach(), x.grad.clone(), z.grad.clone(), gamma.grad.clone(), ln.weight.grad.clone()]
    for p in (x, z, gamma, ln.weight, ln.bias):
        p.grad = None
    with torch.autocast('cuda', dtype=ac_dtype):
        tw = x + gamma * z
        hw = ln(tw)
        (tw.sum() + hw.float().sum()).backward()
    want = [tw.detach(), hw.detach(), x.grad, z.grad, gamma.grad, ln.weight.grad]
    for a, c, nm in zip(got, want, ('t', 'h', 'dx', 'dz', 'dgamma', 'dw')):
        assert a.dtype == c.dtype and torch.equal(a, c), nm
    assert bool(torch.isfinite(got[1]).all())


def test_fp16_rows_switch_turns_only_the_fp16_gates_off():
    from vitadapter import fused
    v = _lib()
    torch.manual_seed(4)
    B, T, C = 2, 336, 192
    x = torch.randn(B, T, C, device='cuda')
    ln = torch.nn.LayerNorm(C, eps=EPS).cuda()
    conv = torch.nn.Conv2d(48, 48, 3, padding=1, groups=48).cuda()
    rows = {}
    for on in (True, False):
        fused.ENABLED['fp16_rows'] = on
        try:
            for dt in (F16, torch.bfloat16):
                z = torch.randn(B, T, C, device='cuda').to(dt)
                tok = torch.randn(B, 21 * 16, 48, device='cuda').to(dt)
                v.prof_enable(True, FAMILIES)
                with torch.autocast('cuda', dtype=dt):
                    fused.layer_norm(ln, x)
                    fused.layer_norm_keep(ln, x)
                    fused.layer_norm_dual_keep(ln, ln, x)
                    fused.residual(x, z)
                    fused.residual_ln(x, z, None, None, ln)
                    y = fused.dwconv_tokens(conv, tok, 8, 8)
                torch.cuda.synchronize()
                v.prof_enable(False)
                rows[on, dt] = (sorted(v.prof_report()), y is not None)
        finally:
            fused.ENABLED['fp16_rows'] = True
            v.prof_enable(False)
    bf = ['dwconv_tokens_fwd', 'layernorm_dual_fwd', 'layernorm_fwd', 'residual_layernorm_fwd', 'scale_residual_fwd']
    assert rows[True, torch.bfloat16] == rows[False, torch.bfloat16] == (bf, True)
    assert rows[True, F16] == ([r + '_f16' for r in bf], True)
    assert rows[False, F16] == ([], False)
