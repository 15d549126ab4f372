"""GPU: the hand-written reductions of the bf16 training step held to fp64 at the production row counts of
BASELINE configs[1]-[4] and at the grid caps of their kernels (kMaxParts = 512 partial rows).

Every case computes its reference in fp64 on the GPU from the exact operands the kernel saw (bf16 inputs
upcast, fp32 inputs as they are; a backward is checked against the kernel's own fp32 mean / rstd).  Each
output element gets its own budget from the data:

    |got - ref| <= C_ACC * 2^-24 * A   (+ 2^-8 * |ref| where the output is bf16)

with A the sum of the absolute values of the terms that form the element (dW: |g|^T |x|, db: sum |g|,
dgamma: sum |g * xhat|, LayerNorm dx: the row's |terms| of its formula).  C_ACC = 64.  Why that is enough:
an fp32 sum whose longest chain of dependent additions is d terms long is off by at most d * 2^-24 * A.
The longest chains here: a LayerNorm backward wave walks ceil(rows / (512 * 8)) = 11 rows at 43 008 rows,
its workgroup adds 8 wave rows, finalize_partials adds 512 / 64 = 8 per accumulator, 3 in its tree and 8
across lanes (38); the dual LayerNorm walks 42 rows on its 256-workgroup grid (42 + 2 + 4 + 3 + 8 = 59);
the DWConv wgrad 17 tokens per slot + 5 slots + 19; the colsum strips 11 + 8 + 19.  The product that
forms a term adds at most 3 roundings (xhat = (x - mean) * rstd, times g).  For the hipBLASLt GEMMs the
order is the library's: a slice of K / split rows accumulates in the matrix cores.  Zero-mean operands make
those partial sums random walks, and the expected error is then about 2^-24 * sqrt(K / split) * |partial|,
orders of magnitude below 64 * 2^-24 * A.  At 43 008 rows one dropped row is worth about 1 sigma of an
element, the budget about 0.1 sigma: a missing row, K slice or partial row fails the case.  (Measured on an
MI355X: the fp32 reductions stay below 0.05 of their budgets.  The bf16 outputs reach 0.995 of theirs, as they
should: 2^-8 |ref| is the round-to-nearest bound of bf16 itself.)

Outputs and every partial-row buffer are filled with NaN before the call (the GEMM's split-K region too:
[0, split * M * N * 4) at the front of its workspace), every case runs twice and must give the same bits,
and every family with a fused.* entry point also runs through it, which must give the same bits as the direct
call (bf16 column sums and the BN-tail statistics are checked through the C ABI alone).
The Linear cases must run the committed GEMM table entry: no live tuning.  Acceptance check for any
replacement of fused._wgrad_bgrad or reduce_splits."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C_ACC = 64
U = 2.0 ** -24
NAN = float('nan')
EPS = 1e-6

TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'vit-adapter_amd', 'tuning',
                     'gemm_table_mi355x_base_det_1024.txt')


def _wgrad_rows():
    """(M, N, K, index, split) of every weight-gradient row ('1 0 1 0 0 ...') of the committed table."""
    out = []
    with open(TABLE) as f:
        for line in f:
            v = line.split()
            if v[:5] == ['1', '0', '1', '0', '0']:
                out.append(tuple(int(t) for t in (v[5], v[6], v[7], v[11], v[12])))
    return out


# Production shapes.  ViT tokens = (H/16)(W/16), adapter tokens = 21 (H/32)(W/32) (maps at strides 8, 16, 32),
# rows = batch x tokens, ConvFFN hidden = 0.25 C.
#   configs[1] ViT-Adapter-T  512^2, batch 2, C 192:   ViT 2 * 32 * 32 = 2 048,  adapter 2 * 21 * 16 * 16 = 10 752
#   configs[2] ViT-Adapter-B 1024^2, batch 2, C 768:   ViT 2 * 64 * 64 = 8 192,  adapter 2 * 21 * 32 * 32 = 43 008
#   configs[3] ViT-Adapter-L  640^2, batch 2, C 1 024: ViT 2 * 40 * 40 = 3 200,  adapter 2 * 21 * 20 * 20 = 16 800
#   configs[4] ViT-Adapter-L 800 x 1344, batch 1, C 1 024: ViT 50 * 84 = 4 200, adapter 21 * 25 * 42 = 22 050
LN_SHAPES = [(2048, 192), (8192, 768), (43008, 768), (3200, 1024), (16800, 1024), (22050, 1024)]
LN_CAP_768 = [(4095, 768), (4096, 768), (4097, 768)]          # 512 workgroups x 8 waves = 4 096 rows
RES_CAP_1024 = [(2047, 1024), (2048, 1024), (2049, 1024)]     # [dw|db|dgamma] at C 1 024: 4 waves, cap 2 048 rows
DUAL_SHAPES = [(43008, 768), (10752, 192), (1023, 768), (1024, 768), (1025, 768)]   # 10 752 = 2 * 21 * 16 * 16
COLSUM_CAP = [(16383, 768), (16384, 768), (16385, 768)]       # 512 strips of 32 rows = 16 384


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    import _vah
    return _vah


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device='cuda')


def _within(got, ref, A, what, bf16=False):
    """Per-element budget C_ACC * 2^-24 * A (+ 2^-8 |ref| for bf16 outputs); NaN (an unwritten element) fails."""
    got = got.double().reshape(-1)
    ref = ref.double().reshape(-1)
    bound = C_ACC * U * A.double().reshape(-1)
    if bf16:
        bound = bound + 2.0 ** -8 * ref.abs()
    err = (got - ref).abs()
    bad = ~(err <= bound)
    nbad = int(bad.sum())
    if nbad:
        i = int(torch.nonzero(bad)[0])
        ratio = (err / bound.clamp_min(1e-300)).nan_to_num(float('inf')).max().item()
        raise AssertionError('%s: %d of %d elements over budget; first at %d: got %r ref %r budget %.3e '
                             '(worst err / budget %.3g)' % (what, nbad, got.numel(), i, got[i].item(), ref[i].item(),
                                                            bound[i].item(), ratio))


def _equal(a, b, what):
    assert torch.equal(a, b), '%s: two identical calls differ (%d elements)' % (what, int((a != b).sum()))


def _ln_data(rows, C, seed):
    torch.manual_seed(seed)
    x = torch.randn(rows, C, device='cuda') * 1.7 + 0.4
    w = torch.randn(C, device='cuda') * 0.3 + 1.0
    b = torch.randn(C, device='cuda') * 0.3
    return x, w, b


def _ln_fwd_ref(x, w, b, C):
    """fp64 LayerNorm statistics and output of fp32 rows; with the budgets of y, mean, rstd."""
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + EPS)
    xh = (xd - mu) * rs
    wd, bd = w.double(), b.double()
    ma = xd.abs().mean(1, keepdim=True)
    A_y = wd.abs() * (xh.abs() + rs * ma) + bd.abs()
    return xh * wd + bd, A_y, mu.view(-1), ma.view(-1), rs.view(-1)


def _check_ln_fwd(y, mean, rstd, x, w, b, C, what):
    yr, A_y, mu, ma, rs = _ln_fwd_ref(x, w, b, C)
    _within(mean, mu, ma, what + ' mean')
    # two-pass variance: rstd relative error of the order of the mean's, scaled by mean|x| / std
    _within(rstd, rs, rs * (1.0 + ma * rs), what + ' rstd')
    _within(y, yr, A_y, what + ' y', bf16=True)


def _ln_bwd_ref(x, g, w, mean, rstd, gres):
    """LayerNorm backward in fp64 from the kernel's operands (its fp32 mean / rstd): dx, dw, db and budgets."""
    xd, gd, wd = x.double(), g.double(), w.double()
    mu, rs = mean.double().view(-1, 1), rstd.double().view(-1, 1)
    xh = (xd - mu) * rs
    gw = gd * wd
    m1 = gw.mean(1, keepdim=True)
    m2 = (gw * xh).mean(1, keepdim=True)
    dx = rs * (gw - m1 - xh * m2)
    A_dx = rs * (gw.abs() + gw.abs().mean(1, keepdim=True) + xh.abs() * (gw * xh).abs().mean(1, keepdim=True))
    if gres is not None:
        dx = dx + gres.double()
        A_dx = A_dx + gres.double().abs()
    dw = (gd * xh).sum(0)
    A_dw = (gd * xh).abs().sum(0)
    return dx, A_dx, dw, A_dw, gd.sum(0), gd.abs().sum(0)


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows,C', LN_SHAPES + LN_CAP_768)
def test_layer_norm_fullsize(rows, C):
    from vitadapter import fused
    v = _lib()
    x, w, b = _ln_data(rows, C, 100 + rows % 97)
    g = torch.randn(rows, C, device='cuda').to(torch.bfloat16)
    st = _stream()
    outs = []
    for _ in range(2):
        y, mean, rstd = _nan(rows, C, dtype=torch.bfloat16), _nan(rows), _nan(rows)
        v.check(v.lib.vah_layernorm_fwd_f32_bf16(x.data_ptr(), w.data_ptr(), b.data_ptr(), rows, C, EPS, y.data_ptr(),
                                                 mean.data_ptr(), rstd.data_ptr(), st), 'layernorm_fwd')
        dx, dw, db = _nan(rows, C), _nan(C), _nan(C)
        ws = _nan(v.lib.vah_reduce_ws_floats(2 * C))
        v.check(v.lib.vah_layernorm_bwd_f32_bf16(x.data_ptr(), g.data_ptr(), w.data_ptr(), mean.data_ptr(),
                                                 rstd.data_ptr(), None, rows, C, dx.data_ptr(), dw.data_ptr(),
                                                 db.data_ptr(), ws.data_ptr(), st), 'layernorm_bwd')
        outs.append((y, mean, rstd, dx, dw, db))
    for a, c, nm in zip(outs[0], outs[1], ('y', 'mean', 'rstd', 'dx', 'dw', 'db')):
        _equal(a, c, nm)
    y, mean, rstd, dx, dw, db = outs[0]
    # the entry point: same kernels, same bits
    ln = torch.nn.LayerNorm(C, eps=EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(w)
        ln.bias.copy_(b)
    xe = x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        ye = fused.layer_norm(ln, xe)
    assert type(ye.grad_fn).__name__ == '_LayerNormBF16Backward'
    ye.backward(g)
    for a, c, nm in ((ye, y, 'y'), (xe.grad, dx, 'dx'), (ln.weight.grad, dw, 'dw'), (ln.bias.grad, db, 'db')):
        assert torch.equal(a, c), 'fused.layer_norm %s differs from the direct call' % nm
    del xe, ye, ln
    _check_ln_fwd(y, mean, rstd, x, w, b, C, 'layer_norm')
    rdx, A_dx, rdw, A_dw, rdb, A_db = _ln_bwd_ref(x, g, w, mean, rstd, None)
    _within(dx, rdx, A_dx, 'layer_norm dx')
    _within(dw, rdw, A_dw, 'layer_norm dgamma')
    _within(db, rdb, A_db, 'layer_norm dbeta')


# ---------------------------------------------------------------------------------------------------------------
# residual + LayerNorm: t = x + sc[b] * gamma * z, h = LayerNorm(t)
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows,C', LN_SHAPES + LN_CAP_768 + RES_CAP_1024)
def test_residual_ln_fullsize(rows, C):
    """With gamma and drop-path scales: batch 2 where the rows split evenly (else 1), the two images with
    different scales (1/0.7 as DropPath(0.3) keeps an image, and 0.45) so a wrong batch index shows."""
    from vitadapter import fused
    v = _lib()
    x, w, b = _ln_data(rows, C, 200 + rows % 89)
    batch = 2 if rows % 2 == 0 else 1
    rpb = rows // batch
    z = torch.randn(rows, C, device='cuda').to(torch.bfloat16)
    gamma = torch.randn(C, device='cuda') * 0.5
    sc = torch.tensor([1.0 / 0.7, 0.45][:batch], device='cuda')
    gh = torch.randn(rows, C, device='cuda').to(torch.bfloat16)
    gt = torch.randn(rows, C, device='cuda')
    st = _stream()
    outs = []
    for _ in range(2):
        t, h, mean, rstd = _nan(rows, C), _nan(rows, C, dtype=torch.bfloat16), _nan(rows), _nan(rows)
        v.check(v.lib.vah_residual_layernorm_fwd(x.data_ptr(), z.data_ptr(), gamma.data_ptr(), sc.data_ptr(), batch, rpb,
                                                 C, w.data_ptr(), b.data_ptr(), EPS, t.data_ptr(), h.data_ptr(),
                                                 mean.data_ptr(), rstd.data_ptr(), st), 'residual_layernorm_fwd')
        dt, dz = _nan(rows, C), _nan(rows, C, dtype=torch.bfloat16)
        dgm, dw, db = _nan(C), _nan(C), _nan(C)
        ws = _nan(v.lib.vah_reduce_ws_floats(3 * C))
        v.check(v.lib.vah_residual_layernorm_bwd(t.data_ptr(), gh.data_ptr(), w.data_ptr(), mean.data_ptr(),
                                                 rstd.data_ptr(), gt.data_ptr(), z.data_ptr(), gamma.data_ptr(),
                                                 sc.data_ptr(), batch, rpb, C, dt.data_ptr(), dz.data_ptr(),
                                                 dgm.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st),
                'residual_layernorm_bwd')
        outs.append((t, h, mean, rstd, dt, dz, dgm, dw, db))
    for a, c, nm in zip(outs[0], outs[1], ('t', 'h', 'mean', 'rstd', 'dt', 'dz', 'dgamma', 'dw', 'db')):
        _equal(a, c, nm)
    t, h, mean, rstd, dt, dz, dgm, dw, db = outs[0]
    # the entry point, with the same per-image scales standing in for the pooled drop-path draw
    ln = torch.nn.LayerNorm(C, eps=EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(w)
        ln.bias.copy_(b)
    xe = x.view(batch, rpb, C).clone().requires_grad_(True)
    ze = z.view(batch, rpb, C).clone().requires_grad_(True)
    ge = gamma.clone().requires_grad_(True)

    class _Drop:
        drop_prob, training = 0.3, True
    take = fused.DROP_POOL.take
    fused.DROP_POOL.take = lambda x_, keep: sc
    try:
        with torch.autocast('cuda', dtype=torch.bfloat16):
            te, he = fused.residual_ln(xe, ze, ge, _Drop(), ln)
    finally:
        fused.DROP_POOL.take = take
    assert type(he.grad_fn).__name__ == '_ResidualLNBackward'
    torch.autograd.backward([te, he], [gt.view(batch, rpb, C), gh.view(batch, rpb, C)])
    for a, c, nm in ((te, t, 't'), (he, h, 'h'), (xe.grad, dt, 'dx'), (ze.grad, dz, 'dz'), (ge.grad, dgm, 'dgamma'),
                     (ln.weight.grad, dw, 'dw'), (ln.bias.grad, db, 'db')):
        assert torch.equal(a.reshape(c.shape), c), 'fused.residual_ln %s differs from the direct call' % nm
    del xe, ze, te, he, ln
    # forward: t in fp32 from x, z, gamma, sc; h = LayerNorm(t)
    scr = sc.double().repeat_interleave(rpb).view(-1, 1)
    sgz = scr * gamma.double() * z.double()
    _within(t, x.double() + sgz, x.double().abs() + sgz.abs(), 'residual_ln t')
    _check_ln_fwd(h, mean, rstd, t, w, b, C, 'residual_ln')
    # backward from the kernel's t, mean, rstd
    rdt, A_dt, rdw, A_dw, rdb, A_db = _ln_bwd_ref(t, gh, w, mean, rstd, gt)
    _within(dt, rdt, A_dt, 'residual_ln dt')
    sgd = scr * gamma.double()
    _within(dz, sgd * rdt, sgd.abs() * A_dt, 'residual_ln dz', bf16=True)
    # dgamma = sum sc * dt * z over the rows: held to the kernel's own dt (checked above) as the operand
    szd = scr * dt.double() * z.double()
    _within(dgm, szd.sum(0), szd.abs().sum(0), 'residual_ln dgamma')
    _within(dw, rdw, A_dw, 'residual_ln dw')
    _within(db, rdb, A_db, 'residual_ln db')


# ---------------------------------------------------------------------------------------------------------------
# two LayerNorms of the same rows
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows,C', DUAL_SHAPES)
def test_layer_norm_dual_fullsize(rows, C):
    from vitadapter import fused
    v = _lib()
    x, wa, ba = _ln_data(rows, C, 300 + rows % 83)
    wb = torch.randn(C, device='cuda') * 0.3 + 1.0
    bb = torch.randn(C, device='cuda') * 0.3
    ga = torch.randn(rows, C, device='cuda').to(torch.bfloat16)
    gb = torch.randn(rows, C, device='cuda').to(torch.bfloat16)
    gres = torch.randn(rows, C, device='cuda')
    st = _stream()
    outs = []
    for _ in range(2):
        ya, yb = _nan(rows, C, dtype=torch.bfloat16), _nan(rows, C, dtype=torch.bfloat16)
        mean, rstd = _nan(rows), _nan(rows)
        v.check(v.lib.vah_layernorm_dual_fwd(x.data_ptr(), wa.data_ptr(), ba.data_ptr(), wb.data_ptr(), bb.data_ptr(),
                                             rows, C, EPS, ya.data_ptr(), yb.data_ptr(), mean.data_ptr(),
                                             rstd.data_ptr(), st), 'layernorm_dual_fwd')
        dx, dp = _nan(rows, C), _nan(4, C)
        ws = _nan(v.lib.vah_reduce_ws_floats(2 * C))
        v.check(v.lib.vah_layernorm_dual_bwd(x.data_ptr(), ga.data_ptr(), gb.data_ptr(), wa.data_ptr(), wb.data_ptr(),
                                             mean.data_ptr(), rstd.data_ptr(), gres.data_ptr(), rows, C, dx.data_ptr(),
                                             dp.data_ptr(), ws.data_ptr(), st), 'layernorm_dual_bwd')
        outs.append((ya, yb, mean, rstd, dx, dp))
    for a, c, nm in zip(outs[0], outs[1], ('ya', 'yb', 'mean', 'rstd', 'dx', 'dparams')):
        _equal(a, c, nm)
    ya, yb, mean, rstd, dx, dp = outs[0]
    na, nb = torch.nn.LayerNorm(C, eps=EPS).cuda(), torch.nn.LayerNorm(C, eps=EPS).cuda()
    with torch.no_grad():
        na.weight.copy_(wa)
        na.bias.copy_(ba)
        nb.weight.copy_(wb)
        nb.bias.copy_(bb)
    xe = x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        xk, yae, ybe = fused.layer_norm_dual_keep(na, nb, xe * 1.0)
    assert type(yae.grad_fn).__name__ == '_LayerNormDualBF16Backward'
    torch.autograd.backward([xk, yae, ybe], [gres, ga, gb])
    for a, c, nm in ((yae, ya, 'ya'), (ybe, yb, 'yb'), (xe.grad, dx, 'dx'), (na.weight.grad, dp[0], 'dwa'),
                     (na.bias.grad, dp[1], 'dba'), (nb.weight.grad, dp[2], 'dwb'), (nb.bias.grad, dp[3], 'dbb')):
        assert torch.equal(a, c), 'fused.layer_norm_dual_keep %s differs from the direct call' % nm
    del xe, xk, yae, ybe
    _check_ln_fwd(ya, mean, rstd, x, wa, ba, C, 'dual a')
    _check_ln_fwd(yb, mean, rstd, x, wb, bb, C, 'dual b')
    # dx = gres + LN_a'(ga) + LN_b'(gb) = gres + LN'(gw) with gw = ga * wa + gb * wb: two fp64 single backwards
    dxa, A_a, dwa, A_wa, dba, A_ba = _ln_bwd_ref(x, ga, wa, mean, rstd, gres)
    dxb, A_b, dwb, A_wb, dbb, A_bb = _ln_bwd_ref(x, gb, wb, mean, rstd, None)
    _within(dx, dxa + dxb, A_a + A_b, 'dual dx')
    for got, ref, A, nm in ((dp[0], dwa, A_wa, 'dwa'), (dp[1], dba, A_ba, 'dba'), (dp[2], dwb, A_wb, 'dwb'),
                            (dp[3], dbb, A_bb, 'dbb')):
        _within(got, ref, A, 'dual ' + nm)


# ---------------------------------------------------------------------------------------------------------------
# scale_residual: y = x + sc[b] * gamma * z; backward dz = sc * gamma * g, dgamma = sum sc * g * z
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows,C', [(43008, 768), (16800, 1024)])
def test_scale_residual_fullsize(rows, C):
    from vitadapter import fused
    v = _lib()
    torch.manual_seed(400 + C)
    batch, rpb = 2, rows // 2
    x = torch.randn(rows, C, device='cuda')
    z = torch.randn(rows, C, device='cuda').to(torch.bfloat16)
    gamma = torch.randn(C, device='cuda') * 0.5
    sc = torch.tensor([1.0 / 0.7, 0.45], device='cuda')
    g = torch.randn(rows, C, device='cuda')
    st = _stream()
    outs = []
    for _ in range(2):
        y = _nan(rows, C)
        v.check(v.lib.vah_scale_residual_fwd(x.data_ptr(), z.data_ptr(), gamma.data_ptr(), sc.data_ptr(), batch, rpb, C,
                                             y.data_ptr(), st), 'scale_residual_fwd')
        dz, dgm = _nan(rows, C, dtype=torch.bfloat16), _nan(C)
        ws = _nan(v.lib.vah_reduce_ws_floats(C))
        v.check(v.lib.vah_scale_residual_bwd(g.data_ptr(), z.data_ptr(), gamma.data_ptr(), sc.data_ptr(), batch, rpb, C,
                                             dz.data_ptr(), dgm.data_ptr(), ws.data_ptr(), st), 'scale_residual_bwd')
        outs.append((y, dz, dgm))
    for a, c, nm in zip(outs[0], outs[1], ('y', 'dz', 'dgamma')):
        _equal(a, c, nm)
    y, dz, dgm = outs[0]
    xe = x.view(batch, rpb, C).clone().requires_grad_(True)
    ze = z.view(batch, rpb, C).clone().requires_grad_(True)
    ge = gamma.clone().requires_grad_(True)

    class _Drop:
        drop_prob, training = 0.3, True
    take = fused.DROP_POOL.take
    fused.DROP_POOL.take = lambda x_, keep: sc
    try:
        ye = fused.residual(xe, ze, ge, _Drop())
    finally:
        fused.DROP_POOL.take = take
    assert type(ye.grad_fn).__name__ == '_ScaleResidualBackward'
    ye.backward(g.view(batch, rpb, C))
    for a, c, nm in ((ye, y, 'y'), (ze.grad, dz, 'dz'), (ge.grad, dgm, 'dgamma')):
        assert torch.equal(a.reshape(c.shape), c), 'fused.residual %s differs from the direct call' % nm
    del xe, ze, ye
    scr = sc.double().repeat_interleave(rpb).view(-1, 1)
    sgz = scr * gamma.double() * z.double()
    _within(y, x.double() + sgz, x.double().abs() + sgz.abs(), 'scale_residual y')
    sg = scr * gamma.double() * g.double()
    _within(dz, sg, sg.abs(), 'scale_residual dz', bf16=True)
    sgz = scr * g.double() * z.double()
    _within(dgm, sgz.sum(0), sgz.abs().sum(0), 'scale_residual dgamma')


# ---------------------------------------------------------------------------------------------------------------
# DWConv 3x3 on the concatenated token maps (2H, 2W), (H, W), (H/2, W/2)
# ---------------------------------------------------------------------------------------------------------------

def _levels(H, W):
    return [(2 * H, 2 * W), (H, W), (H // 2, W // 2)]


def _shifted(m, dy, dx):
    """m (B, h, w, C) read at (y + dy, x + dx), zero outside."""
    B, h, w, C = m.shape
    p = torch.zeros(B, h + 2, w + 2, C, dtype=m.dtype, device=m.device)
    p[:, 1:h + 1, 1:w + 1] = m
    return p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def _dwconv_ref(x, g, w9, bias, H, W):
    """fp64 forward, input gradient and weight / bias gradient (and their budgets) of the token DWConv."""
    B, N, C = x.shape
    xd, gd, wd = x.double(), g.double(), w9.double()
    y, Ay, dx, Adx = [torch.empty(B, N, C, dtype=torch.float64, device='cuda') for _ in range(4)]
    dw = torch.zeros(C, 9, dtype=torch.float64, device='cuda')
    Adw = torch.zeros_like(dw)
    t0 = 0
    for h, w in _levels(H, W):
        xm = xd[:, t0:t0 + h * w].reshape(B, h, w, C)
        gm = gd[:, t0:t0 + h * w].reshape(B, h, w, C)
        ys, ya = bias.double().expand(B, h, w, C).clone(), bias.double().abs().expand(B, h, w, C).clone()
        ds, da = torch.zeros_like(xm), torch.zeros_like(xm)
        for tap in range(9):
            dy, dxx = tap // 3 - 1, tap % 3 - 1
            xs = _shifted(xm, dy, dxx)
            ys += wd[:, tap] * xs
            ya += wd[:, tap].abs() * xs.abs()
            gs = _shifted(gm, -dy, -dxx)
            ds += wd[:, tap] * gs
            da += wd[:, tap].abs() * gs.abs()
            dw[:, tap] += (gm * xs).sum((0, 1, 2))
            Adw[:, tap] += (gm * xs).abs().sum((0, 1, 2))
        y[:, t0:t0 + h * w], Ay[:, t0:t0 + h * w] = ys.reshape(B, h * w, C), ya.reshape(B, h * w, C)
        dx[:, t0:t0 + h * w], Adx[:, t0:t0 + h * w] = ds.reshape(B, h * w, C), da.reshape(B, h * w, C)
        t0 += h * w
    return y, Ay, dx, Adx, dw, Adw, gd.sum((0, 1)), gd.abs().sum((0, 1))


# (B, H, W, C): H, W = the middle (stride-16) level of the adapter maps, C = ConvFFN hidden = 0.25 * 192 / 768 / 1024
#   ViT-Adapter-T 512^2 b2: (2, 32, 32, 48); B 1024^2 b2: (2, 64, 64, 192); L 640^2 b2: (2, 40, 40, 256);
#   800 x 1344 b1: (1, 50, 84, 256) - bottom level 25 x 42 (odd sizes)
@pytest.mark.parametrize('B,H,W,C', [(2, 32, 32, 48), (2, 64, 64, 192), (2, 40, 40, 256), (1, 50, 84, 256)])
def test_dwconv_tokens_fullsize(B, H, W, C):
    from vitadapter import fused
    v = _lib()
    torch.manual_seed(500 + C + H)
    N = 21 * (H // 2) * (W // 2)
    x = torch.randn(B, N, C, device='cuda').to(torch.bfloat16)
    g = torch.randn(B, N, C, device='cuda').to(torch.bfloat16)
    w9 = torch.randn(C, 9, device='cuda') * 0.3
    bias = torch.randn(C, device='cuda') * 0.3
    st = _stream()
    outs = []
    for _ in range(2):
        y, dx = _nan(B, N, C, dtype=torch.bfloat16), _nan(B, N, C, dtype=torch.bfloat16)
        v.check(v.lib.vah_dwconv3x3_tokens_bf16(x.data_ptr(), w9.data_ptr(), bias.data_ptr(), B, H, W, C, 0, y.data_ptr(),
                                                st), 'dwconv_fwd')
        v.check(v.lib.vah_dwconv3x3_tokens_bf16(g.data_ptr(), w9.data_ptr(), None, B, H, W, C, 1, dx.data_ptr(), st),
                'dwconv_dgrad')
        dw, db = _nan(C * 9), _nan(C)
        ws = _nan(v.lib.vah_reduce_ws_floats(10 * C))
        v.check(v.lib.vah_dwconv3x3_tokens_wgrad_bf16(x.data_ptr(), g.data_ptr(), B, H, W, C, dw.data_ptr(), db.data_ptr(),
                                                      ws.data_ptr(), st), 'dwconv_wgrad')
        outs.append((y, dx, dw, db))
    for a, c, nm in zip(outs[0], outs[1], ('y', 'dx', 'dw', 'db')):
        _equal(a, c, nm)
    y, dx, dw, db = outs[0]
    conv = torch.nn.Conv2d(C, C, 3, padding=1, groups=C).cuda()
    with torch.no_grad():
        conv.weight.copy_(w9.view(C, 1, 3, 3))
        conv.bias.copy_(bias)
    xe = x.clone().requires_grad_(True)
    ye = fused.dwconv_tokens(conv, xe, H, W)
    assert ye is not None and type(ye.grad_fn).__name__ == '_DWConvTokensBackward'
    ye.backward(g)
    for a, c, nm in ((ye, y, 'y'), (xe.grad, dx, 'dx'), (conv.weight.grad.reshape(-1), dw, 'dw'),
                     (conv.bias.grad, db, 'db')):
        assert torch.equal(a, c), 'fused.dwconv_tokens %s differs from the direct call' % nm
    del xe, ye, conv
    ry, Ay, rdx, Adx, rdw, Adw, rdb, Adb = _dwconv_ref(x, g, w9, bias, H, W)
    _within(y, ry, Ay, 'dwconv y', bf16=True)
    _within(dx, rdx, Adx, 'dwconv dx', bf16=True)
    _within(dw, rdw, Adw, 'dwconv dw')
    _within(db, rdb, Adb, 'dwconv db')


# ---------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows,C', LN_SHAPES + COLSUM_CAP)
def test_colsum_bf16_fullsize(rows, C):
    v = _lib()
    torch.manual_seed(600 + rows % 101)
    g = torch.randn(rows, C, device='cuda').to(torch.bfloat16)
    st = _stream()
    outs = []
    for _ in range(2):
        out, ws = _nan(C), _nan(v.lib.vah_reduce_ws_floats(C))
        v.check(v.lib.vah_colsum_bf16(g.data_ptr(), rows, C, out.data_ptr(), ws.data_ptr(), st), 'colsum_bf16')
        outs.append(out)
    _equal(outs[0], outs[1], 'colsum_bf16')
    _within(outs[0], g.double().sum(0), g.double().abs().sum(0), 'colsum_bf16')


# maps (B, C, h, w) at strides 8, 16, 32 of the SPM -> tokens: B 1024^2 b2 C 768, L 640^2 b2 C 1024, 800 x 1344 b1 C 1024
@pytest.mark.parametrize('B,C,hw', [(2, 768, [(128, 128), (64, 64), (32, 32)]), (2, 1024, [(80, 80), (40, 40), (20, 20)]),
                                    (1, 1024, [(100, 168), (50, 84), (25, 42)])])
def test_colsum_f32_maps_to_tokens_fullsize(B, C, hw):
    from vitadapter import fused
    v = _lib()
    torch.manual_seed(700 + C + B)
    maps = [torch.randn(B, C, h, w, device='cuda').to(torch.bfloat16).requires_grad_(True) for h, w in hw]
    vecs = [(torch.randn(C, device='cuda') * 0.1).requires_grad_(True) for _ in hw]
    out = fused.maps_to_tokens(maps, vecs)
    assert type(out.grad_fn).__name__ == '_MapsToTokensBackward'
    T = out.shape[1]
    g = torch.randn(B, T, C, device='cuda') + 0.3
    out.backward(g)
    st = _stream()
    t0 = 0
    for (h, w), vec in zip(hw, vecs):
        n = h * w
        res = []
        for _ in range(2):
            o, ws = _nan(C), _nan(v.lib.vah_reduce_ws_floats(C))
            v.check(v.lib.vah_colsum_f32(g[:, t0:].data_ptr(), B, T * C, n, C, o.data_ptr(), ws.data_ptr(), st),
                    'colsum_f32')
            res.append(o)
        _equal(res[0], res[1], 'colsum_f32 %dx%d' % (h, w))
        assert torch.equal(vec.grad, res[0]), 'fused.maps_to_tokens dvec %dx%d differs from the direct call' % (h, w)
        sl = g[:, t0:t0 + n].double()
        _within(res[0], sl.sum((0, 1)), sl.abs().sum((0, 1)), 'colsum_f32 %dx%d' % (h, w))
        t0 += n


# ---------------------------------------------------------------------------------------------------------------
# Linear weight / bias gradients: colsum partials + split-K GEMM + the finalize job of reduce_splits
# ---------------------------------------------------------------------------------------------------------------

def _table_entry(M, N, K):
    import _vah
    key = '1 0 1 0 0 %d %d %d %d %d %d ' % (M, N, K, M, N, N)
    lines = [ln for ln in _vah.gemm_table_dump().splitlines() if ln.startswith(key)]
    return lines[0].split() if lines else None


def _check_table_entry(M, N, K, index, split, rejected0):
    import _vah
    got = _table_entry(M, N, K)
    rej = _vah.lib.vah_gemm_rejected_candidates()
    where = 'hipBLASLt %d, table %s' % (_vah.lib.vah_gemm_library_version(), os.path.basename(TABLE))
    assert got is not None, '%dx%dx%d: no table entry after the call (%s)' % (M, N, K, where)
    assert (int(got[11]), int(got[12])) == (index, split), \
        '%dx%dx%d ran index %s split %s, the table says %d / %d: live-tuned (%s)' % (M, N, K, got[11], got[12], index,
                                                                                     split, where)
    assert rej == rejected0, '%dx%dx%d: %d candidate(s) rejected during the call (%s)' % (M, N, K, rej - rejected0, where)


def _wgrad_direct(g2, x2, gw, gb, split):
    """fused._wgrad_bgrad's calls with every buffer it hands over poisoned: colsum partial rows, outputs and the
    split-K partial products at the front of the GEMM workspace (the library's scratch after them left as is)."""
    from vitadapter import fused
    v = _lib()
    R, M = g2.shape
    N = x2.shape[1]
    cws = _nan(v.lib.vah_reduce_ws_floats(M))
    ws_bytes = fused._GEMM_WS_BYTES + (min(64 * M * N * 4, 160 << 20) if R >= 4096 else 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    if split > 1:
        ws[:split * M * N * 4].view(torch.float32).fill_(NAN)
    gw.fill_(NAN)
    gb.fill_(NAN)
    nparts = ctypes.c_int64(0)
    st = _stream()
    v.check(v.lib.vah_colsum_bf16_partials(g2.data_ptr(), R, M, cws.data_ptr(), ctypes.byref(nparts), st),
            'colsum_partials')
    v.check(v.lib.vah_gemm_bf16_fin(1, 0, M, N, R, g2.data_ptr(), M, x2.data_ptr(), N, gw.data_ptr(), N, 1, ws.data_ptr(),
                                    ws_bytes, cws.data_ptr(), nparts.value, M, gb.data_ptr(), st), 'gemm_bf16_fin')


def _check_wgrad(g2, x2, gw, gb, what):
    gd, xd = g2.double(), x2.double()
    _within(gw, gd.t() @ xd, gd.abs().t() @ xd.abs(), what + ' dW')
    _within(gb, gd.sum(0), gd.abs().sum(0), what + ' db')


@pytest.mark.parametrize('M,N,K,index,split', _wgrad_rows(),
                         ids=['%dx%dx%d-split%d' % (r[0], r[1], r[2], r[4]) for r in _wgrad_rows()])
def test_wgrad_bgrad_table_rows(M, N, K, index, split):
    """One case per weight-gradient row of the committed table: g2 = (K, M) (the output gradient, K token rows),
    x2 = (K, N) (the layer input); dW = g2^T x2 (M, N) fp32, db = column sums of g2."""
    from vitadapter import fused
    import _vah
    torch.manual_seed(800 + M + N + K % 1000)
    g2 = torch.randn(K, M, device='cuda').to(torch.bfloat16)
    x2 = torch.randn(K, N, device='cuda').to(torch.bfloat16)
    rejected0 = _vah.lib.vah_gemm_rejected_candidates()
    ew, eb = fused._wgrad_bgrad(g2, x2)            # the entry point (resolves the table entry on first use)
    _check_table_entry(M, N, K, index, split, rejected0)
    outs = []
    for _ in range(2):
        gw, gb = torch.empty(M, N, device='cuda'), torch.empty(M, device='cuda')
        _wgrad_direct(g2, x2, gw, gb, split)
        outs.append((gw, gb))
    _check_table_entry(M, N, K, index, split, rejected0)
    _equal(outs[0][0], outs[1][0], 'dW')
    _equal(outs[0][1], outs[1][1], 'db')
    assert torch.equal(ew, outs[0][0]) and torch.equal(eb, outs[0][1]), 'fused._wgrad_bgrad differs from the direct call'
    _check_wgrad(g2, x2, outs[0][0], outs[0][1], '%dx%dx%d split %d' % (M, N, K, split))


@pytest.mark.parametrize('fin,fout', [(768, 3072), (3072, 768)], ids=['fc1', 'fc2'])
def test_linear_fullsize(fin, fout):
    """fused.linear end to end for the MLP of ViT-Adapter-B at 1024^2, batch 2 (8 192 rows): y, dx, dW, db in fp64
    from the operands the GEMMs saw (the bf16 copy of the weight)."""
    from vitadapter import fused
    import _vah
    torch.manual_seed(900 + fin)
    rows = 8192
    lin = torch.nn.Linear(fin, fout).cuda()
    with torch.no_grad():
        lin.bias.normal_(0, 0.5)
    x = torch.randn(2, rows // 2, fin, device='cuda').to(torch.bfloat16).requires_grad_(True)
    g = torch.randn(2, rows // 2, fout, device='cuda').to(torch.bfloat16)
    entry = [r for r in _wgrad_rows() if r[:3] == (fout, fin, rows)]
    assert len(entry) == 1, 'no weight-gradient row for %dx%dx%d in the table' % (fout, fin, rows)
    rejected0 = _vah.lib.vah_gemm_rejected_candidates()
    outs = []
    for _ in range(2):
        x.grad = None
        lin.zero_grad()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            y = fused.linear(lin, x)
        assert type(y.grad_fn).__name__ == '_LinearBF16Backward'
        y.backward(g)
        outs.append((y.detach(), x.grad, lin.weight.grad, lin.bias.grad))
    _check_table_entry(fout, fin, rows, entry[0][3], entry[0][4], rejected0)
    for a, c, nm in zip(outs[0], outs[1], ('y', 'dx', 'dW', 'db')):
        _equal(a, c, nm)
    y, dx, dw, db = outs[0]
    xd, gd = x.detach().reshape(rows, fin).double(), g.reshape(rows, fout).double()
    wd = lin.weight.detach().to(torch.bfloat16).double()
    bd = lin.bias.detach().double()
    _within(y.reshape(rows, fout), xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs(), 'linear y', bf16=True)
    _within(dx.reshape(rows, fin), gd @ wd, gd.abs() @ wd.abs(), 'linear dx', bf16=True)
    _check_wgrad(g.reshape(rows, fout), x.detach().reshape(rows, fin), dw, db, 'linear')


# ---------------------------------------------------------------------------------------------------------------
# BN tail statistics
# ---------------------------------------------------------------------------------------------------------------

def test_bn_tail_stats_fullsize():
    """The stride-4 tail of ViT-Adapter-B at 1024^2, batch 2: t = a + upsample_4(x), (2, 768, 256, 256), with a
    channel mean about 8x its std.  sums = [sum t | sum t^2] and the backward's [sum dy | sum dy * xhat] against
    fp64 sums of the same fp32 t (t's own fp32 rounding, |t| * 2^-24 per element, is inside the budget)."""
    from vitadapter import fused
    v = _lib()
    torch.manual_seed(1000)
    N, C, H, W, s = 2, 768, 256, 256, 4
    # std of t about 0.8 (0.7 from a, the rest from the upsampled x); channel means +-6.4
    cm = (torch.randint(0, 2, (C,), device='cuda') * 2 - 1).float().view(1, C, 1, 1) * 6.4
    a = (torch.randn(N, C, H, W, device='cuda') * 0.7 + cm).to(torch.bfloat16)
    x = torch.randn(N, C, H // s, W // s, device='cuda') * 0.7
    st = _stream()
    ops = (a.data_ptr(), 1, None, 0, x.data_ptr(), s, N, C, H, W)
    nws = v.lib.vah_bn_tail_ws_floats(C)
    res = []
    for _ in range(2):
        sums = _nan(2 * C)
        ws = torch.zeros(nws, device='cuda')           # the API's contract: partial rows zero-filled by the caller
        v.check(v.lib.vah_bn_tail_stats(*ops, None, sums.data_ptr(), ws.data_ptr(), st), 'bn_tail_stats')
        res.append(sums)
    _equal(res[0], res[1], 'bn_tail sums')
    sums = res[0]
    # t of the reference expression (bilinear, align_corners=False) in fp64; its terms |a| + |up(x)| carry the budget
    # of the few fp32 roundings that form t in the kernel as well
    up = F.interpolate(x.double(), scale_factor=s, mode='bilinear', align_corners=False)
    t = a.double() + up
    ta = a.double().abs() + up.abs()
    del up
    _within(sums[:C], t.sum((0, 2, 3)), ta.sum((0, 2, 3)), 'bn_tail sum t')
    _within(sums[C:], (t * t).sum((0, 2, 3)), (ta * ta).sum((0, 2, 3)), 'bn_tail sum t^2')
    mean = (t.mean((0, 2, 3))).float()
    rstd = (1.0 / torch.sqrt(t.var((0, 2, 3), unbiased=False) + 1e-5)).float()
    dy = torch.randn(N, C, H, W, device='cuda')
    res = []
    for _ in range(2):
        sums2 = _nan(2 * C)
        ws = torch.zeros(nws, device='cuda')
        v.check(v.lib.vah_bn_tail_bwd_stats(*ops, mean.data_ptr(), rstd.data_ptr(), None, None, 0, None, dy.data_ptr(), 0,
                                            sums2.data_ptr(), ws.data_ptr(), st), 'bn_tail_bwd_stats')
        res.append(sums2)
    _equal(res[0], res[1], 'bn_tail bwd sums')
    sums2 = res[0]
    del ws
    md, rd = mean.double().view(1, C, 1, 1), rstd.double().view(1, C, 1, 1)
    dyd = dy.double()
    del dy
    xh = (t - md) * rd
    _within(sums2[:C], dyd.sum((0, 2, 3)), dyd.abs().sum((0, 2, 3)), 'bn_tail sum dy')
    # xhat from an fp32 t: t's rounding times rstd joins the terms' budget
    _within(sums2[C:], (dyd * xh).sum((0, 2, 3)), (dyd.abs() * (xh.abs() + ta * rd)).sum((0, 2, 3)),
            'bn_tail sum dy * xhat')
