"""GPU: the GroupNorm kernels (csrc/group_norm.hip, include/vitadapter_hip_group_norm.h) against fp64, stage by stage.

Budget, the project's convention (oracle/spm.py, tests/test_spm_fp64_gpu.py, tests/test_spm_f16_fp64_gpu.py):

    |got - ref| <= 256 * 2^-24 * A   + 2^-8 |ref| (bf16 outputs)   or   + 2^-11 |ref| + 2^-25 (fp16 outputs)

A = the sum of the absolute terms behind the element.  256 bounds the longest dependent chain of fp32 additions: a thread
of the statistics kernels walks ceil(T / parts) / row-lanes rows (17 at the production shape: 67200 rows, 512 parts, 8 row
lanes), the row lanes of a workgroup (4 .. 32) are added in order, the second launch adds parts / 32 + 3 per chain + 2 + 8
partial rows, then at most 8 channels of a group and, for dgamma / dbeta, the images.

Every reference is restated here in fp64 and starts from what the kernel saw: the 16-bit operands upcast, and for the
stages after the statistics the kernel's OWN fp32 mean / rstd (and group sums).  The statistics themselves are held to
oracle.spm.finalize_stats (mean: sum |x| / cnt; rstd: rstd (1 + (E[x^2] + mean^2) / (var + eps))).

Every case NaN-fills outputs and workspace, places each output inside a larger NaN buffer whose guard elements must come
back bit-unchanged (in the strided (Lq, N, C) form that includes the rows of the neighbouring levels; mean, rstd, the group
sums, dgamma, dbeta and the workspace sit between 64-float NaN guards as well), and runs twice:
the bits must agree.  ReLU edge: elements whose fp64 pre-activation lies within 2^-20 (relative) of zero may take either
mask; they are left out of dx, their flip is added to the budget of the sums, and their share is asserted <= 1e-4.

The launch arithmetic of the kernels is mirrored below (_parts, _apply_rows, _apply_blocks): the shapes one row under and
over a chunk, the ragged last chunk and the trailing workgroups without rows are derived from it, so a change of
geometry has to be re-derived here."""
import itertools

import pytest
import torch

from oracle import spm

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
CODE = {F32: 0, BF16: 1, F16: 2}
f64 = torch.float64
F16_U, F16_SUB = 2.0 ** -11, 2.0 ** -25
EPS = 1e-5
NAN_BITS = {F32: 0x7FC00BAD, BF16: 0x7FC5, F16: 0x7E05}
INT = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}

# ---- the kernels' launch arithmetic (csrc/group_norm.hip: kGnMaxParts, kGnMinParts, kGnPartRows, kGnApplyRows, kGnApplyBlocks)
MAX_PARTS, MIN_PARTS, PART_ROWS, APPLY_ROWS, APPLY_BLOCKS = 512, 16, 64, 4, 2048


def _parts(N, T):
    cap = max(MIN_PARTS, MAX_PARTS // max(N, 1))
    return min(max((T + PART_ROWS - 1) // PART_ROWS, 1), cap)


def _apply_rows(C):
    """rows a workgroup of the apply kernels takes per step"""
    return (256 // (C // 8)) * APPLY_ROWS


def _apply_blocks(N, T, C):
    return min(max((T + _apply_rows(C) - 1) // _apply_rows(C), 1), max(APPLY_BLOCKS // N, 1))


def _lib():
    import _vah
    return _vah


def _nan_buffer(shape, dtype):
    t = torch.empty(shape, dtype=INT[dtype], device='cuda')
    t.fill_(NAN_BITS[dtype])
    return t.view(dtype)


def _place(N, T, C, dtype, strided):
    """-> (buffer, view (N, T, C), mask of the view's elements in the buffer)"""
    if strided:                       # a level's rows [3, 3 + T) of an (Lq, N, C) buffer with two neighbours
        buf = _nan_buffer((T + 8, N, C), dtype)
        view = buf[3:3 + T].permute(1, 0, 2)
        mask = torch.zeros(buf.shape, dtype=torch.bool, device='cuda')
        mask[3:3 + T] = True
    else:
        buf = _nan_buffer((N * T * C + 4 * C,), dtype)
        view = buf[2 * C:2 * C + N * T * C].view(N, T, C)
        mask = torch.zeros(buf.shape, dtype=torch.bool, device='cuda')
        mask[2 * C:2 * C + N * T * C] = True
    return buf, view, mask


GUARD = 64          # floats on either side of a flat fp32 output (keeps the 16-byte alignment)


def _guarded(n):
    """-> (buffer, view of n floats inside it): statistics, sums and the workspace sit between NaN guards too"""
    buf = _nan_buffer((n + 2 * GUARD,), F32)
    return buf, buf[GUARD:GUARD + n]


def _flat_guards_intact(bufs, what):
    for name, buf in bufs.items():
        bits = buf.view(torch.int32)
        assert bool((bits[:GUARD] == NAN_BITS[F32]).all()) and bool((bits[-GUARD:] == NAN_BITS[F32]).all()), '%s: guard of %s changed' % (what, name)


def _as_input(t, strided):
    """the tensor's values in the layout under test"""
    N, T, C = t.shape
    buf, view, _ = _place(N, T, C, t.dtype, strided)
    view.copy_(t)
    return view


def _arg(t):
    N, T, C = t.shape
    return t.data_ptr(), CODE[t.dtype], (t.stride(1) if T > 1 else C), (t.stride(0) if N > 1 else 0)


def _guards_intact(buf, mask, what):
    bits = buf.view(INT[buf.dtype])
    want = _nan_buffer(buf.shape, buf.dtype).view(INT[buf.dtype])
    assert bool((bits[~mask] == want[~mask]).all()), '%s: guard elements changed' % what


def _bits(t):
    return t.contiguous().view(INT[t.dtype]) if t.dtype in INT else t


def _bound(ref, A, dtype):
    b = spm.bound(ref, A)
    if dtype == BF16:
        return b + spm.BF16_U * ref.abs()
    if dtype == F16:
        return b + F16_U * ref.abs() + F16_SUB
    return b


def _check(what, got, ref, A, dtype=F32, mask=None):
    err = (got.to(f64) - ref).abs()
    b = _bound(ref, A, dtype)
    ok = err <= b
    if mask is not None:
        ok = ok | ~mask
    if not bool(ok.all()):
        i = int(torch.nonzero(~ok.reshape(-1))[0])
        raise AssertionError('%s: %d of %d elements over budget; first flat %d: got %r ref %r budget %.3e' % (
            what, int((~ok).sum()), ok.numel(), i, got.reshape(-1)[i].item(), ref.reshape(-1)[i].item(), b.reshape(-1)[i].item()))
    r = torch.where(err == 0, torch.zeros_like(err), err / b)
    if mask is not None:
        r = r[mask]
    return float(r.max()) if r.numel() else 0.0


def _per_channel(v, N, G, C):
    """(N * G,) group values -> (N, 1, C) fp64"""
    return v.to(f64).view(N, G).repeat_interleave(C // G, dim=1).view(N, 1, C)


def _forward(vah, x, N, T, C, G, w, b, relu, add, ydt, strided_y):
    lib = vah.lib
    nws = lib.vah_group_norm_ws_floats(N, T, C, G)
    assert nws == N * _parts(N, T) * 2 * C
    (wsb, ws), (meanb, mean), (rstdb, rstd) = _guarded(nws), _guarded(N * G), _guarded(N * G)
    ybuf, y, ymask = _place(N, T, C, ydt, strided_y)
    st = vah.raw_stream(x.device)
    vah.check(lib.vah_group_norm_stats(*_arg(x), N, T, C, G, EPS, mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), nws, st), 'stats')
    vah.check(lib.vah_group_norm_apply(*_arg(x), N, T, C, G, mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), b.data_ptr(), int(relu),
                                       add.data_ptr() if add is not None else None, *_arg(y), st), 'apply')
    _flat_guards_intact(dict(ws=wsb, mean=meanb, rstd=rstdb), 'forward')
    return mean, rstd, ybuf, y, ymask


def _backward(vah, x, dy, N, T, C, G, w, b, relu, mean, rstd, dxdt, strided_dx):
    lib = vah.lib
    nws = lib.vah_group_norm_ws_floats(N, T, C, G)
    (wsb, ws), (gsb, gsums), (dgb, dgamma), (dbb, dbeta) = _guarded(nws), _guarded(2 * N * G), _guarded(C), _guarded(C)
    dxbuf, dx, dxmask = _place(N, T, C, dxdt, strided_dx)
    st = vah.raw_stream(x.device)
    vah.check(lib.vah_group_norm_bwd_stats(*_arg(x), *_arg(dy), N, T, C, G, mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), b.data_ptr(),
                                           int(relu), gsums.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), nws, st),
              'bwd_stats')
    vah.check(lib.vah_group_norm_bwd_apply(*_arg(x), *_arg(dy), N, T, C, G, mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), b.data_ptr(),
                                           int(relu), gsums.data_ptr(), *_arg(dx), st), 'bwd_apply')
    _flat_guards_intact(dict(ws=wsb, gsums=gsb, dgamma=dgb, dbeta=dbb), 'backward')
    return gsums, dgamma, dbeta, dxbuf, dx, dxmask


def _operands(N, T, C, xdt, ydt, add, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = (torch.randn(N, T, C, device='cuda', generator=g) * 1.5 + 0.5 * torch.randn(C, device='cuda', generator=g)).to(xdt)
    dy = torch.randn(N, T, C, device='cuda', generator=g).to(ydt)
    w = 1.0 + 0.3 * torch.randn(C, device='cuda', generator=g)
    b = 0.3 * torch.randn(C, device='cuda', generator=g)
    a = torch.randn(N, T, C, device='cuda', generator=g).to(ydt) if add else None
    return x, dy, w, b, a


def _run(case, N, T, C, G, xdt, ydt, relu, add, strided, seed=0, backward=True):
    """forward and backward of one case against fp64; dy and the addend carry y's dtype, dx carries x's"""
    vah = _lib()
    cpg = C // G
    cnt = float(T * cpg)
    x0, dy0, w, b, a = _operands(N, T, C, xdt, ydt, add, seed)
    x, dy = _as_input(x0, strided), _as_input(dy0, strided)
    runs = []
    for _ in range(2):
        mean, rstd, ybuf, y, ymask = _forward(vah, x, N, T, C, G, w, b, relu, a, ydt, strided)
        out = [mean, rstd, ybuf]
        if backward:
            gsums, dgamma, dbeta, dxbuf, dx, dxmask = _backward(vah, x, dy, N, T, C, G, w, b, relu, mean, rstd, xdt, strided)
            out += [gsums, dgamma, dbeta, dxbuf]
        runs.append(out)
    torch.cuda.synchronize()
    for u, v in zip(*runs):
        assert torch.equal(_bits(u), _bits(v)), '%s: two runs differ' % case
    _guards_intact(ybuf, ymask, case + ' y')
    assert torch.equal(x, x0) and torch.equal(dy, dy0)
    ratios = {}

    # ---- statistics: fp64 sums of the operand, conditioning of oracle.spm.finalize_stats
    xd = x0.to(f64)
    xg = xd.view(N, T, G, cpg)
    sums = torch.cat([xg.sum((1, 3)).reshape(-1), (xg * xg).sum((1, 3)).reshape(-1), torch.tensor([cnt], dtype=f64, device='cuda')])
    fin = spm.finalize_stats(sums, N * G, EPS, 0.1)
    ratios['mean'] = _check(case + ' mean', mean, fin['mean'][0], xg.abs().sum((1, 3)).reshape(-1) / cnt)
    ratios['rstd'] = _check(case + ' rstd', rstd, fin['rstd'][0], fin['rstd'][1])

    # ---- apply, from the kernel's own mean / rstd
    mu, rs = _per_channel(mean, N, G, C), _per_channel(rstd, N, G, C)
    wd, bd = w.to(f64), b.to(f64)
    sc = rs * wd
    sh = bd - mu * sc
    pre = xd * sc + sh
    ref = pre.clamp_min(0.) if relu else pre
    A = (xd * sc).abs() + bd.abs() + (mu * sc).abs()
    if a is not None:
        ref, A = ref + a.to(f64), A + a.to(f64).abs()
    ratios['y'] = _check(case + ' y', y, ref, A, ydt)
    if not backward:
        return ratios

    # ---- backward statistics
    _guards_intact(dxbuf, dxmask, case + ' dx')
    gd = dy0.to(f64)
    xh = (xd - mu) * rs
    if relu:
        gp = torch.where(pre > 0, gd, torch.zeros_like(gd))
        edge = pre.abs() <= spm.RELU_EDGE * ((xd * sc).abs() + sh.abs())
    else:
        gp, edge = gd, torch.zeros_like(gd, dtype=torch.bool)
    share = float(edge.double().mean())
    assert share <= 1e-4, (case, share)
    ge = torch.where(edge, gd.abs(), torch.zeros_like(gd))               # a flip of an edge element moves the sums by this
    def group(t):
        return t.view(N, T, G, cpg).sum((1, 3)).reshape(-1)
    ref_s = torch.cat([group(gp * wd), group(gp * wd * xh)])
    A_s = torch.cat([group((gp.abs() + ge) * wd.abs()), group((gp.abs() + ge) * wd.abs() * xh.abs())])
    ratios['gsums'] = _check(case + ' gsums', gsums, ref_s, A_s)
    ratios['dgamma'] = _check(case + ' dgamma', dgamma, (gp * xh).sum((0, 1)), ((gp.abs() + ge) * xh.abs()).sum((0, 1)))
    ratios['dbeta'] = _check(case + ' dbeta', dbeta, gp.sum((0, 1)), (gp.abs() + ge).sum((0, 1)))

    # ---- backward apply, from the kernel's own group sums
    m1 = _per_channel(gsums[:N * G], N, G, C) / cnt
    m2 = _per_channel(gsums[N * G:], N, G, C) / cnt
    ref_dx = rs * (gp * wd - m1 - xh * m2)
    A_dx = rs * ((gp * wd).abs() + m1.abs() + (xd.abs() + mu.abs()) * rs * m2.abs())
    ratios['dx'] = _check(case + ' dx', dx, ref_dx, A_dx, xdt, mask=~edge)
    print('GN %-28s %s edge %.2e' % (case, ' '.join('%s %.3f' % kv for kv in ratios.items()), share))
    return ratios


CG = [(64, 32), (256, 32), (512, 64), (64, 64)]
DTYPES = [(F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32), (F32, BF16), (F32, F16)]


def _small_cases():
    """T in {1, 2, 63, 65} (one row under / over a statistics part of 64 rows) and 64, one row under / over the rows an
    apply workgroup takes per step, and T = 100 (two equal parts of 50; the ragged last part is T = 65: 33 + 32, and the 26-row
    part of test_trailing_workgroups_without_rows) - each for N in {1, 3}, walking through
    the channel layouts, the dtype forms, relu, add and the strided form so that every value of each appears"""
    cases = []
    i = 0
    for T in (1, 2, 63, 64, 65, 100, 'apply-1', 'apply+1'):
        for N in (1, 3):
            C, G = CG[i % 4]
            xdt, ydt = DTYPES[i % 7]
            t = T if isinstance(T, int) else _apply_rows(C) + (1 if T.endswith('+1') else -1)
            cases.append(('T%s_N%d_C%d_G%d_%s_%s%s%s%s' % (T, N, C, G, str(xdt)[6:], str(ydt)[6:], '_relu' if i % 2 else '',
                                                         '_add' if (i // 2) % 2 else '', '_strided' if (i // 3) % 2 else ''),
                          N, t, C, G, xdt, ydt, bool(i % 2), bool((i // 2) % 2), bool((i // 3) % 2)))
            i += 1
    # every channel layout x every dtype form once more, strided, relu and add on, N = 3, T = 65
    for (C, G), (xdt, ydt) in itertools.product(CG, DTYPES):
        cases.append(('all_C%d_G%d_%s_%s' % (C, G, str(xdt)[6:], str(ydt)[6:]), 3, 65, C, G, xdt, ydt, True, True, True))
    return cases


SMALL = _small_cases()


def test_the_case_list_covers_what_it_claims():
    assert {c[3:5] for c in SMALL} == set(CG) and {c[5:7] for c in SMALL} == set(DTYPES)
    for k in (7, 8, 9):
        assert {c[k] for c in SMALL} == {False, True}
    assert {c[1] for c in SMALL} == {1, 3} and {1, 2, 63, 65} <= {c[2] for c in SMALL}
    assert _parts(1, 63) == 1 and _parts(1, 64) == 1 and _parts(1, 65) == 2 and _parts(1, 100) == 2 and _parts(3, 100) == 2
    assert (_apply_rows(64), _apply_rows(256), _apply_rows(512)) == (128, 32, 16)
    assert _apply_blocks(1, _apply_rows(256) - 1, 256) == 1 and _apply_blocks(1, _apply_rows(256) + 1, 256) == 2


@pytest.mark.parametrize('case,N,T,C,G,xdt,ydt,relu,add,strided', SMALL, ids=[c[0] for c in SMALL])
def test_small_shapes(case, N, T, C, G, xdt, ydt, relu, add, strided):
    _run(case, N, T, C, G, xdt, ydt, relu, add, strided, seed=len(case) + T + C)


def test_trailing_workgroups_without_rows():
    """N = 3 caps the parts at 170 per image; T = 10881 gives parts of 65 rows, and the last two get none"""
    N, T = 3, 10881
    parts = _parts(N, T)
    per = (T + parts - 1) // parts
    assert parts == 170 and per == 65 and (parts - 2) * per >= T
    _run('trailing_empty', N, T, 64, 32, BF16, BF16, True, False, False, seed=5)
    # and the apply kernels at their block cap: rows strided over 682 blocks
    assert _apply_blocks(3, 100000, 64) == 682
    _run('apply_cap', 3, 100000, 64, 32, BF16, BF16, False, False, False, seed=6, backward=False)


def test_four_rows_in_flight_at_64_channels():
    """C = 64 has 32 row lanes: a thread enters the four-rows-in-flight loop of the statistics kernels only when its part
    has at least 3 * 32 + 1 = 97 rows.  T = 70000 on the 512-part cap gives parts of 137 rows: lanes 0 .. 8 take one
    unrolled step and a single-row tail, the others the tail alone - forward and backward sums."""
    N, T = 1, 70000
    parts = _parts(N, T)
    per = (T + parts - 1) // parts
    assert parts == 512 and per == 137 and per >= 3 * (256 // (64 // 8)) + 1
    _run('c64_unrolled', N, T, 64, 32, BF16, BF16, True, False, False, seed=9)
    _run('c64_unrolled_g64_f32', N, T, 64, 64, F32, F32, False, False, True, seed=10)


def test_production_shape():
    """the stride-4 GroupNorms of configs[4]: (1, 67200, 256) bf16, 32 groups, with ReLU; and with the upsampled addend"""
    assert _parts(1, 67200) == 512
    _run('configs4_relu', 1, 67200, 256, 32, BF16, BF16, True, False, False, seed=7)
    _run('configs4_add', 1, 67200, 256, 32, BF16, BF16, False, True, False, seed=8)


@pytest.mark.parametrize('poison', [float('inf'), float('-inf'), float('nan')], ids=['inf', '-inf', 'nan'])
@pytest.mark.parametrize('dt', [F32, BF16, F16], ids=['f32', 'bf16', 'f16'])
def test_nonfinite_in_nonfinite_out(dt, poison):
    """the rule of tests/test_nonfinite_gpu.py: an inf or NaN in x leaves every element of its image and group non-finite
    (and nothing else); one in dy leaves the sums it enters and every dx of its image and group non-finite"""
    vah = _lib()
    N, T, C, G = 2, 70, 256, 32
    cpg = C // G
    x, dy, w, b, _ = _operands(N, T, C, dt, dt, False, 11)
    n0, t0, c0 = 1, 37, 100
    g0 = c0 // cpg
    hit = torch.zeros(N, T, C, dtype=torch.bool, device='cuda')
    hit[n0, :, g0 * cpg:(g0 + 1) * cpg] = True
    xp = x.clone()
    xp[n0, t0, c0] = poison
    mean, rstd, _, y, _ = _forward(vah, xp, N, T, C, G, w, b, True, None, dt, False)
    assert not bool(torch.isfinite(y[hit]).any()) and bool(torch.isfinite(y[~hit]).all())
    assert not bool(torch.isfinite(rstd[n0 * G + g0])) and int((~torch.isfinite(rstd)).sum()) == 1
    # backward: clean x, poisoned dy (no ReLU: a masked element feeds nothing)
    mean, rstd, _, y, _ = _forward(vah, x, N, T, C, G, w, b, False, None, dt, False)
    dyp = dy.clone()
    dyp[n0, t0, c0] = poison
    gsums, dgamma, dbeta, _, dx, _ = _backward(vah, x, dyp, N, T, C, G, w, b, False, mean, rstd, dt, False)
    assert not bool(torch.isfinite(dx[hit]).any()) and bool(torch.isfinite(dx[~hit]).all())
    bad = ~torch.isfinite(gsums.view(2, N, G))
    assert bool(bad[:, n0, g0].all()) and int(bad.sum()) == 2
    assert not bool(torch.isfinite(dgamma[c0])) and not bool(torch.isfinite(dbeta[c0]))
    assert int((~torch.isfinite(dgamma)).sum()) == 1 and int((~torch.isfinite(dbeta)).sum()) == 1


@pytest.mark.parametrize('dt', [F32, BF16, F16], ids=['f32', 'bf16', 'f16'])
def test_autograd_glue_matches_torch(dt):
    """fused.group_norm (the autograd.Function around the four calls) against F.group_norm in fp64 on the same operands:
    fp32 dgamma / dbeta, dx in x's dtype, the gradient of the addend, the `out=` form writing into a level of an
    (Lq, N, C) buffer; and VAH_FUSED_DISABLE=group_norm's torch path through the same call"""
    import torch.nn.functional as F
    from vitadapter import fused
    N, T, C, G = 2, 65, 256, 32
    norm = torch.nn.GroupNorm(G, C).cuda()
    x0, dy0, w, b, a0 = _operands(N, T, C, dt, dt, True, 3)
    with torch.no_grad():
        norm.weight.copy_(w), norm.bias.copy_(b)
    tol = {F32: 1e-5, BF16: 2.0 ** -7, F16: 2.0 ** -10}[dt]

    def ref():
        xd, ad = x0.double().requires_grad_(True), a0.double().requires_grad_(True)
        wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
        y = torch.relu(F.group_norm(xd.transpose(1, 2), G, wd, bd, norm.eps).transpose(1, 2)) + ad
        y.backward(dy0.double())
        return y.detach(), xd.grad, ad.grad, wd.grad, bd.grad
    want = ref()
    for enabled in (True, False):
        fused.ENABLED['group_norm'] = enabled
        try:
            norm.zero_grad(set_to_none=True)
            x, a = x0.clone().requires_grad_(True), a0.clone().requires_grad_(True)
            with torch.autocast('cuda', dtype=dt, enabled=dt != F32):
                y = fused.group_norm(norm, x, relu=True, add=a)
            y.backward(dy0.to(y.dtype))
        finally:
            fused.ENABLED['group_norm'] = True
        if enabled:
            assert y.dtype == dt and x.grad.dtype == dt and norm.weight.grad.dtype == F32
        for name, got, ref_t in zip(('y', 'dx', 'dadd', 'dgamma', 'dbeta'), (y, x.grad, a.grad, norm.weight.grad, norm.bias.grad), want):
            err = float((got.double() - ref_t).abs().max() / ref_t.abs().max().clamp_min(1.0))
            assert err <= tol * (4 if name in ('dgamma', 'dbeta') else 1), (enabled, name, err)
    # out=: two levels written into one (Lq, N, C) fp32 buffer, gradients flow back through the buffer
    buf = torch.empty(T + 40, N, C, device='cuda')
    x1 = x0.clone().requires_grad_(True)
    x2 = x0[:, :40].clone().requires_grad_(True)
    r1 = fused.group_norm(norm, x1, out=buf[:T].permute(1, 0, 2))
    fused.group_norm(norm, x2, out=buf[T:].permute(1, 0, 2))
    assert r1.data_ptr() == buf.data_ptr() and buf.requires_grad
    gb = torch.randn(buf.shape, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    buf.backward(gb)
    for xs, rows in ((x1, slice(0, T)), (x2, slice(T, T + 40))):
        xd = xs.detach().double().requires_grad_(True)
        yd = F.group_norm(xd.transpose(1, 2), G, w.double(), b.double(), norm.eps).transpose(1, 2)
        yd.backward(gb[rows].permute(1, 0, 2).double())
        assert float((buf[rows].permute(1, 0, 2).double() - yd).abs().max()) <= 1e-5 + tol * float(yd.abs().max())
        assert float((xs.grad.double() - xd.grad).abs().max()) <= tol * max(1.0, float(xd.grad.abs().max())), rows
