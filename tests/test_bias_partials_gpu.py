"""GPU: bias gradients from the kernels that write dY (csrc/fused_ops.hip: vah_residual_layernorm_bwd_bsum,
vah_scale_residual_bwd_bsum, vah_gelu_bwd_bsum_bf16; vitadapter/fused.py::_BiasPartials).

Each kernel is held to its OWN dY: the partial rows it leaves must add up to the fp64 column sum of the bf16 tensor it
wrote, within the project's budget for an fp32 column sum, 64 * 2^-24 * sum|dz| per column (fp32 partial sums over at most
a few dozen rows per lane, 8 lanes / 4-8 waves per workgroup; the test adds the partial rows itself, in fp64).  Everything
the entry point without `_bsum` also produces is compared with it bit for bit.  Shapes are the smallest that reach every
branch: C = 200 a partly filled wave, 768 the three-vector 8-wave form of the step, 1024 the 4-wave form; 4101 rows =
8 * 512 + 5, the 512-workgroup cap with a grid-stride wrap; 2 * 1031 rows = 412 strips of 5 rows and a ragged one of 2
(row-strip kernel) or 64 strips of 32 and a ragged one of 14 (column-tiled kernels)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BUDGET = 64 * 2.0 ** -24


def _lib():
    import _vah
    return _vah


def _p(t):
    return t.data_ptr() if t is not None else None


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda')


def _stream():
    return _lib().raw_stream(torch.device('cuda', torch.cuda.current_device()))


def _strip32(rows):
    """rows per workgroup of the column-tiled kernels: a multiple of 32, at most 512 strips"""
    return max(32, ((rows + 511) // 512 + 31) // 32 * 32)


def _check_partials(bpart, nparts, dz, C, what):
    """rows [0, nparts) finite, and their sum within the budget of the fp64 column sum of the bf16 dz"""
    assert 1 <= nparts <= 512, (what, nparts)
    rows = bpart[:nparts * C].view(nparts, C)
    assert bool(torch.isfinite(rows).all()), what
    d = dz.reshape(-1, C).double()
    want, mag = d.sum(0), d.abs().sum(0)
    err = (rows.double().sum(0) - want).abs()
    worst = float((err / (BUDGET * mag).clamp_min(1e-300)).max())
    print('%s: nparts %d, worst column error / budget %.3f' % (what, nparts, worst))
    assert bool((err <= BUDGET * mag).all()), (what, worst)


# ---------------------------------------------------------------------------------------
# residual + LayerNorm backward
# ---------------------------------------------------------------------------------------
def _ln_inputs(batch, rpb, C, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    rows = batch * rpb
    t = torch.randn(rows, C, device='cuda', generator=g) * 1.5 + 0.3
    gh = torch.randn(rows, C, device='cuda', generator=g).to(torch.bfloat16)
    gt = torch.randn(rows, C, device='cuda', generator=g) * 0.5
    z = torch.randn(rows, C, device='cuda', generator=g).to(torch.bfloat16)
    w = torch.randn(C, device='cuda', generator=g) * 0.2 + 1.0
    sc = torch.tensor([1.0 / 0.7, 0.0, 1.0 / 0.9][:batch], device='cuda') if batch > 1 else torch.tensor([1.25], device='cuda')
    mean = t.mean(1)
    rstd = torch.rsqrt(t.var(1, unbiased=False) + 1e-6)
    return t, gh, w, mean.contiguous(), rstd.contiguous(), gt, z, sc


def _run_ln(entry, ins, batch, rpb, C, bsum):
    v = _lib()
    t, gh, w, mean, rstd, gt, z, sc = ins
    rows = batch * rpb
    dt, dz = _nan(rows, C), _nan(rows, C, dtype=torch.bfloat16)
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


@pytest.mark.parametrize('C', [200, 768, 1024])
@pytest.mark.parametrize('batch,rpb', [(1, 1), (1, 13), (3, 1367)], ids=['rows1', 'rows13', 'rows4101'])
def test_residual_layernorm_bwd_bsum(batch, rpb, C):
    ins = _ln_inputs(batch, rpb, C, 11 + C + rpb)
    want, _, _ = _run_ln('vah_residual_layernorm_bwd', ins, batch, rpb, C, False)
    got1, bp1, n1 = _run_ln('vah_residual_layernorm_bwd_bsum', ins, batch, rpb, C, True)
    got2, bp2, n2 = _run_ln('vah_residual_layernorm_bwd_bsum', ins, batch, rpb, C, True)
    for k in want:
        assert bool(torch.isfinite(want[k].float()).all()), k
        assert torch.equal(got1[k], want[k]), k
        assert torch.equal(got2[k], want[k]), k
    rows = batch * rpb
    assert n1 == n2 == min(512, (rows + (8 if C <= 768 else 4) - 1) // (8 if C <= 768 else 4))
    assert torch.equal(bp1[:n1 * C], bp2[:n2 * C])
    _check_partials(bp1, n1, got1['dz'], C, 'residual_layernorm_bwd_bsum %dx%d' % (rows, C))


def test_residual_layernorm_bwd_bsum_refuses_gamma():
    v = _lib()
    C, batch, rpb = 200, 1, 13
    t, gh, w, mean, rstd, gt, z, sc = _ln_inputs(batch, rpb, C, 5)
    gamma = torch.ones(C, device='cuda')
    dgamma, dt, dz = _nan(C), _nan(rpb, C), _nan(rpb, C, dtype=torch.bfloat16)
    dw, db, ws = _nan(C), _nan(C), _nan(v.lib.vah_reduce_ws_floats(3 * C))
    bpart, n = _nan(v.lib.vah_reduce_ws_floats(C)), ctypes.c_int64(-1)
    rc = v.lib.vah_residual_layernorm_bwd_bsum(_p(t), _p(gh), _p(w), _p(mean), _p(rstd), _p(gt), _p(z), _p(gamma), _p(sc),
                                               batch, rpb, C, _p(dt), _p(dz), _p(dgamma), _p(dw), _p(db), _p(ws), _p(bpart),
                                               ctypes.byref(n), _stream())
    msg = v.lib.vah_last_error().decode()
    assert rc == -2 and msg.startswith('vah_residual_layernorm_bwd_bsum:') and 'gamma' in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz.float()).all()) and bool(torch.isnan(bpart).all()), 'nothing was launched'
    # misaligned and null arguments: the parent's codes
    args = [_p(t), _p(gh), _p(w), _p(mean), _p(rstd), _p(gt), _p(z), None, _p(sc), batch, rpb, C, _p(dt), _p(dz), None,
            _p(dw), _p(db), _p(ws)]
    assert v.lib.vah_residual_layernorm_bwd_bsum(*args, None, ctypes.byref(n), _stream()) == -1
    assert v.lib.vah_residual_layernorm_bwd_bsum(*args, _p(bpart), None, _stream()) == -1
    assert v.lib.vah_residual_layernorm_bwd_bsum(*args, _p(bpart) + 4, ctypes.byref(n), _stream()) == -4
    bad = list(args)
    bad[13] = _p(dz) + 2
    assert v.lib.vah_residual_layernorm_bwd_bsum(*bad, _p(bpart), ctypes.byref(n), _stream()) == -4
    assert v.lib.vah_residual_layernorm_bwd(*bad, _stream()) == -4
    bad = list(args)
    bad[6] = None
    assert v.lib.vah_residual_layernorm_bwd_bsum(*bad, _p(bpart), ctypes.byref(n), _stream()) == -1
    assert v.lib.vah_residual_layernorm_bwd(*bad, _stream()) == -1


# ---------------------------------------------------------------------------------------
# scale-residual backward
# ---------------------------------------------------------------------------------------
def _run_sr(entry, g, z, gamma, s, batch, rpb, C, bsum):
    v = _lib()
    rows = batch * rpb
    dz = _nan(rows, C, dtype=torch.bfloat16)
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


@pytest.mark.parametrize('C', [196, 200, 768, 1024])
@pytest.mark.parametrize('rows', [1, 13, 2 * 1031])
@pytest.mark.parametrize('form', ['plain', 'gamma', 'no_scale'])
def test_scale_residual_bwd_bsum(form, rows, C):
    """batch 2 with distinct drop-path scales where the row count divides (2 * 1031); one batch element for 1 and 13 rows.
    Without a gamma the column-tiled kernel runs (2062 rows = 64 strips of 32 and a ragged one of 14), except at
    C = 196 (no multiple of 8), which like every gamma case takes the row-strip kernel (412 strips of 5 rows and one of 2)."""
    batch = 2 if rows % 2 == 0 else 1
    rpb = rows // batch
    gen = torch.Generator(device='cuda').manual_seed(3 * rows + C)
    g = torch.randn(rows, C, device='cuda', generator=gen)
    z = torch.randn(rows, C, device='cuda', generator=gen).to(torch.bfloat16)
    gamma = (torch.randn(C, device='cuda', generator=gen) * 0.3 + 1.0) if form == 'gamma' else None
    s = None if form == 'no_scale' else torch.tensor([1.0 / 0.7, 1.0 / 0.9][:batch], device='cuda')
    want, _, _ = _run_sr('vah_scale_residual_bwd', g, z, gamma, s, batch, rpb, C, False)
    got1, bp1, n1 = _run_sr('vah_scale_residual_bwd_bsum', g, z, gamma, s, batch, rpb, C, True)
    got2, bp2, n2 = _run_sr('vah_scale_residual_bwd_bsum', g, z, gamma, s, batch, rpb, C, True)
    assert sorted(want) == sorted(got1)
    for k in want:
        assert bool(torch.isfinite(want[k].float()).all()), k
        assert torch.equal(got1[k], want[k]) and torch.equal(got2[k], want[k]), k
    if form == 'gamma' or C % 8:          # the row-strip kernel: strips of ceil(rows / 512) rows
        per = (rows + 511) // 512
    else:                        # the column-tiled kernel: strips of a multiple of 32 rows
        per = _strip32(rows)
    assert n1 == n2 == (rows + per - 1) // per
    assert torch.equal(bp1[:n1 * C], bp2[:n2 * C])
    _check_partials(bp1, n1, got1['dz'], C, 'scale_residual_bwd_bsum %s %dx%d' % (form, rows, C))


def test_scale_residual_bwd_bsum_arguments():
    v = _lib()
    C, rows = 200, 13
    g, z = torch.randn(rows, C, device='cuda'), torch.randn(rows, C, device='cuda').to(torch.bfloat16)
    dz, bpart, n = _nan(rows, C, dtype=torch.bfloat16), _nan(v.lib.vah_reduce_ws_floats(C)), ctypes.c_int64(-1)
    f, parent = v.lib.vah_scale_residual_bwd_bsum, v.lib.vah_scale_residual_bwd
    extra = (_p(bpart), ctypes.byref(n))
    for bad, code in ((dict(g=_p(g) + 8), -4), (dict(dz=_p(dz) + 4), -4), (dict(z=None), -1), (dict(dz=None), -1)):
        a = dict(g=_p(g), z=_p(z), dz=_p(dz))
        a.update(bad)
        args = (a['g'], a['z'], None, None, 1, rows, C, a['dz'], None, None)
        assert parent(*args, _stream()) == code, bad
        assert f(*args, *extra, _stream()) == code, bad
    args = (_p(g), _p(z), None, None, 1, rows, C, _p(dz), None, None)
    assert f(*args, None, ctypes.byref(n), _stream()) == -1
    assert f(*args, _p(bpart), None, _stream()) == -1
    assert f(*args, _p(bpart) + 8, ctypes.byref(n), _stream()) == -4
    assert f(_p(g), _p(z), None, None, 0, rows, C, _p(dz), None, None, *extra, _stream()) == 0 and n.value == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz.float()).all())


# ---------------------------------------------------------------------------------------
# GELU backward
# ---------------------------------------------------------------------------------------
def _run_gelu(da, h):
    v = _lib()
    rows, C = h.shape
    dh = _nan(rows, C, dtype=torch.bfloat16)
    bpart, n = _nan(v.lib.vah_reduce_ws_floats(C)), ctypes.c_int64(-1)
    v.check(v.lib.vah_gelu_bwd_bsum_bf16(_p(da), _p(h), rows, C, _p(dh), _p(bpart), ctypes.byref(n), _stream()), 'gelu_bwd_bsum')
    torch.cuda.synchronize()
    return dh, bpart, n.value


def _ordered(t):
    """bf16 -> integers in which neighbouring values differ by 1 (and +0 == -0)"""
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


@pytest.mark.parametrize('C', [8, 264, 3072])
@pytest.mark.parametrize('rows', [1, 37, 4101])
def test_gelu_bwd_bsum(rows, C):
    gen = torch.Generator(device='cuda').manual_seed(rows + C)
    h = (torch.randn(rows, C, device='cuda', generator=gen) * 1.5).to(torch.bfloat16)
    da = torch.randn(rows, C, device='cuda', generator=gen).to(torch.bfloat16)
    dh1, bp1, n1 = _run_gelu(da, h)
    dh2, bp2, n2 = _run_gelu(da, h)
    assert bool(torch.isfinite(dh1.float()).all())
    assert torch.equal(dh1, dh2) and n1 == n2 and torch.equal(bp1[:n1 * C], bp2[:n2 * C])
    per = _strip32(rows)
    assert n1 == (rows + per - 1) // per
    ref = _gelu_ref64(da, h)
    assert bool(((dh1.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -20 * da.double().abs()).all())
    assert int((_ordered(dh1) - _ordered(_torch_gelu_bwd(da, h))).abs().max()) <= 1
    _check_partials(bp1, n1, dh1, C, 'gelu_bwd_bsum %dx%d' % (rows, C))


@pytest.mark.parametrize('lo,hi', [(0.0, 0.0), (0.0, 2.0 ** -6), (2.0 ** -6, 0.5), (0.5, 2.0), (2.0, 4.0), (4.0, 6.0), (6.0, 8.0)])
def test_gelu_bwd_values(lo, hi):
    """|h| in [lo, hi], both signs (+-0 in the first case, |h| = 8 exactly in the last): against the fp64 value of
    da * (Phi(h) + h phi(h)) from the same bf16 operands the budget is the bf16 rounding of the result, 2^-8 |ref|, plus
    the fp32 evaluation, 2^-20 |da| (erff and the 1 + erf cancellation in the negative tail are absolute errors of a few
    2^-24 on a factor of da); against torch's GeluBackward kernel no element may differ by more than one bf16 ulp."""
    rows, C = 64, 264
    gen = torch.Generator(device='cuda').manual_seed(int(hi * 1024) + 1)
    mag = lo + (hi - lo) * torch.rand(rows, C, device='cuda', generator=gen)
    sign = torch.where(torch.rand(rows, C, device='cuda', generator=gen) < 0.5, -1.0, 1.0)
    h = (mag * sign).to(torch.bfloat16)
    if hi == 8.0:
        h[0, :8] = torch.tensor([8.0, -8.0] * 4, device='cuda').to(torch.bfloat16)
        assert float(h.float().abs().max()) == 8.0
    if hi == 0.0:
        assert bool((h.view(torch.int16) < 0).any()) and bool((h.view(torch.int16) == 0).any()), 'both zeros'
    da = (torch.randn(rows, C, device='cuda', generator=gen) * 3).to(torch.bfloat16)
    dh, bpart, n = _run_gelu(da, h)
    ref = _gelu_ref64(da, h)
    err = (dh.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * da.double().abs()
    steps = (_ordered(dh) - _ordered(_torch_gelu_bwd(da, h))).abs()
    print('|h| in [%g, %g]: worst error / budget %.3f; differs from torch in %d of %d elements (max %d ulp)'
          % (lo, hi, float((err / bound.clamp_min(1e-300)).max()), int((steps > 0).sum()), steps.numel(), int(steps.max())))
    assert bool((err <= bound).all())
    assert int(steps.max()) <= 1
    _check_partials(bpart, n, dh, C, 'gelu values')


# ---------------------------------------------------------------------------------------
# end to end: a ViT block
# ---------------------------------------------------------------------------------------
DIM, HEADS, TOK = 256, 4, 196


def _block():
    from vitadapter.backbones import vit
    torch.manual_seed(7)
    blk = vit.Block(DIM, HEADS, qkv_bias=True, drop_path=0.3).cuda().train()
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    x = torch.randn(2, TOK, DIM, device='cuda')
    gout = torch.randn(2, TOK, DIM, device='cuda')
    return blk, x, gout


def _step(blk, x, gout, seed=123):
    """forward + backward under bf16 autocast from a fixed RNG state (the drop-path draws) -> output, all gradients"""
    blk.zero_grad(set_to_none=True)
    xr = x.detach().clone().requires_grad_(True)
    torch.manual_seed(seed)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = blk(xr, 14, 14)
    (out.float() * gout).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in blk.named_parameters()}
    grads['x'] = xr.grad.detach().clone()
    return out.detach().clone(), grads


def test_block_bias_gradients_and_launches(monkeypatch):
    from vitadapter import fused
    v = _lib()
    blk, x, gout = _block()
    assert fused.ENABLED['bias_partials'] is True

    def profiled(seed=123):
        v.prof_enable(True, 'colsum_,gelu_')
        try:
            res = _step(blk, x, gout, seed)
        finally:
            v.prof_enable(False)
        return res, {k: r['calls'] for k, r in v.prof_report().items()}

    (out_on, g_on), calls_on = profiled()
    assert fused.BIAS_PARTIALS.passes == {}, 'the pass left nothing behind'
    # the switched-off run, with the dY of every Linear captured on the way
    dys = {}
    names = {id(m): n for n, m in blk.named_modules()}
    plain_linear = fused.linear

    def linear_with_hook(lin, t):
        y = plain_linear(lin, t)
        y.register_hook(lambda g, key=names[id(lin)]: dys.__setitem__(key, g.detach().clone()))
        return y

    monkeypatch.setitem(fused.ENABLED, 'bias_partials', False)
    monkeypatch.setattr(fused, 'linear', linear_with_hook)
    (out_off, g_off), calls_off = profiled()
    monkeypatch.undo()
    assert calls_on == {'colsum_bf16': 1, 'gelu_bwd': 1}, calls_on         # qkv's column sum is all that is left
    assert calls_off == {'colsum_bf16': 4}, calls_off
    assert torch.equal(out_on, out_off)
    bias_keys = ('attn.proj.bias', 'mlp.fc1.bias', 'mlp.fc2.bias')
    for k in g_off:
        assert bool(torch.isfinite(g_on[k]).all()), k
        if k not in bias_keys:
            assert torch.equal(g_on[k], g_off[k]), k
    for k in bias_keys:
        dy = dys[k[:-len('.bias')]]
        assert dy.dtype == torch.bfloat16
        d = dy.reshape(-1, dy.shape[-1]).double()
        want, budget = d.sum(0), BUDGET * d.abs().sum(0)
        for side, g in (('on', g_on), ('off', g_off)):
            err = (g[k].double() - want).abs()
            print('%s %s: worst column error / budget %.3f' % (k, side, float((err / budget).max())))
            assert bool((err <= budget).all()), (k, side)


def test_block_in_a_captured_graph():
    """forward + backward captured into a graph and replayed twice: every gradient equals the eager run's bit for bit
    (the registry runs on host state only; the drop-path draws follow the generator, reseeded before each run)."""
    from vitadapter import fused
    blk, x, gout = _block()
    out_e, g_e = _step(blk, x, gout)
    xs = x.detach().clone().requires_grad_(True)

    def body():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = blk(xs, 14, 14)
        (out.float() * gout).sum().backward()
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            blk.zero_grad(set_to_none=True)
            xs.grad = None
            body()
    torch.cuda.current_stream().wait_stream(side)
    blk.zero_grad(set_to_none=True)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = body()
    assert fused.BIAS_PARTIALS.passes == {}
    for _ in range(2):
        torch.manual_seed(123)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_g, out_e)
        assert torch.equal(xs.grad, g_e['x'])
        for k, p in blk.named_parameters():
            assert torch.equal(p.grad, g_e[k]), k
