"""GPU: the Linear layers under fp16 autocast on the GEMM dispatcher (vitadapter/fused.py: linear, gelu, forward_epoch,
the weight copies, the side stream and the bias partials on fp16 operands; ENABLED['fp16_linear']).

The module is the ViT block of tests/test_bias_partials_gpu.py (dim 256, 4 heads, 196 tokens), run with the loss scaled
by 512 as the reference's fp16 configs do.  Nothing here tunes live: a module fixture puts the dispatcher into mode 0
(hipBLASLt's first heuristic answer) and restores the environment's setting afterwards.

Bounds of the switched-off comparison.  With the switch off the Linears are torch's fp16 library GEMMs: other
accumulation orders (results that differ by an fp16 rounding flip here and there, one ulp = 2^-10 relative), dW and db
rounded to fp16 (2^-11 relative per element) where the dispatcher writes them in fp32.  Between the block's input and
any gradient lie at most 12 tensors stored in fp16 (qkv, attention output, proj, fc1, GELU, fc2 and their gradients);
with one rounding's worth of difference, 2^-11, allowed at each of them and the parameter gradient's own rounding on
top, every tensor has to agree with the fused run to 16 * 2^-11 in relative L2 norm - and, so that a few wrong elements
cannot hide in a norm, every element to 16 * 2^-11 of the tensor's largest magnitude."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DIM, HEADS, TOK = 256, 4, 196
BUDGET = 64 * 2.0 ** -24
F16 = torch.float16
NEW_ROWS = ('gemm_nt_f16', 'gemm_nn_f16', 'gemm_tn_fin_f16', 'gelu_bwd_f16')
FILTER = 'gemm_,gelu_bwd,colsum_bf16,colsum_f16'


def _lib():
    import _vah
    return _vah


@pytest.fixture(scope='module', autouse=True)
def _no_live_tuning():
    v = _lib()
    v.check(v.lib.vah_gemm_set_tuning(0, 32), 'gemm_set_tuning')
    yield
    spec = [int(t) for t in os.environ.get('VAH_GEMM_TUNING', '1,32').split(',')]
    v.check(v.lib.vah_gemm_set_tuning(spec[0], spec[1] if len(spec) > 1 else 32), 'gemm_set_tuning')


def _block(drop_path=0.3):
    from vitadapter.backbones import vit
    torch.manual_seed(7)
    blk = vit.Block(DIM, HEADS, qkv_bias=True, drop_path=drop_path).cuda().train()
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
    x = torch.randn(2, TOK, DIM, device='cuda')
    gout = torch.randn(2, TOK, DIM, device='cuda')
    return blk, x, gout


def _step(blk, x, gout, dtype=F16, seed=123, epoch=False):
    """forward + backward under autocast from a fixed RNG state, the loss scaled by 512 (a sum over the elements divided
    by the token count: |dY| of a few units) -> output, the scaled gradients as autograd left them"""
    from vitadapter import fused
    blk.zero_grad(set_to_none=True)
    xr = x.detach().clone().requires_grad_(True)
    scaler = torch.amp.GradScaler('cuda', init_scale=512.)
    torch.manual_seed(seed)
    with torch.autocast('cuda', dtype=dtype):
        if epoch:
            with fused.forward_epoch(blk):
                out = blk(xr, 14, 14)
        else:
            out = blk(xr, 14, 14)
    scaler.scale((out.float() * gout).sum() / TOK).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in blk.named_parameters()}
    grads['x'] = xr.grad.detach().clone()
    return out.detach().clone(), grads


def _profiled(fn):
    v = _lib()
    v.prof_enable(True, FILTER)
    try:
        res = fn()
    finally:
        v.prof_enable(False)
    return res, {k: r['calls'] for k, r in v.prof_report().items()}


def _f16_name(row):
    return 'colsum_f16' if row == 'colsum_bf16' else row + '_f16'


def test_block_runs_on_the_dispatcher_under_fp16(monkeypatch):
    from vitadapter import fused
    blk, x, gout = _block()
    assert fused.ENABLED['fp16_linear'] is True
    (_, _), rows_bf = _profiled(lambda: _step(blk, x, gout, torch.bfloat16))
    # the fp16 run, with the dY of every Linear captured on the way (a hook that returns nothing leaves the gradient as is)
    dys = {}
    names = {id(m): n for n, m in blk.named_modules()}
    plain_linear = fused.linear

    def linear_with_hook(lin, t):
        y = plain_linear(lin, t)
        y.register_hook(lambda g, key=names[id(lin)]: dys.__setitem__(key, g.detach().clone()))
        return y

    monkeypatch.setattr(fused, 'linear', linear_with_hook)
    (out_on, g_on), rows16 = _profiled(lambda: _step(blk, x, gout))
    monkeypatch.undo()
    assert fused.BIAS_PARTIALS.passes == {}, 'the pass left nothing behind'
    print('ROWS bf16 %s' % sorted(rows_bf.items()))
    print('ROWS fp16 %s' % sorted(rows16.items()))
    for r in NEW_ROWS:
        assert rows16.get(r, 0) > 0, (r, rows16)
    assert not [r for r in rows16 if not r.endswith('_f16')], rows16        # no unsuffixed gemm_*, gelu_bwd, colsum_bf16
    assert rows_bf and not any(r.endswith('_f16') for r in rows_bf), rows_bf
    assert rows16 == {_f16_name(r): n for r, n in rows_bf.items()}, (rows16, rows_bf)
    assert rows16.get('colsum_f16', 0) == 1, rows16                         # qkv's: its dY comes from the attention kernel
    assert out_on.dtype == torch.float32 and bool(torch.isfinite(out_on).all())
    biased = [n for n, m in blk.named_modules() if isinstance(m, torch.nn.Linear) and m.bias is not None]
    assert len(biased) >= 3 and all(n in dys for n in biased), (biased, sorted(dys))
    for n, m in blk.named_modules():
        if isinstance(m, torch.nn.Linear):
            assert m.weight.grad.dtype == torch.float32 and bool(torch.isfinite(m.weight.grad).all()), n
    for n in biased:
        dy = dys[n]
        assert dy.dtype == F16
        d = dy.reshape(-1, dy.shape[-1]).double()
        want, budget = d.sum(0), BUDGET * d.abs().sum(0)
        err = (g_on[n + '.bias'].double() - want).abs()
        print('%s.bias: worst column error / budget %.3f' % (n, float((err / budget).max())))
        assert bool((err <= budget).all()), n

    # switched off: torch's library calls, none of the new rows, and the same numbers within the bounds of the docstring
    monkeypatch.setitem(fused.ENABLED, 'fp16_linear', False)
    (out_off, g_off), rows_off = _profiled(lambda: _step(blk, x, gout))
    monkeypatch.undo()
    assert rows_off == {}, rows_off
    tol = 16 * 2.0 ** -11

    def rel(a, b):
        a, b = a.double(), b.double()
        assert float((a - b).abs().max()) <= tol * float(b.abs().max()), 'an element off by more than the bound'
        return float((a - b).norm()) / float(b.norm())

    worst = ('out', rel(out_off, out_on))
    assert worst[1] <= tol, worst
    assert set(g_off) == set(g_on)
    for k in g_on:
        assert bool(torch.isfinite(g_off[k]).all()) and bool(torch.isfinite(g_on[k]).all()), k
        r = rel(g_off[k], g_on[k])
        worst = max(worst, (k, r), key=lambda kv: kv[1])
        assert r <= tol, (k, r)
    print('switch off vs fused: worst relative L2 %.5f (%s), bound %.5f' % (worst[1], worst[0], tol))


def test_copies_are_kept_per_type():
    """The same module under bf16, then fp16, then bf16, inside forward epochs (the bulk copies): each run equals a
    fresh module's run under that type bit for bit - no run is served the other type's weight copy."""
    blk, x, gout = _block(drop_path=0.0)
    want = {}
    for dt in (torch.bfloat16, F16):
        fresh, _, _ = _block(drop_path=0.0)
        want[dt] = _step(fresh, x, gout, dt, epoch=True)
    for dt in (torch.bfloat16, F16, torch.bfloat16):
        out, grads = _step(blk, x, gout, dt, epoch=True)
        assert torch.equal(out, want[dt][0]), dt
        for k, g in grads.items():
            assert torch.equal(g, want[dt][1][k]), (dt, k)


def _lin_grads(lin, holder, xs, retain=False, extra_use=False):
    from vitadapter import fused
    lin.zero_grad(set_to_none=True)
    with torch.autocast('cuda', dtype=F16):
        total = 0
        for x in xs:
            with fused.forward_epoch(holder):
                y = fused.linear(lin, x)
            assert type(y.grad_fn).__name__ == '_LinearBF16Backward' and y.dtype == F16
            total = total + (y.float() ** 2).sum() / 64
            if extra_use:
                total = total + torch.nn.functional.linear(x.float(), lin.weight.float()).sum()
    total.backward(retain_graph=retain)
    if retain:
        total.backward()
    torch.cuda.synchronize()
    return lin.weight.grad.clone(), lin.bias.grad.clone()


@pytest.mark.parametrize('case', ['two_forwards_one_backward', 'retain_graph_double_backward', 'weight_used_by_another_op'])
def test_second_use_of_a_weight_under_fp16(case):
    """The rules of tests/test_weight_copies.py under fp16: gradients left on the side stream equal the main-stream
    gradients bit for bit, and equal the fp64 gradients of the same fp16 operands within the fp32-sum budget."""
    from vitadapter import fused
    torch.manual_seed(0)
    lin = torch.nn.Linear(64, 72).cuda()
    holder = torch.nn.ModuleList([lin])
    n = 2 if case == 'two_forwards_one_backward' else 1
    xs = [torch.randn(520, 64, device='cuda') for _ in range(n)]
    kw = dict(retain=case == 'retain_graph_double_backward', extra_use=case == 'weight_used_by_another_op')
    old = fused.ENABLED['wgrad_overlap']
    try:
        fused.ENABLED['wgrad_overlap'] = False
        want = _lin_grads(lin, holder, xs, **kw)
        fused.ENABLED['wgrad_overlap'] = True
        for _ in range(3):
            got = _lin_grads(lin, holder, xs, **kw)
            for g, w in zip(got, want):
                assert g.dtype == torch.float32 and torch.equal(g, w), case
    finally:
        fused.ENABLED['wgrad_overlap'] = old
    if kw['extra_use']:        # the other operator's share of dW is torch's (an fp16 product under autocast): not held here
        return
    # fp64 from the operands the GEMMs saw: y = fp16(x16 W16^T + b), dY = fp16(2 y / 64)
    gw, gb, mw, mb = 0, 0, 0, 0
    for x in xs:
        x16 = x.to(F16)
        y = fused.gemm_16(x16, lin.weight.detach().to(F16), trans_b=True, bias=lin.bias.detach()).double()
        dy = (2 * y.float() / 64).to(F16).double()
        gw, mw = gw + dy.t() @ x16.double(), mw + dy.abs().t() @ x16.double().abs()
        gb, mb = gb + dy.sum(0), mb + dy.abs().sum(0)
    k = 2 if kw['retain'] else 1
    assert bool(((want[0].double() - k * gw).abs() <= BUDGET * k * mw).all())
    assert bool(((want[1].double() - k * gb).abs() <= BUDGET * k * mb).all())


def test_parameter_edited_through_data_between_two_forwards():
    from vitadapter import fused
    torch.manual_seed(1)
    lin = torch.nn.Linear(64, 32).cuda()
    pair_a, pair_b = torch.nn.Linear(64, 16).cuda(), torch.nn.Linear(64, 8).cuda()
    x = torch.randn(128, 64, device='cuda', requires_grad=True)
    holder = torch.nn.ModuleList([lin, pair_a, pair_b])

    def run():
        with torch.autocast('cuda', dtype=F16), fused.forward_epoch(holder):
            y = fused.linear(lin, x)
            ya, yb = fused.linear_pair(pair_a, pair_b, x)
        assert y.dtype == ya.dtype == yb.dtype == F16
        assert type(ya.grad_fn).__name__ == '_LinearPairBF16Backward'
        return y, ya, yb

    w0 = lin.weight.detach().clone()
    y0, a0, b0 = run()
    for m in (lin, pair_a, pair_b):
        m.weight.data.mul_(2)             # does not bump Tensor._version
        m.bias.data.zero_()
    y1, a1, b1 = run()
    x16 = x.detach().to(F16).double()
    for got, m in ((y1, lin), (a1, pair_a), (b1, pair_b)):
        w16 = m.weight.detach().to(F16).double()
        want, mag = x16 @ w16.t(), x16.abs() @ w16.abs().t()
        assert bool(((got.double() - want).abs() <= BUDGET * mag + 2.0 ** -11 * want.abs() + 2.0 ** -25).all())
    assert not torch.allclose(y0.float(), y1.float())
    # the backward of the FIRST forward uses the copy of its own forward
    g = torch.randn_like(y0)
    (gx,) = torch.autograd.grad(y0, x, g)
    want, mag = g.double() @ w0.to(F16).double(), g.double().abs() @ w0.to(F16).double().abs()
    assert gx.dtype == torch.float32
    assert bool(((gx.double() - want).abs() <= BUDGET * mag + 2.0 ** -11 * want.abs() + 2.0 ** -25).all())


def test_block_step_in_a_captured_graph():
    """The fp16 block step captured after an eager warm-up of every shape (the dispatcher allocates and synchronises on
    the first use of a problem) and replayed twice with new inputs: bit-equal to the eager step on those inputs."""
    from vitadapter import fused
    blk, x, gout = _block()
    inputs = [torch.randn_like(x) for _ in range(2)]
    eager = [_step(blk, xi, gout) for xi in inputs]
    xs = x.detach().clone().requires_grad_(True)

    def body():
        with torch.autocast('cuda', dtype=F16):
            out = blk(xs, 14, 14)
        ((out.float() * gout).sum() / TOK * 512.).backward()
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
    for xi, (out_e, g_e) in zip(inputs, eager):
        with torch.no_grad():
            xs.copy_(xi)
        torch.manual_seed(123)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_g, out_e)
        assert torch.equal(xs.grad, g_e['x'])
        for k, p in blk.named_parameters():
            assert torch.equal(p.grad, g_e[k]), k
