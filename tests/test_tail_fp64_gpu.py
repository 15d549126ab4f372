"""GPU: every kernel of csrc/tail_ops.hip except bn_finalize_kernel (tests/test_spm_fp64_gpu.py holds that one) held
to fp64 (oracle/tail.py) at the production sizes of BASELINE configs[1]-[4] and at the edges of the kernels' own tiling.

Budgets (oracle/tail.py): |got - ref| <= C 2^-24 A (+ 2^-8 |ref| per bf16 rounding of the output); C = 256 for the
channel sums and the GEMMs, 128 for dxlo, 48 for the elementwise outputs; per tensor also ||err|| <= 0.5 ||budget||.
The layouts (interleave, token <-> plane transposes) and the max-pool are bit-exact against their index statements.

Every tail case, through the C ABI:
  * sums, y, da, db, dxlo and the whole workspace sit inside NaN buffers with a guard band on each side that must
    come back bit-unchanged; they are NaN-filled before each call, except dxlo at scale > 1, which the contract
    has zero-filled by the caller.  The workspace is NaN-filled, not zero-filled: the C planes of one (n, chunk)
    write every column of its partial row and tail_finalize reads the written rows only.
  * every call runs twice and must give the same bits, dxlo included: a low-res row's footprint is 2s hi-res rows
    and every tile but the last has at least 2s rows, so at most two workgroups add to a row, and a + b = b + a.
  * mean / rstd come from vah_bn_finalize_stats on the kernel's sums, mdy / mdyx = sums / count as fused._BNTail
    forms them; the references of the passes behind them start from these fp32 values.
  * the same case once more through fused.bn_tail / fused.bn_relu, forward and backward, must return the bits of
    the direct calls (weight and bias gradients: the backward sums).

Tiling edges (fill_operands): rows_per_block = 8192 / W rounded down to a multiple of 2s; W = 336: 24 rows, last
chunk 8; W = 168 at s = 2: 48 rows, last chunk 4 = 2s; 160 x 160: 48 rows, last chunk 16; N = 64 at 256 x 256 fills
the 512 partial rows exactly, N = 65 takes the second plan, N = 128 needs 80 KB of LDS (the raised-limit path),
N = 170 110 KB.  W / 4 = 84 and 42 are the non-power-of-two divisors of the quad decode.

Run with -s for one RATIO line per checked output and the worst ratio per family at the end.  Acceptance check for any
change to tail_ops.hip."""
import math

import pytest
import torch

from oracle import tail

pytestmark = pytest.mark.gpu

NAN = float('nan')
EPS, MOMENTUM = 1e-5, 0.1
GUARD = 4096                       # elements; keeps every output 16-byte aligned
BF, F32 = torch.bfloat16, torch.float32
f64 = torch.float64
WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for key in sorted(WORST):
        r, case = WORST[key]
        print('WORST %-24s %.4f (%s)' % (key, r, case))


def _record(family, case, r):
    print('RATIO %s %s %.4f' % (family, case, r))
    prev = WORST.get(family)
    if prev is None or r > prev[0]:
        WORST[family] = (r, case)


def _vah():
    import _vah
    return _vah


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ck(rc, what):
    _vah().check(rc, what)


def _p(t):
    return t.data_ptr() if t is not None else None


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    ia, ib = _bits(a), _bits(b)
    assert torch.equal(ia, ib), '%s: %d of %d elements differ in their bits' % (what, int((ia != ib).sum()), ia.numel())


class _Guarded:
    """a tensor of `shape` in the middle of a buffer with GUARD elements on each side; buffer and bands hold `fill`"""

    def __init__(self, shape, dtype, fill=NAN):
        self.n, self.fill = math.prod(shape), fill
        self.buf = torch.full((self.n + 2 * GUARD,), fill, dtype=dtype, device='cuda')
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        self.band = _bits(self.buf[:1]).clone()

    def reset(self, inner=None):
        self.buf.fill_(self.fill)
        if inner is not None:
            self.t.fill_(inner)
        return self

    def intact(self, what):
        for band in (self.buf[:GUARD], self.buf[GUARD + self.n:]):
            assert bool((_bits(band) == self.band).all()), '%s: a write landed in the guard band outside the output' % what


class _L2:
    """per tensor: every element within its budget (oracle check), and ||err|| <= 0.5 ||budget|| over the whole tensor,
    accumulated over the channel blocks"""

    def __init__(self, case):
        self.case, self.acc = case, {}

    def add(self, family, what, got, ref, A, c, bf16=False, mask=None):
        r = tail.check('%s %s' % (self.case, what), got, ref, A, bf16=bf16, mask=mask, c_acc=c)
        family += ' bf16' if bf16 else ' fp32'
        _record(family, self.case, r)
        if bf16:
            _record(family + ' (acc)', self.case, tail.rounding_excess(got, ref, A, mask, c_acc=c))
        err = (got.to(f64) - ref).abs()
        b = tail.bound(ref, A, bf16, c)
        if mask is not None:
            err, b = err[mask], b[mask]
        e = self.acc.setdefault(what, [0.0, 0.0])
        e[0] += float((err * err).sum())
        e[1] += float((b * b).sum())

    def finish(self):
        for what, (e2, b2) in self.acc.items():
            r = math.sqrt(e2) / math.sqrt(b2) if b2 > 0 else (0.0 if e2 == 0 else float('inf'))
            _record('L2 ' + what, self.case, r)
            assert r <= 0.5, '%s %s: ||err|| = %.3g ||budget||' % (self.case, what, r)


# ---------------------------------------------------------------------------------------------------------------
# the tail: vah_bn_tail_stats / apply / bwd_stats / bwd_apply
# ---------------------------------------------------------------------------------------------------------------
def _case(name, N, C, H, W, s, a=BF, b=None, x=True, shift=False, affine=True, relu=False, y=F32, dy=F32, evalm=False,
          big=False, wrapper=True):
    return pytest.param(dict(name=name, N=N, C=C, H=H, W=W, s=s, a=a, b=b, x=x, shift=shift, affine=affine, relu=relu, y=y,
                             dy=dy, evalm=evalm, big=big, wrapper=wrapper), id=name)


def _norm1(name, N, C, H, W, **kw):            # vit_adapter.py:170: bf16 up(c2) + c1, fp32 x at scale 4, the conv biases
    return _case(name, N, C, H, W, 4, a=BF, shift=True, **kw)


def _norm23(name, N, C, H, W, s, **kw):        # fp32 c2 / c3 from the token rows, scale 2 / 1
    return _case(name, N, C, H, W, s, a=F32, **kw)


TAIL_CASES = [
    _norm1('c2_norm1', 2, 768, 256, 256, big=True), _norm23('c2_norm2', 2, 768, 128, 128, 2), _norm23('c2_norm3', 2, 768, 64, 64, 1),
    _norm1('c1_norm1', 2, 192, 128, 128), _norm23('c1_norm2', 2, 192, 64, 64, 2, big=True), _norm23('c1_norm3', 2, 192, 32, 32, 1),
    _norm1('c3_norm1', 2, 1024, 160, 160), _norm23('c3_norm2', 2, 1024, 80, 80, 2), _norm23('c3_norm3', 2, 1024, 40, 40, 1, big=True),
    _norm1('c4_norm1', 1, 1024, 200, 336), _norm23('c4_norm2', 1, 1024, 100, 168, 2), _norm23('c4_norm3', 1, 1024, 50, 84, 1),
    _case('c1_norm1_two_operands', 2, 192, 128, 128, 4, a=BF, b=BF, shift=True, big=True),
    _norm1('cap_n64', 64, 4, 256, 256), _norm1('cap_n65', 65, 4, 256, 256), _norm1('cap_n128_lds80k', 128, 4, 256, 256),
    _norm1('cap_n170_lds110k', 170, 4, 256, 256), _norm23('cap_n512', 512, 4, 16, 16, 2),
    _case('scale8_tiles', 1, 4, 128, 256, 8, a=BF, shift=True), _case('scale8_fp32_b', 3, 5, 48, 64, 8, a=F32, b=F32),
    _case('one_quad_rows', 3, 5, 40, 4, 1, a=F32),
    _case('eval_norm1', 2, 24, 96, 32, 4, a=BF, b=BF, shift=True, evalm=True), _case('eval_norm2', 2, 16, 64, 48, 2, a=F32, evalm=True),
    _case('no_affine', 2, 16, 32, 48, 2, a=F32, affine=False, wrapper=False),
    _case('relu_stem', 2, 64, 512, 512, 1, a=BF, x=False, relu=True, y=BF, dy=BF),
    _case('relu_fp32', 2, 32, 512, 256, 1, a=F32, x=False, relu=True, y=F32, dy=F32),
]


def _tail_data(k):
    N, C, H, W, s = k['N'], k['C'], k['H'], k['W'], k['s']
    dev = 'cuda'
    if k['relu']:
        a = (torch.randn(N, C, H, W, device=dev) * 1.5 + 0.3).to(k['a'])
    else:
        # channel means that differ in sign; `big`: several standard deviations large, so that t - mean cancels
        cm = ((torch.randint(0, 2, (C,), device=dev) * 2 - 1).float() * 6.4 if k['big'] else torch.randn(C, device=dev) * 0.5)
        a = (torch.randn(N, C, H, W, device=dev) * 0.7 + cm.view(1, C, 1, 1)).to(k['a'])
    b = (torch.randn(N, C, H, W, device=dev) * 0.5 + 0.25).to(k['b']) if k['b'] is not None else None
    x = torch.randn(N, C, H // s, W // s, device=dev) * 0.7 if k['x'] else None
    shift = torch.randn(C, device=dev) * 0.7 if k['shift'] else None
    gamma = torch.randn(C, device=dev) * 0.3 + 1.0 if k['affine'] else None
    beta = torch.randn(C, device=dev) * 0.5 if k['affine'] else None
    dy = torch.randn(N, C, H, W, device=dev).to(k['dy'])
    rm, rv = torch.randn(C, device=dev) * 0.5, torch.rand(C, device=dev) * 1.5 + 0.5
    return a, b, x, shift, gamma, beta, dy, rm, rv


def _twice(what, call, outs):
    """run `call` twice on freshly reset outputs; same bits, guard bands intact; -> clones of the outputs"""
    res = []
    for _ in range(2):
        for g, inner in outs:
            g.reset(inner)
        call()
        torch.cuda.synchronize()
        for g, _i in outs:
            g.intact(what)
        res.append([g.t.clone() for g, _i in outs])
    for u, v in zip(*res):
        _same_bits(u, v, what + ' (second call)')
    return res[0]


def _direct_tail(k, a, b, x, shift, gamma, beta, dy, rm, rv):
    """the four passes through the C ABI as fused._BNTail strings them together"""
    lib = _vah().lib
    N, C, H, W, s = k['N'], k['C'], k['H'], k['W'], k['s']
    ops = (_p(a), int(a.dtype == BF), _p(b), int(b is not None and b.dtype == BF), _p(x), s, N, C, H, W)
    assert lib.vah_bn_tail_supported(N, C, H, W, s, int(x is not None)) == 1
    st = _st()
    ws = _Guarded((lib.vah_bn_tail_ws_floats(C),), F32)
    out = {}
    if not k['evalm']:
        sums = _Guarded((2 * C,), F32)
        out['sums'], = _twice(k['name'] + ' stats', lambda: _ck(lib.vah_bn_tail_stats(
            *ops, _p(shift), _p(sums.t), _p(ws.t), st), 'bn_tail_stats'), [(sums, None), (ws, None)])[:1]
        full = torch.cat([out['sums'], torch.full((1,), float(N * H * W), device='cuda')])
        mean, rstd = torch.full((C,), NAN, device='cuda'), torch.full((C,), NAN, device='cuda')
        _ck(lib.vah_bn_finalize_stats(_p(full), C, EPS, MOMENTUM, _p(rm), _p(rv), _p(mean), _p(rstd), st), 'bn_finalize_stats')
        count = full[2 * C:]
    else:
        mean, rstd = rm.float().contiguous(), torch.rsqrt(rv.float() + EPS)
    out['mean'], out['rstd'] = mean, rstd
    y = _Guarded((N, C, H, W), k['y'])
    out['y'], = _twice(k['name'] + ' apply', lambda: _ck(lib.vah_bn_tail_apply(
        *ops, _p(mean), _p(rstd), _p(gamma), _p(beta), int(k['relu']), _p(shift), _p(y.t), int(k['y'] == BF), st),
        'bn_tail_apply'), [(y, None)])
    del y
    sums2 = _Guarded((2 * C,), F32)
    out['bsums'], = _twice(k['name'] + ' bwd_stats', lambda: _ck(lib.vah_bn_tail_bwd_stats(
        *ops, _p(mean), _p(rstd), _p(gamma), _p(beta), int(k['relu']), _p(shift), _p(dy), int(dy.dtype == BF), _p(sums2.t),
        _p(ws.t), st), 'bn_tail_bwd_stats'), [(sums2, None), (ws, None)])[:1]
    means = out['bsums'] / count if not k['evalm'] else torch.zeros_like(out['bsums'])
    out['mdy'], out['mdyx'] = means[:C], means[C:]
    da = _Guarded((N, C, H, W), a.dtype)
    db = _Guarded((N, C, H, W), b.dtype) if b is not None else None
    # dxlo: zero-filled by contract where the adjoint adds into it (scale > 1), NaN where it is stored (scale 1)
    dx = _Guarded(tuple(x.shape), F32) if x is not None else None
    outs = [(da, None)] + ([(db, None)] if db is not None else []) + ([(dx, 0.0 if s > 1 else None)] if dx is not None else [])
    res = _twice(k['name'] + ' bwd_apply', lambda: _ck(lib.vah_bn_tail_bwd_apply(
        *ops, _p(mean), _p(rstd), _p(gamma), _p(beta), int(k['relu']), _p(shift), _p(dy), int(dy.dtype == BF), _p(means[:C]),
        _p(means[C:]), _p(da.t), _p(db.t) if db is not None else None, _p(dx.t) if dx is not None else None, st),
        'bn_tail_bwd_apply'), outs)
    out['da'] = res[0]
    out['db'] = res[1] if db is not None else None
    out['dxlo'] = res[-1] if dx is not None else None
    return out


def _check_tail(k, a, b, x, shift, gamma, beta, dy, out):
    """every output against the fp64 statement, a block of channels at a time"""
    N, C, H, W, s, relu, name = k['N'], k['C'], k['H'], k['W'], k['s'], k['relu'], k['name']
    cb = max(1, min(C, (48 << 20) // (N * H * W)))
    l2 = _L2(name)
    left_out = 0
    for c0 in range(0, C, cb):
        sl = slice(c0, min(C, c0 + cb))

        def ch(v):
            return v[sl] if v is not None else None

        def two(v):
            return torch.cat([v[sl], v[C + sl.start:C + sl.stop]])

        t, At = tail.tail_sum(a[:, sl], b[:, sl] if b is not None else None, x[:, sl] if x is not None else None, s, ch(shift))
        if not k['evalm']:
            ref, A = tail.stats(t, At)
            l2.add('tail sums', 'sums', two(out['sums']), ref, A, tail.C_ACC)
        mean, rstd = ch(out['mean']), ch(out['rstd'])
        ref, A, pre, edge = tail.apply(t, At, mean, rstd, ch(gamma), ch(beta), relu)
        l2.add('tail y', 'y', out['y'][:, sl], ref, A, tail.C_ELT, bf16=k['y'] == BF)
        del ref, A
        ref, A = tail.bwd_stats(t, At, dy[:, sl], mean, rstd, pre, edge, relu)
        l2.add('tail backward sums', 'bsums', two(out['bsums']), ref, A, tail.C_ACC)
        ref, A = tail.bwd_apply(t, At, dy[:, sl], mean, rstd, ch(gamma), pre, relu, ch(out['mdy']), ch(out['mdyx']))
        keep = ~edge if relu else None
        left_out += int(edge.sum())
        l2.add('tail da', 'da', out['da'][:, sl], ref, A, tail.C_ELT, bf16=a.dtype == BF, mask=keep)
        if b is not None:
            l2.add('tail db', 'db', out['db'][:, sl], ref, A, tail.C_ELT, bf16=b.dtype == BF, mask=keep)
        if x is not None:
            lo, LA = tail.upsample_t(ref, s)[0], tail.upsample_t(A, s)[0]
            l2.add('tail dxlo' if s > 1 else 'tail dxlo (scale 1)', 'dxlo', out['dxlo'][:, sl], lo, LA,
                   tail.C_LO if s > 1 else tail.C_ELT)          # scale 1: dt itself, stored
        del t, At, ref, A, pre, edge
    l2.finish()
    # a condition, not a measurement: the exclusion must not be able to hide a broken mask
    assert left_out <= 1e-4 * a.numel(), '%s: %d elements at the ReLU edge' % (name, left_out)
    if relu:
        print('RELU-EDGE %s left out %d of %d' % (name, left_out, a.numel()))


def _wrapper_tail(k, a, b, x, shift, gamma, beta, dy, rm, rv, out):
    """the same case through fused.bn_tail / fused.bn_relu: the direct calls' bits"""
    from vitadapter import fused
    C = k['C']
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM, affine=True).cuda()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    bn.train(not k['evalm'])
    leaves = [v.detach().clone().requires_grad_(True) if v is not None else None for v in (a, b, x, shift)]
    a2, b2, x2, sh2 = leaves
    with torch.autocast('cuda', dtype=BF):
        if k['relu']:
            assert fused.ENABLED['bn_relu'] and fused._bn_fusable(bn, a2) and a2.numel() >= fused.BN_RELU_MIN_NUMEL
            y = fused.bn_relu(bn, a2)
        else:
            assert fused.ENABLED['bn_tail'] and fused._bn_fusable(bn, a2)
            y = fused.bn_tail(bn, a2, b2, x2, k['s'], sh2)
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith('_BNTail'), 'the fused path did not run'
    _same_bits(y.detach(), out['y'], k['name'] + ' fused y')
    y.backward(dy)
    _same_bits(a2.grad, out['da'], k['name'] + ' fused da')
    if b is not None:
        _same_bits(b2.grad, out['db'], k['name'] + ' fused db')
    if x is not None:
        _same_bits(x2.grad, out['dxlo'], k['name'] + ' fused dxlo')
    _same_bits(bn.bias.grad, out['bsums'][:C], k['name'] + ' fused dbias')
    _same_bits(bn.weight.grad, out['bsums'][C:], k['name'] + ' fused dweight')
    if shift is not None:
        if k['evalm']:
            # d/d(shift) with running statistics = gamma rstd sum(dy): two more roundings on the checked sum
            ref = gamma.double() * out['rstd'].double() * out['bsums'][:C].double()
            tail.check(k['name'] + ' dshift', sh2.grad, ref, ref.abs(), c_acc=4.0)
        else:
            assert not bool(sh2.grad.any()), 'BatchNorm in training removes channel constants'


@pytest.mark.parametrize('k', TAIL_CASES)
def test_tail_passes(k):
    torch.manual_seed(1000 + sum(k[n] for n in 'NCHWs'))
    data = _tail_data(k)
    a, b, x, shift, gamma, beta, dy, rm, rv = data
    out = _direct_tail(k, a, b, x, shift, gamma, beta, dy, rm.clone(), rv.clone())
    _check_tail(k, a, b, x, shift, gamma, beta, dy, out)
    if k['wrapper']:
        _wrapper_tail(k, a, b, x, shift, gamma, beta, dy, rm, rv, out)


# beyond the limits of the fused path: the batch above the 512 partial rows of the workspace, and a second-plan tile
# above 150 KB of LDS.  The C ABI refuses them alike in all four entry points, on the host; fused.bn_tail then
# evaluates the reference expression, which is held to the same fp64 statement.  Its statistics are torch's, not
# the kernel's, so the reference takes mean and rstd in fp64 as well and the budgets carry their conditioning:
# an error of the mean moves every y of the channel by |sc| mean(A_t) C 2^-24, one of rstd by |y - beta| kappa,
# (and in the backward: dt's terms by 1 + kappa, the two means by their own sums' budgets)
# kappa = (E t^2 + mean^2) / (var + eps) (the cancellation in var = E t^2 - mean^2, as oracle/spm.finalize_stats).
@pytest.mark.parametrize('N,C,H,W,s', [(513, 4, 8, 8, 1), (171, 2, 256, 256, 4)], ids=['n513', 'n171_lds160k'])
def test_tail_beyond_the_fused_limits(N, C, H, W, s):
    from vitadapter import fused
    lib = _vah().lib
    torch.manual_seed(N)
    a = torch.randn(N, C, H, W, device='cuda') * 0.7 + torch.randn(C, device='cuda').view(1, C, 1, 1) * 0.5
    x = torch.randn(N, C, H // s, W // s, device='cuda') * 0.7
    dy = torch.randn(N, C, H, W, device='cuda')
    gamma, beta = torch.randn(C, device='cuda') * 0.3 + 1.0, torch.randn(C, device='cuda') * 0.5
    # real pointers: a refusal is decided before any launch
    v = [torch.zeros(2 * C, device='cuda') for _ in range(6)]
    ws = torch.zeros(lib.vah_bn_tail_ws_floats(C), device='cuda')
    ops = (_p(a), 0, None, 0, _p(x), s, N, C, H, W)
    da, dx = torch.zeros_like(a), torch.zeros_like(x)
    rcs = [lib.vah_bn_tail_stats(*ops, None, _p(v[0]), _p(ws), _st()),
           lib.vah_bn_tail_apply(*ops, _p(v[1]), _p(v[2]), None, None, 0, None, _p(da), 0, _st()),
           lib.vah_bn_tail_bwd_stats(*ops, _p(v[1]), _p(v[2]), None, None, 0, None, _p(dy), 0, _p(v[3]), _p(ws), _st()),
           lib.vah_bn_tail_bwd_apply(*ops, _p(v[1]), _p(v[2]), None, None, 0, None, _p(dy), 0, _p(v[4]), _p(v[5]), _p(da), None,
                                     _p(dx), _st())]
    torch.cuda.synchronize()
    assert rcs == [-2] * 4 and lib.vah_bn_tail_supported(N, C, H, W, s, 1) == 0
    assert not bool(da.any()) and not bool(dx.any()) and not bool(ws.any())
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    a2, x2 = a.clone().requires_grad_(True), x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=BF):
        y = fused.bn_tail(bn, a2, None, x2, s)
    assert y.dtype == F32
    y.backward(dy)
    t, At = tail.tail_sum(a, None, x, s, None)
    cnt = N * H * W
    sums, _ = tail.stats(t, At)
    mean = sums[:C] / cnt
    ex2 = sums[C:] / cnt
    var = ex2 - mean * mean
    rstd = 1.0 / torch.sqrt(var + EPS)
    kappa = ((ex2 + mean * mean) / (var + EPS)).view(1, C, 1, 1)
    ref, A, pre, edge = tail.apply(t, At, mean, rstd, gamma, beta, False)
    sc = (rstd * gamma.double()).abs().view(1, C, 1, 1)
    A = A + sc * At.mean((0, 2, 3), keepdim=True) + (ref - beta.double().view(1, C, 1, 1)).abs() * kappa
    name = 'beyond n%d' % N
    _record('tail reference path', name, tail.check(name + ' y', y.detach(), ref, A))
    bs, BA = tail.bwd_stats(t, At, dy, mean, rstd, pre, edge, False)
    dt, DA = tail.bwd_apply(t, At, dy, mean, rstd, gamma, pre, False, bs[:C] / cnt, bs[C:] / cnt)
    xh = ((t - mean.view(1, C, 1, 1)) * rstd.view(1, C, 1, 1)).abs()
    DA = DA * (1.0 + kappa) + sc * (BA[:C].view(1, C, 1, 1) + BA[C:].view(1, C, 1, 1) * (1.0 + xh)) / cnt
    _record('tail reference path', name, tail.check(name + ' da', a2.grad, dt, DA))
    lo, LA = tail.upsample_t(dt, s)[0], tail.upsample_t(DA, s)[0]
    _record('tail reference path', name, tail.check(name + ' dx', x2.grad, lo, LA))


# ---------------------------------------------------------------------------------------------------------------
# NCHW max-pool: vah_maxpool3s2_{fwd,bwd}_bf16
# ---------------------------------------------------------------------------------------------------------------
# (N, C, H, W, data): 'relu' = post-ReLU activations (ties among zeros), 'few' = three values (ties among maxima).
# W = 1344 / 2 = 672, 520 and 516 lie past the 512 input columns of one backward block; 516 is not a multiple of 8
POOL_CASES = [(2, 64, 512, 512, 'relu'), (2, 64, 512, 512, 'few'), (1, 64, 400, 672, 'relu'), (1, 64, 400, 672, 'few'),
              (2, 3, 30, 520, 'few'), (2, 3, 30, 516, 'relu'), (2, 3, 30, 516, 'few'), (1, 3, 17, 9, 'few'), (2, 2, 1, 1, 'relu'),
              (2, 2, 1, 8, 'few'), (2, 2, 2, 2, 'few'), (2, 2, 8, 1, 'relu'), (1, 3, 2, 17, 'few'), (1, 3, 19, 2, 'relu')]


@pytest.mark.parametrize('N,C,H,W,kind', POOL_CASES)
def test_nchw_max_pool(N, C, H, W, kind):
    from vitadapter import fused
    lib = _vah().lib
    torch.manual_seed(H * 7 + W)
    if kind == 'relu':
        x = torch.randn(N, C, H, W, device='cuda').clamp_min(0.).to(BF)
    else:
        x = torch.randint(0, 3, (N, C, H, W), device='cuda').to(BF)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    # gradients kept away from zero: the exponents of a pixel's terms stay within 2^9 of each other
    r = torch.randn(N, C, Ho, Wo, device='cuda')
    gy = (torch.where(r < 0, -1.0, 1.0) * (r.abs() + 2.0 ** -6)).to(BF)
    name = 'pool %dx%dx%dx%d %s' % (N, C, H, W, kind)
    y, idx = _Guarded((N, C, Ho, Wo), BF), _Guarded((N, C, Ho, Wo), torch.uint8, fill=0xEE)
    gy_, idx_ = _twice(name + ' fwd', lambda: _ck(lib.vah_maxpool3s2_fwd_bf16(_p(x), N * C, H, W, _p(y.t), _p(idx.t), _st()),
                                                  'maxpool_fwd'), [(y, None), (idx, None)])
    m, pos = tail.maxpool_forward(x.view(N * C, H, W))
    assert torch.equal(gy_.view(N * C, Ho, Wo).double(), m), name + ' y'
    assert torch.equal(idx_.view(N * C, Ho, Wo), pos), name + ' recorded position'
    gx = _Guarded((N, C, H, W), BF)
    got, = _twice(name + ' bwd', lambda: _ck(lib.vah_maxpool3s2_bwd_bf16(_p(gy), _p(idx_), N * C, H, W, _p(gx.t), _st()),
                                             'maxpool_bwd'), [(gx, None)])
    ref = tail.maxpool_backward(gy.view(N * C, Ho, Wo), pos, H, W)
    loose = tail.maxpool_inexact(gy.view(N * C, Ho, Wo), pos, H, W)
    assert int(loose.sum()) <= 8, name + ': the data should leave (almost) every fp32 sum exact'
    want = ref.to(BF)                      # one rounding: ref is an fp32 number outside `loose`
    got = got.view(N * C, H, W)
    differ = _bits(got) != _bits(want)
    assert not bool((differ & ~loose).any()), '%s gx: %d pixels differ' % (name, int((differ & ~loose).sum()))
    assert bool(((_bits(got).int() - _bits(want).int()).abs() <= 1).all()), name + ' gx: more than the last bit'
    # the wrapper
    pool = torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    x2 = x.clone().requires_grad_(True)
    y2 = fused.max_pool(pool, x2)
    assert type(y2.grad_fn).__name__.startswith('_MaxPool3s2')
    _same_bits(y2.detach(), gy_, name + ' fused y')
    y2.backward(gy)
    _same_bits(x2.grad.view(N * C, H, W), got, name + ' fused gx')


# ---------------------------------------------------------------------------------------------------------------
# sub-pixel interleave (vah_pixel_shuffle2_bf16) and fused.up_from_tokens
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C,h,w', [(2, 768, 128, 128), (2, 1024, 80, 80), (1, 1024, 100, 168), (3, 5, 3, 8)])
def test_interleave_is_the_index_expression(B, C, h, w):
    lib = _vah().lib
    torch.manual_seed(B * C + w)
    name = 'interleave %dx%dx%dx%d' % (B, C, h, w)
    U = torch.randn(B, 4 * C, h * w, device='cuda').to(BF)
    add = torch.randn(B, C, 2 * h, 2 * w, device='cuda').to(BF)
    planes = _Guarded((B, C, 2 * h, 2 * w), BF)
    got, = _twice(name, lambda: _ck(lib.vah_pixel_shuffle2_bf16(_p(U), B, C, h, w, _p(planes.t), 0, None, _st()), 'pixel_shuffle2'),
                  [(planes, None)])
    want = tail.interleave(U, C, h, w)
    _same_bits(got, want, name + ' forward')
    got_a, = _twice(name + ' + addend', lambda: _ck(lib.vah_pixel_shuffle2_bf16(_p(U), B, C, h, w, _p(planes.t), 0, _p(add), _st()),
                                                    'pixel_shuffle2'), [(planes, None)])
    _same_bits(got_a, (want.float() + add.float()).to(BF), name + ' forward + addend')       # one fp32 sum, one rounding
    back = _Guarded((B, 4 * C, h * w), BF)
    inv, = _twice(name + ' inverse', lambda: _ck(lib.vah_pixel_shuffle2_bf16(_p(got), B, C, h, w, _p(back.t), 1, None, _st()),
                                                 'pixel_shuffle2'), [(back, None)])
    _same_bits(inv, U, name + ' inverse(forward)')
    inv, = _twice(name + ' inverse', lambda: _ck(lib.vah_pixel_shuffle2_bf16(_p(add), B, C, h, w, _p(back.t), 1, None, _st()),
                                                 'pixel_shuffle2'), [(back, None)])
    _same_bits(inv, tail.deinterleave(add), name + ' inverse')


@pytest.mark.parametrize('with_add', [False, True], ids=['plain', 'addend'])
@pytest.mark.parametrize('B,h,w,C,Co', [(2, 128, 128, 768, 768), (1, 100, 168, 1024, 1024)])
def test_up_from_tokens_fp64(B, h, w, C, Co, with_add):
    """out, d rows (bf16) and d weight (fp32) of fused.up_from_tokens in fp64 on the bf16 operands.  With an addend the
    output is rounded to bf16 twice (the GEMM's U, then the sum): 2^-8 (|U| + |U + add|) on top of the fp32 term."""
    from vitadapter import fused
    torch.manual_seed(h + w + with_add)
    name = 'up %dx%dx%d %s' % (B, h, w, 'addend' if with_add else 'plain')
    up = torch.nn.ConvTranspose2d(C, Co, 2, 2).cuda()
    rows = torch.randn(B, h * w, C, device='cuda', requires_grad=True)
    add = torch.randn(B, Co, 2 * h, 2 * w, device='cuda').to(BF).requires_grad_(True) if with_add else None
    g = torch.randn(B, Co, 2 * h, 2 * w, device='cuda').to(BF)
    with torch.autocast('cuda', dtype=BF):
        out = fused.up_from_tokens(up, rows, h, w, add)
        assert out is not None and out.dtype == BF, 'the GEMM form did not run'
        out.backward(g)
    xb = rows.detach().to(BF)
    wc = tail.up_weight_rows(up.weight.detach().to(BF))
    for bi in range(B):
        Ur, UA = tail.up_product(xb[bi:bi + 1], wc)
        ref, A = tail.interleave(Ur, Co, h, w), tail.interleave(UA, Co, h, w)
        if with_add:
            tot = ref + add.detach()[bi:bi + 1].double()
            err = (out.detach()[bi:bi + 1].double() - tot).abs()
            bud = tail.C_ACC * tail.U * A + tail.BF16_U * (ref.abs() + tot.abs())
            r = float((err / bud).nan_to_num(0.0, posinf=float('inf')).max())
            assert r <= 1.0, '%s out: worst err / budget %.3g' % (name, r)
            _record('up_from_tokens out + addend', name, r)
        else:
            _record('up_from_tokens out', name, tail.check(name + ' out', out.detach()[bi:bi + 1], ref, A, bf16=True))
            _record('up_from_tokens out (acc)', name, tail.rounding_excess(out.detach()[bi:bi + 1], ref, A))
        del Ur, UA, ref, A
    dU = tail.deinterleave(g)
    wd = wc.double()
    dw, dwa = torch.zeros(4 * Co, C, dtype=f64, device='cuda'), torch.zeros(4 * Co, C, dtype=f64, device='cuda')
    for bi in range(B):
        d = dU[bi].double()
        ref, A = d.T @ wd, d.abs().T @ wd.abs()
        _record('up_from_tokens d rows', name, tail.check(name + ' d rows', rows.grad[bi], ref, A, bf16=True))
        _record('up_from_tokens d rows (acc)', name, tail.rounding_excess(rows.grad[bi], ref, A))
        dw += d @ xb[bi].double()
        dwa += d.abs() @ xb[bi].double().abs()
    def as_weight(m):
        return m.view(2, 2, Co, C).permute(3, 2, 0, 1)
    _record('up_from_tokens d weight', name, tail.check(name + ' d weight', up.weight.grad, as_weight(dw), as_weight(dwa)))
    if with_add:
        _same_bits(add.grad, g, name + ' d addend')


# ---------------------------------------------------------------------------------------------------------------
# token <-> plane layouts: vah_transpose_tokens
# ---------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [(2, 768, [(128, 128), (64, 64), (32, 32)]), (1, 1024, [(100, 168), (50, 84), (25, 42)]),
                (2, 192, [(64, 64), (32, 32), (16, 16)]), (3, 50, [(3, 7), (1, 33), (5, 1)])]
TOKEN_GUARD = 12345.0


@pytest.mark.parametrize('planes_dtype', [F32, BF], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('B,C,hw', LAYOUT_CASES)
def test_token_plane_layouts(B, C, hw, planes_dtype):
    from vitadapter import fused
    lib = _vah().lib
    torch.manual_seed(B * C)
    T = sum(h * w for h, w in hw)
    name = 'layout %dx%dx%d %s' % (B, T, C, 'bf16' if planes_dtype == BF else 'fp32')
    pb = int(planes_dtype == BF)
    tokens = torch.randn(B, T, C, device='cuda')
    t0, maps = 0, []
    for h, w in hw:
        dst = _Guarded((B, C, h * w), planes_dtype)
        got, = _twice(name + ' to planes', lambda: _ck(lib.vah_transpose_tokens(_p(tokens), B, T, t0, h * w, C, _p(dst.t), 1, pb, None,
                                                                                 _st()), 'transpose_tokens'), [(dst, None)])
        _same_bits(got, tail.tokens_to_planes(tokens, t0, h * w).to(planes_dtype), name + ' to planes')
        maps.append(got.view(B, C, h, w))
        t0 += h * w
    vecs = [torch.randn(C, device='cuda'), None, torch.randn(C, device='cuda')]
    t0, parts = 0, []
    for (h, w), m, v in zip(hw, maps, vecs):
        dst = _Guarded((B, T, C), F32, fill=TOKEN_GUARD)
        got, = _twice(name + ' to tokens', lambda: _ck(lib.vah_transpose_tokens(_p(m), B, T, t0, h * w, C, _p(dst.t), 0, pb, _p(v), _st()),
                                                       'transpose_tokens'), [(dst, None)])
        want = torch.full((B, T, C), TOKEN_GUARD, device='cuda')          # rows outside [t0, t0 + T) keep the guard value
        want[:, t0:t0 + h * w] = tail.planes_to_tokens(m.flatten(2), v)
        _same_bits(got, want, name + ' to tokens')
        parts.append(got[:, t0:t0 + h * w])
        t0 += h * w
    # the wrappers: the direct calls' bits, forward and backward
    tk = tokens.clone().requires_grad_(True)
    outs = fused.tokens_to_maps(tk, hw)
    assert type(outs[0].grad_fn).__name__.startswith('_TokensToMaps')
    gms = [torch.randn_like(o) for o in outs]
    if planes_dtype == F32:
        for o, m in zip(outs, maps):
            _same_bits(o.detach(), m, name + ' fused.tokens_to_maps')
    torch.autograd.backward(outs, gms)
    _same_bits(tk.grad, torch.cat([tail.planes_to_tokens(g.flatten(2), None) for g in gms], 1), name + ' fused.tokens_to_maps backward')
    ms = [m.clone().requires_grad_(True) for m in maps]
    vs = [v.clone().requires_grad_(True) if v is not None else None for v in vecs]
    tok = fused.maps_to_tokens(ms, vs)
    assert type(tok.grad_fn).__name__.startswith('_MapsToTokens')
    _same_bits(tok.detach(), torch.cat(parts, 1), name + ' fused.maps_to_tokens')
    gt = torch.randn_like(tok)
    tok.backward(gt)
    t0 = 0
    for (h, w), m in zip(hw, ms):
        _same_bits(m.grad, tail.tokens_to_planes(gt, t0, h * w).to(planes_dtype).view(B, C, h, w), name + ' fused.maps_to_tokens backward')
        t0 += h * w
