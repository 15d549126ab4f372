"""GPU: the fp16 instantiations of the output-tail kernels (csrc/tail_ops.hip: the `_f16` entry points, what fp16
autocast runs) held to fp64 (oracle/tail.py, which upcasts whatever 16-bit operands it is given) - the fp16 counterpart of
tests/test_tail_fp64_gpu.py, whose generators and discipline it imports: outputs, sums and workspaces NaN-filled inside
guard bands that must come back intact (dxlo zero-filled at scale > 1), every call twice with the same bits, and the
fused.* wrappers under fp16 autocast returning the direct calls' bits.

Budget.  16-bit operands are fp16, every sum is fp32, each fp16 output is rounded once at its store; sums, mean, rstd,
dxlo and the workspaces stay fp32.  Per element, with A and the chain constants of oracle/tail.py (C = 48 elementwise,
128 dxlo, 256 channel sums and GEMMs)

    |got - ref| <= C 2^-24 A                                  fp32 outputs
    |got - ref| <= C 2^-24 A + 2^-11 |ref| + 2^-25            fp16 outputs

2^-11 is fp16's round-to-nearest bound (11 significant bits), 2^-25 half the spacing of its subnormals: both follow from
the format.  Per tensor ||err|| <= 0.5 ||budget||.  The interleave, the token <-> plane transposes and the max-pool
(value, recorded position) are bit-exact against the index statements; the max-pool gradient is the fp16 rounding of the
exact sum wherever an fp32 sum of fp16 terms is exact (exponents within 11: 24 - 11 significant bits - 2 carry bits).

Shapes: the smallest at which these kernels take each of their paths (the bf16 file holds the production sizes).
rows_per_block = 8192 / W rounded down to a multiple of 2s: W = 336 at s = 4: 24 rows, H = 32 leaves a last chunk of
8 = 2s; W = 168 at s = 2: 48 rows, H = 52 leaves 4 = 2s; s = 8 at W = 256: 32 rows, H = 48 leaves 16 = 2s.  W / 4 = 84,
42 and 12 are the non-power-of-two divisors of the quad decode, W = 4 the one-quad row.  N = 65 at 256 x 256 takes the
second plan (N chunks > 512).  One production-size tail (2 x 768 x 256 x 256 at scale 4).

fp16 only:
  (a) dy drawn at 2^-18, where most fp16 values are subnormal: da / db held to the budget above with no extra term, and
      their subnormal results are there (not flushed);
  (b) the fp32 -> fp16 conversion of the store: vah_bn_tail_apply_f16 with mean 0, rstd 1, no affine on an fp32 `a` that
      sweeps ties, subnormals, +-65504, the first value that rounds to inf, and +-inf, bit for bit a.to(float16);
  (c) fused.up_from_tokens under fp16 autocast (torch's fp16 library GEMMs) against the fp64 product of the same fp16
      operands: 256 2^-24 A plus one fp16 rounding per stored product (U; U, then U + addend; d rows; for d weight one
      per image, the images summed in fp32).

Case (a) and the per-tensor rule.  Among fp16's subnormals a correctly rounded result errs uniformly within +-2^-25, an
error of norm 2^-25 / sqrt(3) = 0.577 2^-25 per element, while the budget of an element there is 2^-25 + 2^-11 |ref| (the
accumulation term is 2^-10 of that).  ||err|| <= 0.5 ||budget|| can therefore be met by exact rounding only where
0.577 <= 0.5 (1 + 2^14 |ref|), that is for results of typical size |ref| >= 0.155 2^-14 = 2^-16.7: the upper three
binades of the subnormal range.  The bf16 file's generators give gamma rstd of about 1, which would put da / db of
`subnormal_dy_norm1` at 2^-18, where no rounding of the fp64 reference meets the rule (torch's own scores 0.55).  The
case therefore multiplies that generator's gamma by 8: dy stays at 2^-18, da / db come to about 2^-15 (exact rounding
of normal values of that spread scores 0.40 - 0.43), more than half of them still subnormal, which is asserted, and a
flushed result would miss its element's budget by a factor of 2^9.  The "L2 ... (fp64 reference rounded to fp16)" rows printed with -s give what torch's own rounding of the fp64
reference scores under the same rule.  `subnormal_dy_relu` keeps the generator's gamma: half of its da are masked to
values far below 2^-25, whose budget they do not use.

Run with -s for one RATIO line per checked output and the worst ratio per family at the end."""
import math

import pytest
import torch

from oracle import tail
from test_tail_fp64_gpu import (EPS, MOMENTUM, TOKEN_GUARD, _bits, _ck, _Guarded, _p, _same_bits, _st, _tail_data, _twice,
                                _vah)

pytestmark = pytest.mark.gpu

NAN = float('nan')
F16, F32 = torch.float16, torch.float32
f64 = torch.float64
F16_U = 2.0 ** -11            # round to nearest with 11 significant bits
F16_SUB = 2.0 ** -25          # half the spacing of fp16's subnormals
F16_MIN_NORMAL = 2.0 ** -14
SCALED = 2.0 ** -18           # a loss-scaled output gradient: fp16 subnormals
WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for key in sorted(WORST):
        r, case = WORST[key]
        print('WORST f16 %-28s %.4f (%s)' % (key, r, case))


def _record(family, case, r):
    print('RATIO f16 %s %s %.4f' % (family, case, r))
    prev = WORST.get(family)
    if prev is None or r > prev[0]:
        WORST[family] = (r, case)


def _sym(name):
    return getattr(_vah().lib, _vah().TAIL_F16_TWINS[name])


def _bound(ref, A, c, f16):
    b = tail.bound(ref, A, False, c)
    return b + F16_U * ref.to(f64).abs() + F16_SUB if f16 else b


def _worst(err, b):
    if err.numel() == 0:
        return 0.0
    return float(torch.where(err == 0, torch.zeros_like(err), err / b).nan_to_num(float('inf')).max())


def _check(what, got, ref, A, c, f16, mask=None, bud=None):
    """every element within its budget -> (worst ratio, sum err^2, sum budget^2)"""
    assert got.dtype == (F16 if f16 else F32), what
    r64 = ref.to(f64)
    err = (got.to(f64) - r64).abs()
    b = _bound(ref, A, c, f16) if bud is None else bud
    bad = ~(err <= b)
    if mask is not None:
        bad &= mask
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError('%s: %d of %d elements over budget; first at flat %d: got %r ref %r budget %.3e (worst err / '
                             'budget %.3g)' % (what, int(bad.sum()), bad.numel(), i, got.reshape(-1)[i].item(),
                                               r64.reshape(-1)[i].item(), b.reshape(-1)[i].item(),
                                               _worst(err[bad], b[bad])))
    if mask is not None:
        err, b = err[mask], b[mask]
    return _worst(err, b), float((err * err).sum()), float((b * b).sum())


class _L2:
    """per tensor: every element within its budget, and ||err|| <= 0.5 ||budget|| over the whole tensor, accumulated over
    the channel blocks"""

    def __init__(self, case):
        self.case, self.acc = case, {}

    def add(self, family, what, got, ref, A, c, f16=False, mask=None):
        r, e2, b2 = _check('%s %s' % (self.case, what), got, ref, A, c, f16, mask)
        _record(family + (' fp16' if f16 else ' fp32'), self.case, r)
        e = self.acc.setdefault(what, [0.0, 0.0, 0.0])
        e[0] += e2
        e[1] += b2
        if f16:             # a figure, not a check: what the correctly rounded reference itself would score
            ideal = (ref.to(F16).to(f64) - ref).abs()
            e[2] += float(((ideal[mask] if mask is not None else ideal) ** 2).sum())

    def finish(self):
        for what, (e2, b2, i2) in self.acc.items():
            r = math.sqrt(e2) / math.sqrt(b2) if b2 > 0 else (0.0 if e2 == 0 else float('inf'))
            _record('L2 ' + what, self.case, r)
            if i2 > 0:
                _record('L2 ' + what + ' (fp64 reference rounded to fp16)', self.case, math.sqrt(i2) / math.sqrt(b2))
            assert r <= 0.5, '%s %s: ||err|| = %.3g ||budget||' % (self.case, what, r)


# ---------------------------------------------------------------------------------------------------------------
# the tail: vah_bn_tail_{stats,apply,bwd_stats,bwd_apply}_f16
# ---------------------------------------------------------------------------------------------------------------
def _case(name, N, C, H, W, s, a=F16, b=None, x=True, shift=False, affine=True, relu=False, y=F32, dy=F32, evalm=False,
          big=False, wrapper=True, dy_scale=1.0, gamma_scale=1.0):
    return pytest.param(dict(name=name, N=N, C=C, H=H, W=W, s=s, a=a, b=b, x=x, shift=shift, affine=affine, relu=relu, y=y,
                             dy=dy, evalm=evalm, big=big, wrapper=wrapper, dy_scale=dy_scale, gamma_scale=gamma_scale),
                        id=name)


TAIL_CASES = [
    # level 1's production form: fp16 up(c2), fp16 c1, fp32 x at scale 4, the conv biases; W / 4 = 84, chunks of 24 + 8 rows
    _case('norm1_two_operands_w336', 2, 6, 32, 336, 4, a=F16, b=F16, shift=True, big=True),
    _case('norm2_fp32_w168', 2, 5, 52, 168, 2, a=F32),                   # W / 4 = 42, chunks of 48 + 4 rows
    _case('norm3_fp32_scale1_w48', 2, 5, 50, 48, 1, a=F32),              # W / 4 = 12
    _case('fp16_a_alone', 2, 7, 24, 48, 2, a=F16),
    _case('fp16_a_fp32_b', 2, 4, 16, 64, 4, a=F16, b=F32, shift=True),
    _case('scale8_tiles', 1, 4, 48, 256, 8, a=F16, shift=True),          # chunks of 32 + 16 rows
    _case('scale8_fp32_b', 3, 5, 48, 64, 8, a=F32, b=F32),
    _case('one_quad_rows', 3, 5, 40, 4, 1, a=F16),                       # W / 4 == 1
    _case('second_plan_n65', 65, 2, 256, 256, 4, a=F16, shift=True),     # N chunks > 512
    _case('production_norm1', 2, 768, 256, 256, 4, a=F16, shift=True, big=True),
    _case('eval_norm1', 2, 24, 96, 32, 4, a=F16, b=F16, shift=True, evalm=True),
    _case('eval_norm2', 2, 16, 64, 48, 2, a=F32, evalm=True),
    _case('no_affine', 2, 16, 32, 48, 2, a=F16, affine=False, wrapper=False),
    _case('relu_fp16', 2, 8, 128, 256, 1, a=F16, x=False, relu=True, y=F16, dy=F16),
    _case('relu_fp32', 2, 8, 64, 256, 1, a=F32, x=False, relu=True, y=F32, dy=F32),
    # (a) loss-scaled gradients: dy, da, db in fp16's subnormal range (gamma x 8: da / db in its upper binades, see above)
    _case('subnormal_dy_norm1', 2, 6, 32, 336, 4, a=F16, b=F16, shift=True, dy=F16, dy_scale=SCALED, gamma_scale=8.0),
    _case('subnormal_dy_relu', 2, 8, 64, 256, 1, a=F16, x=False, relu=True, y=F16, dy=F16, dy_scale=SCALED),
]


def _data(k):
    a, b, x, shift, gamma, beta, dy, rm, rv = _tail_data(k)          # the bf16 file's generators, in this case's dtypes
    if k['dy_scale'] != 1.0:
        dy = (dy.float() * k['dy_scale']).to(k['dy'])
    if k['gamma_scale'] != 1.0:
        gamma = gamma * k['gamma_scale']
    return a, b, x, shift, gamma, beta, dy, rm, rv


def _direct_tail(k, a, b, x, shift, gamma, beta, dy, rm, rv):
    """the four passes through the C ABI as fused._BNTail strings them together"""
    lib = _vah().lib
    N, C, H, W, s = k['N'], k['C'], k['H'], k['W'], k['s']
    ops = (_p(a), int(a.dtype == F16), _p(b), int(b is not None and b.dtype == F16), _p(x), s, N, C, H, W)
    assert lib.vah_bn_tail_supported(N, C, H, W, s, int(x is not None)) == 1
    st = _st()
    ws = _Guarded((lib.vah_bn_tail_ws_floats(C),), F32)
    out = {}
    if not k['evalm']:
        sums = _Guarded((2 * C,), F32)
        out['sums'], = _twice(k['name'] + ' stats', lambda: _ck(_sym('vah_bn_tail_stats')(
            *ops, _p(shift), _p(sums.t), _p(ws.t), st), 'bn_tail_stats_f16'), [(sums, None), (ws, None)])[:1]
        full = torch.cat([out['sums'], torch.full((1,), float(N * H * W), device='cuda')])
        mean, rstd = torch.full((C,), NAN, device='cuda'), torch.full((C,), NAN, device='cuda')
        _ck(lib.vah_bn_finalize_stats(_p(full), C, EPS, MOMENTUM, _p(rm), _p(rv), _p(mean), _p(rstd), st), 'bn_finalize_stats')
        count = full[2 * C:]
    else:
        mean, rstd = rm.float().contiguous(), torch.rsqrt(rv.float() + EPS)
    out['mean'], out['rstd'] = mean, rstd
    y = _Guarded((N, C, H, W), k['y'])
    out['y'], = _twice(k['name'] + ' apply', lambda: _ck(_sym('vah_bn_tail_apply')(
        *ops, _p(mean), _p(rstd), _p(gamma), _p(beta), int(k['relu']), _p(shift), _p(y.t), int(k['y'] == F16), st),
        'bn_tail_apply_f16'), [(y, None)])
    del y
    sums2 = _Guarded((2 * C,), F32)
    out['bsums'], = _twice(k['name'] + ' bwd_stats', lambda: _ck(_sym('vah_bn_tail_bwd_stats')(
        *ops, _p(mean), _p(rstd), _p(gamma), _p(beta), int(k['relu']), _p(shift), _p(dy), int(dy.dtype == F16), _p(sums2.t),
        _p(ws.t), st), 'bn_tail_bwd_stats_f16'), [(sums2, None), (ws, None)])[:1]
    means = out['bsums'] / count if not k['evalm'] else torch.zeros_like(out['bsums'])
    out['mdy'], out['mdyx'] = means[:C], means[C:]
    da = _Guarded((N, C, H, W), a.dtype)
    db = _Guarded((N, C, H, W), b.dtype) if b is not None else None
    # dxlo: zero-filled by contract where the adjoint adds into it (scale > 1), NaN where it is stored (scale 1)
    dx = _Guarded(tuple(x.shape), F32) if x is not None else None
    outs = [(da, None)] + ([(db, None)] if db is not None else []) + ([(dx, 0.0 if s > 1 else None)] if dx is not None else [])
    res = _twice(k['name'] + ' bwd_apply', lambda: _ck(_sym('vah_bn_tail_bwd_apply')(
        *ops, _p(mean), _p(rstd), _p(gamma), _p(beta), int(k['relu']), _p(shift), _p(dy), int(dy.dtype == F16), _p(means[:C]),
        _p(means[C:]), _p(da.t), _p(db.t) if db is not None else None, _p(dx.t) if dx is not None else None, st),
        'bn_tail_bwd_apply_f16'), outs)
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
        l2.add('tail y', 'y', out['y'][:, sl], ref, A, tail.C_ELT, f16=k['y'] == F16)
        del ref, A
        ref, A = tail.bwd_stats(t, At, dy[:, sl], mean, rstd, pre, edge, relu)
        l2.add('tail backward sums', 'bsums', two(out['bsums']), ref, A, tail.C_ACC)
        ref, A = tail.bwd_apply(t, At, dy[:, sl], mean, rstd, ch(gamma), pre, relu, ch(out['mdy']), ch(out['mdyx']))
        keep = ~edge if relu else None
        left_out += int(edge.sum())
        l2.add('tail da', 'da', out['da'][:, sl], ref, A, tail.C_ELT, f16=a.dtype == F16, mask=keep)
        if b is not None:
            l2.add('tail db', 'db', out['db'][:, sl], ref, A, tail.C_ELT, f16=b.dtype == F16, mask=keep)
        if x is not None:
            lo, LA = tail.upsample_t(ref, s)[0], tail.upsample_t(A, s)[0]
            l2.add('tail dxlo' if s > 1 else 'tail dxlo (scale 1)', 'dxlo', out['dxlo'][:, sl], lo, LA,
                   tail.C_LO if s > 1 else tail.C_ELT)          # scale 1: dt itself, stored
        del t, At, ref, A, pre, edge
    # a condition, not a measurement: the exclusion must not be able to hide a broken mask
    assert left_out <= 1e-4 * a.numel(), '%s: %d elements at the ReLU edge' % (name, left_out)
    if relu:
        print('RELU-EDGE f16 %s left out %d of %d' % (name, left_out, a.numel()))
    return l2


def _wrapper_tail(k, a, b, x, shift, gamma, beta, dy, rm, rv, out, monkeypatch):
    """the same case through fused.bn_tail / fused.bn_relu under fp16 autocast: the direct calls' bits"""
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
    with torch.autocast('cuda', dtype=F16):
        assert fused.ENABLED['fp16_tail'] and fused._tail_dtype() == F16
        if k['relu']:
            # the size from which the two-pass form pays is a tuning constant; the test's shapes lie below it
            monkeypatch.setattr(fused, 'BN_RELU_MIN_NUMEL', 1)
            assert fused.ENABLED['bn_relu'] and fused._bn_fusable(bn, a2)
            y = fused.bn_relu(bn, a2)
        else:
            assert fused.ENABLED['bn_tail'] and fused._bn_fusable(bn, a2)
            y = fused.bn_tail(bn, a2, b2, x2, k['s'], sh2)
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith('_BNTail'), 'the fused path did not run'
    _same_bits(y.detach(), out['y'], k['name'] + ' fused y')
    y.backward(dy.to(y.dtype))          # bn_relu returns a's dtype: its dy arrives in fp16 (fp16 -> fp32 is exact: same bits)
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


def _subnormal_share(t):
    v = t.float().abs()
    return float(((v > 0) & (v < F16_MIN_NORMAL)).double().mean())


@pytest.mark.parametrize('k', TAIL_CASES)
def test_tail_passes_f16(k, monkeypatch):
    torch.manual_seed(1000 + sum(k[n] for n in 'NCHWs'))
    data = _data(k)
    a, b, x, shift, gamma, beta, dy, rm, rv = data
    out = _direct_tail(k, a, b, x, shift, gamma, beta, dy, rm.clone(), rv.clone())
    l2 = _check_tail(k, a, b, x, shift, gamma, beta, dy, out)          # per element; the per-tensor rule closes the test
    if k['dy_scale'] != 1.0:
        # (a): the operands and the results live among fp16's subnormals, and the results are there
        assert _subnormal_share(dy) > 0.5, 'dy should be mostly subnormal'
        for nm in ('da', 'db'):
            if out[nm] is not None and out[nm].dtype == F16:
                share = _subnormal_share(out[nm])
                print('SUBNORMAL f16 %s %s: %.3f of the elements subnormal and non-zero' % (k['name'], nm, share))
                assert share > (0.2 if k['relu'] else 0.5), '%s %s: subnormal results flushed (%.3f)' % (k['name'], nm, share)
    if k['wrapper']:
        _wrapper_tail(k, a, b, x, shift, gamma, beta, dy, rm, rv, out, monkeypatch)
    l2.finish()


def test_apply_store_is_torchs_fp16_conversion():
    """(b) y = (a - 0) * 1 with no affine is `a` itself in fp32 (one fma with exact operands); what the store makes of it
    must be torch's a.to(float16): nearest even, overflow to inf (not clamped, not NaN), subnormals kept.  (No zero of
    either sign among the sweep: -0 * 1 + 0 is +0, a property of the normalisation, not of the store.)"""
    sub = 2.0 ** -24
    vals = [1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 + 2.0 ** -10 - 2.0 ** -23,
            2.0 ** -14, 2.0 ** -14 - sub, 2.0 ** -14 - sub / 2, 2.0 ** -14 + sub / 2,
            sub, sub / 2, sub / 2 * (1 + 2.0 ** -23), sub / 2 * (1 - 2.0 ** -24), 1.5 * sub, 2.5 * sub, 3.5 * sub, sub / 4, 2.0 ** -30,
            65504.0, 65504.0 + 15.99, 65519.996, 65520.0, 65520.0 + 0.004, 65536.0, 1e6, 3e38, float('inf')]
    g = torch.Generator().manual_seed(5)
    k = torch.arange(1, 1025, dtype=f64)
    vals = torch.cat([torch.tensor(vals, dtype=f64), k * sub, (k + 0.5) * sub, (k + 0.25) * sub,          # subnormals, their ties
                      (1.0 + (2 * k + 1) * 2.0 ** -11) * 2.0 ** -7,                                          # ties of normals
                      torch.randn(4096, generator=g, dtype=f64) * torch.exp2(torch.randint(-30, 18, (4096,), generator=g).double())])
    a = torch.cat([vals, -vals]).float()
    a = torch.cat([a, torch.ones(-a.numel() % 16)]).cuda().view(1, 1, -1, 16)
    H, W = a.shape[2:]
    mean, rstd = torch.zeros(1, device='cuda'), torch.ones(1, device='cuda')
    y = _Guarded((1, 1, H, W), F16)
    got, = _twice('conversion', lambda: _ck(_sym('vah_bn_tail_apply')(
        _p(a), 0, None, 0, None, 1, 1, 1, H, W, _p(mean), _p(rstd), None, None, 0, None, _p(y.t), 1, _st()), 'bn_tail_apply_f16'),
        [(y, None)])
    want = a.to(F16)
    assert bool(torch.isinf(want).any()) and bool(((want.float().abs() > 0) & (want.float().abs() < F16_MIN_NORMAL)).any())
    assert not bool(torch.isnan(got).any())
    _same_bits(got, want, 'fp32 -> fp16 store')
    # and back: fp16 -> fp32 is exact, subnormals included (a = the fp16 values, y fp32)
    h = want[torch.isfinite(want) & (want != 0)].contiguous()
    h = torch.cat([h, torch.ones(-h.numel() % 16, dtype=F16, device='cuda')]).view(1, 1, -1, 16)
    y32 = _Guarded(tuple(h.shape), F32)
    got, = _twice('widening', lambda: _ck(_sym('vah_bn_tail_apply')(
        _p(h), 1, None, 0, None, 1, 1, 1, h.shape[2], 16, _p(mean), _p(rstd), None, None, 0, None, _p(y32.t), 0, _st()),
        'bn_tail_apply_f16'), [(y32, None)])
    _same_bits(got, h.float(), 'fp16 -> fp32 load')


# beyond the limits of the fused path (the batch above the 512 partial rows; a second-plan tile above 150 KB of LDS): the
# `_f16` entry points refuse on the host like their twins, and fused.bn_tail under fp16 autocast evaluates the reference
# expression, held to the same fp64 statement with the conditioning of torch's own statistics in the budget (as the bf16
# file: kappa = (E t^2 + mean^2) / (var + eps)).
@pytest.mark.parametrize('N,C,H,W,s', [(513, 4, 8, 8, 1), (171, 2, 256, 256, 4)], ids=['n513', 'n171_lds160k'])
def test_tail_beyond_the_fused_limits_f16(N, C, H, W, s):
    from vitadapter import fused
    lib = _vah().lib
    torch.manual_seed(N)
    a = torch.randn(N, C, H, W, device='cuda') * 0.7 + torch.randn(C, device='cuda').view(1, C, 1, 1) * 0.5
    x = torch.randn(N, C, H // s, W // s, device='cuda') * 0.7
    dy = torch.randn(N, C, H, W, device='cuda')
    gamma, beta = torch.randn(C, device='cuda') * 0.3 + 1.0, torch.randn(C, device='cuda') * 0.5
    v = [torch.zeros(2 * C, device='cuda') for _ in range(6)]
    ws = torch.zeros(lib.vah_bn_tail_ws_floats(C), device='cuda')
    ops = (_p(a), 0, None, 0, _p(x), s, N, C, H, W)
    da, dx = torch.zeros_like(a), torch.zeros_like(x)
    rcs = [_sym('vah_bn_tail_stats')(*ops, None, _p(v[0]), _p(ws), _st()),
           _sym('vah_bn_tail_apply')(*ops, _p(v[1]), _p(v[2]), None, None, 0, None, _p(da), 0, _st()),
           _sym('vah_bn_tail_bwd_stats')(*ops, _p(v[1]), _p(v[2]), None, None, 0, None, _p(dy), 0, _p(v[3]), _p(ws), _st()),
           _sym('vah_bn_tail_bwd_apply')(*ops, _p(v[1]), _p(v[2]), None, None, 0, None, _p(dy), 0, _p(v[4]), _p(v[5]), _p(da), None,
                                         _p(dx), _st())]
    torch.cuda.synchronize()
    assert rcs == [-2] * 4 and lib.vah_bn_tail_supported(N, C, H, W, s, 1) == 0
    assert not bool(da.any()) and not bool(dx.any()) and not bool(ws.any())
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    a2, x2 = a.clone().requires_grad_(True), x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=F16):
        assert fused._bn_fusable(bn, a2)
        y = fused.bn_tail(bn, a2, None, x2, s)
    assert y.dtype == F32 and not type(y.grad_fn).__name__.startswith('_BNTail')
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


def test_the_other_16_bit_type_takes_the_reference_expression():
    """a bf16 operand under fp16 autocast, or the reverse, or fp16 with the switch off: nothing fused"""
    from vitadapter import fused
    bn = torch.nn.BatchNorm2d(8).cuda().train()
    x = torch.randn(2, 8, 4, 8, device='cuda')
    for ac, other in ((F16, torch.bfloat16), (torch.bfloat16, F16)):
        a = torch.randn(2, 8, 8, 16, device='cuda').to(other).requires_grad_(True)
        with torch.autocast('cuda', dtype=ac):
            assert not fused._bn_fusable(bn, a)
            y = fused.bn_tail(bn, a, None, x, 2)
            assert not type(y.grad_fn).__name__.startswith('_BNTail')
            good = fused.bn_tail(bn, a.detach().to(ac).requires_grad_(True), None, x, 2)
            assert type(good.grad_fn).__name__.startswith('_BNTail')
            tok = fused.maps_to_tokens([a], [None])
            assert not type(tok.grad_fn).__name__.startswith('_MapsToTokens')
    a = torch.randn(2, 8, 8, 16, device='cuda').half().requires_grad_(True)
    fused.ENABLED['fp16_tail'] = False
    try:
        with torch.autocast('cuda', dtype=F16):
            assert fused._tail_dtype() is None and not fused.tail_takes_conv_bias(bn, a)
            y = fused.bn_tail(bn, a, None, x, 2)
            assert not type(y.grad_fn).__name__.startswith('_BNTail')
            pool = torch.nn.MaxPool2d(3, 2, 1)
            assert not type(fused.max_pool(pool, a).grad_fn).__name__.startswith('_MaxPool3s2')
            h = fused.halve(x.requires_grad_(True))
            assert 'Upsample' in type(h.grad_fn).__name__
    finally:
        fused.ENABLED['fp16_tail'] = True
    with torch.autocast('cuda', dtype=F16):
        h = fused.halve(x)
        assert 'AvgPool' in type(h.grad_fn).__name__ and h.dtype == F32


# ---------------------------------------------------------------------------------------------------------------
# NCHW max-pool: vah_maxpool3s2_{fwd,bwd}_f16
# ---------------------------------------------------------------------------------------------------------------
# W = 520 and 516 lie past the 512 input columns of one backward block; 516 is not a multiple of 8
POOL_CASES = [(2, 3, 30, 520, 'few'), (2, 3, 30, 516, 'relu'), (2, 3, 30, 516, 'few'), (1, 3, 17, 9, 'few'), (2, 2, 1, 1, 'relu'),
              (2, 2, 1, 8, 'few'), (2, 2, 2, 2, 'few'), (2, 2, 8, 1, 'relu'), (1, 3, 2, 17, 'few'), (1, 3, 19, 2, 'relu'),
              (1, 4, 64, 1040, 'relu')]


def _pool_inexact16(gy, idx, H, W):
    """pixels where an fp32 sum of the (at most four) fp16 gradients, in whatever order, need not be exact: the binary
    exponents of its non-zero terms lie more than 11 apart (11-bit significands, two carry bits: within 11 every partial
    sum fits 24 bits).  From the reference alone, as oracle/tail.maxpool_inexact is for bf16's 8 bits."""
    P = gy.shape[0]
    g = gy.to(f64).reshape(P, -1)
    e = torch.frexp(g).exponent.to(f64)
    flat = tail._pool_flat(idx, W)
    hi = torch.full((P, H * W), -1e9, dtype=f64, device=gy.device)
    lo = torch.full((P, H * W), 1e9, dtype=f64, device=gy.device)
    hi.scatter_reduce_(1, flat, torch.where(g != 0, e, torch.full_like(e, -1e9)), 'amax')
    lo.scatter_reduce_(1, flat, torch.where(g != 0, e, torch.full_like(e, 1e9)), 'amin')
    return ((hi - lo > 11) & (hi > -1e8)).view(P, H, W)


@pytest.mark.parametrize('N,C,H,W,kind', POOL_CASES)
def test_nchw_max_pool_f16(N, C, H, W, kind):
    from vitadapter import fused
    torch.manual_seed(H * 7 + W)
    if kind == 'relu':
        x = torch.randn(N, C, H, W, device='cuda').clamp_min(0.).to(F16)
    else:
        x = torch.randint(0, 3, (N, C, H, W), device='cuda').to(F16)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    # gradients kept away from zero: the exponents of a pixel's terms stay within 2^9 of each other
    r = torch.randn(N, C, Ho, Wo, device='cuda')
    gy = (torch.where(r < 0, -1.0, 1.0) * (r.abs() + 2.0 ** -6)).to(F16)
    name = 'pool %dx%dx%dx%d %s' % (N, C, H, W, kind)
    y, idx = _Guarded((N, C, Ho, Wo), F16), _Guarded((N, C, Ho, Wo), torch.uint8, fill=0xEE)
    gy_, idx_ = _twice(name + ' fwd', lambda: _ck(_sym('vah_maxpool3s2_fwd_bf16')(_p(x), N * C, H, W, _p(y.t), _p(idx.t), _st()),
                                                  'maxpool_fwd_f16'), [(y, None), (idx, None)])
    m, pos = tail.maxpool_forward(x.view(N * C, H, W))
    assert torch.equal(gy_.view(N * C, Ho, Wo).double(), m), name + ' y'
    assert torch.equal(idx_.view(N * C, Ho, Wo), pos), name + ' recorded position'
    gx = _Guarded((N, C, H, W), F16)
    got, = _twice(name + ' bwd', lambda: _ck(_sym('vah_maxpool3s2_bwd_bf16')(_p(gy), _p(idx_), N * C, H, W, _p(gx.t), _st()),
                                             'maxpool_bwd_f16'), [(gx, None)])
    ref = tail.maxpool_backward(gy.view(N * C, Ho, Wo), pos, H, W)
    loose = _pool_inexact16(gy.view(N * C, Ho, Wo), pos, H, W)
    assert int(loose.sum()) <= 8, name + ': the data should leave (almost) every fp32 sum exact'
    want = ref.to(F16)                     # one rounding: ref is an fp32 number outside `loose`
    got = got.view(N * C, H, W)
    differ = _bits(got) != _bits(want)
    assert not bool((differ & ~loose).any()), '%s gx: %d pixels differ' % (name, int((differ & ~loose).sum()))
    assert bool(((_bits(got).int() - _bits(want).int()).abs() <= 1).all()), name + ' gx: more than the last bit'
    # the wrapper: fp16 NCHW input
    pool = torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    x2 = x.clone().requires_grad_(True)
    y2 = fused.max_pool(pool, x2)
    assert type(y2.grad_fn).__name__.startswith('_MaxPool3s2') and y2.dtype == F16
    _same_bits(y2.detach(), gy_, name + ' fused y')
    y2.backward(gy)
    _same_bits(x2.grad.view(N * C, H, W), got, name + ' fused gx')


# ---------------------------------------------------------------------------------------------------------------
# sub-pixel interleave (vah_pixel_shuffle2_f16) and fused.up_from_tokens under fp16 autocast
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C,h,w', [(3, 5, 16, 16), (1, 8, 100, 168), (3, 5, 3, 8)])
def test_interleave_is_the_index_expression_f16(B, C, h, w):
    torch.manual_seed(B * C + w)
    name = 'interleave %dx%dx%dx%d' % (B, C, h, w)
    fn = _sym('vah_pixel_shuffle2_bf16')
    U = torch.randn(B, 4 * C, h * w, device='cuda').to(F16)
    add = torch.randn(B, C, 2 * h, 2 * w, device='cuda').to(F16)
    U.view(-1)[::7] *= SCALED                    # some subnormals, and sums that land among them
    add.view(-1)[::7] *= -SCALED
    planes = _Guarded((B, C, 2 * h, 2 * w), F16)
    got, = _twice(name, lambda: _ck(fn(_p(U), B, C, h, w, _p(planes.t), 0, None, _st()), 'pixel_shuffle2_f16'), [(planes, None)])
    want = tail.interleave(U, C, h, w)
    _same_bits(got, want, name + ' forward')
    got_a, = _twice(name + ' + addend', lambda: _ck(fn(_p(U), B, C, h, w, _p(planes.t), 0, _p(add), _st()), 'pixel_shuffle2_f16'),
                    [(planes, None)])
    _same_bits(got_a, (want.double() + add.double()).to(F16), name + ' forward + addend')       # one exact sum, one rounding
    back = _Guarded((B, 4 * C, h * w), F16)
    inv, = _twice(name + ' inverse', lambda: _ck(fn(_p(got), B, C, h, w, _p(back.t), 1, None, _st()), 'pixel_shuffle2_f16'),
                  [(back, None)])
    _same_bits(inv, U, name + ' inverse(forward)')
    inv, = _twice(name + ' inverse', lambda: _ck(fn(_p(add), B, C, h, w, _p(back.t), 1, None, _st()), 'pixel_shuffle2_f16'),
                  [(back, None)])
    _same_bits(inv, tail.deinterleave(add), name + ' inverse')


@pytest.mark.parametrize('with_add', [False, True], ids=['plain', 'addend'])
@pytest.mark.parametrize('B,h,w,C,Co', [(3, 16, 16, 64, 48), (2, 100, 168, 32, 24)])
def test_up_from_tokens_fp64_f16(B, h, w, C, Co, with_add):
    """(c) out, d rows (fp16) and d weight (fp32) of fused.up_from_tokens under fp16 autocast in fp64 on the fp16 operands.
    Every stored product is rounded to fp16 once: U; with an addend U, then the sum (2^-11 (|U| + |U + add|) + 2 * 2^-25);
    d rows; d weight's per-image products, summed over the images in fp32."""
    from vitadapter import fused
    torch.manual_seed(h + w + with_add)
    name = 'up %dx%dx%d %s' % (B, h, w, 'addend' if with_add else 'plain')
    up = torch.nn.ConvTranspose2d(C, Co, 2, 2).cuda()
    rows = torch.randn(B, h * w, C, device='cuda', requires_grad=True)
    add = torch.randn(B, Co, 2 * h, 2 * w, device='cuda').to(F16).requires_grad_(True) if with_add else None
    g = torch.randn(B, Co, 2 * h, 2 * w, device='cuda').to(F16)
    with torch.autocast('cuda', dtype=F16):
        out = fused.up_from_tokens(up, rows, h, w, add)
        assert out is not None and out.dtype == F16 and type(out.grad_fn).__name__.startswith('_UpFromTokens'), 'the GEMM form did not run'
        out.backward(g)
    xh = rows.detach().to(F16)
    wc = tail.up_weight_rows(up.weight.detach().to(F16))
    for bi in range(B):
        Ur, UA = tail.up_product(xh[bi:bi + 1], wc)
        ref, A = tail.interleave(Ur, Co, h, w), tail.interleave(UA, Co, h, w)
        o = out.detach()[bi:bi + 1]
        if with_add:
            tot = ref + add.detach()[bi:bi + 1].double()
            bud = tail.C_ACC * tail.U * A + F16_U * (ref.abs() + tot.abs()) + 2 * F16_SUB
            _record('up_from_tokens out + addend', name, _check(name + ' out', o, tot, A, tail.C_ACC, True, bud=bud)[0])
        else:
            _record('up_from_tokens out', name, _check(name + ' out', o, ref, A, tail.C_ACC, True)[0])
        del Ur, UA, ref, A
    dU = tail.deinterleave(g)
    wd = wc.double()
    dw = torch.zeros(4 * Co, C, dtype=f64, device='cuda')
    dwb = torch.zeros(4 * Co, C, dtype=f64, device='cuda')
    for bi in range(B):
        d = dU[bi].double()
        ref, A = d.T @ wd, d.abs().T @ wd.abs()
        assert rows.grad.dtype == F32       # rounded to fp16 by the GEMM, handed back in the rows' dtype
        dr = rows.grad[bi]
        assert torch.equal(dr, dr.to(F16).float()), 'd rows should be fp16 values'
        _record('up_from_tokens d rows', name, _check(name + ' d rows', dr.to(F16), ref, A, tail.C_ACC, True)[0])
        part, pa = d @ xh[bi].double(), d.abs() @ xh[bi].double().abs()
        dw += part
        dwb += _bound(part, pa, tail.C_ACC, True)          # one fp16 rounding per image's product

    def as_weight(m):
        return m.view(2, 2, Co, C).permute(3, 2, 0, 1)
    assert up.weight.grad.dtype == F32
    _record('up_from_tokens d weight', name, _check(name + ' d weight', up.weight.grad, as_weight(dw), None, tail.C_ACC, False,
                                                    bud=as_weight(dwb))[0])
    if with_add:
        _same_bits(add.grad, g, name + ' d addend')


# ---------------------------------------------------------------------------------------------------------------
# token <-> plane layouts: vah_transpose_tokens_f16
# ---------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [(3, 50, [(3, 7), (1, 33), (5, 1)]), (2, 72, [(16, 16), (8, 8), (4, 4)])]


@pytest.mark.parametrize('planes_dtype', [F32, F16], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('B,C,hw', LAYOUT_CASES)
def test_token_plane_layouts_f16(B, C, hw, planes_dtype):
    from vitadapter import fused
    fn = _sym('vah_transpose_tokens')
    torch.manual_seed(B * C)
    T = sum(h * w for h, w in hw)
    name = 'layout %dx%dx%d %s' % (B, T, C, 'fp16' if planes_dtype == F16 else 'fp32')
    pb = int(planes_dtype == F16)
    tokens = torch.randn(B, T, C, device='cuda')
    # values that round into fp16's subnormals, none of them to a zero: the way back adds vec[c] or +0, and -0 + 0 is +0
    tokens.view(-1)[::5] = (tokens.view(-1)[::5].sign() * (tokens.view(-1)[::5].abs() + 0.5)) * SCALED
    tokens.view(-1)[::11] *= 1e5                 # and beyond its range
    t0, maps = 0, []
    for h, w in hw:
        dst = _Guarded((B, C, h * w), planes_dtype)
        got, = _twice(name + ' to planes', lambda: _ck(fn(_p(tokens), B, T, t0, h * w, C, _p(dst.t), 1, pb, None, _st()),
                                                       'transpose_tokens_f16'), [(dst, None)])
        _same_bits(got, tail.tokens_to_planes(tokens, t0, h * w).to(planes_dtype), name + ' to planes')
        maps.append(got.view(B, C, h, w))
        t0 += h * w
    maps = [m.clamp(-60000, 60000) for m in maps]          # finite maps for the way back
    vecs = [torch.randn(C, device='cuda'), None, torch.randn(C, device='cuda')]
    t0, parts = 0, []
    for (h, w), m, v in zip(hw, maps, vecs):
        dst = _Guarded((B, T, C), F32, fill=TOKEN_GUARD)
        got, = _twice(name + ' to tokens', lambda: _ck(fn(_p(m), B, T, t0, h * w, C, _p(dst.t), 0, pb, _p(v), _st()),
                                                       'transpose_tokens_f16'), [(dst, None)])
        want = torch.full((B, T, C), TOKEN_GUARD, device='cuda')          # rows outside [t0, t0 + T) keep the guard value
        want[:, t0:t0 + h * w] = tail.planes_to_tokens(m.flatten(2), v)
        _same_bits(got, want, name + ' to tokens')
        parts.append(got[:, t0:t0 + h * w])
        t0 += h * w
    # the wrappers under fp16 autocast: the direct calls' bits, forward and backward
    with torch.autocast('cuda', dtype=F16):
        assert fused._maps_dtype() == F16
        tk = tokens.clone().requires_grad_(True)
        outs = fused.tokens_to_maps(tk, hw)
        assert type(outs[0].grad_fn).__name__.startswith('_TokensToMaps')
        gms = [torch.randn_like(o) for o in outs]
        for o, (h, w), t0 in zip(outs, hw, (0, hw[0][0] * hw[0][1], hw[0][0] * hw[0][1] + hw[1][0] * hw[1][1])):
            _same_bits(o.detach(), tail.tokens_to_planes(tokens, t0, h * w).view(B, C, h, w), name + ' fused.tokens_to_maps')
        torch.autograd.backward(outs, gms)
        _same_bits(tk.grad, torch.cat([tail.planes_to_tokens(g.flatten(2), None) for g in gms], 1),
                   name + ' fused.tokens_to_maps backward')
        ms = [m.clone().requires_grad_(True) for m in maps]
        vs = [v.clone().requires_grad_(True) if v is not None else None for v in vecs]
        tok = fused.maps_to_tokens(ms, vs)
        assert type(tok.grad_fn).__name__.startswith('_MapsToTokens')
        _same_bits(tok.detach(), torch.cat(parts, 1), name + ' fused.maps_to_tokens')
        gt = torch.randn_like(tok)
        gt.view(-1)[::5] *= SCALED               # to planes only: a -0 stays a -0
        tok.backward(gt)
    t0 = 0
    for (h, w), m in zip(hw, ms):
        _same_bits(m.grad, tail.tokens_to_planes(gt, t0, h * w).to(planes_dtype).view(B, C, h, w), name + ' fused.maps_to_tokens backward')
        t0 += h * w
