"""GPU: the fixed forms of the output-tail kernels (csrc/tail_ops.hip: norm1 = 16-bit a + fp32 x at scale 4 + shift,
norm2 = fp32 a + x at scale 2, norm3 = fp32 a + x at scale 1; 8-pixel items, the upsample adjoint with the weights of
the scale as constants) through the C ABI, for both 16-bit types, held to

  * fp64 (oracle/tail.py, from the exact operands) within the budgets of tests/test_tail_fp64_gpu.py and
    tests/test_tail_f16_fp64_gpu.py: C = 48 for y and da, 128 for dxlo, 256 for the channel sums, 2^-8 (bf16) / 2^-11
    (fp16, + 2^-25 for its subnormals) per 16-bit rounding, and ||err|| <= 0.5 ||budget|| per tensor.  Outputs, sums and
    the workspace are NaN-filled inside guard bands that must come back intact (dxlo zero-filled at scale > 1), and every
    call runs twice with the same bits;
  * the general form of the same entry points (VAH_TAIL_FORM=general, read per call): given the same mean / rstd / mdy /
    mdyx, y, da and dxlo carry the same bits; the channel sums, which the 8-pixel items associate differently, agree
    within one fp64 budget (C = 256) of each other;
  * the profiler: a fixed-form call and a general-form call report the same rows, calls and bytes.

Shapes, the smallest at which each mechanism can go wrong; (N, C) = (3, 5) with maps below one tile: 16 x 16 and 24 x 48
at scale 4 (two items per row, each with a border column, and six with interior ones; 24 x 40 was asked for, but the
entry points refuse it - with an x, W / scale must be a multiple of 4 - which `test_24x40_at_scale_4_is_refused` pins,
and 24 x 48 is the nearest map they take), 8 x 8 and 12 x 24 at scale 2, 6 x 8 at scale 1.  Several chunks per plane:
72 x 1024 at scale 4 (rows_per_block = 8 = 2s, 9 chunks) and 40 x 2048 at scale 2 (4 = 2s rows, 10 chunks): every tile
is one footprint high, so every low-res row but the two outermost is shared between two tiles and takes the atomic
path; both heights are whole numbers of tiles, so 76 x 1024 and 42 x 2048 add the partial last chunk: s rows, half a
footprint.  The number of chunks is the plan's, recomputed here (`_plan`), asserted > 1 and read back from the
workspace: stats writes exactly N * chunks partial rows.  6 x 12 at scale 1 has W % 8 == 4 and must take the general
form: there the two runs' channel sums carry the same bits as well.

Run with -s for one RATIO line per checked output."""
import contextlib
import math
import os

import pytest
import torch

from oracle import tail
from test_tail_f16_fp64_gpu import _bound as _f16_bound
from test_tail_fp64_gpu import EPS, MOMENTUM, _ck, _Guarded, _p, _same_bits, _st, _tail_data, _twice, _vah

pytestmark = pytest.mark.gpu

NAN = float('nan')
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
f64 = torch.float64
SWITCH = 'VAH_TAIL_FORM'


@contextlib.contextmanager
def _general_form():
    """VAH_TAIL_FORM=general for the calls inside (os.environ writes through to the C environment the library reads)"""
    before = os.environ.get(SWITCH)
    os.environ[SWITCH] = 'general'
    try:
        yield
    finally:
        if before is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = before


def _sym(name, t16):
    v = _vah()
    return getattr(v.lib, name if t16 == BF else v.TAIL_F16_TWINS[name])


def _plan(N, H, W, s):
    """rows_per_block, chunks of plan_tail (first plan: N * chunks <= 512)"""
    rpb = max(1, 8192 // W)
    rpb = min(max(2 * s, rpb // (2 * s) * (2 * s)), H)
    chunks = -(-H // rpb)
    assert N * chunks <= 512
    return rpb, chunks


# name, form, N, C, H, W, fixed (False: W % 8 == 4, the general form), chunks > 1
SHAPES = [
    ('norm1_16x16', 1, 3, 5, 16, 16, True, False), ('norm1_24x48', 1, 3, 5, 24, 48, True, False),
    ('norm1_72x1024', 1, 1, 2, 72, 1024, True, True), ('norm1_76x1024_half_footprint', 1, 1, 2, 76, 1024, True, True),
    ('norm2_8x8', 2, 3, 5, 8, 8, True, False), ('norm2_12x24', 2, 3, 5, 12, 24, True, False),
    ('norm2_40x2048', 2, 1, 2, 40, 2048, True, True), ('norm2_42x2048_half_footprint', 2, 1, 2, 42, 2048, True, True),
    ('norm3_6x8', 3, 3, 5, 6, 8, True, False), ('norm3_6x12_general', 3, 3, 5, 6, 12, False, False),
]


def _key(name, form, N, C, H, W, t16):
    """the case in the vocabulary of test_tail_fp64_gpu._tail_data; the flags are fused._BNTail's for the three levels"""
    a, s, shift = {1: (t16, 4, True), 2: (F32, 2, False), 3: (F32, 1, False)}[form]
    return dict(name='%s %s' % (name, 'bf16' if t16 == BF else 'fp16'), N=N, C=C, H=H, W=W, s=s, a=a, b=None, x=True, shift=shift,
                affine=True, relu=False, y=F32, dy=F32, evalm=False, big=form == 1)


def _passes(k, t16, data, given=None):
    """the four passes through the C ABI as fused._BNTail strings them together; `given`: an earlier run whose mean /
    rstd / mdy / mdyx the normalise passes take (the statistics passes still run, for their sums)"""
    a, b, x, shift, gamma, beta, dy, rm, rv = data
    lib = _vah().lib
    N, C, H, W, s, name = k['N'], k['C'], k['H'], k['W'], k['s'], k['name']
    ops = (_p(a), int(a.dtype == t16), None, 0, _p(x), s, N, C, H, W)
    assert lib.vah_bn_tail_supported(N, C, H, W, s, 1) == 1
    st = _st()
    ws = _Guarded((lib.vah_bn_tail_ws_floats(C),), F32)
    out = {}
    sums = _Guarded((2 * C,), F32)
    out['sums'], out['ws'] = _twice(name + ' stats', lambda: _ck(_sym('vah_bn_tail_stats', t16)(
        *ops, _p(shift), _p(sums.t), _p(ws.t), st), 'bn_tail_stats'), [(sums, None), (ws, None)])
    if given is None:
        full = torch.cat([out['sums'], torch.full((1,), float(N * H * W), device='cuda')])
        mean, rstd = torch.full((C,), NAN, device='cuda'), torch.full((C,), NAN, device='cuda')
        rm2, rv2 = rm.clone(), rv.clone()                   # updated in place
        _ck(lib.vah_bn_finalize_stats(_p(full), C, EPS, MOMENTUM, _p(rm2), _p(rv2), _p(mean), _p(rstd), st), 'bn_finalize_stats')
    else:
        mean, rstd = given['mean'], given['rstd']
    out['mean'], out['rstd'] = mean, rstd
    y = _Guarded((N, C, H, W), F32)
    out['y'], = _twice(name + ' apply', lambda: _ck(_sym('vah_bn_tail_apply', t16)(
        *ops, _p(mean), _p(rstd), _p(gamma), _p(beta), 0, _p(shift), _p(y.t), 0, st), 'bn_tail_apply'), [(y, None)])
    sums2 = _Guarded((2 * C,), F32)
    out['bsums'], = _twice(name + ' bwd_stats', lambda: _ck(_sym('vah_bn_tail_bwd_stats', t16)(
        *ops, _p(mean), _p(rstd), _p(gamma), _p(beta), 0, _p(shift), _p(dy), 0, _p(sums2.t), _p(ws.t), st),
        'bn_tail_bwd_stats'), [(sums2, None), (ws, None)])[:1]
    means = out['bsums'] / float(N * H * W) if given is None else torch.cat([given['mdy'], given['mdyx']])
    out['mdy'], out['mdyx'] = means[:C], means[C:]
    da, dx = _Guarded((N, C, H, W), a.dtype), _Guarded(tuple(x.shape), F32)
    # dxlo: zero-filled by contract where the adjoint adds into it (scale > 1), NaN where it is stored (scale 1)
    out['da'], out['dxlo'] = _twice(name + ' bwd_apply', lambda: _ck(_sym('vah_bn_tail_bwd_apply', t16)(
        *ops, _p(mean), _p(rstd), _p(gamma), _p(beta), 0, _p(shift), _p(dy), 0, _p(means[:C]), _p(means[C:]), _p(da.t), None,
        _p(dx.t), st), 'bn_tail_bwd_apply'), [(da, None), (dx, 0.0 if s > 1 else None)])
    return out


class _Held:
    """every element within its budget, and ||err|| <= 0.5 ||budget|| per tensor"""

    def __init__(self, case):
        self.case = case

    def add(self, what, got, ref, A, c, t16=None):
        r64 = ref.to(f64)
        if t16 == F16:
            b = _f16_bound(ref, A, c, True)             # C 2^-24 A + 2^-11 |ref| + 2^-25
        else:
            b = tail.bound(ref, A, t16 == BF, c)        # C 2^-24 A (+ 2^-8 |ref|)
        assert got.dtype == (t16 or F32), what
        err = (got.to(f64) - r64).abs()
        worst = float(torch.where(err == 0, torch.zeros_like(err), err / b).nan_to_num(float('inf')).max())
        l2 = math.sqrt(float((err * err).sum())) / math.sqrt(float((b * b).sum()))
        print('RATIO forms %s %s worst %.4f L2 %.4f' % (self.case, what, worst, l2))
        assert bool((err <= b).all()), '%s %s: worst err / budget %.3g' % (self.case, what, worst)
        assert l2 <= 0.5, '%s %s: ||err|| = %.3g ||budget||' % (self.case, what, l2)


def _held_to_fp64(k, t16, data, out):
    a, b, x, shift, gamma, beta, dy, rm, rv = data
    s = k['s']
    h = _Held(k['name'])
    t, At = tail.tail_sum(a, None, x, s, shift)
    ref, A = tail.stats(t, At)
    h.add('sums', out['sums'], ref, A, tail.C_ACC)
    ref, A, pre, edge = tail.apply(t, At, out['mean'], out['rstd'], gamma, beta, False)
    h.add('y', out['y'], ref, A, tail.C_ELT)
    ref, A = tail.bwd_stats(t, At, dy, out['mean'], out['rstd'], pre, edge, False)
    h.add('bsums', out['bsums'], ref, A, tail.C_ACC)
    ref, A = tail.bwd_apply(t, At, dy, out['mean'], out['rstd'], gamma, pre, False, out['mdy'], out['mdyx'])
    h.add('da', out['da'], ref, A, tail.C_ELT, t16 if a.dtype == t16 else None)
    lo, LA = tail.upsample_t(ref, s)[0], tail.upsample_t(A, s)[0]
    h.add('dxlo', out['dxlo'], lo, LA, tail.C_LO if s > 1 else tail.C_ELT)          # scale 1: dt itself, stored
    return t, At, pre, edge


@pytest.mark.parametrize('t16', [BF, F16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('name,form,N,C,H,W,fixed,tiled', SHAPES, ids=[c[0] for c in SHAPES])
def test_fixed_form_against_fp64_and_the_general_form(name, form, N, C, H, W, fixed, tiled, t16):
    assert os.environ.get(SWITCH) is None, 'the suite runs with the switch unset'
    assert (W % 8 == 0) == fixed
    k = _key(name, form, N, C, H, W, t16)
    torch.manual_seed(4000 + form * 1000 + H + W)
    data = _tail_data(k)
    a, b, x, shift, gamma, beta, dy, rm, rv = data
    assert b is None and (shift is not None) == (form == 1) and a.dtype == (t16 if form == 1 else F32)
    rpb, chunks = _plan(N, H, W, k['s'])
    assert (chunks > 1) == tiled, 'chunks = %d' % chunks
    if tiled:
        assert rpb == 2 * k['s'], 'every tile one footprint high: the interior low-res rows are all shared'
    out = _passes(k, t16, data)
    # the plan the library made: stats wrote N * chunks partial rows of 2 C floats and nothing else
    written = ~torch.isnan(out['ws'])
    assert bool(written[:N * chunks * 2 * C].all()) and not bool(written[N * chunks * 2 * C:].any()), 'partial rows'
    t, At, pre, edge = _held_to_fp64(k, t16, data, out)
    with _general_form():
        gen = _passes(k, t16, data, given=out)
    for what in ('y', 'da', 'dxlo'):
        _same_bits(out[what], gen[what], '%s %s: fixed form against the general form' % (k['name'], what))
    # the sums: each form within the fp64 budget of the reference, and of each other
    h = _Held(k['name'] + ' (general form)')
    pairs = (('sums', tail.stats(t, At)), ('bsums', tail.bwd_stats(t, At, dy, out['mean'], out['rstd'], pre, edge, False)))
    for what, (ref, A) in pairs:
        h.add(what, gen[what], ref, A, tail.C_ACC)
        diff = (out[what].to(f64) - gen[what].to(f64)).abs()
        assert bool((diff <= tail.bound(ref, A, False, tail.C_ACC)).all()), '%s %s: the two forms differ by %.3g budgets' % (
            k['name'], what, float((diff / tail.bound(ref, A, False, tail.C_ACC)).max()))
        if not fixed:
            _same_bits(out[what], gen[what], '%s %s: W %% 8 == 4 takes the general form' % (k['name'], what))


def test_24x40_at_scale_4_is_refused():
    """the shape rule of the four entry points is unchanged: a 10-column low-res map is no multiple of 4 columns"""
    lib = _vah().lib
    assert lib.vah_bn_tail_supported(3, 5, 24, 40, 4, 1) == 0 and lib.vah_bn_tail_supported(3, 5, 24, 48, 4, 1) == 1


@pytest.mark.parametrize('t16', [BF, F16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('name,form,N,C,H,W', [c[:6] for c in SHAPES if c[0] in ('norm1_24x48', 'norm2_12x24', 'norm3_6x8')])
def test_both_forms_report_the_same_profiler_rows(name, form, N, C, H, W, t16):
    v = _vah()
    k = _key(name, form, N, C, H, W, t16)
    torch.manual_seed(5000 + form)
    data = _tail_data(k)
    reports = []
    for general in (False, True):
        v.prof_enable(True, 'bn_tail')
        try:
            with (_general_form() if general else contextlib.nullcontext()):
                _passes(k, t16, data)
            torch.cuda.synchronize()
            rep = v.prof_report()
        finally:
            v.prof_enable(False)
        reports.append({row: (r['calls'], r['bytes'], r['def_bytes']) for row, r in rep.items()})
    suffix = '' if t16 == BF else '_f16'
    assert sorted(reports[0]) == sorted('bn_tail_%s%s' % (p, suffix) for p in ('stats', 'apply', 'bwd_stats', 'bwd_apply'))
    assert reports[0] == reports[1], 'fixed %r general %r' % (reports[0], reports[1])
    assert all(calls == 2 and nbytes > 0 for calls, nbytes, _d in reports[0].values())
