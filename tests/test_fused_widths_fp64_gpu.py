"""GPU: the row kernels of csrc/fused_ops.hip held to fp64 at every template form and every launch rule that depends on
the channel width - above all at 384 channels (ViT-Adapter-S: NV = 2 float4 slots per lane, a ragged second slot) - in
bf16 and fp16, through direct C-ABI calls (_vah.call).  tests/test_reductions_fullsize_gpu.py (bf16) and
tests/test_fused_f16_fp64_gpu.py (fp16) hold the same kernels at production row counts and C = 192 / 768 / 1024; this file
holds what they leave out: NV = 2 and 8, a partly filled last slot in a multi-slot form, both wave counts of the backward,
a partly filled last column tile, and the grid caps at 384.  Shapes are the smallest that still reach each form.

References and data makers are those of tests/test_reductions_fullsize_gpu.py, used as they are (they take the kernel's
own operands: 16-bit inputs upcast, a backward uses the kernel's own fp32 mean / rstd); the GELU reference is that of
tests/test_bias_partials_gpu.py.  Budget per element, the project's, unchanged:

    |got - ref| <= C_ACC * 2^-24 * A   + 2^-8 |ref| (bf16 outputs)   or   + 2^-11 |ref| + 2^-25 (fp16 outputs)

A = the sum of the absolute terms of the element, C_ACC = 64.  No new tolerance: 64 was derived for chains of up to 59
dependent fp32 additions at production row counts (test_reductions_fullsize_gpu.py), and the chains here are shorter.  The
longest is the row statistic at NV = 8: 8 slots x 4 components = 32 terms per lane, then 6 steps across the wave (four
inside a row of 16 lanes, two across the rows) - 38.  A parameter gradient at the grid cap (4097 rows at C = 384) adds
2 rows per wave, 8 waves, 8 + 3 + 8 partial rows: 29.  GELU's dh carries, as in the files named above, 2^-20 |da| for the
fp32 evaluation of erff / expf in place of the 64 * 2^-24 * A term.

Every output and workspace sits NaN-filled between two sentinel guard bands (_Guarded of the fp16 file: fp32 outputs
too - mean, rstd, dw, db, dgamma, partial rows, workspace); the part of a workspace behind the partial rows the launch
arithmetic gives must still be NaN afterwards.  Every case runs twice and must give the same bits.  At C = 384 and one
width per other NV the fused.* entry points under torch.autocast must give the bits of the direct call.

The launch arithmetic of fused_ops.hip is mirrored below (_nv, _waves, the block counts, the three strip rules, the
DWConv slots).  The case lists are derived from it, and the partial-row counts the library reports are held to it, so a
change of geometry has to be re-derived here.  tests/test_fused_widths_refs_cpu.py shows on the CPU that the budget
separates an fp32 evaluation in the kernel's order from the faults this file is meant to catch.

Measured on an MI355X, worst err / budget over all cases of a family (the file: 493 cases, 6.6 s wall time, no case over
1.2 s, which is the first call's library load):

    family              bf16 outputs         fp16 outputs         fp32 outputs
    layer_norm          y 0.995              y 0.987              mean 0.016  rstd 0.019  dx 0.041  dgamma 0.057  dbeta 0.014
    residual_ln         h 0.995  dz 0.995    h 0.987  dz 0.990    t 0.029  mean 0.016  rstd 0.019  dt 0.044  dgamma 0.051
                                                                  dw 0.050  db 0.015  bias partials 0.014
    layer_norm_dual     ya, yb 0.994         ya, yb 0.988         mean 0.015  rstd 0.016  dx 0.036  dwa, dwb 0.046  dba, dbb 0.015
    scale_residual      dz 0.995             dz 0.990             y 0.029  dgamma 0.028  bias partials 0.009
    gelu_bwd            dh 0.995             dh 0.997             bias partials 0.013
    colsum                                                        out 0.007  partial rows 0.007
    dwconv_tokens       y 0.991  dx 0.994    y 0.973  dx 0.979    dw 0.025  db 0.003

The 16-bit outputs sit at their format's rounding bound, as they should.  The fp32 quantities stay below 0.06; the largest
are the LayerNorm weight gradients at 1 .. 9 rows: a column of so few terms, each g * xhat with its three roundings
(3 / 64 = 0.047), comes close to its worst case, where the production row counts of the files above average it out
(<= 0.05 there).  The float32 emulation of tests/test_fused_widths_refs_cpu.py gives 0.035 .. 0.043 for the same sums."""
import ctypes

import pytest
import torch

from test_bias_partials_gpu import _gelu_ref64
from test_fused_f16_fp64_gpu import _Drop, _fixed_drop, _Guarded, _norm
from test_reductions_fullsize_gpu import C_ACC, EPS, U, _dwconv_ref, _ln_bwd_ref, _ln_data, _ln_fwd_ref

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
IDS = ['bf16', 'fp16']

# ---------------------------------------------------------------------------------------------------------------
# the launch arithmetic of csrc/fused_ops.hip
# ---------------------------------------------------------------------------------------------------------------
MAX_PARTS = 512                                                   # kMaxParts
NV_TOP = ((256, 1), (512, 2), (768, 3), (1024, 4), (2048, 8))     # ln_fwd_launch / ln_bwd_launch: C <= top takes NV
DUAL_MAX_C = 1024                                                 # ln_dual_fwd / ln_dual_bwd stop at NV 4
LDS_TWO_WORKGROUPS = 80 * 1024                                    # ln_bwd_launch: 8 waves while the LDS fits twice per CU


def _nv(C):
    """float4 slots per lane of the LayerNorm kernels"""
    for top, nv in NV_TOP:
        if C <= top:
            return nv
    raise ValueError(C)


def _ragged(C):
    """is the last slot partly filled (lanes with lane + 64 * (NV - 1) >= C / 4)?"""
    return C // 4 < 64 * _nv(C)


def _waves(C, ncol):
    """waves per workgroup of ln_bwd_kernel; ncol = 2 ([dw | db]) or 3 (the residual form: [dw | db | dgamma])"""
    wbytes = (2 if ncol == 3 else 1) * C * 4                      # w (and gamma) kept in LDS
    return 8 if 8 * ncol * C * 4 + wbytes <= LDS_TWO_WORKGROUPS else 4


def _bwd_blocks(rows, C, ncol):
    w = _waves(C, ncol)
    return min((rows + w - 1) // w, MAX_PARTS)


def _dual_bwd_blocks(rows):
    return min((rows + 3) // 4, MAX_PARTS // 2)                   # partial rows of 4C floats in a 2C workspace


def _strips_of_32(rows):
    """(rows per strip, strips) of the column-tiled kernels (scale_bsum_bwd_kernel, gelu_bwd_bsum_kernel)"""
    rpb = max(32, ((rows + MAX_PARTS - 1) // MAX_PARTS + 31) // 32 * 32)
    return rpb, (rows + rpb - 1) // rpb


def _row_strips(rows):
    """(rows per strip, strips) of the row-strip scale_residual_bwd_kernel"""
    rpb = (rows + MAX_PARTS - 1) // MAX_PARTS
    return rpb, (rows + rpb - 1) // rpb


def _colsum_strips(rows, C):
    """(rows per strip, strips) of colsum16_partials: it aims at 2048 workgroups, not at 512 strips"""
    parts = min(MAX_PARTS, max(1, 2048 // _col_tiles(C)))
    rpb = max(32, (rows + parts - 1) // parts)
    return rpb, (rows + rpb - 1) // rpb


def _col_tiles(C):
    return (C + 255) // 256


def _ragged_tile(C):
    """is the last 256-column tile partly filled (lanes with c0 >= C)?"""
    return C % 256 != 0


def _dw_slots(C):
    """token slots per workgroup of the depthwise kernels"""
    return 256 // (C // 4)


def _switch(ncol):
    """the two widths on either side of the 8 -> 4 wave switch"""
    c = max(c for c in range(4, 2049, 4) if _waves(c, ncol) == 8)
    return c, c + 4


# ---------------------------------------------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------------------------------------------
MODEL_WIDTHS = (192, 256, 384, 768, 1024)        # trunk widths of the presets; 256 is the pixel decoder's encoder
LN_ROWS = (1, 3, 4, 5, 7, 8, 9, 33)              # 4 rows per forward workgroup, 4 / 8 backward waves, several workgroups
TILE_ROWS = (1, 31, 32, 33, 65)                  # strips of 32 = 8 row lanes x 4 rows in flight
SMALL_C = 384


def _ln_widths(top_c=2048):
    """per NV: the first width of the form (one live lane in the last slot), one vector short of full, full, and the
    model widths inside; then the two widths on either side of each wave switch"""
    out, lo = [], 0
    for top, nv in NV_TOP:
        out += sorted({lo + 4, top - 4, top} | {c for c in MODEL_WIDTHS if lo < c <= top})
        lo = top
    out += list(_switch(3)) + list(_switch(2))
    return [c for c in out if c <= top_c]


def _walk(widths, rows_all, every=(SMALL_C,)):
    """(rows, C): two row counts per width, walking through ``rows_all``; the widths in ``every`` (384, and the first
    4-wave width of a backward form) get all of them"""
    cases, n = [], len(rows_all)
    for i, C in enumerate(widths):
        if C in every:
            cases += [(r, C) for r in rows_all]
        else:
            cases += [(rows_all[i % n], C), (rows_all[(i + n // 2 + 1) % n], C)]
    return cases


LN_CAP = [(MAX_PARTS * 8 - 1, SMALL_C), (MAX_PARTS * 8, SMALL_C), (MAX_PARTS * 8 + 1, SMALL_C)]        # 4095, 4096, 4097
DUAL_CAP = [(MAX_PARTS // 2 * 4 - 1, SMALL_C), (MAX_PARTS // 2 * 4, SMALL_C), (MAX_PARTS // 2 * 4 + 1, SMALL_C)]
LN_CASES = _walk(_ln_widths(), LN_ROWS, every=(SMALL_C, _switch(2)[1])) + LN_CAP
GAMMA_SC = [(True, True), (False, True), (True, False), (False, False)]        # the combinations of RES_VARIANTS
# the four combinations walk through the cases (coprime step: every NV and both wave counts see all four), and
# 384 channels run all four at a row count with two workgroups
RES_CASES = list(dict.fromkeys(
    [(r, c) + GAMMA_SC[i % 4] for i, (r, c) in enumerate(_walk(_ln_widths(), LN_ROWS, every=(SMALL_C, _switch(3)[1])))] +
    [(9, SMALL_C) + gs for gs in GAMMA_SC] + [(r, c, True, True) for r, c in LN_CAP] + [(LN_CAP[2][0], SMALL_C, False, True)]))
DROPS = (None, 'ga', 'gb', 'gres')
DUAL_CASES = [(r, c, DROPS[i % 4]) for i, (r, c) in enumerate(_walk(_ln_widths(DUAL_MAX_C), LN_ROWS))] + \
    [(r, c, None) for r, c in DUAL_CAP]
SR_WIDTHS = (8, 12, 248, 256, 264, 384, 388, 1152)         # 12, 388: C % 8 != 0, the strip kernel in every form
TILE_WIDTHS = (8, 248, 256, 264, 384, 1152, 1536)
SR_CASES = _walk(SR_WIDTHS, TILE_ROWS, every=(384, 1152))
TILE_CASES = _walk(TILE_WIDTHS, TILE_ROWS, every=(384, 1152))
DW_C = 96                                                  # ConvFFN hidden of the Small model: 0.25 * 384
DW_CASES = [(2, 4, 6), (1, 2, 2)]
ENTRY_WIDTHS = (252, SMALL_C, 764, 1020, 2044)             # fused.*: 384 and one (ragged) width per other NV


def test_the_case_list_covers_what_it_claims():
    assert _ln_widths() == [4, 192, 252, 256, 260, 384, 508, 512, 516, 764, 768, 772, 1020, 1024, 1028, 2044, 2048,
                            784, 788, 1204, 1208]
    assert LN_CAP == [(4095, 384), (4096, 384), (4097, 384)] and [c[0] for c in DUAL_CAP] == [1023, 1024, 1025]
    for name, cases, ncols in (('layer_norm', LN_CASES, (2,)), ('residual_ln', RES_CASES, (3,)), ('dual', DUAL_CASES, ())):
        widths = {c[1] for c in cases}
        nvs = {_nv(c) for c in widths}
        assert nvs == ({1, 2, 3, 4, 8} if name != 'dual' else {1, 2, 3, 4}), (name, nvs)
        for nv in nvs:      # a ragged and a full last slot in every form, the first lane alone in the last slot
            assert {_ragged(c) for c in widths if _nv(c) == nv} == {False, True}, (name, nv)
            assert any(c // 4 == 64 * (nv - 1) + 1 for c in widths if _nv(c) == nv and nv < 8) or nv == 8, (name, nv)
        assert 1028 in widths or name == 'dual'
        for ncol in ncols:  # both sides of the wave switch, and both wave counts at several row counts
            lo, hi = _switch(ncol)
            assert {lo, hi} <= widths and _waves(lo, ncol) == 8 and _waves(hi, ncol) == 4
            for w in (4, 8):
                assert len({r for r, c, *_ in cases if _waves(c, ncol) == w}) >= 6, (name, w)
        assert {r for r, c, *_ in cases if c == SMALL_C} >= set(LN_ROWS), name
        assert set(LN_ROWS) <= {c[0] for c in cases}
    # the grid caps at 384: the last row of 4096 fills 512 workgroups of 8 waves, row 4097 is a second flight
    assert [_bwd_blocks(r, SMALL_C, n) for r, _ in LN_CAP for n in (2, 3)] == [512] * 6 and _waves(SMALL_C, 3) == 8
    assert _bwd_blocks(4088, SMALL_C, 2) == 511
    assert [_dual_bwd_blocks(r) for r, _ in DUAL_CAP] == [256] * 3 and _dual_bwd_blocks(1020) == 255
    assert {c[:2] for c in RES_CASES} >= set(LN_CAP) and {c[:2] for c in DUAL_CASES} >= set(DUAL_CAP)
    # every gamma / sc combination in every NV, at both wave counts, and at 384; every dropped operand of the dual in every NV
    for nv in (1, 2, 3, 4, 8):
        assert {c[2:] for c in RES_CASES if _nv(c[1]) == nv} == set(GAMMA_SC), nv
    for w in (4, 8):
        assert {c[2:] for c in RES_CASES if _waves(c[1], 3) == w} == set(GAMMA_SC), w
    assert {c[2:] for c in RES_CASES if c[1] == SMALL_C} == set(GAMMA_SC)
    for nv in (1, 2, 3, 4):
        assert {c[2] for c in DUAL_CASES if _nv(c[1]) == nv} == set(DROPS), nv
    # the column-tiled kernels: a ragged and a full last tile, one and several tiles, every row count at 384 and 1152
    for name, cases in (('scale_residual', SR_CASES), ('gelu / colsum', TILE_CASES)):
        widths = {c for _, c in cases}
        assert {_ragged_tile(c) for c in widths if c % 8 == 0} == {False, True}, name
        assert {_col_tiles(c) for c in widths} >= {1, 2, 5}, name
        assert _ragged_tile(384) and _ragged_tile(1152) and not _ragged_tile(256)
        for c in (384, 1152):
            assert {r for r, cc in cases if cc == c} == set(TILE_ROWS), (name, c)
        assert {r for r, _ in cases} == set(TILE_ROWS)
    assert {c % 8 for _, c in SR_CASES} == {0, 4}             # the strip kernel's own widths
    assert [_strips_of_32(r) for r in TILE_ROWS] == [(32, 1), (32, 1), (32, 1), (32, 2), (32, 3)]
    assert _dw_slots(DW_C) == 10 and 256 - 10 * (DW_C // 4) == 16
    assert {_nv(c) for c in ENTRY_WIDTHS} == {1, 2, 3, 4, 8} and SMALL_C in ENTRY_WIDTHS and all(_ragged(c) for c in ENTRY_WIDTHS)


# ---------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    import _vah
    return _vah


def _p(t):
    return t.data_ptr() if t is not None else None


def _bound(ref, A, out=None):
    """the budget: C_ACC * 2^-24 * A, + 2^-8 |ref| for a bf16 output, + 2^-11 |ref| + 2^-25 for an fp16 output"""
    bound = C_ACC * U * A.double().reshape(-1)
    if out == BF16:
        bound = bound + 2.0 ** -8 * ref.abs()
    elif out == F16:
        bound = bound + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    return bound


def _worst(got, ref, A, out=None, bound=None):
    """worst err / budget over the elements (inf for a NaN, an element that was not written)"""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    bound = _bound(ref, A, out) if bound is None else bound.double().reshape(-1)
    err = (got - ref).abs()
    over = ~(err <= bound)
    ratio = torch.where(over & (bound == 0), torch.full_like(err, float('inf')), err / bound.clamp_min(1e-300))
    return float(ratio.nan_to_num(float('inf')).max()) if ratio.numel() else 0.0, over, err, bound


def _within(got, ref, A, what, out=None, bound=None):
    """Prints the worst err / budget ratio, then asserts that every element is inside its budget."""
    ratio, over, err, bound = _worst(got, ref, A, out, bound)
    print('RATIO %-34s %s %.4g' % (what, {None: 'f32', BF16: 'bf16', F16: 'fp16'}[out], ratio))
    nbad = int(over.sum())
    if nbad:
        i = int(torch.nonzero(over)[0])
        raise AssertionError('%s: %d of %d elements over budget; first at %d: got %r ref %r budget %.3e (worst err / budget '
                             '%.3g)' % (what, nbad, over.numel(), i, got.reshape(-1)[i].item(), ref.reshape(-1)[i].item(),
                                        bound[i].item(), ratio))


def _equal(a, b, what):
    assert torch.equal(a, b), '%s: two identical calls differ (%d elements)' % (what, int((a != b).sum()))


def _partial_rows(ws, nparts, K, what):
    """the first nparts rows of K floats were written, nothing behind them was"""
    assert bool(torch.isfinite(ws[:nparts * K]).all()), '%s: a partial row of the %d x %d the launch writes is not finite' % (what, nparts, K)
    assert bool(torch.isnan(ws[nparts * K:]).all()), '%s: the workspace was written behind its %d partial rows' % (what, nparts)


def _check_ln_fwd(y, mean, rstd, x, w, b, C, what, dtype):
    yr, A_y, mu, ma, rs = _ln_fwd_ref(x, w, b, C)
    _within(mean, mu, ma, what + ' mean')
    _within(rstd, rs, rs * (1.0 + ma * rs), what + ' rstd')
    _within(y, yr, A_y, what + ' y', out=dtype)


def _check_bpart(bpart, nparts, dz, C, what):
    """the partial rows add up (in fp64) to the column sums of the 16-bit tensor the kernel wrote"""
    _partial_rows(bpart, nparts, C, what)
    d = dz.reshape(-1, C).double()
    _within(bpart[:nparts * C].view(nparts, C).double().sum(0), d.sum(0), d.abs().sum(0), what)


SCALES = (1.0 / 0.7, 0.45, 1.0 / 0.9, 0.0, 1.25)           # DropPath(0.3) and (0.1) keeping an image, a dropped image


def _split(rows):
    """(batch, scales): batch 2 where the rows split evenly, else 3 or 5 where they do, else one image"""
    batch = next((n for n in (2, 3, 5) if rows % n == 0), 1)
    return batch, torch.tensor(SCALES[:batch], device='cuda')


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows,C', LN_CASES)
def test_layer_norm_widths(rows, C, dtype):
    """Forward, backward without and with the residual-branch gradient gres."""
    from vitadapter import fused
    v = _lib()
    x, w, b = _ln_data(rows, C, 100 + rows % 97 + C)
    g = torch.randn(rows, C, device='cuda').to(dtype)
    gres = torch.randn(rows, C, device='cuda')
    nparts = _bwd_blocks(rows, C, 2)
    st = _stream()
    outs = []
    for _ in range(2):
        gd = _Guarded()
        y, mean, rstd = gd.nan(rows, C, dtype=dtype), gd.nan(rows), gd.nan(rows)
        v.call('vah_layernorm_fwd_f32_bf16', dtype, x.data_ptr(), w.data_ptr(), b.data_ptr(), rows, C, EPS, y.data_ptr(),
               mean.data_ptr(), rstd.data_ptr(), st)
        res = [y, mean, rstd]
        for gr in (None, gres):
            dx, dw, db = gd.nan(rows, C), gd.nan(C), gd.nan(C)
            ws = gd.nan(v.lib.vah_reduce_ws_floats(2 * C))
            v.call('vah_layernorm_bwd_f32_bf16', dtype, x.data_ptr(), g.data_ptr(), w.data_ptr(), mean.data_ptr(),
                   rstd.data_ptr(), _p(gr), rows, C, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st)
            res += [dx, dw, db, ws]
        torch.cuda.synchronize()
        gd.check('layer_norm %dx%d' % (rows, C))
        outs.append(res)
    names = ('y', 'mean', 'rstd', 'dx', 'dw', 'db', 'ws', 'dx+gres', 'dw (gres)', 'db (gres)', 'ws (gres)')
    for a, c, nm in zip(outs[0], outs[1], names):
        if not nm.startswith('ws'):
            _equal(a, c, nm)
    y, mean, rstd, dx, dw, db, ws0, dxr, dwr, dbr, ws1 = outs[0]
    for wsk in (ws0, ws1):
        _partial_rows(wsk, nparts, 2 * C, 'layer_norm workspace')
    if C in ENTRY_WIDTHS:                    # the entry points: same kernels, same bits
        ln = _norm(C, w, b)
        xe = x.clone().requires_grad_(True)
        with torch.autocast('cuda', dtype=dtype):
            ye = fused.layer_norm(ln, xe)
        assert type(ye.grad_fn).__name__ == '_LayerNormBF16Backward' and ye.dtype == dtype
        ye.backward(g)
        for a, c, nm in ((ye, y, 'y'), (xe.grad, dx, 'dx'), (ln.weight.grad, dw, 'dw'), (ln.bias.grad, db, 'db')):
            assert torch.equal(a, c), 'fused.layer_norm %s differs from the direct call' % nm
        ln.zero_grad(set_to_none=True)
        xe = x.clone().requires_grad_(True)
        with torch.autocast('cuda', dtype=dtype):
            xk, ye = fused.layer_norm_keep(ln, xe * 1.0)
        assert type(ye.grad_fn).__name__ == '_LayerNormBF16Backward'
        torch.autograd.backward([xk, ye], [gres, g])
        for a, c, nm in ((ye, y, 'y'), (xe.grad, dxr, 'dx'), (ln.weight.grad, dwr, 'dw'), (ln.bias.grad, dbr, 'db')):
            assert torch.equal(a, c), 'fused.layer_norm_keep %s differs from the direct call' % nm
        del xe, xk, ye, ln
    _check_ln_fwd(y, mean, rstd, x, w, b, C, 'layer_norm', dtype)
    for gr, (a, bw, bb), tag in ((None, (dx, dw, db), ''), (gres, (dxr, dwr, dbr), ' +gres')):
        rdx, A_dx, rdw, A_dw, rdb, A_db = _ln_bwd_ref(x, g, w, mean, rstd, gr)
        _within(a, rdx, A_dx, 'layer_norm dx' + tag)
        _within(bw, rdw, A_dw, 'layer_norm dgamma' + tag)
        _within(bb, rdb, A_db, 'layer_norm dbeta' + tag)


# ---------------------------------------------------------------------------------------------------------------
# residual + LayerNorm: t = x + sc[b] * gamma * z, h = LayerNorm(t)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows,C,with_gamma,with_sc', RES_CASES)
def test_residual_ln_widths(rows, C, with_gamma, with_sc, dtype):
    """With / without gamma and the DropPath scales (the images with different scales so a wrong batch index shows); the
    backward with and without the stream gradient gt; without a gamma also the `_bsum` form, which must give the bits of
    the plain one and partial rows that add up to the column sums of its dz."""
    from vitadapter import fused
    v = _lib()
    x, w, b = _ln_data(rows, C, 200 + rows % 89 + C)
    batch, sc = _split(rows)
    if not with_sc:
        sc = None
    rpb = rows // batch
    z = torch.randn(rows, C, device='cuda').to(dtype)
    gamma = torch.randn(C, device='cuda') * 0.5 if with_gamma else None
    gh = torch.randn(rows, C, device='cuda').to(dtype)
    gt = torch.randn(rows, C, device='cuda')
    gp, sp = _p(gamma), _p(sc)
    nparts = _bwd_blocks(rows, C, 3)
    st = _stream()
    outs, sums = [], []
    for _ in range(2):
        gd = _Guarded()
        t, h, mean, rstd = gd.nan(rows, C), gd.nan(rows, C, dtype=dtype), gd.nan(rows), gd.nan(rows)
        v.call('vah_residual_layernorm_fwd', dtype, x.data_ptr(), z.data_ptr(), gp, sp, batch, rpb, C, w.data_ptr(), b.data_ptr(),
               EPS, t.data_ptr(), h.data_ptr(), mean.data_ptr(), rstd.data_ptr(), st)
        res, bres = [t, h, mean, rstd], []
        for gtt in (gt, None):
            for bsum in ((False,) if with_gamma else (False, True)):
                dt, dz = gd.nan(rows, C), gd.nan(rows, C, dtype=dtype)
                dgm, dw, db = gd.nan(C), gd.nan(C), gd.nan(C)
                ws = gd.nan(v.lib.vah_reduce_ws_floats(3 * C))
                args = (t.data_ptr(), gh.data_ptr(), w.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(gtt), z.data_ptr(), gp, sp,
                        batch, rpb, C, dt.data_ptr(), dz.data_ptr(), dgm.data_ptr() if with_gamma else None, dw.data_ptr(),
                        db.data_ptr(), ws.data_ptr())
                if bsum:
                    bpart, n = gd.nan(v.lib.vah_reduce_ws_floats(C)), ctypes.c_int64(-1)
                    v.call('vah_residual_layernorm_bwd_bsum', dtype, *args, bpart.data_ptr(), ctypes.byref(n), st)
                    bres += [dt, dz, dw, db, ws, bpart, n.value]
                else:
                    v.call('vah_residual_layernorm_bwd', dtype, *args, st)
                    res += [dt, dz, dgm, dw, db, ws]
        torch.cuda.synchronize()
        gd.check('residual_ln %dx%d' % (rows, C))
        outs.append(res)
        sums.append(bres)
    for k, (a, c) in enumerate(zip(outs[0], outs[1])):
        if k in (9, 15):                          # workspaces
            continue
        if not with_gamma and k in (6, 12):       # dgamma is not written without gamma
            assert bool(torch.isnan(a).all())
            continue
        _equal(a, c, 'output %d' % k)
    t, h, mean, rstd, dt, dz, dgm, dw, db, ws0, dt0, dz0, dgm0, dw0, db0, ws1 = outs[0]
    for wsk in (ws0, ws1):
        _partial_rows(wsk, nparts, 3 * C, 'residual_ln workspace')
    for k, plain in enumerate(((dt, dz, dw, db), (dt0, dz0, dw0, db0)) if not with_gamma else ()):
        bdt, bdz, bdw, bdb, bws, bpart, n = sums[0][7 * k:7 * k + 7]
        tag = 'residual_ln_bsum' + (' gt=0' if k else '')
        for a, c, nm in zip((bdt, bdz, bdw, bdb), plain, ('dt', 'dz', 'dw', 'db')):
            assert torch.equal(a, c), '%s %s differs from the entry point without _bsum' % (tag, nm)
        assert n == sums[1][7 * k + 6] == nparts, (tag, n, nparts)
        _equal(bpart[:n * C], sums[1][7 * k + 5][:n * C], tag + ' partial rows')
        _partial_rows(bws, nparts, 2 * C, tag + ' workspace')       # [dw | db] rows beside the bias partials
        _check_bpart(bpart, n, bdz, C, tag + ' partial rows')
    if C in ENTRY_WIDTHS and C <= 1024:           # the entry point (fused.residual_ln takes the fused form up to 1024)
        ln = _norm(C, w, b)
        xe = x.view(batch, rpb, C).clone().requires_grad_(True)
        ze = z.view(batch, rpb, C).clone().requires_grad_(True)
        ge = gamma.clone().requires_grad_(True) if with_gamma else None
        with _fixed_drop(sc), torch.autocast('cuda', dtype=dtype):
            te, he = fused.residual_ln(xe, ze, ge, _Drop() if with_sc else None, ln)
        assert type(he.grad_fn).__name__ == '_ResidualLNBackward' and he.dtype == dtype and te.dtype == torch.float32
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
    _check_ln_fwd(h, mean, rstd, t, w, b, C, 'residual_ln', dtype)
    sgd = scr * gmd
    for gtt, (a_dt, a_dz, a_dgm, a_dw, a_db), tag in ((gt, (dt, dz, dgm, dw, db), ''), (None, (dt0, dz0, dgm0, dw0, db0), ' gt=0')):
        rdt, A_dt, rdw, A_dw, rdb, A_db = _ln_bwd_ref(t, gh, w, mean, rstd, gtt)
        _within(a_dt, rdt, A_dt, 'residual_ln dt' + tag)
        _within(a_dz, sgd * rdt, sgd.abs() * A_dt, 'residual_ln dz' + tag, out=dtype)
        if with_gamma:       # dgamma = sum sc * dt * z: held to the kernel's own dt (checked above) as the operand
            szd = scr * a_dt.double() * z.double()
            _within(a_dgm, szd.sum(0), szd.abs().sum(0), 'residual_ln dgamma' + tag)
        _within(a_dw, rdw, A_dw, 'residual_ln dw' + tag)
        _within(a_db, rdb, A_db, 'residual_ln db' + tag)


# ---------------------------------------------------------------------------------------------------------------
# two LayerNorms of the same rows
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows,C,drop', DUAL_CASES)
def test_layer_norm_dual_widths(rows, C, drop, dtype):
    from vitadapter import fused
    v = _lib()
    x, wa, ba = _ln_data(rows, C, 300 + rows % 83 + C)
    wb = torch.randn(C, device='cuda') * 0.3 + 1.0
    bb = torch.randn(C, device='cuda') * 0.3
    ga = torch.randn(rows, C, device='cuda').to(dtype) if drop != 'ga' else None
    gb = torch.randn(rows, C, device='cuda').to(dtype) if drop != 'gb' else None
    gres = torch.randn(rows, C, device='cuda') if drop != 'gres' else None
    nparts = _dual_bwd_blocks(rows)
    st = _stream()
    outs = []
    for _ in range(2):
        gd = _Guarded()
        ya, yb = gd.nan(rows, C, dtype=dtype), gd.nan(rows, C, dtype=dtype)
        mean, rstd = gd.nan(rows), gd.nan(rows)
        v.call('vah_layernorm_dual_fwd', dtype, x.data_ptr(), wa.data_ptr(), ba.data_ptr(), wb.data_ptr(), bb.data_ptr(), rows, C,
               EPS, ya.data_ptr(), yb.data_ptr(), mean.data_ptr(), rstd.data_ptr(), st)
        dx, dp = gd.nan(rows, C), gd.nan(4, C)
        ws = gd.nan(v.lib.vah_reduce_ws_floats(2 * C))
        v.call('vah_layernorm_dual_bwd', dtype, x.data_ptr(), _p(ga), _p(gb), wa.data_ptr(), wb.data_ptr(), mean.data_ptr(),
               rstd.data_ptr(), _p(gres), rows, C, dx.data_ptr(), dp.data_ptr(), ws.data_ptr(), st)
        torch.cuda.synchronize()
        gd.check('layer_norm_dual %dx%d' % (rows, C))
        outs.append((ya, yb, mean, rstd, dx, dp, ws))
    for a, c, nm in zip(outs[0], outs[1], ('ya', 'yb', 'mean', 'rstd', 'dx', 'dparams')):
        _equal(a, c, nm)
    ya, yb, mean, rstd, dx, dp, ws = outs[0]
    _partial_rows(ws, nparts, 4 * C, 'dual workspace')
    if C in ENTRY_WIDTHS:
        na, nb = _norm(C, wa, ba), _norm(C, wb, bb)
        xe = x.clone().requires_grad_(True)
        with torch.autocast('cuda', dtype=dtype):
            xk, yae, ybe = fused.layer_norm_dual_keep(na, nb, xe * 1.0)
        assert type(yae.grad_fn).__name__ == '_LayerNormDualBF16Backward' and yae.dtype == dtype and ybe.dtype == dtype
        heads = [(t_, g_) for t_, g_ in ((xk, gres), (yae, ga), (ybe, gb)) if g_ is not None]
        torch.autograd.backward([h_[0] for h_ in heads], [h_[1] for h_ in heads])
        for a, c, nm in ((yae, ya, 'ya'), (ybe, yb, 'yb'), (xe.grad, dx, 'dx'), (na.weight.grad, dp[0], 'dwa'),
                         (na.bias.grad, dp[1], 'dba'), (nb.weight.grad, dp[2], 'dwb'), (nb.bias.grad, dp[3], 'dbb')):
            assert torch.equal(a, c), 'fused.layer_norm_dual_keep %s differs from the direct call' % nm
        del xe, xk, yae, ybe
    _check_ln_fwd(ya, mean, rstd, x, wa, ba, C, 'dual a', dtype)
    _check_ln_fwd(yb, mean, rstd, x, wb, bb, C, 'dual b', dtype)
    zero = torch.zeros(rows, C, dtype=dtype, device='cuda')
    dxa, A_a, dwa, A_wa, dba, A_ba = _ln_bwd_ref(x, ga if ga is not None else zero, wa, mean, rstd, gres)
    dxb, A_b, dwb, A_wb, dbb, A_bb = _ln_bwd_ref(x, gb if gb is not None else zero, wb, mean, rstd, None)
    _within(dx, dxa + dxb, A_a + A_b, 'dual dx')
    for got, ref, A, nm in ((dp[0], dwa, A_wa, 'dwa'), (dp[1], dba, A_ba, 'dba'), (dp[2], dwb, A_wb, 'dwb'),
                            (dp[3], dbb, A_bb, 'dbb')):
        _within(got, ref, A, 'dual ' + nm)


# ---------------------------------------------------------------------------------------------------------------
# scale_residual: y = x + sc[b] * gamma * z; backward dz = sc * gamma * g, dgamma = sum sc * g * z
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('with_gamma', [True, False], ids=['gamma', 'plain'])
@pytest.mark.parametrize('rows,C', SR_CASES)
def test_scale_residual_widths(rows, C, with_gamma, dtype):
    """Forward; the backward (with a gamma the row-strip kernel, without one the flat scale-only pass); the `_bsum`
    backward (without a gamma and C % 8 == 0 the column-tiled kernel, else the row-strip kernel with its second
    accumulator), which must give the bits of the plain one."""
    from vitadapter import fused
    v = _lib()
    torch.manual_seed(400 + C + rows)
    batch, sc = _split(rows)
    rpb = rows // batch
    x = torch.randn(rows, C, device='cuda')
    z = torch.randn(rows, C, device='cuda').to(dtype)
    gamma = torch.randn(C, device='cuda') * 0.5 if with_gamma else None
    gp = _p(gamma)
    g = torch.randn(rows, C, device='cuda')
    tiled = not with_gamma and C % 8 == 0
    nparts = (_strips_of_32(rows) if tiled else _row_strips(rows))[1]
    st = _stream()
    outs = []
    for _ in range(2):
        gd = _Guarded()
        y = gd.nan(rows, C)
        v.call('vah_scale_residual_fwd', dtype, x.data_ptr(), z.data_ptr(), gp, sc.data_ptr(), batch, rpb, C, y.data_ptr(), st)
        res = [y]
        for bsum in (False, True):
            dz, dgm = gd.nan(rows, C, dtype=dtype), gd.nan(C)
            ws = gd.nan(v.lib.vah_reduce_ws_floats(C))
            args = (g.data_ptr(), z.data_ptr(), gp, sc.data_ptr(), batch, rpb, C, dz.data_ptr(), dgm.data_ptr() if with_gamma else None,
                    ws.data_ptr() if with_gamma else None)
            if bsum:
                bpart, n = gd.nan(v.lib.vah_reduce_ws_floats(C)), ctypes.c_int64(-1)
                v.call('vah_scale_residual_bwd_bsum', dtype, *args, bpart.data_ptr(), ctypes.byref(n), st)
                res += [dz, dgm, ws, bpart, n.value]
            else:
                v.call('vah_scale_residual_bwd', dtype, *args, st)
                res += [dz, dgm, ws]
        torch.cuda.synchronize()
        gd.check('scale_residual %dx%d' % (rows, C))
        outs.append(res)
    y, dz, dgm, ws, bdz, bdgm, bws, bpart, n = outs[0]
    _equal(y, outs[1][0], 'y')
    _equal(dz, outs[1][1], 'dz')
    assert torch.equal(bdz, dz) and torch.equal(outs[1][4], dz), 'dz of the _bsum entry point differs'
    assert n == outs[1][8] == nparts, (n, nparts)
    _equal(bpart[:n * C], outs[1][7][:n * C], 'partial rows')
    if with_gamma:
        _equal(dgm, outs[1][2], 'dgamma')
        assert torch.equal(bdgm, dgm) and torch.equal(outs[1][5], dgm), 'dgamma of the _bsum entry point differs'
        for wsk in (ws, bws):
            _partial_rows(wsk, _row_strips(rows)[1], C, 'scale_residual workspace')
    else:
        assert bool(torch.isnan(torch.cat([dgm, bdgm, ws, bws])).all()), 'no gamma: dgamma and the workspace stay untouched'
    _check_bpart(bpart, n, bdz, C, 'scale_residual_bsum partial rows')
    if C in (12, SMALL_C, 1152):              # the entry point; with the branch marked as a fused Linear's output the _bsum form
        for marked in (False, True):
            xe = x.view(batch, rpb, C).clone().requires_grad_(True)
            ze = z.view(batch, rpb, C).clone().requires_grad_(True)
            if marked:
                setattr(ze, fused._BiasPartials.ATTR, True)
            ge = gamma.clone().requires_grad_(True) if with_gamma else None
            with _fixed_drop(sc), torch.autocast('cuda', dtype=dtype):
                ye = fused.residual(xe, ze, ge, _Drop())
            assert type(ye.grad_fn).__name__ == '_ScaleResidualBackward'
            ye.backward(g.view(batch, rpb, C))
            for a, c, nm in [(ye, y, 'y'), (ze.grad, dz, 'dz')] + ([(ge.grad, dgm, 'dgamma')] if with_gamma else []):
                assert torch.equal(a.reshape(c.shape), c), 'fused.residual %s differs from the direct call' % nm
            del xe, ze, ye
        fused.BIAS_PARTIALS.begin_epoch()
    scr = sc.double().repeat_interleave(rpb).view(-1, 1)
    gmd = gamma.double() if with_gamma else 1.0
    sgz = scr * gmd * z.double()
    _within(y, x.double() + sgz, x.double().abs() + sgz.abs(), 'scale_residual y')
    sg = scr * gmd * g.double()
    _within(dz, sg, sg.abs(), 'scale_residual dz', out=dtype)
    if with_gamma:
        sgz = scr * g.double() * z.double()
        _within(dgm, sgz.sum(0), sgz.abs().sum(0), 'scale_residual dgamma')


# ---------------------------------------------------------------------------------------------------------------
# GELU backward with the column sums of its result; column sums of a 16-bit matrix
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows,C', TILE_CASES)
def test_gelu_bwd_bsum_widths(rows, C, dtype):
    """dh against the fp64 value of da * (Phi(h) + h phi(h)) from the same 16-bit operands: the rounding of the result plus
    2^-20 |da| for the fp32 evaluation (tests/test_bias_partials_gpu.py, tests/test_gemm_f16_fp64_gpu.py)."""
    from vitadapter import fused
    v = _lib()
    gen = torch.Generator(device='cuda').manual_seed(rows + C)
    h = (torch.randn(rows, C, device='cuda', generator=gen) * 1.5).to(dtype)
    da = torch.randn(rows, C, device='cuda', generator=gen).to(dtype)
    nparts = _strips_of_32(rows)[1]
    st = _stream()
    outs = []
    for _ in range(2):
        gd = _Guarded()
        dh, bpart, n = gd.nan(rows, C, dtype=dtype), gd.nan(v.lib.vah_reduce_ws_floats(C)), ctypes.c_int64(-1)
        v.call('vah_gelu_bwd_bsum_bf16', dtype, da.data_ptr(), h.data_ptr(), rows, C, dh.data_ptr(), bpart.data_ptr(), ctypes.byref(n), st)
        torch.cuda.synchronize()
        gd.check('gelu_bwd_bsum %dx%d' % (rows, C))
        outs.append((dh, bpart, n.value))
    dh, bpart, n = outs[0]
    assert n == outs[1][2] == nparts, (n, nparts)
    _equal(dh, outs[1][0], 'dh')
    _equal(bpart[:n * C], outs[1][1][:n * C], 'partial rows')
    if C in (SMALL_C, 1152, 1536):            # 1536: fc1 of the Small trunk
        he = h.clone().requires_grad_(True)
        setattr(he, fused._BiasPartials.ATTR, True)           # as fused.linear marks its output
        with torch.autocast('cuda', dtype=dtype):
            a = fused.gelu(torch.nn.GELU(), he)
        assert type(a.grad_fn).__name__ == '_GeluBF16Backward'
        a.backward(da)
        assert torch.equal(he.grad, dh), 'fused.gelu dh differs from the direct call'
        fused.BIAS_PARTIALS.begin_epoch()
    ref = _gelu_ref64(da, h).reshape(-1)
    rnd = 2.0 ** -8 * ref.abs() if dtype == BF16 else 2.0 ** -11 * ref.abs() + 2.0 ** -25
    _within(dh, ref, None, 'gelu_bwd dh', out=dtype, bound=rnd + 2.0 ** -20 * da.double().abs().reshape(-1))
    _check_bpart(bpart, n, dh, C, 'gelu_bwd partial rows')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows,C', TILE_CASES)
def test_colsum_widths(rows, C, dtype):
    v = _lib()
    torch.manual_seed(600 + rows + C)
    g = torch.randn(rows, C, device='cuda').to(dtype)
    nparts = _colsum_strips(rows, C)[1]
    st = _stream()
    outs = []
    for _ in range(2):
        gd = _Guarded()
        out, ws = gd.nan(C), gd.nan(v.lib.vah_reduce_ws_floats(C))
        v.call('vah_colsum_bf16', dtype, g.data_ptr(), rows, C, out.data_ptr(), ws.data_ptr(), st)
        part, n = gd.nan(v.lib.vah_reduce_ws_floats(C)), ctypes.c_int64(-1)
        v.call('vah_colsum_bf16_partials', dtype, g.data_ptr(), rows, C, part.data_ptr(), ctypes.byref(n), st)
        torch.cuda.synchronize()
        gd.check('colsum %dx%d' % (rows, C))
        outs.append((out, ws, part, n.value))
    out, ws, part, n = outs[0]
    assert n == outs[1][3] == nparts, (n, nparts)
    _equal(out, outs[1][0], 'colsum')
    _equal(part[:n * C], outs[1][2][:n * C], 'partial rows')
    assert torch.equal(ws[:n * C], part[:n * C]), 'vah_colsum and vah_colsum_partials leave different partial rows'
    _partial_rows(ws, n, C, 'colsum workspace')
    _within(out, g.double().sum(0), g.double().abs().sum(0), 'colsum')
    _check_bpart(part, n, g, C, 'colsum partial rows')


# ---------------------------------------------------------------------------------------------------------------
# DWConv 3x3 on the concatenated token maps at the Small ConvFFN width
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('B,H,W', DW_CASES)
def test_dwconv_tokens_small_width(B, H, W, dtype):
    """C = 96: 24 channel groups, 10 token slots per workgroup and 16 idle lanes; (1, 2, 2) has a 1 x 1 bottom map."""
    from vitadapter import fused
    v = _lib()
    C = DW_C
    torch.manual_seed(500 + C + H)
    N = 21 * (H // 2) * (W // 2)
    x = torch.randn(B, N, C, device='cuda').to(dtype)
    g = torch.randn(B, N, C, device='cuda').to(dtype)
    w9 = torch.randn(C, 9, device='cuda') * 0.3
    bias = torch.randn(C, device='cuda') * 0.3
    st = _stream()
    outs = []
    for _ in range(2):
        gd = _Guarded()
        y, dx = gd.nan(B, N, C, dtype=dtype), gd.nan(B, N, C, dtype=dtype)
        v.call('vah_dwconv3x3_tokens_bf16', dtype, x.data_ptr(), w9.data_ptr(), bias.data_ptr(), B, H, W, C, 0, y.data_ptr(), st)
        v.call('vah_dwconv3x3_tokens_bf16', dtype, g.data_ptr(), w9.data_ptr(), None, B, H, W, C, 1, dx.data_ptr(), st)
        dw, db = gd.nan(C * 9), gd.nan(C)
        ws = gd.nan(v.lib.vah_reduce_ws_floats(10 * C))
        v.call('vah_dwconv3x3_tokens_wgrad_bf16', dtype, x.data_ptr(), g.data_ptr(), B, H, W, C, dw.data_ptr(), db.data_ptr(),
               ws.data_ptr(), st)
        torch.cuda.synchronize()
        gd.check('dwconv_tokens')
        outs.append((y, dx, dw, db))
    for a, c, nm in zip(outs[0], outs[1], ('y', 'dx', 'dw', 'db')):
        _equal(a, c, nm)
    y, dx, dw, db = outs[0]
    conv = torch.nn.Conv2d(C, C, 3, padding=1, groups=C).cuda()
    with torch.no_grad():
        conv.weight.copy_(w9.view(C, 1, 3, 3))
        conv.bias.copy_(bias)
    xe = x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=dtype):
        ye = fused.dwconv_tokens(conv, xe, H, W)
    assert ye is not None and type(ye.grad_fn).__name__ == '_DWConvTokensBackward' and ye.dtype == dtype
    ye.backward(g)
    for a, c, nm in ((ye, y, 'y'), (xe.grad, dx, 'dx'), (conv.weight.grad.reshape(-1), dw, 'dw'), (conv.bias.grad, db, 'db')):
        assert torch.equal(a, c), 'fused.dwconv_tokens %s differs from the direct call' % nm
    del xe, ye, conv
    ry, Ay, rdx, Adx, rdw, Adw, rdb, Adb = _dwconv_ref(x, g, w9, bias, H, W)
    _within(y, ry, Ay, 'dwconv y', out=dtype)
    _within(dx, rdx, Adx, 'dwconv dx', out=dtype)
    _within(dw, rdw, Adw, 'dwconv dw')
    _within(db, rdb, Adb, 'dwconv db')
