"""CPU: what tests/test_fused_widths_fp64_gpu.py rests on, checked without a GPU.

1. Its Python mirror of the launch arithmetic of csrc/fused_ops.hip (_nv, _waves, block counts, the three strip rules)
   against values worked out by hand from the launch helpers, both wave switches included, and the coverage its case
   lists claim.
2. Its budget (64 * 2^-24 * A, + 2^-8 |ref| for bf16, + 2^-11 |ref| + 2^-25 for fp16) separates right from wrong.  The
   kernels' fp32 evaluation order is emulated in torch float32 - per lane a running sum over its float4 slots, then the
   six steps across the 64 lanes; per wave a running sum over the rows it walks, the waves of a workgroup in order, then
   finalize_partials - and must lie inside the budget of the fp64 references (those of
   tests/test_reductions_fullsize_gpu.py, on CPU tensors) for mean, rstd, y, dx, dw and db.  Each of the faults the GPU
   file is there to catch must lie outside it on at least one element: the last float4 of a row left out of the
   statistics, the clamped duplicate of the last vector counted once more, one row dropped from dw / db, one row's dz
   written with the other image's drop-path scale, the last 128 columns of a 384-wide column sum left at zero.
   C in {260, 384, 508, 1028}: one live lane in the last slot, the Small width, one vector short of full, NV = 8."""
import pytest
import torch

import test_fused_widths_fp64_gpu as W
from test_reductions_fullsize_gpu import EPS, _ln_bwd_ref, _ln_fwd_ref

BF16, F16 = torch.bfloat16, torch.float16
WIDTHS = [260, 384, 508, 1028]
ROWS = 9                 # 8 waves: two workgroups, the second with one row; 4 waves (1028 in the residual form): three


# ---------------------------------------------------------------------------------------------------------------
# 1. the mirror
# ---------------------------------------------------------------------------------------------------------------
def test_nv_by_hand():
    want = {4: 1, 192: 1, 256: 1, 260: 2, 384: 2, 512: 2, 516: 3, 768: 3, 772: 4, 1024: 4, 1028: 8, 2048: 8}
    assert {c: W._nv(c) for c in want} == want
    with pytest.raises(ValueError):
        W._nv(2052)
    # ragged: fewer float4 groups than 64 * NV lanes-slots
    assert [W._ragged(c) for c in (252, 256, 260, 384, 508, 512, 1028, 2044, 2048)] == [True, False, True, True, True, False,
                                                                                       True, True, False]


def test_wave_switches_by_hand():
    # plain form: 8 waves x [dw | db] x C floats + w = (64 + 4) C bytes <= 81920  <=>  C <= 1204.7
    assert 68 * 1204 == 81872 <= 80 * 1024 < 68 * 1208 == 82144
    assert (W._waves(1204, 2), W._waves(1208, 2)) == (8, 4) and W._switch(2) == (1204, 1208)
    # residual form: 8 waves x [dw | db | dgamma] + w + gamma = (96 + 8) C bytes <= 81920  <=>  C <= 787.7
    assert 104 * 784 == 81536 <= 80 * 1024 < 104 * 788 == 81952
    assert (W._waves(784, 3), W._waves(788, 3)) == (8, 4) and W._switch(3) == (784, 788)
    assert [W._waves(c, 2) for c in (4, 384, 768, 1024, 2048)] == [8, 8, 8, 8, 4]
    assert [W._waves(c, 3) for c in (4, 384, 768, 1024, 2048)] == [8, 8, 8, 4, 4]


def test_block_counts_by_hand():
    assert [W._bwd_blocks(r, 384, 2) for r in (1, 8, 9, 33, 4088, 4095, 4096, 4097)] == [1, 1, 2, 5, 511, 512, 512, 512]
    assert [W._bwd_blocks(r, 1024, 3) for r in (4, 5, 9, 2047, 2048, 2049)] == [1, 2, 3, 512, 512, 512]
    assert [W._dual_bwd_blocks(r) for r in (1, 5, 1020, 1023, 1024, 1025)] == [1, 2, 255, 256, 256, 256]


def test_strip_rules_by_hand():
    # strips of a multiple of 32 rows, at most 512 of them
    assert [W._strips_of_32(r) for r in (1, 32, 33, 65, 2062, 16384, 16385)] == [(32, 1), (32, 1), (32, 2), (32, 3), (32, 65),
                                                                                (32, 512), (64, 257)]
    # the row-strip kernel: ceil(rows / 512) rows each
    assert [W._row_strips(r) for r in (1, 65, 512, 513, 2062)] == [(1, 1), (1, 65), (1, 512), (2, 257), (5, 413)]
    # colsum16_partials: min(512, 2048 / column tiles) strips of at least 32 rows
    assert W._colsum_strips(65, 384) == (32, 3) and W._colsum_strips(8192, 3072) == (49, 168)
    assert W._colsum_strips(16385, 768) == (33, 497) != W._strips_of_32(16385)
    assert [W._col_tiles(c) for c in (8, 256, 264, 384, 1152, 1536)] == [1, 1, 2, 2, 5, 6]
    assert [W._ragged_tile(c) for c in (8, 256, 384, 1152, 1536)] == [True, False, True, True, False]
    assert [W._dw_slots(c) for c in (48, 96, 192, 256)] == [21, 10, 5, 4]


def test_case_lists():
    W.test_the_case_list_covers_what_it_claims()
    assert len(W.LN_CASES) == len(set(W.LN_CASES)) and len(W.RES_CASES) == len(set(W.RES_CASES))
    assert max(r * c for r, c, *_ in W.LN_CASES + W.RES_CASES + W.DUAL_CASES + W.SR_CASES + W.TILE_CASES) == 4097 * 384
    assert set(WIDTHS) <= {c for _, c in W.LN_CASES}


# ---------------------------------------------------------------------------------------------------------------
# 2. the kernels' evaluation order in float32
# ---------------------------------------------------------------------------------------------------------------
LANES = torch.arange(64)


def _lane_sum(terms, fault=None):
    """wave_sum of the per-lane running sums over the float4 slots: lane l holds elements 4 * (l + 64 j) .. + 3 of slot j
    (dead slots add zeros).  Faults: 'skip_last' leaves the last float4 of the row out; 'dup_last' counts it once more,
    in the first dead slot - where the clamped load of the forward kernel puts it."""
    rows, C = terms.shape
    nv = W._nv(C)
    pad = torch.zeros(rows, 64 * nv * 4, dtype=torch.float32)
    pad[:, :C] = terms
    if fault == 'skip_last':
        pad[:, C - 4:C] = 0.
    elif fault == 'dup_last':
        assert W._ragged(C)
        pad[:, C:C + 4] = terms[:, C - 4:]
    t = pad.view(rows, nv, 64, 4)
    s = torch.zeros(rows, 64, dtype=torch.float32)
    for j in range(nv):
        s = s + (((t[:, j, :, 0] + t[:, j, :, 1]) + t[:, j, :, 2]) + t[:, j, :, 3])
    for step in (1, 2, 4, 8, 16, 32):
        s = s + s[:, LANES ^ step]
    return s[:, 0]


def _emu_fwd(x, w, b, dtype, fault=None):
    C = x.shape[1]
    mu = _lane_sum(x, fault) / float(C)
    d = x - mu[:, None]
    rs = torch.rsqrt(_lane_sum(d * d, fault) / float(C) + torch.tensor(EPS, dtype=torch.float32))
    return (d * rs[:, None] * w + b).to(dtype), mu, rs


def _finalize(part):
    """finalize_partials for at most 56 partial rows: 8 partial-row lanes, each a running sum, then the lanes in order"""
    n = part.shape[0]
    assert n <= 56
    t = torch.zeros(part.shape[1], dtype=torch.float32)
    for pl in range(8):
        acc = torch.zeros(part.shape[1], dtype=torch.float32)
        for p in range(pl, n, 8):
            acc = acc + part[p]
        t = t + acc
    return t


def _column_sums(terms, waves, blocks, drop_row=None):
    """sum over the rows as ln_bwd_kernel forms it: wave wv of workgroup blk walks rows blk * waves + wv + k * blocks * waves"""
    rows = terms.shape[0]
    part = []
    for blk in range(blocks):
        t = torch.zeros(terms.shape[1], dtype=torch.float32)
        for wv in range(waves):
            acc = torch.zeros(terms.shape[1], dtype=torch.float32)
            for row in range(blk * waves + wv, rows, blocks * waves):
                if row != drop_row:
                    acc = acc + terms[row]
            t = t + acc
        part.append(t)
    return _finalize(torch.stack(part))


def _emu_bwd(x, g, w, mean, rstd, gres, ncol, drop_row=None):
    rows, C = x.shape
    inv = torch.tensor(1.0, dtype=torch.float32) / float(C)
    xh = (x - mean[:, None]) * rstd[:, None]
    gf = g.float()
    gw = gf * w
    m1 = _lane_sum(gw) * inv
    m2 = _lane_sum(gw * xh) * inv
    dx = gres + rstd[:, None] * (gw - m1[:, None] - xh * m2[:, None])
    waves, blocks = W._waves(C, ncol), W._bwd_blocks(rows, C, ncol)
    return dx, _column_sums(gf * xh, waves, blocks, drop_row), _column_sums(gf, waves, blocks, drop_row)


def _data(C, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(ROWS, C, generator=gen) * 1.7 + 0.4           # the distribution of _ln_data
    w = torch.randn(C, generator=gen) * 0.3 + 1.0
    b = torch.randn(C, generator=gen) * 0.3
    g = torch.randn(ROWS, C, generator=gen).to(dtype)
    gres = torch.randn(ROWS, C, generator=gen)
    return x, w, b, g, gres


def _fwd_ratios(y, mu, rs, x, w, b, dtype):
    C = x.shape[1]
    yr, A_y, mur, ma, rsr = _ln_fwd_ref(x, w, b, C)
    return dict(mean=W._worst(mu, mur, ma)[0], rstd=W._worst(rs, rsr, rsr * (1.0 + ma * rsr))[0],
                y=W._worst(y, yr, A_y, dtype)[0])


def _bwd_ratios(dx, dw, db, x, g, w, mu, rs, gres):
    rdx, A_dx, rdw, A_dw, rdb, A_db = _ln_bwd_ref(x, g, w, mu, rs, gres)
    return dict(dx=W._worst(dx, rdx, A_dx)[0], dw=W._worst(dw, rdw, A_dw)[0], db=W._worst(db, rdb, A_db)[0])


@pytest.mark.parametrize('dtype', [BF16, F16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('C', WIDTHS)
def test_the_kernels_order_in_fp32_is_inside_the_budget(C, dtype):
    x, w, b, g, gres = _data(C, dtype, C)
    y, mu, rs = _emu_fwd(x, w, b, dtype)
    ratios = _fwd_ratios(y, mu, rs, x, w, b, dtype)
    for ncol in (2, 3):
        dx, dw, db = _emu_bwd(x, g, w, mu, rs, gres, ncol)
        ratios.update({'%s (%d waves)' % (k, W._waves(C, ncol)): r for k, r in _bwd_ratios(dx, dw, db, x, g, w, mu, rs, gres).items()})
    print('C %d %s: %s' % (C, dtype, ' '.join('%s %.3f' % kv for kv in ratios.items())))
    assert all(r <= 1.0 for r in ratios.values()), ratios
    # the fp32 quantities sit far inside (the GPU files report <= 0.05); a 16-bit output sits at its rounding bound
    assert max(r for k, r in ratios.items() if k != 'y') <= 0.25 and 0.5 <= ratios['y'] <= 1.0, ratios


@pytest.mark.parametrize('dtype', [BF16, F16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('C', WIDTHS)
@pytest.mark.parametrize('fault', ['skip_last', 'dup_last'])
def test_a_wrong_last_vector_in_the_statistics_is_outside(fault, C, dtype):
    """4 of C elements missing from (or counted twice in) the sums move the mean by about |x| * 4 / C, thousands of
    budgets; the y computed from such statistics leaves its budget too."""
    x, w, b, g, gres = _data(C, dtype, C + 1)
    ratios = _fwd_ratios(*_emu_fwd(x, w, b, dtype, fault), x, w, b, dtype)
    print('C %d %s %s: %s' % (C, dtype, fault, ratios))
    assert ratios['mean'] > 1.0 and ratios['rstd'] > 1.0 and ratios['y'] > 1.0, ratios


@pytest.mark.parametrize('dtype', [BF16, F16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('C', WIDTHS)
@pytest.mark.parametrize('ncol', [2, 3])
def test_a_dropped_row_in_dw_db_is_outside(ncol, C, dtype):
    """the last row (the one row of the last workgroup) left out of the column sums"""
    x, w, b, g, gres = _data(C, dtype, C + 2)
    _, mu, rs = _emu_fwd(x, w, b, dtype)
    dx, dw, db = _emu_bwd(x, g, w, mu, rs, gres, ncol, drop_row=ROWS - 1)
    ratios = _bwd_ratios(dx, dw, db, x, g, w, mu, rs, gres)
    print('C %d %s ncol %d: %s' % (C, dtype, ncol, ratios))
    assert ratios['dx'] <= 1.0 and ratios['dw'] > 1.0 and ratios['db'] > 1.0, ratios


@pytest.mark.parametrize('dtype', [BF16, F16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('C', WIDTHS)
def test_dz_with_the_other_images_scale_is_outside(C, dtype):
    """dz = sc[b] * gamma * dt, two images of 4 rows with the scales of the GPU file: row 3 written with sc[1]"""
    rows = 8
    x, w, b, g, gres = (t[:rows] if t.dim() == 2 else t for t in _data(C, dtype, C + 3))
    _, mu, rs = _emu_fwd(x, w, b, dtype)
    dt, _, _ = _emu_bwd(x, g, w, mu, rs, gres, 3)
    gamma = torch.randn(C, generator=torch.Generator().manual_seed(C)) * 0.5
    sc = torch.tensor(W.SCALES[:2], dtype=torch.float32)
    rdt, A_dt = _ln_bwd_ref(x, g, w, mu, rs, gres)[:2]
    sgd = sc.double().repeat_interleave(rows // 2).view(-1, 1) * gamma.double()
    for wrong in (False, True):
        scr = sc.repeat_interleave(rows // 2)
        if wrong:
            scr[3] = sc[1]
        dz = (scr[:, None] * gamma * dt).to(dtype)
        ratio, over = W._worst(dz, sgd * rdt, sgd.abs() * A_dt, dtype)[:2]
        print('C %d %s wrong scale %s: worst err / budget %.3f' % (C, dtype, wrong, ratio))
        assert (ratio > 1.0) == wrong
        if wrong:           # every over-budget element lies in the row with the wrong scale
            assert set((torch.nonzero(over).view(-1) // C).tolist()) == {3}


@pytest.mark.parametrize('dtype', [BF16, F16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('rows', [33, 65])
def test_a_column_tile_left_at_zero_is_outside(rows, dtype):
    """384 columns = a full tile of 256 and half a tile: colsum_bf16_kernel's order (8 row lanes, each a running sum over
    every 8th row of the strip; the lanes in order; the strips through finalize_partials), then columns 256 .. 383 zero"""
    C = 384
    g = torch.randn(rows, C, generator=torch.Generator().manual_seed(rows)).to(dtype)
    rpb, parts = W._colsum_strips(rows, C)
    part = []
    for p in range(parts):
        t = torch.zeros(C, dtype=torch.float32)
        for rl in range(8):
            acc = torch.zeros(C, dtype=torch.float32)
            for r in range(p * rpb + rl, min(rows, (p + 1) * rpb), 8):
                acc = acc + g[r].float()
            t = t + acc
        part.append(t)
    out = _finalize(torch.stack(part))
    ref, A = g.double().sum(0), g.double().abs().sum(0)
    good = W._worst(out, ref, A)[0]
    out[256:] = 0.
    bad, over = W._worst(out, ref, A)[:2]
    print('colsum %d x 384 %s: worst err / budget %.3f, with the half tile at zero %.3g' % (rows, dtype, good, bad))
    assert good <= 0.25 and bad > 1.0
    assert not bool(over[:256].any()) and int(over[256:].sum()) >= 120       # a column sum is rarely that close to zero
