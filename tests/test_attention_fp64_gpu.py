"""GPU: every path of the MFMA attention kernels, bf16 and fp16, held to fp64 (oracle/attention.py).

Paths: whole sequence (csrc/attn_flash.hip), resident window for every NB = ceil(win^2 / 32) = 1..7
(csrc/attn_win.hip), general window above 224 tokens (csrc/attn_fwd.hip, attn_bwd.hip), explicit bias and BEiT's
relative position bias (attn_flash.hip with bias, csrc/relpos.hip).  Each case

  * calls the C entry points directly, every output NaN-filled first (out, lse, the packed dqkv, ds_out, delta_ws,
    the workspaces, dtable and the relpos-grad ws), and checks o, lse, dq, dk, dv (and dbias from ds_out, dtable)
    against the fp64 reference from the exact 16-bit operands: (a) every element within its budget, (b)
    ||err|| <= 0.5 ||budget|| (budgets: oracle/attention.py);
  * checks lse of every real query, and +inf for the padded-grid queries of a window;
  * repeats the direct calls and requires the same bits (the backward is documented bitwise reproducible; the relpos
    table gradient is documented reproducible to fp32 rounding and is held to that);
  * runs the same inputs once through kernels.attention / window_attention / attention_bias / attention_relpos, whose
    output and gradient must equal the direct call's bit for bit.

Input regimes (oracle.attention.make_inputs): 'peaked', 'flat' (mean-shifted V: an extra or missing key moves every
output) and, for the whole-sequence kernels, 'late' (the row maximum rises in every 64-key tile: the online rescale).
Bias operands get NaN in their columns N..ldb, which the contract says are ignored.

Run with -s to see one RATIO line per checked tensor and the worst ratio per path and dtype at the end.  Acceptance
check for any change to the attention or relpos kernels."""
import math

import pytest
import torch

from oracle import attention as oa

pytestmark = pytest.mark.gpu

SCALE = 64 ** -0.5
NAN = float('nan')
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}
RESIDENT_MAX = 224

# whole sequence (B, N, H): edges of the 64-key tiles and 128-query blocks, then configs[1], [2], [4] of BASELINE
SEQ_CASES = [(2, 1, 2), (2, 63, 2), (2, 64, 2), (2, 65, 2), (2, 127, 2), (2, 128, 2), (2, 129, 2), (2, 333, 2),
             (2, 1024, 3), (2, 4096, 12), (1, 4200, 16)]
# windows (B, grid_h, grid_w, H, win): grids cut raggedly in both directions; NB 1..7, the 224 / 225 boundary, 256,
# then configs[2] (64 x 64, 12 heads) and configs[4] (50 x 84, 16 heads)
WIN_CASES = [(2, 3, 4, 2, 1), (2, 12, 7, 2, 5), (2, 13, 19, 2, 8), (2, 20, 11, 2, 9), (2, 15, 25, 2, 11),
             (2, 26, 13, 2, 12), (2, 14, 27, 2, 13), (2, 30, 17, 2, 14), (2, 64, 64, 12, 14), (1, 50, 84, 16, 14),
             (2, 17, 31, 2, 15), (2, 20, 33, 2, 16)]
# explicit bias (B, N, H): 1601 x 16 heads = configs[3]
BIAS_CASES = [(2, 5, 2), (2, 64, 2), (2, 197, 2), (1, 1025, 2), (2, 1601, 16)]
# relpos: (B, hw, H, windowed) - BEiT with class token at 14 x 14 and 40 x 40 (configs[3]); a 14 x 14 window of the
# detection BEiT (beit_det.py: no class token, windows as the batch)
RELPOS_CASES = [(2, (14, 14), 4, False), (2, (40, 40), 16, False), (6, (14, 14), 4, True)]

WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for key in sorted(WORST):
        a, b, case = WORST[key]
        print('WORST %-10s %-4s %-6s a=%.3f b=%.3f (%s)' % (key + (a, b, case)))


def _record(path, dtn, case, name, ab):
    a, b = ab
    print('RATIO %s %s %s %s a=%.4f b=%.4f' % (path, dtn, case, name, a, b))
    key = (path, dtn, name)
    prev = WORST.get(key)
    WORST[key] = (a, b, case) if prev is None else (max(a, prev[0]), max(b, prev[1]), case if a > prev[0] else prev[2])


def _check(path, dtn, case, name, got, ref, bud):
    _record(path, dtn, case, name, oa.check('%s %s %s %s' % (path, dtn, case, name), got, ref, bud))


def _vah():
    import _vah
    return _vah


def _call(name, dtype, *args):
    from vitadapter import kernels
    with _vah().on(torch.device('cuda')):
        kernels._call(name, dtype, *args)


def _stream():
    return _vah().raw_stream(torch.device('cuda'))


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device='cuda')


def _nan_bytes(n):
    return torch.full((max(int(n), 1),), 255, dtype=torch.uint8, device='cuda')     # 0xFF..: NaN as fp32, bf16 and fp16


def _inputs(B, N, H, regime, seed, dtype):
    qkv, dout = oa.make_inputs(B, N, H, regime, seed, SCALE)
    return qkv.to('cuda', dtype).contiguous(), dout.to('cuda', dtype).contiguous()


def _ptrs(qkv):
    C, esz = qkv.shape[3] * 64, qkv.element_size()
    base = qkv.data_ptr()
    return base, base + C * esz, base + 2 * C * esz


def _same(a, b, what):
    assert torch.equal(a, b), '%s: %d elements differ' % (what, int((a != b).sum()))


# ------------------------------------------------------------------------------------------------ whole sequence + bias
def _seq_direct(qkv, dout, bias_ops=None):
    """Direct forward + backward of the whole-sequence entry points.  bias_ops: (bias, bias_t, ldb) 16-bit operands."""
    B, N, _, H, _ = qkv.shape
    T, C = qkv.dtype, H * 64
    lib = _vah().lib
    q, k, v = _ptrs(qkv)
    out, lse = _nan((B, N, H, 64), T), _nan((B, H, N))
    if bias_ops is None:
        vt = _nan((B * H * 64 * lib.vah_attn_padded_len(N),), T)
        _call('vah_attn_fwd_bf16', T, q, k, v, 3 * C, N * 3 * C, B, H, N, SCALE, vt.data_ptr(), out.data_ptr(), C,
              lse.data_ptr(), _stream())
    else:
        bl, blt, ldb = bias_ops
        _call('vah_attn_bias_fwd_bf16', T, q, k, v, 3 * C, N * 3 * C, B, H, N, SCALE, bl.data_ptr(), ldb, out.data_ptr(),
              C, lse.data_ptr(), _stream())
    dqkv = _nan(tuple(qkv.shape), T)
    dq, dk, dv = _ptrs(dqkv)
    ds = None
    if bias_ops is None:
        ws = _nan_bytes(lib.vah_attn_bwd_workspace_bytes(B, H, N))
        _call('vah_attn_bwd_bf16', T, q, k, v, 3 * C, N * 3 * C, out.data_ptr(), dout.data_ptr(), C, lse.data_ptr(), B, H,
              N, SCALE, ws.data_ptr(), dq, dk, dv, 3 * C, N * 3 * C, _stream())
    else:
        ds, delta = _nan((B, H, N, ldb), T), _nan((B, H, N))
        _call('vah_attn_bias_bwd_bf16', T, q, k, v, 3 * C, N * 3 * C, out.data_ptr(), dout.data_ptr(), C, lse.data_ptr(),
              B, H, N, SCALE, bl.data_ptr(), blt.data_ptr(), ldb, ds.data_ptr(), delta.data_ptr(), dq, dk, dv, 3 * C,
              N * 3 * C, _stream())
    torch.cuda.synchronize()
    return out, lse, dqkv, ds


def _operands(qkv, dout):
    """(Z, H, N, 64) views of q, k, v, dO of a packed (Z, N, 3, H, 64) projection."""
    q, k, v = (t.transpose(1, 2) for t in qkv.unbind(2))
    return q, k, v, dout.transpose(1, 2)


def _check_seq(path, dtn, case, out, lse, dqkv, ref, dtype):
    _check(path, dtn, case, 'o', out.transpose(1, 2), ref['o'], oa.budget(ref, 'o', dtype))
    _check(path, dtn, case, 'lse', lse, ref['lse'], oa.budget(ref, 'lse', dtype))
    for i, n in enumerate(('dq', 'dk', 'dv')):
        _check(path, dtn, case, n, dqkv[:, :, i].transpose(1, 2), ref[n], oa.budget(ref, n, dtype))


SEQ_PARAMS = [(dtn, c, r) for dtn in DTYPES for c in SEQ_CASES for r in ('peaked', 'flat', 'late')]


@pytest.mark.parametrize('dtn,case,regime', SEQ_PARAMS, ids=['%s-B%d-N%d-H%d-%s' % ((d,) + c + (r,)) for d, c, r in SEQ_PARAMS])
def test_seq_attention_fp64(dtn, case, regime):
    from vitadapter import kernels
    dtype = DTYPES[dtn]
    B, N, H = case
    qkv, dout = _inputs(B, N, H, regime, N * 31 + H, dtype)
    out, lse, dqkv, _ = _seq_direct(qkv, dout)
    ref = oa.reference(*_operands(qkv, dout), SCALE)
    _check_seq('seq', dtn, '%s/N%d/%s' % (case, N, regime), out, lse, dqkv, ref, dtype)
    del ref
    out2, lse2, dqkv2, _ = _seq_direct(qkv, dout)
    _same(out, out2, 'repeat out')
    _same(lse, lse2, 'repeat lse')
    _same(dqkv, dqkv2, 'repeat dqkv')
    x = qkv.clone().requires_grad_(True)
    o3 = kernels.attention(x, SCALE)
    o3.backward(dout)
    _same(out, o3.detach(), 'kernels.attention out')
    _same(dqkv, x.grad, 'kernels.attention grad')


def _bias_ops(bias, N, dtype):
    """16-bit bias * log2(e) and its per-head transpose as the kernels read them, (H, N, ldb), NaN in columns N..ldb."""
    H = bias.shape[0]
    ldb = (N + 63) // 64 * 64
    b2 = bias.float() * 1.4426950408889634
    bl, blt = _nan((H, N, ldb), dtype), _nan((H, N, ldb), dtype)
    bl[:, :, :N] = b2
    blt[:, :, :N] = b2.transpose(1, 2)
    return bl, blt, ldb


def _check_bias_grad(path, dtn, case, ds, N, ref, dtype):
    assert not torch.isnan(ds[..., :N]).any(), 'ds_out: unwritten columns < N'
    _check(path, dtn, case, 'dbias', ds[..., :N].double().sum(0), ref['dbias'], oa.budget(ref, 'dbias', dtype))


BIAS_PARAMS = [(dtn, c, r) for dtn in DTYPES for c in BIAS_CASES for r in ('peaked', 'flat')]


@pytest.mark.parametrize('dtn,case,regime', BIAS_PARAMS, ids=['%s-B%d-N%d-H%d-%s' % ((d,) + c + (r,)) for d, c, r in BIAS_PARAMS])
def test_bias_attention_fp64(dtn, case, regime):
    from vitadapter import kernels
    dtype = DTYPES[dtn]
    B, N, H = case
    qkv, dout = _inputs(B, N, H, regime, N * 17 + H, dtype)
    bias = torch.randn((H, N, N), generator=torch.Generator().manual_seed(N + 5)).cuda()
    bl, blt, ldb = _bias_ops(bias, N, dtype)
    out, lse, dqkv, ds = _seq_direct(qkv, dout, (bl, blt, ldb))
    tag = '%s/N%d/%s' % (case, N, regime)
    ref = oa.reference(*_operands(qkv, dout), SCALE, bl[:, :, :N].double() / oa.LOG2E)
    _check_seq('bias', dtn, tag, out, lse, dqkv, ref, dtype)
    _check_bias_grad('bias', dtn, tag, ds, N, ref, dtype)
    del ref
    out2, lse2, dqkv2, ds2 = _seq_direct(qkv, dout, (bl, blt, ldb))
    _same(out, out2, 'repeat out')
    _same(lse, lse2, 'repeat lse')
    _same(dqkv, dqkv2, 'repeat dqkv')
    _same(ds[..., :N], ds2[..., :N], 'repeat ds_out')
    x = qkv.clone().requires_grad_(True)
    bleaf = bias.clone().requires_grad_(True)
    o3 = kernels.attention_bias(x, bleaf, SCALE)
    assert o3 is not None
    o3.backward(dout)
    _same(out, o3.detach(), 'kernels.attention_bias out')
    _same(dqkv, x.grad, 'kernels.attention_bias grad')
    _same(ds[..., :N].float().sum(0), bleaf.grad, 'kernels.attention_bias bias grad')


# ------------------------------------------------------------------------------------------------ relative position bias
def _relpos_index(hw, windowed):
    if windowed:
        from vitadapter.backbones.beit_det import window_relative_position_index
        assert hw[0] == hw[1]
        return window_relative_position_index(hw[0]), (2 * hw[0] - 1) ** 2
    from vitadapter.backbones.beit import relative_position_index
    return relative_position_index(hw)


def _relpos_grad(ds, index, B, H, N, ldb, T_):
    lib = _vah().lib
    dtable = _nan((T_, H))
    ws = _nan((lib.vah_relpos_bias_grad_ws_floats(T_, H),))
    _call('vah_relpos_bias_grad', ds.dtype, ds.data_ptr(), index.data_ptr(), B, H, N, ldb, T_, ws.data_ptr(),
          dtable.data_ptr(), _stream())
    torch.cuda.synchronize()
    return dtable


def _fp32_order_bound(ds, index, N, T_):
    """Two fp32 sums of the same n terms in any two orders differ by at most 2 n 2^-24 sum |terms|: per table entry."""
    a = ds[..., :N].double().abs().sum(0)                                        # (H, N, N)
    cnt = torch.bincount(index.reshape(-1), minlength=T_).double() * ds.shape[0]  # terms per entry, over the batch
    return 2 * 2.0 ** -24 * cnt[:, None] * oa.scatter_table(a, index, T_)


RELPOS_PARAMS = [(dtn, c, r) for dtn in DTYPES for c in RELPOS_CASES for r in ('peaked', 'flat')]


@pytest.mark.parametrize('dtn,case,regime', RELPOS_PARAMS,
                         ids=['%s-B%d-%dx%d-H%d-%s-%s' % (d, c[0], c[1][0], c[1][1], c[2], 'win' if c[3] else 'cls', r)
                              for d, c, r in RELPOS_PARAMS])
def test_relpos_attention_fp64(dtn, case, regime):
    from vitadapter import kernels
    dtype = DTYPES[dtn]
    B, hw, H, windowed = case
    index, T_ = _relpos_index(hw, windowed)
    N = index.shape[0]
    index = index.cuda().contiguous()
    ldb = (N + 63) // 64 * 64
    qkv, dout = _inputs(B, N, H, regime, N * 13 + H, dtype)
    table = (torch.randn((T_, H), generator=torch.Generator().manual_seed(T_)) * 1.5).cuda()

    # build: bit-exact against one rounding of table * log2(e); zeros beyond N
    bl, blt = _nan((H, N, ldb), dtype), _nan((H, N, ldb), dtype)
    _call('vah_relpos_bias_build', dtype, table.data_ptr(), index.data_ptr(), T_, H, N, ldb, bl.data_ptr(), blt.data_ptr(),
          _stream())
    torch.cuda.synchronize()
    want = (table[index.reshape(-1)].reshape(N, N, H).permute(2, 0, 1) * 1.4426950408889634).to(dtype)
    _same(bl[:, :, :N], want, 'relpos bias')
    _same(blt[:, :, :N], want.transpose(1, 2), 'relpos bias_t')
    assert (bl[:, :, N:] == 0).all() and (blt[:, :, N:] == 0).all(), 'relpos build: padding columns not zero'

    out, lse, dqkv, ds = _seq_direct(qkv, dout, (bl, blt, ldb))
    tag = '%s/N%d/%s' % (case, N, regime)
    ref = oa.reference(*_operands(qkv, dout), SCALE, bl[:, :, :N].double() / oa.LOG2E)
    _check_seq('relpos', dtn, tag, out, lse, dqkv, ref, dtype)
    _check_bias_grad('relpos', dtn, tag, ds, N, ref, dtype)
    dtable = _relpos_grad(ds, index, B, H, N, ldb, T_)
    _check('relpos', dtn, tag, 'dtable', dtable, oa.scatter_table(ref['dbias'], index, T_),
           oa.scatter_table(oa.budget(ref, 'dbias', dtype), index, T_))
    del ref
    bound = _fp32_order_bound(ds, index, N, T_)
    dtable2 = _relpos_grad(ds, index, B, H, N, ldb, T_)
    assert ((dtable2.double() - dtable.double()).abs() <= bound).all(), 'relpos grad: repeat beyond fp32 rounding'

    x = qkv.clone().requires_grad_(True)
    tleaf = table.clone().requires_grad_(True)
    o3 = kernels.attention_relpos(x, tleaf, index, SCALE)
    assert o3 is not None
    o3.backward(dout)
    _same(out, o3.detach(), 'kernels.attention_relpos out')
    _same(dqkv, x.grad, 'kernels.attention_relpos grad')
    assert ((tleaf.grad.double() - dtable.double()).abs() <= bound).all(), 'kernels.attention_relpos table grad'


# ------------------------------------------------------------------------------------------------ windows
def _win_index(B, gh, gw, win):
    """(Z, win * win) row of each window token in the (B * gh * gw) token order, -1 for padded-grid tokens; windows in
    the kernels' order z = (b, wy, wx)."""
    nwy, nwx = -(-gh // win), -(-gw // win)
    ar = lambda n: torch.arange(n, device='cuda')                                          # noqa: E731
    b = ar(B).view(B, 1, 1, 1, 1)
    y = (ar(nwy) * win).view(1, nwy, 1, 1, 1) + ar(win).view(1, 1, 1, win, 1)
    x = (ar(nwx) * win).view(1, 1, nwx, 1, 1) + ar(win).view(1, 1, 1, 1, win)
    idx = torch.where((y < gh) & (x < gw), (b * gh + y) * gw + x, torch.full_like(b * y * x, -1))
    return idx.reshape(B * nwy * nwx, win * win)


def _win_direct(qkv, dout, gh, gw, win):
    B, N, _, H, _ = qkv.shape
    T, C = qkv.dtype, H * 64
    lib = _vah().lib
    Nw = win * win
    Z = B * (-(-gh // win)) * (-(-gw // win))
    q, k, v = _ptrs(qkv)
    out, lse = _nan((B, N, H, 64), T), _nan((Z, H, Nw))
    vt = _nan((Z * H * 64 * lib.vah_attn_padded_len(Nw),), T) if Nw > RESIDENT_MAX else None
    _call('vah_attn_win_fwd_bf16', T, q, k, v, 3 * C, B, gh, gw, win, H, SCALE, vt.data_ptr() if vt is not None else 0,
          out.data_ptr(), C, lse.data_ptr(), _stream())
    dqkv = _nan(tuple(qkv.shape), T)
    dq, dk, dv = _ptrs(dqkv)
    ws = _nan_bytes(lib.vah_attn_bwd_workspace_bytes(Z, H, Nw)) if Nw > RESIDENT_MAX else None
    _call('vah_attn_win_bwd_bf16', T, q, k, v, 3 * C, out.data_ptr(), dout.data_ptr(), C, lse.data_ptr(), B, gh, gw, win,
          H, SCALE, ws.data_ptr() if ws is not None else 0, dq, dk, dv, 3 * C, _stream())
    torch.cuda.synchronize()
    return out, lse, dqkv


WIN_PARAMS = [(dtn, c, r) for dtn in DTYPES for c in WIN_CASES for r in ('peaked', 'flat')]


def test_window_cases_cover_every_resident_nb_and_the_general_path():
    """The profiler has one row for all NB: coverage of the 7 resident instantiations is asserted over the case list."""
    for dtn in DTYPES:
        wins = [c[4] for d, c, _ in WIN_PARAMS if d == dtn]
        assert {-(-w * w // 32) for w in wins if w * w <= RESIDENT_MAX} == set(range(1, 8)), dtn
        assert {w * w for w in wins if w * w > RESIDENT_MAX} >= {225, 256}, dtn
        assert any(w * w <= RESIDENT_MAX and (gh % w and gw % w) for _, gh, gw, _, w in
                   [c for d, c, _ in WIN_PARAMS if d == dtn] if w > 1)


@pytest.mark.parametrize('dtn,case,regime', WIN_PARAMS,
                         ids=['%s-B%d-%dx%d-H%d-win%d-%s' % ((d,) + c + (r,)) for d, c, r in WIN_PARAMS])
def test_window_attention_fp64(dtn, case, regime):
    from vitadapter import kernels
    dtype = DTYPES[dtn]
    B, gh, gw, H, win = case
    N = gh * gw
    path = 'win_res' if win * win <= RESIDENT_MAX else 'win_gen'
    tag = '%dx%d/win%d/%s' % (gh, gw, win, regime)
    qkv, dout = _inputs(B, N, H, regime, N * 7 + win, dtype)
    out, lse, dqkv = _win_direct(qkv, dout, gh, gw, win)

    idx = _win_index(B, gh, gw, win)
    valid = idx >= 0
    gat = lambda t: torch.where(valid[..., None, None], t.reshape(B * N, H, 64)[idx.clamp_min(0)], 0).to(dtype)  # noqa: E731
    qw = gat(qkv[:, :, 0]), gat(qkv[:, :, 1]), gat(qkv[:, :, 2]), gat(dout)          # (Z, Nw, H, 64), zero padding rows
    ref = oa.reference(*(t.transpose(1, 2) for t in qw), SCALE)
    rows = idx[valid]                                                               # each real token exactly once
    assert rows.numel() == B * N and torch.equal(rows.sort().values, torch.arange(B * N, device='cuda'))

    def real(t):
        return t.transpose(1, 2)[valid]                                             # (B * N, H, 64) in window order

    _check(path, dtn, tag, 'o', out.reshape(B * N, H, 64)[rows], real(ref['o']), real(oa.budget(ref, 'o', dtype)))
    _check(path, dtn, tag, 'lse', lse.transpose(1, 2)[valid], ref['lse'].transpose(1, 2)[valid],
           oa.budget(ref, 'lse', dtype).transpose(1, 2)[valid])
    pad_lse = lse.transpose(1, 2)[~valid]
    assert (pad_lse == math.inf).all(), 'window lse of padded-grid queries must be +inf'
    for i, n in enumerate(('dq', 'dk', 'dv')):
        _check(path, dtn, tag, n, dqkv[:, :, i].reshape(B * N, H, 64)[rows], real(ref[n]), real(oa.budget(ref, n, dtype)))
    del ref
    out2, lse2, dqkv2 = _win_direct(qkv, dout, gh, gw, win)
    _same(out, out2, 'repeat out')
    _same(lse, lse2, 'repeat lse')
    _same(dqkv, dqkv2, 'repeat dqkv')
    x = qkv.clone().requires_grad_(True)
    o3 = kernels.window_attention(x, SCALE, gh, gw, win)
    assert o3 is not None
    o3.backward(dout)
    _same(out, o3.detach(), 'kernels.window_attention out')
    _same(dqkv, x.grad, 'kernels.window_attention grad')
