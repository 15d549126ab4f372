"""GPU: the row map on the reduction launch of the weight-gradient GEMM (csrc/gemm.hip reduce_splits_mapped,
vah_gemm_bf16_fin_rowmap of include/vitadapter_hip_epoch.h).

The committed table row 432 x 768 x 8192 at split 4 - the pair-core product of the three-level MSDeformAttn modules at
base_det - is resolved the way tests/test_reduce_splits_layout_gpu.py resolves its row: only that row is loaded, nothing is
tuned live, and gemm_table_dump must show its index and split after the calls.  With the head-interleaved permutation
of such a module as the map, dW and db must be bit-equal to index_select (by the inverse permutation) of the unmapped
call's results - the loads and the slice-order add chain do not know about the map - with output and workspace
NaN-filled beforehand, and two mapped calls must agree bit for bit.  A product the dispatcher runs with split 1 (K = 64:
no reduction launch to carry the map) reports "not applied" and leaves dW and db as the unmapped call does."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float('nan')
M, N, K = 432, 768, 8192
HEADS = 12

TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'vit-adapter_amd', 'tuning',
                     'gemm_table_mi355x_base_det_1024.txt')


def _committed_row():
    key = ['1', '0', '1', '0', '0', str(M), str(N), str(K), str(M), str(N), str(N)]
    with open(TABLE) as f:
        lines = f.read().splitlines()
    rows = [ln.split() for ln in lines[1:] if ln.split()[:11] == key]
    assert lines[0].startswith('#hipblaslt') and len(rows) == 1, 'the committed table has no single %dx%dx%d row' % (M, N, K)
    return lines[0], rows[0]


def _entry(m, n, k):
    import _vah
    key = '1 0 1 0 0 %d %d %d %d %d %d ' % (m, n, k, m, n, n)
    lines = [ln for ln in _vah.gemm_table_dump().splitlines() if ln.startswith(key)]
    return (int(lines[0].split()[11]), int(lines[0].split()[12])) if lines else None


def _perm(m, heads):
    """rows [offsets of head h | logits of head h]: the permutation fused._PairCoreCopies makes, and its inverse"""
    na = m * 2 // 3
    po, pl = na // heads, (m - na) // heads
    fw = torch.cat([torch.cat((torch.arange(h * po, (h + 1) * po), na + torch.arange(h * pl, (h + 1) * pl))) for h in range(heads)])
    inv = torch.empty_like(fw)
    inv[fw] = torch.arange(m)
    return fw.cuda(), inv.cuda()


def _run(g2, x2, row_map, split):
    """One call with every buffer poisoned -> (dW, db, applied); row_map None: vah_gemm_bf16_fin."""
    from vitadapter import fused
    import _vah
    k, m = g2.shape
    n = x2.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    ws_bytes = fused._GEMM_WS_BYTES + min(64 * m * n * 4, 160 << 20)
    D = torch.full((m, n), NAN, device='cuda')
    gb = torch.full((m,), NAN, device='cuda')
    cws = torch.full((_vah.lib.vah_reduce_ws_floats(m),), NAN, device='cuda')
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    ws[:split * m * n * 4].view(torch.float32).fill_(NAN)
    nparts = ctypes.c_int64(0)
    _vah.check(_vah.lib.vah_colsum_bf16_partials(g2.data_ptr(), k, m, cws.data_ptr(), ctypes.byref(nparts), st), 'colsum_partials')
    applied = ctypes.c_int(-1)
    if row_map is None:
        _vah.check(_vah.lib.vah_gemm_bf16_fin(1, 0, m, n, k, g2.data_ptr(), m, x2.data_ptr(), n, D.data_ptr(), n, 1, ws.data_ptr(),
                                              ws_bytes, cws.data_ptr(), nparts.value, m, gb.data_ptr(), st), 'gemm_bf16_fin')
    else:
        _vah.check(_vah.lib.vah_gemm_bf16_fin_rowmap(1, 0, m, n, k, g2.data_ptr(), m, x2.data_ptr(), n, D.data_ptr(), n, 1,
                                                     ws.data_ptr(), ws_bytes, cws.data_ptr(), nparts.value, m, gb.data_ptr(),
                                                     row_map.data_ptr(), ctypes.byref(applied), st), 'gemm_bf16_fin_rowmap')
    torch.cuda.synchronize()
    return D, gb, applied.value


def test_mapped_rows_equal_index_select_of_the_unmapped_result():
    from vitadapter import fused
    import _vah
    version, row = _committed_row()
    index, split = int(row[11]), int(row[12])
    assert split == 4, 'the committed row is expected at split 4 (the table changed: pick another split-4 row)'
    if _vah.gemm_table_load(version + '\n' + ' '.join(row) + '\n') != 1:
        pytest.skip('the committed table is of another hipBLASLt build: its algorithm indices mean nothing here')
    torch.manual_seed(4300)
    g2 = torch.randn(K, M, device='cuda').to(torch.bfloat16)
    x2 = torch.randn(K, N, device='cuda').to(torch.bfloat16)
    fw, inv = _perm(M, HEADS)
    row_map = fw.to(torch.int32)
    rejected0 = _vah.lib.vah_gemm_rejected_candidates()
    D0, b0, _ = _run(g2, x2, None, split)
    if _entry(M, N, K) != (index, split):
        pytest.skip('index %d / split %d of the committed row did not resolve on this hipBLASLt (ran %r)' % (index, split, _entry(M, N, K)))
    D1, b1, applied1 = _run(g2, x2, row_map, split)
    D2, b2, applied2 = _run(g2, x2, row_map, split)
    assert _vah.lib.vah_gemm_rejected_candidates() == rejected0 and _entry(M, N, K) == (index, split)
    assert applied1 == 1 and applied2 == 1
    assert not bool(torch.isnan(D0).any()) and not bool(torch.isnan(D1).any()) and not bool(torch.isnan(b1).any())
    assert torch.equal(D1, D0.index_select(0, inv)), 'mapped dW is not index_select of the unmapped dW'
    assert torch.equal(b1, b0.index_select(0, inv)), 'mapped db is not index_select of the unmapped db'
    assert torch.equal(D1, D2) and torch.equal(b1, b2), 'two mapped calls differ'
    assert not torch.equal(D1, D0), 'the permutation moved nothing: the case tests nothing'
    # the glue: _wgrad_bgrad_mapped is this call
    ew, eb, eapplied = fused._wgrad_bgrad_mapped(g2, x2, row_map)
    torch.cuda.synchronize()
    assert eapplied is True and torch.equal(ew, D1) and torch.equal(eb, b1)


def test_split_one_reports_not_applied_and_leaves_the_unmapped_result():
    import _vah
    m, n, k = 24, 16, 64                   # K < 4096: the dispatcher has no split candidates, hipBLASLt writes D itself
    torch.manual_seed(4301)
    g2 = torch.randn(k, m, device='cuda').to(torch.bfloat16)
    x2 = torch.randn(k, n, device='cuda').to(torch.bfloat16)
    fw, inv = _perm(m, 2)
    D0, b0, _ = _run(g2, x2, None, 1)
    D1, b1, applied = _run(g2, x2, fw.to(torch.int32), 1)
    assert _entry(m, n, k)[1] == 1
    assert applied == 0
    assert torch.equal(D1, D0) and torch.equal(b1, b0)
    assert not bool(torch.isnan(D1).any()) and not bool(torch.isnan(b1).any())
