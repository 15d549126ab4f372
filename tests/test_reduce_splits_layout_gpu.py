"""GPU: reduce_splits (csrc/gemm.hip) over the output layouts it stores to.

One weight-gradient product of the committed table, 768 x 256 x 8192 at split 4, runs through vah_gemm_bf16_fin
three times: with ldd = N (D is one flat array), ldd = N + 4 (rows stay 16-byte aligned: one vector store per float4
position) and ldd = N + 2 (rows are not: four scalar stores).  The split slices' hipBLASLt problem does not depend on
ldd, so the table text loaded here copies the committed row's algorithm index and split for the other two ldd values:
nothing is tuned live, and gemm_table_dump must show that index and split after the calls.

Every element of D is held to fp64 with the budget of tests/test_reductions_fullsize_gpu.py (64 * 2^-24 * |g|^T |x|),
the padding columns between N and ldd must keep their NaN fill, the bias gradient of the finalize job riding on the
launch is held to fp64 too, and the three results must agree bit for bit in the N columns: the sum over the slices is
one chain in slice order whatever the store path."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

C_ACC = 64
U = 2.0 ** -24
NAN = float('nan')
M, N, K = 768, 256, 8192
PADS = (0, 4, 2)

TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'vit-adapter_amd', 'tuning',
                     'gemm_table_mi355x_base_det_1024.txt')


def _committed_row():
    """(version line, fields) of the committed 768 x 256 x 8192 weight-gradient row."""
    key = ['1', '0', '1', '0', '0', str(M), str(N), str(K), str(M), str(N), str(N)]
    with open(TABLE) as f:
        lines = f.read().splitlines()
    rows = [ln.split() for ln in lines[1:] if ln.split()[:11] == key]
    assert lines[0].startswith('#hipblaslt') and len(rows) == 1, 'the committed table has no single %dx%dx%d row' % (M, N, K)
    return lines[0], rows[0]


def _entry(ldd):
    import _vah
    key = '1 0 1 0 0 %d %d %d %d %d %d ' % (M, N, K, M, N, ldd)
    lines = [ln for ln in _vah.gemm_table_dump().splitlines() if ln.startswith(key)]
    return (int(lines[0].split()[11]), int(lines[0].split()[12])) if lines else None


def _within(got, ref, A, what):
    err = (got.double() - ref).abs()
    bound = C_ACC * U * A
    bad = ~(err <= bound)                                   # a NaN (an element never written) fails
    assert not bool(bad.any()), '%s: %d of %d elements over budget (worst err / budget %.3g)' % (
        what, int(bad.sum()), got.numel(), (err / bound.clamp_min(1e-300)).nan_to_num(float('inf')).max().item())


def test_reduce_splits_store_layouts():
    from vitadapter import fused
    import _vah
    version, row = _committed_row()
    index, split = int(row[11]), int(row[12])
    assert split == 4, 'the committed row is expected at split 4 (the table changed: pick another split-4 row)'
    text = version + '\n' + ''.join(' '.join(row[:10] + [str(N + pad)] + row[11:]) + '\n' for pad in PADS)
    if _vah.gemm_table_load(text) != len(PADS):
        pytest.skip('the committed table is of another hipBLASLt build: its algorithm indices mean nothing here')

    torch.manual_seed(4100)
    g2 = torch.randn(K, M, device='cuda').to(torch.bfloat16)
    x2 = torch.randn(K, N, device='cuda').to(torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    rejected0 = _vah.lib.vah_gemm_rejected_candidates()
    ws_bytes = fused._GEMM_WS_BYTES + min(64 * M * N * 4, 160 << 20)
    results = []
    for pad in PADS:
        ldd = N + pad
        D = torch.full((M, ldd), NAN, device='cuda')
        gb = torch.full((M,), NAN, device='cuda')
        cws = torch.full((_vah.lib.vah_reduce_ws_floats(M),), NAN, device='cuda')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
        ws[:split * M * N * 4].view(torch.float32).fill_(NAN)
        nparts = ctypes.c_int64(0)
        _vah.check(_vah.lib.vah_colsum_bf16_partials(g2.data_ptr(), K, M, cws.data_ptr(), ctypes.byref(nparts), st),
                   'colsum_partials')
        _vah.check(_vah.lib.vah_gemm_bf16_fin(1, 0, M, N, K, g2.data_ptr(), M, x2.data_ptr(), N, D.data_ptr(), ldd, 1,
                                              ws.data_ptr(), ws_bytes, cws.data_ptr(), nparts.value, M, gb.data_ptr(), st),
                   'gemm_bf16_fin ldd %d' % ldd)
        torch.cuda.synchronize()
        if _entry(ldd) != (index, split):
            pytest.skip('ldd %d: index %d / split %d of the committed row did not resolve on this hipBLASLt (ran %r)'
                        % (ldd, index, split, _entry(ldd)))
        results.append((ldd, D, gb))
    assert _vah.lib.vah_gemm_rejected_candidates() == rejected0, 'candidates were rejected during the calls: something was tuned live'

    gd, xd = g2.double(), x2.double()
    ref, A = gd.t() @ xd, gd.abs().t() @ xd.abs()
    rb, Ab = gd.sum(0), gd.abs().sum(0)
    for ldd, D, gb in results:
        _within(D[:, :N], ref, A, 'dW at ldd %d' % ldd)
        _within(gb, rb, Ab, 'db at ldd %d' % ldd)
        assert bool(torch.isnan(D[:, N:]).all()), 'ldd %d: a padding column was written' % ldd
    for ldd, D, gb in results[1:]:
        assert torch.equal(D[:, :N], results[0][1]), 'dW at ldd %d differs from dW at ldd %d' % (ldd, N)
        assert torch.equal(gb, results[0][2]), 'db at ldd %d differs from db at ldd %d' % (ldd, N)
