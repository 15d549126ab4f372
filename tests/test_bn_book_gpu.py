"""GPU: vah_bn_finalize_stats_book (csrc/tail_ops.hip, include/vitadapter_hip_epoch.h) against vah_bn_finalize_stats.

At C = 8, 64 (one partial workgroup) and 100 (not a multiple of the wave) mean, rstd and the running statistics must be
bit-equal to the entry point without bookkeeping run on the same sums with the count filled in by torch; sums[2 * C]
must then hold the count, num_batches_tracked must have advanced by one, and null pointers for the counter and for the
running statistics are accepted.  The glue (fused.bn_finalize) is held to the same through a BatchNorm module."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1


def _sums(C, count, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(count, C, generator=g) * 3 + torch.randn(C, generator=g)
    s = torch.cat([x.sum(0), (x * x).sum(0), torch.full((1,), float('nan'))]).cuda()
    if C > 8:
        s[3], s[C + 3] = float('inf'), float('inf')          # a channel that saw an inf: NaN variance, as torch's
    return s


def _plain(sums, C, count, rm, rv):
    import _vah
    sums = sums.clone()
    sums[2 * C:].fill_(float(count))
    mean, rstd = torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
    _vah.check(_vah.lib.vah_bn_finalize_stats(sums.data_ptr(), C, EPS, MOM, rm.data_ptr() if rm is not None else None,
                                              rv.data_ptr() if rv is not None else None, mean.data_ptr(), rstd.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), 'bn_finalize_stats')
    return mean, rstd


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('C', [8, 64, 100])
def test_book_equals_finalize_and_keeps_the_books(C):
    import _vah
    count = 37 * C + 5
    sums = _sums(C, 50, C)
    rm0, rv0 = torch.randn(C, device='cuda'), torch.rand(C, device='cuda') + 0.5
    rm_a, rv_a, rm_b, rv_b = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    mean_a, rstd_a = _plain(sums, C, count, rm_a, rv_a)
    mean_b, rstd_b = torch.full((C,), float('nan'), device='cuda'), torch.full((C,), float('nan'), device='cuda')
    nbt = torch.tensor(41, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    _vah.check(_vah.lib.vah_bn_finalize_stats_book(sums.data_ptr(), C, float(count), EPS, MOM, rm_b.data_ptr(), rv_b.data_ptr(),
                                                   mean_b.data_ptr(), rstd_b.data_ptr(), nbt.data_ptr(), st), 'book')
    torch.cuda.synchronize()
    assert _same(mean_a, mean_b) and _same(rstd_a, rstd_b) and _same(rm_a, rm_b) and _same(rv_a, rv_b)
    assert float(sums[2 * C]) == float(count) and int(nbt) == 42
    if C > 8:
        assert bool(torch.isnan(rstd_b[3])) and bool(torch.isfinite(rstd_b[4]))
    # null counter, null running statistics
    sums2 = _sums(C, 50, C)
    mean_c, rstd_c = torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
    _vah.check(_vah.lib.vah_bn_finalize_stats_book(sums2.data_ptr(), C, float(count), EPS, MOM, None, None, mean_c.data_ptr(),
                                                   rstd_c.data_ptr(), None, st), 'book without tracking')
    torch.cuda.synchronize()
    assert _same(mean_c, mean_a) and _same(rstd_c, rstd_a) and float(sums2[2 * C]) == float(count)


@pytest.mark.parametrize('track', [True, False])
def test_glue_one_launch_equals_the_separate_steps(track):
    from vitadapter import fused
    C, count = 100, 4100
    outs = []
    for on in (False, True):
        norm = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOM, track_running_stats=track).cuda()
        sums = _sums(C, 50, 7)
        old = fused.ENABLED['epoch_copies']
        fused.ENABLED['epoch_copies'] = on
        try:
            mean, rstd, cnt = fused.bn_finalize(norm, sums, C, count, None, torch.cuda.current_stream().cuda_stream)
        finally:
            fused.ENABLED['epoch_copies'] = old
        torch.cuda.synchronize()
        assert cnt.shape == (1,) and float(cnt) == float(count) and cnt.data_ptr() == sums[2 * C:].data_ptr()
        if track:
            assert int(norm.num_batches_tracked) == 1
        outs.append((mean, rstd) + ((norm.running_mean, norm.running_var) if track else ()))
    for a, b in zip(*outs):
        assert _same(a, b)
