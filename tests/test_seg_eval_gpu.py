"""GPU: the counting kernels of the mIoU evaluation (csrc/seg_eval.hip) against tests/seg_eval_ref.py.  Counts are integers:
every comparison is exact.

Shapes are the smallest at which the kernel takes another path: one pixel; less than a wave; two images with row and image
strides larger than the extents; a shape of at least three workgroups with a partial last one (derived from
vah_segeval_ws_bytes); a uint8 view that starts at column 1 with an odd width, so label addresses are odd and the 16-byte
loads of pred alternate with the 8-byte path from row to row.  C covers one class, the per-wave histograms (3 * C <= 1024) and
the shared one (171 is still per-wave, 4096 is not and is the largest).  The maps are blobs with single-pixel noise, with
predictions of -1, -2^40, C, C + 1 and 2^40 and labels in [C, 255) among the valid ones."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_eval_ref as ref  # noqa: E402

from vitadapter import SegEvaluator, evaluation, fused  # noqa: E402

pytestmark = pytest.mark.gpu
_vah = fused._vah
lib = _vah.lib

CLASSES = (1, 2, 19, 150, 171, 4096)
BIG = (1, 97, 107)              # 10379 pixels: three workgroups of 4096, the last one partial
SHAPES = {'one': (1, 1, 1), 'small': (1, 7, 13), 'strided': (2, 61, 67), 'big': BIG, 'column1': (2, 30, 37)}
_CACHE = {}


def dev():
    return torch.device('cuda:0')


def maps(shape, C, seed=0):
    """(pred int64, label uint8-range int64) numpy arrays, built once per (shape, C, seed)"""
    key = (shape, C, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * seed + C + shape[1])
        label = ref.blobs(rng, shape, min(C, 255), cell=5)
        pred = label.copy()
        noise = rng.random(shape)
        pred[noise < 0.15] = rng.integers(0, C, size=shape)[noise < 0.15]
        for i, v in enumerate((-1, -(1 << 40), C, C + 1, 1 << 40)):
            pred[(noise >= 0.15 + 0.01 * i) & (noise < 0.16 + 0.01 * i)] = v
        if C < 254:
            label[(noise >= 0.5) & (noise < 0.53)] = rng.integers(C, 255, size=shape)[(noise >= 0.5) & (noise < 0.53)]
        label[noise > 0.95] = 255
        _CACHE[key] = (pred, label)
    return _CACHE[key]


def place(a, name, dtype):
    """the array on the device in the layout of the named shape"""
    t = torch.from_numpy(a).to(dtype)
    N, H, W = t.shape
    if name == 'strided':
        buf = torch.full((N, H + 3, W + 5), 77, dtype=dtype)
        buf[:, :H, :W] = t
        return buf.to(dev())[:, :H, :W]
    if name == 'column1':
        buf = torch.full((N, H, W + 3), 77, dtype=dtype)
        buf[:, :, 1:W + 1] = t
        return buf.to(dev())[:, :, 1:W + 1]
    return t.to(dev())


def count(pred, label, C, **kw):
    totals = torch.zeros((3, C), dtype=torch.int64, device=dev())
    fused.seg_eval_update(pred, label, totals, C, **kw)
    return totals.cpu().numpy()


def test_the_shapes_are_what_the_docstring_says():
    C = 19
    rows = lib.vah_segeval_ws_bytes(*BIG, C) // (3 * C * 4)
    total = BIG[0] * BIG[1] * BIG[2]
    assert rows >= 3 and rows == -(-total // 4096) and total % 4096 != 0
    assert lib.vah_segeval_ws_bytes(1, 7, 13, C) == 3 * C * 4


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int64], ids=['u8', 'i64'])
@pytest.mark.parametrize('C', CLASSES)
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_counts_equal_the_reference(name, C, dtype):
    assert fused.ENABLED['seg_eval']
    pred, label = maps(SHAPES[name], C)
    p, g = place(pred, name, torch.int64), place(label, name, dtype)
    if name == 'column1' and dtype == torch.uint8:
        assert g.data_ptr() % 2 == 1 and g.stride(1) == SHAPES[name][2] + 3
    if name == 'strided':
        assert p.stride(1) > p.shape[2] and p.stride(0) > p.shape[1] * p.stride(1) - 1
    _vah.prof_enable(True, 'seg_eval')
    got = count(p, g, C)
    rows = _vah.prof_report()
    _vah.prof_enable(False)
    assert rows['seg_eval_count']['calls'] == 1 and rows['seg_eval_merge']['calls'] == 1, rows
    assert np.array_equal(got, ref.counts(pred, label, C))


@pytest.mark.parametrize('C', [19, 150])
@pytest.mark.parametrize('kw', [dict(ignore_index=255), dict(ignore_index=0), dict(ignore_index=-1), dict(reduce_zero_label=True),
                                dict(reduce_zero_label=True, ignore_index=7), dict(label_map={0: 3, 3: 1, 1: 255, 200: 0, 255: 2}),
                                dict(label_map={0: 3, 3: 1, 1: 255, 200: 0}, reduce_zero_label=True)],
                         ids=['ig255', 'ig0', 'ig-1', 'rz', 'rz-ig7', 'map', 'map-rz'])
def test_flags(C, kw):
    pred, label = maps(SHAPES['strided'], C)
    if kw.get('ignore_index') == -1:                 # int64 labels with negative values, some of them the ignore index
        label = label.copy()
        label[::2, ::3, ::5] = -1
        label[1::2, ::3, 1::5] = -7
        g = place(label, 'strided', torch.int64)
    else:
        g = place(label, 'strided', torch.uint8)
    got = count(place(pred, 'strided', torch.int64), g, C, **kw)
    assert np.array_equal(got, ref.counts(pred, label, C, **kw))
    if 'label_map' not in kw:
        assert np.array_equal(got, ref.counts_loop(pred[:1, :9], label[:1, :9], C, **kw)
                              + ref.counts(pred[:1, 9:], label[:1, 9:], C, **kw) + ref.counts(pred[1:], label[1:], C, **kw))


@pytest.mark.parametrize('run', [1, 2, 3, 63, 64, 65, 127, 128, 129, 256, 300, 512, 513])
def test_runs_that_end_at_lane_wave_step_and_row_boundaries(run):
    # a row is 256 pixels: half a workgroup step of 512, two wave steps of 128, 128 lane pairs.  Runs of `run` pixels in
    # pixel order end at (run 1, 2, 3) pixel, lane and odd boundaries, at (64, 128) the boundaries of a wave's even / odd
    # sequences and of its step, at 256 the row end, at 512 the workgroup step, and next to each of them
    C, shape = 19, (1, 40, 256)
    idx = np.arange(shape[1] * shape[2]).reshape(shape)
    label = (idx // run) % C
    pred = ((idx + 1) // run * 7) % C                 # its runs end one pixel before the label's
    got = count(torch.from_numpy(pred).to(dev()), torch.from_numpy(label).to(torch.uint8).to(dev()), C)
    assert np.array_equal(got, ref.counts(pred, label, C))


def test_patterns():
    C, shape = 19, (2, 61, 67)
    yy, xx = np.meshgrid(np.arange(shape[1]), np.arange(shape[2]), indexing='ij')
    checker = np.broadcast_to(((yy + xx) % 2) * 4 + 3, shape).astype(np.int64)          # classes 3 and 7
    const = np.full(shape, 5, dtype=np.int64)
    ignored = np.full(shape, 255, dtype=np.int64)
    half = const.copy()
    half[0] = 255                                    # an all-ignored image next to a counted one
    for pred, label in ((const, const), (const, checker), (checker, checker), (checker, const), (const, ignored), (checker, half)):
        got = count(torch.from_numpy(pred).to(dev()), torch.from_numpy(label).to(torch.uint8).to(dev()), C)
        assert np.array_equal(got, ref.counts(pred, label, C))
    assert count(torch.from_numpy(const).to(dev()), torch.from_numpy(ignored).to(torch.uint8).to(dev()), C).sum() == 0
    one = count(torch.from_numpy(const).to(dev()), torch.from_numpy(const).to(dev()), C)
    assert one[:, 5].tolist() == [const.size] * 3 and one.sum() == 3 * const.size


def test_totals_are_added_to_and_keep_their_upper_bits():
    C = 150
    pred, label = maps(BIG, C)
    p, g = torch.from_numpy(pred).to(dev()), torch.from_numpy(label).to(torch.uint8).to(dev())
    totals = torch.full((3, C), 1 << 40, dtype=torch.int64, device=dev())
    totals[1] += 5
    fused.seg_eval_update(p, g, totals, C)
    fused.seg_eval_update(p, g, totals, C)              # two calls add
    want = 2 * ref.counts(pred, label, C) + (1 << 40)
    want[1] += 5
    assert np.array_equal(totals.cpu().numpy(), want)


def test_the_call_captures_into_a_graph():
    C = 19
    pred, label = maps(BIG, C)
    p, g = torch.from_numpy(pred).to(dev()), torch.from_numpy(label).to(torch.uint8).to(dev())
    totals = torch.zeros((3, C), dtype=torch.int64, device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused.seg_eval_update(p, g, totals, C)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused.seg_eval_update(p, g, totals, C)           # captured, not run
    torch.cuda.synchronize()
    one = ref.counts(pred, label, C)
    assert np.array_equal(totals.cpu().numpy(), one)
    for k in (2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(totals.cpu().numpy(), k * one)


@pytest.mark.parametrize('C', [19, 4096])
def test_nothing_outside_ws_and_totals_is_written(C):
    pred, label = maps(BIG, C)
    N, H, W = BIG
    p, g = torch.from_numpy(pred).to(dev()), torch.from_numpy(label).to(torch.uint8).to(dev())
    nbytes = lib.vah_segeval_ws_bytes(N, H, W, C)
    guard = 4096
    ws = torch.full((guard + nbytes + guard,), 0xA5, dtype=torch.uint8, device=dev())
    tot = torch.full((512 + 3 * C + 512,), -6148914691236517206, dtype=torch.int64, device=dev())
    tot[512:512 + 3 * C] = 0
    assert (ws.data_ptr() + guard) % 16 == 0
    with _vah.on(dev()):
        _vah.check(lib.vah_segeval_update(p.data_ptr(), H * W, W, g.data_ptr(), 1, H * W, W, N, H, W, C, 255, 0, None, 0,
                                          tot.data_ptr() + 512 * 8, ws.data_ptr() + guard, nbytes, _vah.raw_stream(dev())),
                   'vah_segeval_update')
    torch.cuda.synchronize()
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[guard + nbytes:] == 0xA5).all())
    assert bool((tot[:512] == -6148914691236517206).all()) and bool((tot[512 + 3 * C:] == -6148914691236517206).all())
    assert np.array_equal(tot[512:512 + 3 * C].reshape(3, C).cpu().numpy(), ref.counts(pred, label, C))
    # every byte of the workspace the call asked for is a partial count: the rows add up to the totals
    rows = ws[guard:guard + nbytes].view(torch.int32).reshape(-1, 3 * C).to(torch.int64).sum(0)
    assert torch.equal(rows, tot[512:512 + 3 * C])


def test_switch_off_other_dtypes_and_the_evaluator():
    C = 150
    pred, label = maps(SHAPES['strided'], C)
    p, g = place(pred, 'strided', torch.int64), place(label, 'strided', torch.uint8)
    kw = dict(reduce_zero_label=True, label_map={4: 9})
    want = ref.counts(pred, label, C, **kw)
    keep = fused.ENABLED['seg_eval']
    try:
        fused.ENABLED['seg_eval'] = False
        assert np.array_equal(count(p, g, C, **kw), want)
    finally:
        fused.ENABLED['seg_eval'] = keep
    assert np.array_equal(count(p, g.int(), C, **kw), want)                     # int32 labels: the torch expression
    small = np.clip(pred, -5, 1000)                                             # int32 predictions: +-2^40 do not fit
    assert np.array_equal(count(place(small, 'strided', torch.int32), g, C, **kw), ref.counts(small, label, C, **kw))
    assert np.array_equal(count(p, g, C, label_map={4: 9, 300: 1}, reduce_zero_label=True), want)   # a key the table cannot hold
    ev = SegEvaluator(C, **kw)
    ev.update(p[:1], g[:1])
    ev.update(p[1], g[1:][:, None])
    ev.update(pred[:0], label[:0])                                              # an empty batch
    assert ev.totals.is_cuda and np.array_equal(ev.totals.cpu().numpy(), want)
    m = ev.compute(('mIoU', 'mDice'))
    r = ref.metrics(want, ('mIoU', 'mDice'))
    for k in r:
        assert np.array_equal(np.isnan(m[k]), np.isnan(r[k])) and np.allclose(m[k], r[k], rtol=1e-12, atol=0, equal_nan=True)
    areas = evaluation.intersect_and_union(p[0], g[0], C, 255, {4: 9}, True)
    one = ref.counts(pred[0], label[0], C, **kw)
    assert areas[0].is_cuda and areas[0].dtype == torch.int64
    assert np.array_equal(torch.stack([areas[0], areas[2], areas[3]]).cpu().numpy(), one)
    assert np.array_equal(areas[1].cpu().numpy(), one[1] + one[2] - one[0])
