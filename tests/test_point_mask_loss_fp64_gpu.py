"""GPU: the sampled-mask-loss kernels (csrc/point_mask_loss.hip) by direct C calls against the fp64 reference and the budgets of
tests/point_mask_loss_ref.py.  Every output is NaN-filled first and sits between guard elements; the workspace is filled with
0xFF bytes, so nothing is owed to what a buffer held.

Predictions 1 x 1, 2 x 3, 5 x 7, 32 x 48 (targets 11 x 9, uint8 and fp32, no multiple of any of them) with P in {1, 63, 64, 65,
257} plus the edge set, and one 160 x 160 case (K 3, P 12 544, targets 640 x 640 uint8) on the head's own mixture of points
(the lowest-|logit| three quarters of an oversample plus uniform ones); a row stride wider than the map; all P points in one
cell; all points outside the map; rows scrambled with unused maps in between, tgt_rows with a repeat, K = 0.  A pixel no tap
can reach is +0.0 with the sign bit clear; two calls give equal bits in every output; the K rows presented in reversed order
give the same bits per row; a non-finite prediction element makes non-finite what torch's fp64 expression makes non-finite.

A ratio is max |err| / budget; every one must be <= 1, and one above 0.5 means the budget is to be re-derived, not widened.
Worst ratios of a run on an MI355X (the RATIO lines; MEASURED repeats them):
    xs 0.206   ts 0.213   bce 0.032   dice 0.047   sums 0.050   dmaps 0.200
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _vah
import point_loss_ref as base
import point_mask_loss_ref as ref

pytestmark = pytest.mark.gpu

lib = _vah.lib
NAN = float('nan')
GUARD = 12345.0
NAMES = ('xs', 'ts', 'bce', 'dice', 'sums', 'dmaps')
# worst ratios over all cases, copied from the RATIO lines of a run on an MI355X
MEASURED = {
    'xs': '0.206 over all cases',
    'ts': '0.213 over all cases',
    'bce': '0.032 over all cases',
    'dice': '0.047 over all cases',
    'sums': '0.050 over all cases',
    'dmaps': '0.200 over all cases',
}
WORST = {}


def _dev():
    return torch.device('cuda:0')


def _note(name, r):
    WORST[name] = max(WORST.get(name, 0.0), r)
    print('RATIO %s %.3f (worst so far %.3f)' % (name, r, WORST[name]))
    assert r <= 1.0, (name, r)


def _guarded(shape):
    n = int(math.prod(shape))
    buf = torch.full((n + 16,), NAN, device=_dev())
    buf[:8] = GUARD
    buf[n + 8:] = GUARD
    return buf, buf[8:8 + n].view(shape)


def _idx(rows):
    return None if rows is None else torch.as_tensor(rows, dtype=torch.int32, device=_dev())


def _ptr(t):
    return t.data_ptr() if t is not None else None


def c_call(pred, tgt, points, rows, tgt_rows, g_bce, g_dice, eps=1.0):
    """pred: a DEVICE tensor (Mp, h, w) (possibly a strided view); the rest on the CPU.  -> dict of CPU outputs"""
    dev = _dev()
    t, p = tgt.to(dev), points.to(dev).contiguous()
    ri, ti = _idx(rows), _idx(tgt_rows)
    K, P, _ = p.shape
    Mp, h, w = pred.shape
    nbytes = lib.vah_pml_ws_bytes(K, P, h, w)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev)
    bufs = {name: _guarded(shape) for name, shape in (('bce', (K,)), ('dice', (K,)), ('xs', (K, P)), ('ts', (K, P)), ('sums', (K, 4)),
                                                     ('dmaps', (K, h, w)))}
    o = {k: v[1] for k, v in bufs.items()}
    st = _vah.raw_stream(dev)
    rc = lib.vah_pml_forward(pred.data_ptr(), pred.stride(0), pred.stride(1), Mp, h, w, t.data_ptr(), {torch.float32: 0, torch.uint8: 3}[t.dtype],
                             t.stride(0), t.stride(1), t.shape[0], t.shape[1], t.shape[2], p.data_ptr(), P, _ptr(ri), _ptr(ti), K, eps,
                             o['bce'].data_ptr(), o['dice'].data_ptr(), o['xs'].data_ptr(), o['ts'].data_ptr(), o['sums'].data_ptr(),
                             ws.data_ptr(), nbytes, st)
    _vah.check(rc, 'vah_pml_forward')
    ws.fill_(255)
    gb, gd = g_bce.to(dev), g_dice.to(dev)
    rc = lib.vah_pml_backward(p.data_ptr(), o['xs'].data_ptr(), o['ts'].data_ptr(), o['sums'].data_ptr(), gb.data_ptr(), gd.data_ptr(), K, P,
                              h, w, eps, o['dmaps'].data_ptr(), ws.data_ptr(), nbytes, st)
    _vah.check(rc, 'vah_pml_backward')
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        b = buf.cpu()
        assert bool((b[:8] == GUARD).all()) and bool((b[-8:] == GUARD).all()), 'guard of %s overwritten' % name
    return {k: v.cpu() for k, v in o.items()}


def _check(got, want, finite=True):
    for name in NAMES:
        if finite:
            assert bool(torch.isfinite(got[name]).all()), '%s: an element was not written' % name
        _note(name, base.ratio(got[name], want[name][0], want[name][1]))
    far = ~want['reach']
    assert bool((got['dmaps'][far] == 0.0).all()) and not bool(torch.signbit(got['dmaps'][far]).any()), 'an untouched pixel is not +0.0'


def _same_bits(a, b, names=NAMES):
    for name in names:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


def _points(K, P, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((K, P, 2), generator=g) * 1.2 - 0.1


def _pred(M, h, w, seed):
    return torch.randn((M, h, w), generator=torch.Generator().manual_seed(seed)) * 4


def _tgt(M, H, W, dtype, seed):
    t = torch.rand((M, H, W), generator=torch.Generator().manual_seed(seed))
    return (t < 0.5).to(torch.uint8) if dtype == torch.uint8 else t


def _grads(K, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((K,), generator=g), torch.randn((K,), generator=g)


ROWS, TGT_ROWS = [6, 1, 4, 3], [2, 0, 2, 1]             # scrambled with unused maps in between / with a repeat


@pytest.mark.parametrize('dtype', [torch.float32, torch.uint8], ids=['f32', 'u8'])
@pytest.mark.parametrize('hw', [(1, 1), (2, 3), (5, 7), (32, 48)], ids=lambda s: '%dx%d' % s)
def test_small_maps(hw, dtype):
    h, w = hw
    pred, tgt = _pred(8, h, w, 11 + h), _tgt(3, 11, 9, dtype, 7)
    dpred = pred.to(_dev())
    edge = base.edge_points(h, w)
    K = len(ROWS)
    g_bce, g_dice = _grads(K)
    for P in (1, 63, 64, 65, 257, edge.shape[0]):
        pts = _points(K, P, 100 + P)
        if P == edge.shape[0]:
            pts[0], pts[2] = edge, edge.flip(0)
        want = ref.reference(pred, tgt, pts, ROWS, TGT_ROWS, 1.0, g_bce, g_dice)
        got = c_call(dpred, tgt, pts, ROWS, TGT_ROWS, g_bce, g_dice)
        _check(got, want)
        _same_bits(got, c_call(dpred, tgt, pts, ROWS, TGT_ROWS, g_bce, g_dice))
    # identity rows (NULL index arrays)
    pts = _points(3, 65, 9)
    want = ref.reference(pred, tgt, pts, None, None, 1.0, g_bce[:3], g_dice[:3])
    _check(c_call(dpred, tgt, pts, None, None, g_bce[:3], g_dice[:3]), want)


def test_row_stride_wider_than_the_map():
    h, w, K = 5, 7, len(ROWS)
    pred, tgt = _pred(8, h, w, 3), _tgt(3, 11, 9, torch.uint8, 4)
    wide = torch.zeros((8, h + 1, w + 5))
    wide[:, :h, :w] = pred
    view = wide.to(_dev())[:, :h, :w]
    twide = torch.zeros((3, 12, 16), dtype=torch.uint8)
    twide[:, :11, :9] = tgt
    pts = _points(K, 65, 21)
    g_bce, g_dice = _grads(K)
    want = ref.reference(pred, tgt, pts, ROWS, TGT_ROWS, 1.0, g_bce, g_dice)
    _check(c_call(view, tgt, pts, ROWS, TGT_ROWS, g_bce, g_dice), want)
    dev_t = twide.to(_dev())[:, :11, :9]
    assert not dev_t.is_contiguous()
    _check(c_call(view, dev_t, pts, ROWS, TGT_ROWS, g_bce, g_dice), want)


@pytest.mark.parametrize('hw', [(5, 7), (32, 48)], ids=lambda s: '%dx%d' % s)
def test_all_points_in_one_cell(hw):
    """the longest list a row can have: P points in one cell, in the interior and in the corner cell that has one tap"""
    h, w = hw
    K, P = len(ROWS), 257
    pred, tgt = _pred(8, h, w, 5), _tgt(3, 11, 9, torch.float32, 6)
    g = torch.Generator().manual_seed(8)
    frac = torch.rand((K, P, 2), generator=g) * 0.98 + 0.01
    cell = torch.tensor([[min(2, w - 2), min(1, h - 2)], [-1, -1], [w - 1, 0], [0, h - 1]], dtype=torch.float32)[:, None]
    pts = (cell + frac + 0.5) / torch.tensor([w, h], dtype=torch.float32)
    g_bce, g_dice = _grads(K)
    want = ref.reference(pred, tgt, pts, ROWS, TGT_ROWS, 1.0, g_bce, g_dice)
    assert int(want['touched'][0].sum()) == 4 and int(want['touched'][1].sum()) == 1
    got = c_call(pred.to(_dev()), tgt, pts, ROWS, TGT_ROWS, g_bce, g_dice)
    _check(got, want)
    _same_bits(got, c_call(pred.to(_dev()), tgt, pts, ROWS, TGT_ROWS, g_bce, g_dice))


def test_all_points_outside_the_map():
    h, w, K, P = 5, 7, 2, 65
    pred, tgt = _pred(8, h, w, 5), _tgt(3, 11, 9, torch.uint8, 6)
    pts = _points(K, P, 3) + torch.tensor([2.0, -3.0])
    g_bce, g_dice = _grads(K)
    got = c_call(pred.to(_dev()), tgt, pts, [5, 2], [1, 1], g_bce, g_dice)
    assert bool((got['xs'] == 0).all()) and bool((got['ts'] == 0).all())
    want = ref.reference(pred, tgt, pts, [5, 2], [1, 1], 1.0, g_bce, g_dice)
    _check(got, want)
    assert float((got['bce'].double() - P * math.log(2.0)).abs().max()) <= float(want['bce'][1].max())
    assert bool((got['dmaps'] == 0.0).all()) and not bool(torch.signbit(got['dmaps']).any())


def test_empty_call_reads_no_pointer():
    assert lib.vah_pml_forward(None, 35, 7, 8, 5, 7, None, 3, 99, 9, 3, 11, 9, None, 65, None, None, 0, 1.0, None, None, None, None, None,
                               None, 0, _vah.raw_stream(_dev())) == 0
    assert lib.vah_pml_backward(None, None, None, None, None, None, 0, 65, 5, 7, 1.0, None, None, 0, _vah.raw_stream(_dev())) == 0


@pytest.fixture(scope='module')
def big():
    """160 x 160, K 3, P 12 544, targets 640 x 640 uint8, the head's own mixture of points"""
    h = w = 160
    K, P = 3, 12544
    pred = _pred(5, h, w, 31)
    g = torch.Generator().manual_seed(32)
    yy, xx = torch.meshgrid(torch.arange(640), torch.arange(640), indexing='ij')
    tgt = torch.stack([(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).to(torch.uint8)
                       for cy, cx, ry, rx in ((200, 300, 150, 90), (400, 100, 80, 200), (320, 500, 260, 120), (50, 50, 40, 40))])
    rows, tgt_rows = [4, 0, 2], [1, 3, 1]
    over = torch.rand((K, 3 * P, 2), generator=g)
    logits = F.grid_sample(pred[rows][:, None], 2.0 * over[:, None] - 1.0, mode='bilinear', padding_mode='zeros', align_corners=False)[:, 0, 0]
    keep = torch.topk(-logits.abs(), int(0.75 * P), dim=1)[1]
    pts = torch.cat([torch.gather(over, 1, keep[..., None].expand(-1, -1, 2)), torch.rand((K, P - int(0.75 * P), 2), generator=g)], 1)
    g_bce, g_dice = _grads(K)
    want = ref.reference(pred, tgt, pts, rows, tgt_rows, 1.0, g_bce, g_dice)
    got = c_call(pred.to(_dev()), tgt, pts, rows, tgt_rows, g_bce, g_dice)
    return pred, tgt, pts, rows, tgt_rows, g_bce, g_dice, want, got


def test_production_shape(big):
    *_, want, got = big
    _check(got, want)
    assert not bool(want['reach'].all())                  # there are pixels no point touches: their +0.0 is part of the check


def test_production_shape_same_bits_twice_and_with_the_rows_reversed(big):
    pred, tgt, pts, rows, tgt_rows, g_bce, g_dice, _, got = big
    dpred = pred.to(_dev())
    _same_bits(got, c_call(dpred, tgt, pts, rows, tgt_rows, g_bce, g_dice))
    rev = c_call(dpred, tgt, pts.flip(0), rows[::-1], tgt_rows[::-1], g_bce.flip(0), g_dice.flip(0))
    _same_bits(got, {k: v.flip(0) for k, v in rev.items()})


def test_small_shape_same_bits_with_the_rows_reversed():
    h, w, K = 5, 7, len(ROWS)
    pred, tgt = _pred(8, h, w, 3), _tgt(3, 11, 9, torch.float32, 4)
    pts = _points(K, 257, 2)
    pts[1] = base.edge_points(h, w)[:257].repeat(12, 1)[:257]
    g_bce, g_dice = _grads(K)
    dpred = pred.to(_dev())
    got = c_call(dpred, tgt, pts, ROWS, TGT_ROWS, g_bce, g_dice)
    rev = c_call(dpred, tgt, pts.flip(0), ROWS[::-1], TGT_ROWS[::-1], g_bce.flip(0), g_dice.flip(0))
    _same_bits(got, {k: v.flip(0) for k, v in rev.items()})


@pytest.mark.parametrize('bad', [float('inf'), float('-inf'), float('nan')], ids=['+inf', '-inf', 'nan'])
def test_nonfinite_prediction_element(bad):
    """points on a dyadic grid, so that the fp32 and the exact coordinate agree; element [1][1] of the first row's map is
    sampled with weight 0 by the point on the centre of pixel (0, 0) (its tap 11), with weight 1 by the point on its own
    centre and with weights in between by others.  Whatever torch's fp64 expression and its autograd make non-finite is
    non-finite from the kernels (tests/test_nonfinite_gpu.py's rule)."""
    pred = torch.arange(32, dtype=torch.float32).reshape(2, 4, 4).clone() / 8 - 1
    pred[1, 1, 1] = bad
    tgt = _tgt(2, 4, 4, torch.float32, 2)
    pts = torch.tensor([[0.125, 0.125], [0.375, 0.375], [0.25, 0.25], [0.125, 0.375], [0.875, 0.875], [1.0, 1.0], [0.875, 0.125],
                        [0.625, 0.625], [1.125, 0.875], [0.375, 0.125]])[None].repeat(2, 1, 1)
    rows, tgt_rows = [1, 0], [0, 1]
    g_bce, g_dice = torch.tensor([0.5, 1.5]), torch.tensor([2.0, -1.0])
    got = c_call(pred.to(_dev()), tgt, pts, rows, tgt_rows, g_bce, g_dice)
    maps = pred.double()[rows].clone().requires_grad_(True)
    x = base.grid_sample64(maps, pts)
    t = base.grid_sample64(tgt.double()[tgt_rows], pts)
    bce = F.binary_cross_entropy_with_logits(x, t, reduction='none').sum(1)
    s = x.sigmoid()
    dice = 1 - (2 * (s * t).sum(1) + 1.0) / (s.sum(1) + t.sum(1) + 1.0)
    (bce * g_bce.double() + dice * g_dice.double()).sum().backward()
    for name, theirs in (('xs', x.detach()), ('bce', bce.detach()), ('dice', dice.detach()), ('dmaps', maps.grad)):
        lost = ~torch.isfinite(theirs) & torch.isfinite(got[name])
        assert not bool(lost.any()), (name, 'finite where torch is not', lost.nonzero().tolist())
    assert not bool(torch.isfinite(got['xs'][0, 0])) and not bool(torch.isfinite(got['bce'][0]))      # the weight-0 tap counts
    # the row that does not read the element is untouched by it
    assert all(bool(torch.isfinite(got[name][1]).all()) for name in NAMES)
    want = ref.reference(pred, tgt, pts, rows, tgt_rows, 1.0, g_bce, g_dice)
    for name in NAMES:
        base.ratio(got[name][1], want[name][0][1], want[name][1][1])
