"""GPU: the SpatialPriorModule kernels on NHWC bf16 (csrc/conv.hip, csrc/spm_nhwc.hip, and bn_finalize_kernel of
csrc/tail_ops.hip) held to fp64 (oracle/spm.py) at the production sizes of BASELINE configs[1]-[4], at the walk
boundaries of their persistent grids, and on tiny maps.

Budgets (oracle/spm.py): |got - ref| <= C_ACC 2^-24 A (+ 2^-8 |ref| for bf16 outputs), C_ACC = 256; finalize_stats to
4 fp32 ulps of its conditioning; max-pool forward and window index, and the NHWC16 layout, exact.

Every case
  * NaN-fills every output and workspace first (conv and pool outputs, the wgrad partials of
    vah_conv3x3_wgrad_ws_floats, the BatchNorm workspace and sums, mean / rstd), and places the conv, pool, BatchNorm
    and layout outputs inside a larger NaN buffer with one image row (or one row of the matrix) of guard band on each
    side, which must come back bit-unchanged: a write outside the ragged last tile fails;
  * runs twice and requires the same bits;
  * at production size, runs once more through spm_nhwc._Conv3x3 / _BNRelu / _MaxPool / image_to_nhwc16, which must
    give the direct call's bits (the stem's zero-padded weight columns and the [:, :3] slice of its gradient included).

Walk boundaries.  The launches are persistent grids: a workgroup walks tiles slot, slot + slots, ... .  Slot counts,
from launch_taps / launch_wgrad (kCUs = 256):
  * launch_taps<CK, WY, WC, MAXP, TMAX>: slots = ceil(per_cu * 256 / (Cout / 64 * groups)), per_cu = 2 when the
    dynamic LDS (64 w_stride(CK, T) + HY HX px_stride(CK)) is at most 80 KiB, else 1; at most ntiles.
      <16,8,1,2,9>  (Cin 16, stride 1)       35.8 KB  -> 512 slots at Cout 64
      <16,2,2,3,9>  (stem, Cin 16, stride 2) 35.1 KB  -> 512 slots at Cout 64
      <64,2,2,11,9> (stride 2, Cin >= 64)    121.6 KB -> 256 / (Cout / 64)
      <64,8,1,6,9>  (stride 1 forward and input gradient) 123.7 KB -> 256 / (Cout / 64)
      <64,8,1,6,4>  (stride-2 input gradient, 4 parity groups) 76.6 KB -> 512 / (4 Cin / 64): 128 at Cin 64
    tiles = N ceil(ny / WY) ceil(nx / 32) per group.
  * launch_wgrad<CK, WY>: slots = ceil(256 / (Cout / 64 * Cin / CK)), at most ntiles; tiles = N ceil(OH / WY)
    ceil(OW / 32); <16,2>, <64,2>: stride 2, <16,4>, <64,4>: stride 1.
_taps_walk / _wgrad_walk mirror this arithmetic, and every WALK case asserts its instantiation, slot count and
tiles per workgroup: a change of launch geometry must show up here and be re-derived.

Run with -s for one RATIO line per checked output and the worst ratio per family at the end.  Acceptance check for any
change to conv.hip or spm_nhwc.hip."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import spm

pytestmark = pytest.mark.gpu

NAN = float('nan')
EPS, MOMENTUM = 1e-5, 0.1
C_FIN = 4.0
CUS = 256

# BASELINE configs[1]-[4]: (image H, W, batch)
CONFIGS = {'c1': (512, 512, 2), 'c2': (1024, 1024, 2), 'c3': (640, 640, 2), 'c4': (800, 1344, 1)}


def _layers(H, W):
    """the six 3 x 3 convs of the SPM as (name, input H, W, Cin, Cout, stride, weight Cin); the two stride-1 stem
    convs have the same shape and are tested once"""
    return [('stem0', H, W, 16, 64, 2, 3), ('stem1', H // 2, W // 2, 64, 64, 1, 64), ('conv2', H // 4, W // 4, 64, 128, 2, 64),
            ('conv3', H // 8, W // 8, 128, 256, 2, 128), ('conv4', H // 16, W // 16, 256, 256, 2, 256)]


CONV_CASES = [(c,) + l for c, (H, W, N) in CONFIGS.items() for l in _layers(H, W)]
# BatchNorm rows x C: the conv outputs (the three stem BatchNorms share a shape)
BN_CASES = [('%s_%s' % (c, l[0]), N * ((l[1] - 1) // l[5] + 1) * ((l[2] - 1) // l[5] + 1), l[4])
            for c, (H, W, N) in CONFIGS.items() for l in _layers(H, W) if l[0] != 'stem1']
# the 512-part cap of bn_nhwc_stats (parts = min(512, ceil(rows / 64))): 511 parts; 512 with a 1-row last one;
# 512 of exactly 64 rows; 65 rows per part, so the last 8 parts are empty and the one before holds 9 rows
BN_CAP_CASES = [('cap_%d' % r, r, 64) for r in (32704, 32705, 32768, 32769)]

# (name, kind, N, H, W, Cin, Cout, S, instantiation, slots, most tiles per workgroup, fewest)
# "just above": a few workgroups walk a second tile, and that tile is ragged; ">= 3": every workgroup walks 3 or more
WALK_CASES = [
    ('t16s1_above', 'fwd', 1, 123, 1029, 16, 64, 1, 'taps<16,8,1,2,9>', 512, 2, 1),       # 528 tiles; rows 120..122
    ('t16s1_walk3', 'fwd', 2, 200, 1000, 16, 64, 1, 'taps<16,8,1,2,9>', 512, 4, 3),       # 1 600 tiles; x 992..999
    ('t16s2_above', 'fwd', 1, 517, 199, 16, 64, 2, 'taps<16,2,2,3,9>', 512, 2, 1),        # 520 tiles; OH 259, OW 100
    ('t16s2_walk3', 'fwd', 3, 512, 400, 16, 64, 2, 'taps<16,2,2,3,9>', 512, 6, 5),        # 2 688 tiles
    ('t64s2_above', 'fwd', 1, 517, 45, 64, 128, 2, 'taps<64,2,2,11,9>', 128, 2, 1),       # 130 tiles; OH 259, OW 23
    ('t64s2_walk3', 'fwd', 2, 256, 130, 128, 256, 2, 'taps<64,2,2,11,9>', 64, 6, 6),      # 384 tiles, 2 chunks, OW 65
    ('t64s1_above', 'fwd', 1, 261, 250, 64, 64, 1, 'taps<64,8,1,6,9>', 256, 2, 1),        # 264 tiles; rows 256..260
    ('t64s1_walk3', 'dgrad', 3, 256, 256, 64, 128, 1, 'taps<64,8,1,6,9>', 256, 3, 3),     # 768 tiles, dY 128 channels
    ('t64s2dg_above', 'dgrad', 1, 261, 499, 64, 128, 2, 'taps<64,8,1,6,4>', 128, 2, 1),   # 136 tiles per parity
    ('t64s2dg_walk3', 'dgrad', 2, 512, 512, 64, 64, 2, 'taps<64,8,1,6,4>', 128, 4, 4),    # 512 tiles per parity
    ('w16s2_above', 'wgrad', 1, 341, 179, 16, 64, 2, 'wgrad<16,2>', 256, 2, 1),           # 258 tiles; OH 171, OW 90
    ('w16s2_walk3', 'wgrad', 3, 256, 200, 16, 64, 2, 'wgrad<16,2>', 256, 3, 3),           # 768 tiles; OW 100
    ('w16s1_above', 'wgrad', 1, 257, 120, 16, 64, 1, 'wgrad<16,4>', 256, 2, 1),           # 260 tiles; row 256
    ('w16s1_walk3', 'wgrad', 3, 256, 128, 16, 64, 1, 'wgrad<16,4>', 256, 3, 3),           # 768 tiles
    ('w64s2_above', 'wgrad', 1, 169, 139, 64, 128, 2, 'wgrad<64,2>', 128, 2, 1),          # 129 tiles; OH 85, OW 70
    ('w64s2_walk3', 'wgrad', 3, 128, 96, 128, 256, 2, 'wgrad<64,2>', 32, 6, 6),           # 192 tiles on 32 slots
    ('w64s1_above', 'wgrad', 1, 258, 125, 64, 64, 1, 'wgrad<64,4>', 256, 2, 1),           # 260 tiles; rows 256, 257
    ('w64s1_walk3', 'wgrad', 3, 256, 128, 64, 64, 1, 'wgrad<64,4>', 256, 3, 3),           # 768 tiles
]

# tiny maps: H or W in {1, 2, 3} (empty parity slices of the stride-2 input gradient), W = 33 (one pixel into the second
# x tile), batch 1 and 3: (N, H, W, Cin, Cout, S), every kind that exists for the shape
TINY_CASES = [(1, 1, 1, 64, 64, 1), (1, 1, 1, 64, 64, 2), (3, 2, 3, 64, 128, 2), (1, 3, 2, 64, 64, 1), (3, 1, 33, 64, 64, 2),
              (1, 33, 1, 16, 64, 2), (3, 2, 33, 16, 64, 1), (1, 3, 33, 128, 64, 1), (3, 33, 3, 64, 64, 2), (1, 2, 2, 256, 256, 2),
              (3, 3, 1, 64, 128, 1)]

WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for key in sorted(WORST):
        r, case = WORST[key]
        print('WORST %-16s %.3f (%s)' % (key, r, case))


def _record(family, case, r):
    print('RATIO %s %s %.4f' % (family, case, r))
    prev = WORST.get(family)
    if prev is None or r > prev[0]:
        WORST[family] = (r, case)


def _check16(family, case, what, got, ref, A, mask=None):
    """a bf16 output: within its budget; records the ratio, and the accumulation part alone (beyond half an ulp)"""
    _record(family, case, spm.check(case + ' ' + what, got, ref, A, bf16=True, mask=mask))
    _record(family + ' (acc)', case, spm.rounding_excess(got, ref, A, mask))


def _vah():
    import _vah
    return _vah


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ck(rc, what):
    _vah().check(rc, what)


class _Guarded:
    """a tensor of `shape` in the middle of a NaN (uint8: 0xEE) buffer with `guard` elements on each side"""

    def __init__(self, shape, dtype, guard):
        self.n, self.g = math.prod(shape), guard
        self.fill = 0xEE if dtype == torch.uint8 else NAN
        self.buf = torch.full((self.n + 2 * guard,), self.fill, dtype=dtype, device='cuda')
        self.t = self.buf[guard:guard + self.n].view(shape)
        self.ref = self.buf[:1].clone()

    def reset(self):
        self.buf.fill_(self.fill)

    def assert_intact(self, what):
        for band in (self.buf[:self.g], self.buf[self.g + self.n:]):
            if band.dtype == torch.uint8:
                ok = bool((band == self.ref).all())
            else:
                ok = torch.equal(band.view(torch.int16 if band.element_size() == 2 else torch.int32),
                                 self.ref.view(torch.int16 if band.element_size() == 2 else torch.int32).expand(band.shape))
            assert ok, '%s: a write landed in the guard band outside the output' % what


def _equal(a, b, what):
    assert torch.equal(a, b), '%s: %d elements differ' % (what, int((a != b).sum()))


def _same_bits(a, b, what):
    """bit equality that treats the bf16 / fp32 NaN pattern like any other"""
    ia = a.contiguous().view(torch.int16 if a.element_size() == 2 else (torch.int32 if a.element_size() == 4 else torch.uint8))
    ib = b.contiguous().view(ia.dtype)
    _equal(ia, ib, what)


# ---------------------------------------------------------------- launch geometry (mirror of conv.hip)
def _px_stride(ck):
    return ck * 2 + 16


def _w_stride(ck, T):
    return T * ck * 2 + 16


def _taps_walk(kind, N, H, W, Cin, Cout, S):
    """(instantiation, slots, most tiles per workgroup, fewest) of the forward / input-gradient launch"""
    if kind == 'fwd':
        OH, OW = (H - 1) // S + 1, (W - 1) // S + 1
        gin, gout, gs = Cin, Cout, S
        groups = [(9, 3, 3, OH, OW)]                         # taps, tap extent y / x, positions y / x
    else:
        gin, gout, gs = Cout, Cin, 1
        if S == 1:
            groups = [(9, 3, 3, H, W)]
        else:
            groups = [((1 + a) * (1 + b), 1 + a, 1 + b, (H - a + 1) // 2, (W - b + 1) // 2) for a in (0, 1) for b in (0, 1)]
            groups = [g for g in groups if g[3] > 0 and g[4] > 0]
    if gin == 16:
        ck, wy, name = (16, 8, 'taps<16,8,1,2,9>') if gs == 1 else (16, 2, 'taps<16,2,2,3,9>')
    elif gs == 2:
        ck, wy, name = 64, 2, 'taps<64,2,2,11,9>'
    else:
        ck, wy = 64, 8
        name = 'taps<64,8,1,6,9>' if max(g[0] for g in groups) > 4 else 'taps<64,8,1,6,4>'
    lds, tiles = 0, []
    for T, ey, ex, ny, nx in groups:
        HY, HX = (wy - 1) * gs + ey, 31 * gs + ex
        lds = max(lds, 64 * _w_stride(ck, T) + HY * HX * _px_stride(ck))
        tiles.append(N * -(-ny // wy) * -(-nx // 32))
    per_cu = 1 if lds > 80 * 1024 else 2
    others = (gout // 64) * len(groups)
    slots = max(1, min(-(-(per_cu * CUS) // others), max(tiles)))
    return name, slots, -(-max(tiles) // slots), max(tiles) // slots


def _wgrad_walk(N, H, W, Cin, Cout, S):
    OH, OW = (H - 1) // S + 1, (W - 1) // S + 1
    ck, wy = (16 if Cin == 16 else 64), (4 if S == 1 else 2)
    tiles = N * -(-OH // wy) * -(-OW // 32)
    slots = min(-(-CUS // ((Cout // 64) * (Cin // ck))), tiles)
    return 'wgrad<%d,%d>' % (ck, wy), slots, -(-tiles // slots), tiles // slots


# ---------------------------------------------------------------- direct calls
def _fwd(x, w9, S, out):
    N, H, W, Cin = x.shape
    OH, OW = out.shape[1:3]
    ty = (ctypes.c_int * 9)(*[t // 3 - 1 for t in range(9)])
    tx = (ctypes.c_int * 9)(*[t % 3 - 1 for t in range(9)])
    _ck(_vah().lib.vah_conv_taps_nhwc_bf16(x.data_ptr(), N, H, W, Cin, w9.data_ptr(), w9.shape[0], 9, ty, tx, S, out.data_ptr(),
                                           OH, OW, OH, OW, 1, 0, 0, _st()), 'conv_taps')


def _dgrad(gy, wt9, S, gx):
    N, OH, OW, Cout = gy.shape
    _, H, W, Cin = gx.shape
    _ck(_vah().lib.vah_conv3x3_dgrad_nhwc_bf16(gy.data_ptr(), N, OH, OW, Cout, wt9.data_ptr(), Cin, S, gx.data_ptr(), H, W, _st()),
        'conv_dgrad')


def _wgrad(x, gy, S, ws, dw):
    N, H, W, Cin = x.shape
    _, OH, OW, Cout = gy.shape
    _ck(_vah().lib.vah_conv3x3_wgrad_nhwc_bf16(x.data_ptr(), N, H, W, Cin, gy.data_ptr(), OH, OW, Cout, S, ws.data_ptr(), ws.numel(),
                                               dw.data_ptr(), _st()), 'conv_wgrad')


def _twice(call, outs, what):
    """call() twice from NaN-filled outputs: guard bands intact, same bits; returns the first results"""
    first = None
    for _ in range(2):
        for o in outs:
            o.reset()
        call()
        torch.cuda.synchronize()
        for o in outs:
            o.assert_intact(what)
        got = [o.t.clone() for o in outs]
        if first is None:
            first = got
        else:
            for a, b in zip(first, got):
                _same_bits(a, b, what + ': repeated call')
    return first


def _conv_operands(N, H, W, Cin, Cout, S, wcin, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    if Cin == 16:                                     # the stem reads the bf16 NHWC16 image
        x = spm.image_to_nhwc16(torch.randn(N, 3, H, W, device='cuda', generator=g))
    else:                                             # post-ReLU activations: about half zeros
        x = torch.randn(N, H, W, Cin, device='cuda', generator=g).clamp_min(0).to(torch.bfloat16)
    w32 = torch.randn(Cout, wcin, 3, 3, device='cuda', generator=g) * (9 * wcin) ** -0.5
    OH, OW = (H - 1) // S + 1, (W - 1) // S + 1
    gy = torch.randn(N, OH, OW, Cout, device='cuda', generator=g).to(torch.bfloat16)
    return x, w32, gy


def _run_conv(case, N, H, W, Cin, Cout, S, wcin, kinds, seed, wrapper=False):
    from vitadapter import conv
    x, w32, gy = _conv_operands(N, H, W, Cin, Cout, S, wcin, seed)
    wb = F.pad(w32, (0, 0, 0, 0, 0, Cin - wcin)).to(torch.bfloat16)
    w9, wt9 = conv.forward_weight(wb), conv.dgrad_weight(wb)
    OH, OW = gy.shape[1:3]
    res = {}
    if 'fwd' in kinds:
        out = _Guarded((N, OH, OW, Cout), torch.bfloat16, OW * Cout)
        got, = _twice(lambda: _fwd(x, w9, S, out.t), [out], case + ' forward')
        ref, A = spm.conv_forward(x, w9, S)
        _check16('conv fwd', case, 'forward', got, ref, A)
        res['fwd'] = got
        del ref, A
    if 'dgrad' in kinds and Cin != 16:
        gx = _Guarded((N, H, W, Cin), torch.bfloat16, W * Cin)
        got, = _twice(lambda: _dgrad(gy, wt9, S, gx.t), [gx], case + ' input grad')
        ref, A = spm.conv_input_grad(gy, wt9, S, H, W)
        _check16('conv dgrad', case, 'input grad', got, ref, A)
        res['dgrad'] = got
        del ref, A
    if 'wgrad' in kinds:
        ws = _Guarded((_vah().lib.vah_conv3x3_wgrad_ws_floats(Cin, Cout),), torch.float32, 0)
        dw = _Guarded((Cout, 9, Cin), torch.float32, 9 * Cin)
        _, got = _twice(lambda: _wgrad(x, gy, S, ws.t, dw.t), [ws, dw], case + ' weight grad')
        ref, A = spm.conv_weight_grad(x, gy, S)
        _record('conv wgrad', case, spm.check(case + ' weight grad', got, ref, A))
        if wcin < Cin:
            assert (got[..., wcin:] == 0).all()
        res['wgrad'] = got
        del ref, A
    if wrapper:
        from vitadapter import spm_nhwc
        xr = x.clone().requires_grad_(Cin != 16)
        wr = w32.clone().requires_grad_(True)
        y = spm_nhwc._Conv3x3.apply(xr, wr, S)
        y.backward(gy)
        torch.cuda.synchronize()
        _same_bits(y.detach(), res['fwd'], case + ' _Conv3x3 forward')
        if Cin != 16:
            _same_bits(xr.grad, res['dgrad'], case + ' _Conv3x3 input grad')
        else:
            assert xr.grad is None
        _same_bits(wr.grad, res['wgrad'].view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)[:, :wcin].contiguous(), case + ' _Conv3x3 weight grad')


@pytest.mark.parametrize('cfg,layer,H,W,Cin,Cout,S,wcin', CONV_CASES, ids=['%s_%s' % c[:2] for c in CONV_CASES])
def test_conv_production(cfg, layer, H, W, Cin, Cout, S, wcin):
    N = CONFIGS[cfg][2]
    _run_conv('%s_%s' % (cfg, layer), N, H, W, Cin, Cout, S, wcin, ('fwd', 'dgrad', 'wgrad'), seed=H + W + Cin + Cout, wrapper=True)


@pytest.mark.parametrize('case', WALK_CASES, ids=[c[0] for c in WALK_CASES])
def test_conv_walk_boundary(case):
    name, kind, N, H, W, Cin, Cout, S, inst, slots, most, fewest = case
    geo = _wgrad_walk(N, H, W, Cin, Cout, S) if kind == 'wgrad' else _taps_walk(kind, N, H, W, Cin, Cout, S)
    assert geo == (inst, slots, most, fewest), (name, geo)
    _run_conv(name, N, H, W, Cin, Cout, S, 3 if Cin == 16 else Cin, (kind,), seed=len(name) * 7 + N)


@pytest.mark.parametrize('shape', TINY_CASES, ids=['x'.join(map(str, c)) for c in TINY_CASES])
def test_conv_tiny(shape):
    N, H, W, Cin, Cout, S = shape
    _run_conv('tiny_' + 'x'.join(map(str, shape)), N, H, W, Cin, Cout, S, 3 if Cin == 16 else Cin, ('fwd', 'dgrad', 'wgrad'),
              seed=H * 100 + W)


# ---------------------------------------------------------------- BatchNorm
def _run_bn(case, rows, C, seed):
    lib = _vah().lib
    g = torch.Generator(device='cuda').manual_seed(seed)
    sig = torch.rand(C, device='cuda', generator=g) * 1.5 + 0.5
    off = 3.0 * sig * torch.sign(torch.randn(C, device='cuda', generator=g))          # a mean offset of 3 sigma
    x = (torch.randn(rows, C, device='cuda', generator=g) * sig + off).to(torch.bfloat16)
    dy = torch.randn(rows, C, device='cuda', generator=g).to(torch.bfloat16)
    w = torch.randn(C, device='cuda', generator=g) * 0.3 + 1.0
    b = torch.randn(C, device='cuda', generator=g) * 0.3
    rm0 = torch.randn(C, device='cuda', generator=g) * 0.1
    rv0 = torch.rand(C, device='cuda', generator=g) + 0.5
    nws = lib.vah_bn_nhwc_ws_floats(C)
    ws, sums, sums2 = _Guarded((nws,), torch.float32, 0), _Guarded((2 * C + 1,), torch.float32, 0), _Guarded((2 * C,), torch.float32, 0)
    mean, rstd = _Guarded((C,), torch.float32, 0), _Guarded((C,), torch.float32, 0)
    y, ye, dx = (_Guarded((rows, C), torch.bfloat16, C) for _ in range(3))
    st = _st()

    def run():
        ws.reset()
        _ck(lib.vah_bn_nhwc_stats(x.data_ptr(), rows, C, sums.t.data_ptr(), ws.t.data_ptr(), st), 'bn_nhwc_stats')
        sums.t[2 * C:].fill_(float(rows))
        rm, rv = rm0.clone(), rv0.clone()
        _ck(lib.vah_bn_finalize_stats(sums.t.data_ptr(), C, EPS, MOMENTUM, rm.data_ptr(), rv.data_ptr(), mean.t.data_ptr(),
                                      rstd.t.data_ptr(), st), 'bn_finalize_stats')
        _ck(lib.vah_bn_nhwc_apply(x.data_ptr(), rows, C, mean.t.data_ptr(), rstd.t.data_ptr(), w.data_ptr(), b.data_ptr(), 1,
                                  y.t.data_ptr(), st), 'bn_nhwc_apply')
        ws.reset()
        _ck(lib.vah_bn_nhwc_bwd_stats(x.data_ptr(), dy.data_ptr(), rows, C, mean.t.data_ptr(), rstd.t.data_ptr(), w.data_ptr(),
                                      b.data_ptr(), 1, sums2.t.data_ptr(), ws.t.data_ptr(), st), 'bn_nhwc_bwd_stats')
        means = sums2.t / sums.t[2 * C:]
        _ck(lib.vah_bn_nhwc_bwd_apply(x.data_ptr(), dy.data_ptr(), rows, C, mean.t.data_ptr(), rstd.t.data_ptr(), w.data_ptr(),
                                      b.data_ptr(), 1, means[:C].data_ptr(), means[C:].data_ptr(), dx.t.data_ptr(), st),
            'bn_nhwc_bwd_apply')
        rse = torch.rsqrt(rv + EPS)                                 # eval mode: the running statistics, as _BNRelu forms them
        _ck(lib.vah_bn_nhwc_apply(x.data_ptr(), rows, C, rm.data_ptr(), rse.data_ptr(), w.data_ptr(), b.data_ptr(), 1,
                                  ye.t.data_ptr(), st), 'bn_nhwc_apply eval')
        torch.cuda.synchronize()
        return [t.t.clone() for t in (sums, mean, rstd, y, sums2, dx, ye)] + [rm, rv, means, rse]

    outs = [sums, sums2, mean, rstd, y, ye, dx]
    for o in outs:
        o.reset()
    first = run()
    for o in outs:
        o.assert_intact(case + ' BatchNorm')
    for o in outs:
        o.reset()
    for a, c in zip(first, run()):
        _same_bits(a, c, case + ' BatchNorm: repeated call')
    s_k, mu_k, rs_k, y_k, s2_k, dx_k, ye_k, rm, rv, means, rse = first

    ref, A = spm.bn_stats(x)
    _record('bn stats', case, spm.check(case + ' stats', s_k[:2 * C], ref, A))
    fin = spm.finalize_stats(s_k, C, EPS, MOMENTUM, rm0, rv0)
    r = 0.
    for k, got in (('mean', mu_k), ('rstd', rs_k), ('running_mean', rm), ('running_var', rv)):
        r = max(r, spm.check(case + ' finalize ' + k, got, fin[k][0], fin[k][1], c_acc=C_FIN))
    _record('bn finalize', case, r)
    yr, Ay = spm.bn_apply(x, mu_k, rs_k, w, b, True)
    _check16('bn apply', case, 'apply', y_k, yr, Ay)
    yr, Ay = spm.bn_apply(x, rm, rse, w, b, True)
    _check16('bn apply eval', case, 'eval apply', ye_k, yr, Ay)
    del yr, Ay
    ref, A, edge = spm.bn_bwd_stats(x, dy, mu_k, rs_k, w, b, True)
    assert float(edge.double().mean()) < 1e-4, (case, int(edge.sum()))
    _record('bn bwd stats', case, spm.check(case + ' bwd stats', s2_k, ref, A))
    dxr, Adx = spm.bn_bwd_apply(x, dy, mu_k, rs_k, w, b, True, means[:C], means[C:])
    assert torch.isfinite(dx_k).all()
    _check16('bn bwd apply', case, 'bwd apply', dx_k, dxr, Adx, mask=~edge)
    del dxr, Adx, edge
    return x, dy, w, b, rm0, rv0, first


@pytest.mark.parametrize('case,rows,C', BN_CASES, ids=[c[0] for c in BN_CASES])
def test_bn_production(case, rows, C):
    from vitadapter import spm_nhwc
    x, dy, w, b, rm0, rv0, (s_k, mu_k, rs_k, y_k, s2_k, dx_k, ye_k, rm, rv, means, rse) = _run_bn(case, rows, C, seed=rows % 997 + C)
    norm = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM).cuda().train()
    with torch.no_grad():
        norm.weight.copy_(w), norm.bias.copy_(b), norm.running_mean.copy_(rm0), norm.running_var.copy_(rv0)
    xr = x.clone().requires_grad_(True)
    yw = spm_nhwc._BNRelu.apply(xr, norm.weight, norm.bias, norm, True)
    yw.backward(dy)
    torch.cuda.synchronize()
    _same_bits(yw.detach(), y_k, case + ' _BNRelu forward')
    _same_bits(xr.grad, dx_k, case + ' _BNRelu input grad')
    _same_bits(norm.bias.grad, s2_k[:C], case + ' _BNRelu dbias')
    _same_bits(norm.weight.grad, s2_k[C:], case + ' _BNRelu dweight')
    _same_bits(norm.running_mean, rm, case + ' running mean')
    _same_bits(norm.running_var, rv, case + ' running var')
    norm.eval()
    with torch.no_grad():
        _same_bits(spm_nhwc._BNRelu.apply(x, norm.weight, norm.bias, norm, True), ye_k, case + ' _BNRelu eval')


@pytest.mark.parametrize('case,rows,C', BN_CAP_CASES, ids=[c[0] for c in BN_CAP_CASES])
def test_bn_stats_cap(case, rows, C):
    _run_bn(case, rows, C, seed=rows)


# ---------------------------------------------------------------- max-pool, image layout
POOL_CASES = [('%s_stem' % c, N, H // 2, W // 2, 'relu') for c, (H, W, N) in CONFIGS.items()] + [('c1_few_values', 2, 256, 256, 'few'),
                                                                                               ('odd_few_values', 3, 37, 75, 'few')]


@pytest.mark.parametrize('case,N,H,W,kind', POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_maxpool(case, N, H, W, kind):
    from vitadapter import spm_nhwc
    lib = _vah().lib
    C = 64
    g = torch.Generator(device='cuda').manual_seed(H + W)
    if kind == 'relu':                  # post-ReLU: ties among zeros are the common case
        x = torch.randn(N, H, W, C, device='cuda', generator=g).clamp_min(0).to(torch.bfloat16)
    else:                               # a handful of distinct values: ties between non-zero values
        vals = torch.tensor([-1.0, 0.375, 1.25, 2.5, 2.5], device='cuda')
        x = vals[torch.randint(0, 5, (N, H, W, C), device='cuda', generator=g)].to(torch.bfloat16)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(N, OH, OW, C, device='cuda', generator=g).to(torch.bfloat16)
    y, idx = _Guarded((N, OH, OW, C), torch.bfloat16, OW * C), _Guarded((N, OH, OW, C), torch.uint8, OW * C)
    gx = _Guarded((N, H, W, C), torch.bfloat16, W * C)
    st = _st()

    def fwd():
        _ck(lib.vah_maxpool3s2_nhwc_fwd_bf16(x.data_ptr(), N, H, W, C, y.t.data_ptr(), idx.t.data_ptr(), st), 'maxpool fwd')

    y_k, i_k = _twice(fwd, [y, idx], case + ' max-pool')
    yr, ir = spm.maxpool_forward(x)
    _equal(y_k.double(), yr, case + ' max-pool output')
    _equal(i_k, ir, case + ' max-pool window index')
    idx.t.copy_(i_k)

    def bwd():
        _ck(lib.vah_maxpool3s2_nhwc_bwd_bf16(gy.data_ptr(), idx.t.data_ptr(), N, H, W, C, gx.t.data_ptr(), st), 'maxpool bwd')

    gx_k, = _twice(bwd, [gx], case + ' max-pool backward')
    gr, A = spm.maxpool_backward(gy, ir, H, W)
    _check16('maxpool bwd', case, 'max-pool backward', gx_k, gr, A)
    xr = x.clone().requires_grad_(True)
    yw = spm_nhwc._MaxPool.apply(xr)
    yw.backward(gy)
    torch.cuda.synchronize()
    _same_bits(yw.detach(), y_k, case + ' _MaxPool forward')
    _same_bits(xr.grad, gx_k, case + ' _MaxPool backward')


@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_image_to_nhwc16(cfg):
    from vitadapter import spm_nhwc
    H, W, N = CONFIGS[cfg]
    x = torch.randn(N, 3, H, W, device='cuda') * 3
    y = _Guarded((N, H, W, 16), torch.bfloat16, W * 16)

    def run():
        _ck(_vah().lib.vah_image_to_nhwc16_bf16(x.data_ptr(), N, H, W, y.t.data_ptr(), _st()), 'image_to_nhwc16')

    got, = _twice(run, [y], cfg + ' image_to_nhwc16')
    _same_bits(got, spm.image_to_nhwc16(x), cfg + ' image_to_nhwc16')
    assert (got[..., 3:].view(torch.int16) == 0).all()
    _same_bits(spm_nhwc.image_to_nhwc16(x), got, cfg + ' spm_nhwc.image_to_nhwc16')
