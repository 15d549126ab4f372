"""GPU: the depthwise 3x3 token kernels (csrc/fused_ops.hip) at the smallest shapes at which a form that walks strips
of a map can go wrong, through the C entry points, in bf16 and fp16.

(B, H, W) = (1, 2, 2): maps 4 x 4, 2 x 2, 1 x 1 - in the 1 x 1 map every neighbour is outside, and every map is
smaller than a strip; (3, 2, 6): non-square maps, three images (a read across an image boundary changes the
result); (2, 10, 14): maps 20 x 28, 10 x 14, 5 x 7 - odd sizes, strip ends inside a map and past its last row.
C = 8 (128 token slots per workgroup), 192 (the model's, 5 slots and 16 idle lanes), 200 (C % 8 != 0), 1024 (one slot).
The inputs are random, so they differ per map and per image.

Reference: fp64 conv2d(groups=C) per map on the CPU from the same 16-bit inputs.
  forward, input gradient: |out - ref| <= u |ref| + 16 * 2^-24 * sum |w x|, u = 2^-8 (bf16) / 2^-11 (fp16): one
                           rounding of an fp32 sum of at most ten terms
  dw, db:                  |got - ref| <= 64 * 2^-24 * sum |terms| (the budget of tests/test_reductions_fullsize_gpu.py)
Outputs and the workspace are NaN-filled before each call, two calls must agree bit for bit, and zero-batch and
bad-shape calls return what they always did."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
NAN = float('nan')
DTYPES = {'bf16': (torch.bfloat16, 2.0 ** -8), 'fp16': (torch.float16, 2.0 ** -11)}
SHAPES = [(1, 2, 2), (3, 2, 6), (2, 10, 14)]
CHANNELS = [8, 192, 200, 1024]


def _levels(H, W):
    return [(2 * H, 2 * W), (H, W), (H // 2, W // 2)]


def _reference(x, g, w9, bias, H, W):
    """fp64 on the CPU: y, sum|w x| (+|bias|), dx, sum|w g|, dw, sum|g x|, db, sum|g| of the three maps."""
    B, N, C = x.shape
    xd, gd, wd = x.double().cpu(), g.double().cpu(), w9.double().cpu().view(C, 1, 3, 3)
    bd = bias.double().cpu()
    wf = wd.flip(2, 3)
    ys, yas, dxs, dxas = [], [], [], []
    dw, adw = torch.zeros(C, 9, dtype=torch.float64), torch.zeros(C, 9, dtype=torch.float64)
    t0 = 0
    for h, w in _levels(H, W):
        xm = xd[:, t0:t0 + h * w].reshape(B, h, w, C).permute(0, 3, 1, 2)
        gm = gd[:, t0:t0 + h * w].reshape(B, h, w, C).permute(0, 3, 1, 2)
        tok = lambda m: m.permute(0, 2, 3, 1).reshape(B, h * w, C)
        ys.append(tok(F.conv2d(xm, wd, bd, padding=1, groups=C)))
        yas.append(tok(F.conv2d(xm.abs(), wd.abs(), bd.abs(), padding=1, groups=C)))
        dxs.append(tok(F.conv2d(gm, wf, None, padding=1, groups=C)))
        dxas.append(tok(F.conv2d(gm.abs(), wf.abs(), None, padding=1, groups=C)))
        xp = F.pad(xm, (1, 1, 1, 1))
        for tap in range(9):
            dy, dx = tap // 3, tap % 3
            prod = gm * xp[:, :, dy:dy + h, dx:dx + w]
            dw[:, tap] += prod.sum((0, 2, 3))
            adw[:, tap] += prod.abs().sum((0, 2, 3))
        t0 += h * w
    return (torch.cat(ys, 1), torch.cat(yas, 1), torch.cat(dxs, 1), torch.cat(dxas, 1), dw, adw,
            gd.sum((0, 1)), gd.abs().sum((0, 1)))


def _within(got, ref, bound, what):
    err = (got.double().cpu().reshape(ref.shape) - ref).abs()
    bad = ~(err <= bound)                                       # a NaN (an element never written) fails
    assert not bool(bad.any()), '%s: %d of %d elements over budget (worst err / budget %.3g)' % (
        what, int(bad.sum()), ref.numel(), (err / bound.clamp_min(1e-300)).nan_to_num(float('inf')).max().item())


def _call(dtype, x, g, w9, bias, B, H, W, C):
    import _vah
    N = x.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    y = torch.full((B, N, C), NAN, dtype=dtype, device='cuda')
    dx = torch.full((B, N, C), NAN, dtype=dtype, device='cuda')
    dw, db = torch.full((C * 9,), NAN, device='cuda'), torch.full((C,), NAN, device='cuda')
    ws = torch.full((_vah.lib.vah_reduce_ws_floats(10 * C),), NAN, device='cuda')
    _vah.call('vah_dwconv3x3_tokens_bf16', dtype, x.data_ptr(), w9.data_ptr(), bias.data_ptr(), B, H, W, C, 0, y.data_ptr(), st)
    _vah.call('vah_dwconv3x3_tokens_bf16', dtype, g.data_ptr(), w9.data_ptr(), None, B, H, W, C, 1, dx.data_ptr(), st)
    _vah.call('vah_dwconv3x3_tokens_wgrad_bf16', dtype, x.data_ptr(), g.data_ptr(), B, H, W, C, dw.data_ptr(), db.data_ptr(),
              ws.data_ptr(), st)
    torch.cuda.synchronize()
    return y, dx, dw, db


@pytest.mark.parametrize('dt', sorted(DTYPES))
@pytest.mark.parametrize('C', CHANNELS)
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_dwconv_small_maps(B, H, W, C, dt):
    dtype, u = DTYPES[dt]
    torch.manual_seed(7000 + 100 * H + W + C)
    N = 21 * (H // 2) * (W // 2)
    x = torch.randn(B, N, C, device='cuda').to(dtype)
    g = torch.randn(B, N, C, device='cuda').to(dtype)
    w9 = torch.randn(C, 9, device='cuda') * 0.3
    bias = torch.randn(C, device='cuda') * 0.3
    first = _call(dtype, x, g, w9, bias, B, H, W, C)
    again = _call(dtype, x, g, w9, bias, B, H, W, C)
    for a, b, nm in zip(first, again, ('y', 'dx', 'dw', 'db')):
        assert torch.equal(a, b), '%s: two identical calls differ (%d elements)' % (nm, int((a != b).sum()))
    y, dx, dw, db = first
    ry, ay, rdx, adx, rdw, adw, rdb, adb = _reference(x, g, w9, bias, H, W)
    _within(y, ry, u * ry.abs() + 16 * U24 * ay, 'y')
    _within(dx, rdx, u * rdx.abs() + 16 * U24 * adx, 'dx')
    _within(dw, rdw, 64 * U24 * adw, 'dw')
    _within(db, rdb, 64 * U24 * adb, 'db')


@pytest.mark.parametrize('dt', sorted(DTYPES))
def test_dwconv_zero_batch_and_bad_shapes(dt):
    import _vah
    dtype, _ = DTYPES[dt]
    C, H, W = 8, 2, 2
    st = torch.cuda.current_stream().cuda_stream
    fwd, wgrad = _vah.sym('vah_dwconv3x3_tokens_bf16', dtype), _vah.sym('vah_dwconv3x3_tokens_wgrad_bf16', dtype)
    x = torch.zeros(1, 21, C, dtype=dtype, device='cuda')
    y = torch.full((1, 21, C), NAN, dtype=dtype, device='cuda')
    w9, bias = torch.ones(C, 9, device='cuda'), torch.ones(C, device='cuda')
    dw, db = torch.full((C * 9,), NAN, device='cuda'), torch.full((C,), NAN, device='cuda')
    ws = torch.full((_vah.lib.vah_reduce_ws_floats(10 * C),), NAN, device='cuda')
    # zero batch: the forward writes nothing, the weight gradient is zero
    for mode in (0, 1):
        assert fwd(x.data_ptr(), w9.data_ptr(), bias.data_ptr(), 0, H, W, C, mode, y.data_ptr(), st) == 0
    assert wgrad(x.data_ptr(), x.data_ptr(), 0, H, W, C, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.float()).all()) and bool((dw == 0).all()) and bool((db == 0).all())
    # bad shapes: VAH_E_SHAPE (-2) before anything is launched
    for b, h, w, c in ((-1, H, W, C), (1, 3, W, C), (1, H, 3, C), (1, 0, W, C), (1, H, W, 6), (1, H, W, 0), (1, H, W, 1028)):
        assert fwd(x.data_ptr(), w9.data_ptr(), bias.data_ptr(), b, h, w, c, 0, y.data_ptr(), st) == -2, (b, h, w, c)
        assert wgrad(x.data_ptr(), x.data_ptr(), b, h, w, c, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st) == -2, (b, h, w, c)
    # null pointers: VAH_E_NULL (-1); a misaligned activation pointer: VAH_E_ALIGN (-4)
    assert fwd(None, w9.data_ptr(), bias.data_ptr(), 1, H, W, C, 0, y.data_ptr(), st) == -1
    assert wgrad(x.data_ptr(), None, 1, H, W, C, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st) == -1
    assert fwd(x.data_ptr() + 2, w9.data_ptr(), bias.data_ptr(), 1, H, W, C, 0, y.data_ptr(), st) == -4
    assert wgrad(x.data_ptr() + 2, x.data_ptr(), 1, H, W, C, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st) == -4
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.float()).all())
