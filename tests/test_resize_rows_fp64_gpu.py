"""GPU: the bilinear resize kernels on channels-last rows (csrc/resize_rows.hip, include/vitadapter_hip_resize.h) against
the fp64 restatement of tests/resize_rows_ref.py, called through the C ABI.

Budgets per element, A = sum |w| |v| of its terms, n = the number of terms of an adjoint element (the last term of each is
absent for fp32 outputs):
    forward   16 * 2^-24 * A + half a rounding unit of the output dtype at |ref|
    adjoint   (n + 16) * 2^-24 * A + the output's rounding unit at |ref|
The taps are bit-identical to the restatement's (un-contracted fp32 operations), so nothing is allowed for them.  Each
test prints its worst error / budget ratio.

Every output is pre-filled with NaN and sits between guard rows that must stay bit-unchanged; the strided form is the
middle level of a three-level (Lq, N, C) buffer whose other levels are NaN and must stay bit-unchanged."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_rows_ref as ref  # noqa: E402
import _vah  # noqa: E402

pytestmark = pytest.mark.gpu

lib = _vah.lib
CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
NAMES = {torch.float32: 'fp32', torch.bfloat16: 'bf16', torch.float16: 'fp16'}
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FWD_FORMS = [(F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16)]          # x -> y
BWD_FORMS = [(F32, F32), (BF16, F32), (F16, F32), (BF16, BF16), (F16, F16)]          # dy -> dx
CHANNELS = (8, 72, 256)
BATCHES = (1, 3)
GUARD = 3          # rows before and after an output
U24 = 2.0 ** -24


def dev():
    return torch.device('cuda:0')


def _arg(t):
    n, rows, c = t.shape
    return t.data_ptr(), CODES[t.dtype], (t.stride(1) if rows > 1 else c), (t.stride(0) if n > 1 else 0)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _level(rows, n, c, dtype, fill=None):
    """-> buf (7 + rows + 5, n, c) NaN-filled, and its middle level seen as (n, rows, c); ``fill`` (n, rows, c) goes there"""
    buf = torch.full((7 + rows + 5, n, c), float('nan'), dtype=dtype, device=dev())
    view = buf[7:7 + rows].permute(1, 0, 2)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _guarded(n, rows, c, dtype):
    """-> buf ((GUARD + n * rows + GUARD) * c,) NaN-filled, and the contiguous (n, rows, c) view between the guards"""
    buf = torch.full(((2 * GUARD + n * rows) * c,), float('nan'), dtype=dtype, device=dev())
    return buf, buf[GUARD * c:(GUARD + n * rows) * c].view(n, rows, c)


def _run(entry, src, dst, n, c, hw_in, hw_out, align):
    nws = lib.vah_resize_rows_ws_bytes(*hw_in, *hw_out)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev())
    fn = getattr(lib, entry)
    _vah.check(fn(*_arg(src), n, c, *hw_in, *hw_out, int(align), *_arg(dst), ws.data_ptr(), nws, _vah.raw_stream(dev())), entry)
    torch.cuda.synchronize()


def forward(x, hw_in, hw_out, align, ydt, strided_out=False):
    """x (N, Hi * Wi, C) cuda rows (any served layout) -> y, checked for untouched surroundings"""
    n, _, c = x.shape
    rows = hw_out[0] * hw_out[1]
    buf, y = _level(rows, n, c, ydt) if strided_out else _guarded(n, rows, c, ydt)
    before = _bits(buf).clone()
    _run('vah_resize_rows_forward', x, y, n, c, hw_in, hw_out, align)
    _surroundings_unchanged(buf, before, rows, n, c, strided_out)
    return y


def backward(dy, hw_in, hw_out, align, xdt, strided_out=False):
    n, _, c = dy.shape
    rows = hw_in[0] * hw_in[1]
    buf, dx = _level(rows, n, c, xdt) if strided_out else _guarded(n, rows, c, xdt)
    before = _bits(buf).clone()
    _run('vah_resize_rows_backward', dy, dx, n, c, hw_in, hw_out, align)
    _surroundings_unchanged(buf, before, rows, n, c, strided_out)
    return dx


def _surroundings_unchanged(buf, before, rows, n, c, strided):
    after = _bits(buf)
    if strided:
        assert torch.equal(after[:7], before[:7]) and torch.equal(after[7 + rows:], before[7 + rows:]), 'another level was written'
    else:
        assert torch.equal(after[:GUARD * c], before[:GUARD * c]), 'guard rows before the output were written'
        assert torch.equal(after[(GUARD + n * rows) * c:], before[(GUARD + n * rows) * c:]), 'guard rows after the output were written'


def _data(n, rows, c, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, rows, c, generator=gen).to(dtype)


def _ratio(got, want, budget):
    got = got.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), 'a NaN of the pre-fill is left, or a non-finite result'
    return float((np.abs(got - want) / np.maximum(budget, 1e-300)).max())


@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('hw_in,hw_out', ref.SHAPES)
def test_forward_against_fp64(hw_in, hw_out, align):
    worst = {True: 0.0, False: 0.0}           # fp32 outputs, 16-bit outputs
    for c in CHANNELS:
        for n in BATCHES:
            for xdt in (F32, BF16, F16):
                x_cpu = _data(n, hw_in[0] * hw_in[1], c, xdt, 7 * c + n)
                want, a = ref.forward(x_cpu.float().numpy(), hw_in, hw_out, align)
                x_flat = x_cpu.to(dev())
                lvl, x_lvl = _level(x_cpu.shape[1], n, c, xdt, fill=x_flat)
                lvl_before = _bits(lvl).clone()
                for ydt in [y for x_, y in FWD_FORMS if x_ == xdt]:
                    budget = 16 * U24 * a + 0.5 * ref.rounding_unit(want, NAMES[ydt])
                    y = forward(x_flat, hw_in, hw_out, align, ydt)
                    r = _ratio(y, want, budget)
                    assert r <= 1.0, (c, n, xdt, ydt, 'contiguous', r)
                    y2 = forward(x_lvl, hw_in, hw_out, align, ydt)
                    assert torch.equal(_bits(y2), _bits(y)), (c, n, xdt, ydt, 'the strided input gives other bits')
                    y3 = forward(x_flat, hw_in, hw_out, align, ydt)
                    assert torch.equal(_bits(y3), _bits(y)), (c, n, xdt, ydt, 'two runs differ')
                    worst[ydt == F32] = max(worst[ydt == F32], r)
                assert torch.equal(_bits(lvl), lvl_before), 'the input buffer was written'
    print('resize_rows_fwd %s -> %s align %d: worst error / budget %.3f (fp32 outputs), %.3f (16-bit outputs)'
          % (hw_in, hw_out, align, worst[True], worst[False]))


@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('hw_in,hw_out', ref.SHAPES)
def test_adjoint_against_fp64(hw_in, hw_out, align):
    worst = {True: 0.0, False: 0.0}
    for c in CHANNELS:
        for n in BATCHES:
            for gdt in (F32, BF16, F16):
                g_cpu = _data(n, hw_out[0] * hw_out[1], c, gdt, 11 * c + n)
                want, a, terms = ref.adjoint(g_cpu.float().numpy(), hw_in, hw_out, align)
                g_flat = g_cpu.to(dev())
                lvl, g_lvl = _level(g_cpu.shape[1], n, c, gdt, fill=g_flat)
                for xdt in [x for g_, x in BWD_FORMS if g_ == gdt]:
                    budget = (terms[None, :, None] + 16) * U24 * a + ref.rounding_unit(want, NAMES[xdt])
                    dx = backward(g_flat, hw_in, hw_out, align, xdt)
                    r = _ratio(dx, want, budget)
                    assert r <= 1.0, (c, n, gdt, xdt, 'contiguous', r)
                    # untapped inputs: zeros over the NaN pre-fill
                    assert (dx[:, torch.as_tensor(terms == 0)] == 0).all()
                    for dy_, strided in ((g_lvl, False), (g_flat, True), (g_flat, False)):       # strided dy; strided dx; again
                        dx2 = backward(dy_, hw_in, hw_out, align, xdt, strided_out=strided)
                        assert torch.equal(_bits(dx2), _bits(dx)), (c, n, gdt, xdt, strided, 'other bits')
                    worst[xdt == F32] = max(worst[xdt == F32], r)
    print('resize_rows_bwd %s -> %s align %d: worst error / budget %.3f (fp32 outputs), %.3f (16-bit outputs)'
          % (hw_in, hw_out, align, worst[True], worst[False]))


def _maps(rows, hw):
    n, _, c = rows.shape
    return rows.reshape(n, hw[0], hw[1], c).permute(0, 3, 1, 2)


def _rows(maps):
    n, c, h, w = maps.shape
    return maps.permute(0, 2, 3, 1).reshape(n, h * w, c)


def _torch_pair(x, dy, hw_in, hw_out, align):
    """F.interpolate and its autograd on the GPU, fp32, as rows"""
    x = x.detach().clone().requires_grad_(True)
    y = _rows(F.interpolate(_maps(x, hw_in), size=hw_out, mode='bilinear', align_corners=align))
    y.backward(dy)
    return y.detach(), x.grad


@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('hw_in,hw_out', ref.SHAPES)
def test_against_torch_on_the_gpu(hw_in, hw_out, align):
    """fp32, within the bound tests/test_resize_rows_ref_cpu.py holds the restatement to: torch may contract src differently"""
    n, c = 3, 8
    x = _data(n, hw_in[0] * hw_in[1], c, F32, 5).to(dev())
    dy = _data(n, hw_out[0] * hw_out[1], c, F32, 6).to(dev())
    ty, tdx = _torch_pair(x, dy, hw_in, hw_out, align)
    k = 2.0 * 2.0 ** -23 * max(hw_in) + 16 * U24
    _, a = ref.forward(x.cpu().numpy(), hw_in, hw_out, align)
    r1 = _ratio(forward(x, hw_in, hw_out, align, F32), ty.cpu().numpy().astype(np.float64), k * a)
    _, a, _ = ref.adjoint(dy.cpu().numpy(), hw_in, hw_out, align)
    r2 = _ratio(backward(dy, hw_in, hw_out, align, F32), tdx.cpu().numpy().astype(np.float64), k * a)
    print('against torch %s -> %s align %d: forward %.3f adjoint %.3f of the bound' % (hw_in, hw_out, align, r1, r2))
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)


def test_production_case():
    """100 x 168 -> 200 x 336, C 256, N 1: fp32 -> bf16 forward from the strided level, bf16 -> fp32 adjoint"""
    hw_in, hw_out, c = (100, 168), (200, 336), 256
    x_cpu = _data(1, hw_in[0] * hw_in[1], c, F32, 1)
    want, a = ref.forward(x_cpu.numpy(), hw_in, hw_out, False)
    _, x_lvl = _level(x_cpu.shape[1], 1, c, F32, fill=x_cpu.to(dev()))
    y = forward(x_lvl, hw_in, hw_out, False, BF16)
    r1 = _ratio(y, want, 16 * U24 * a + 0.5 * ref.rounding_unit(want, 'bf16'))
    g_cpu = _data(1, hw_out[0] * hw_out[1], c, BF16, 2)
    want, a, terms = ref.adjoint(g_cpu.float().numpy(), hw_in, hw_out, False)
    dx = backward(g_cpu.to(dev()), hw_in, hw_out, False, F32)
    r2 = _ratio(dx, want, (terms[None, :, None] + 16) * U24 * a)
    assert torch.equal(_bits(backward(g_cpu.to(dev()), hw_in, hw_out, False, F32)), _bits(dx))
    print('production case: forward %.3f adjoint %.3f of the budget' % (r1, r2))
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)


@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('value', [float('inf'), float('nan')])
@pytest.mark.parametrize('where', ['corner', 'interior'])
def test_nonfinite_positions_are_torchs(where, value, align):
    """one inf / NaN in x (in dy): the non-finite positions of y (of dx) are those of F.interpolate (its autograd) in
    fp32 - a tap with weight zero still multiplies"""
    hw_in, hw_out, n, c = (16, 24), (33, 49), 1, 8
    x = _data(n, hw_in[0] * hw_in[1], c, F32, 3).to(dev())
    dy = _data(n, hw_out[0] * hw_out[1], c, F32, 4).to(dev())
    x[0, 0 if where == 'corner' else 5 * hw_in[1] + 7, 2] = value
    dy[0, hw_out[0] * hw_out[1] - 1 if where == 'corner' else 11 * hw_out[1] + 20, 5] = value
    ty, tdx = _torch_pair(x, dy, hw_in, hw_out, align)
    y = forward(x, hw_in, hw_out, align, F32)
    dx = backward(dy, hw_in, hw_out, align, F32)
    assert (~torch.isfinite(ty)).any() and (~torch.isfinite(tdx)).any()
    assert torch.equal(~torch.isfinite(y), ~torch.isfinite(ty))
    assert torch.equal(~torch.isfinite(dx), ~torch.isfinite(tdx))


def test_fp16_store_overflows_to_inf():
    hw_in, hw_out, c = (2, 2), (3, 3), 8
    x = torch.full((1, 4, c), 60000.0, device=dev())
    x[0, 3] = 70000.0                                    # blends of 60000 and 70000: some above 65504, all finite in fp32
    want, _ = ref.forward(x.cpu().numpy(), hw_in, hw_out, False)
    y = forward(x, hw_in, hw_out, False, F16)
    over = torch.as_tensor(want > 65520.0)
    assert over.any() and not over.all()
    assert torch.isinf(y.cpu()[over]).all() and torch.isfinite(y.cpu()[~over]).all()
    g = torch.full((1, 9, c), 30000.0, dtype=F16, device=dev())
    dx = backward(g, hw_in, hw_out, False, F16)           # every input pixel collects 2.25 * 30000
    assert torch.isinf(dx).all()
    assert torch.isfinite(backward(g, hw_in, hw_out, False, F32)).all()
