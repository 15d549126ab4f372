"""GPU: the fused MSDeformAttn core held to fp64 (oracle/msda_fused.py) in the forms the model runs.

Direct calls of the C entry points (vah_msda_fused_forward, vah_msda_fused_forward_win, vah_msda_fused_backward_tiled,
vah_msda_fused_backward), one call per entry point and case, every output and every workspace filled with NaN / 0xFF
bytes first: the header says workspace contents are arbitrary and every result is fully written.

Forms (oracle.msda_fused.FORMS): F1 is what vitadapter/fused.py::_MSDAPairCore launches under bf16 autocast - bf16 values,
fp32 offsets and logits read in place from one interleaved matrix (row stride 3*L*P, logits = offsets + 2*L*P), bf16
gradients written with the same strides; F1p the same with padded rows whose gap words must come back untouched; F2 - F5
the contiguous dtype combinations.  Cases (oracle.msda_fused.CASES; DESIGN.md has the table): ragged maps, 3 and 4
levels, shared lists, rows spread beyond the binning window, more tiles / groups / queries than the fast paths of the
schedule and the binning pass hold, hand-placed border samples, levels that do not tile the value rows, an invalid level.

Checked: out; grad_value and d_logits at every element; d_offsets where the sample is more than 1e-3 px away from a kink
(tests/test_msda_fused_oracle_cpu.py pins the reference, the mask and what the inputs reach).  Bounds:
oracle.msda_fused.bounds.  Run with -s for one FIGURE line per checked tensor."""
import functools
import types

import pytest
import torch

from oracle import msda_fused as mfo

pytestmark = pytest.mark.gpu

_DT = {torch.float32: 0, torch.bfloat16: 1}
E_UNSUPPORTED = -3
HALO = 5                                    # ops.functions.ms_deform_attn_fused.WIN_HALO
FIRST = ['ext_ragged', 'inj_ragged', 'four_levels']
NON_TILING = ['non_tiling_trailing_rows', 'non_tiling_gap_between_levels', 'non_tiling_overlapping_levels']

FORWARD = ([(c, f) for c in FIRST for f in ('F1', 'F1p', 'F2', 'F3', 'F4', 'F5')] +
           [(c, 'F1') for c in ['inj_ragged_ref3', 'shared_lists', 'wide_rows', 'many_tiles', 'long_queries', 'many_groups',
                                'borders'] + NON_TILING])
TILED = ([(c, f) for c in FIRST for f in ('F1', 'F1p', 'F2', 'F3', 'F4', 'F5')] +
         [(c, 'F1') for c in ['inj_ragged_ref3', 'shared_lists', 'wide_rows', 'many_tiles', 'borders'] + NON_TILING] +
         [(c, 'F4') for c in NON_TILING])
ATOMICS = [(c, f) for c in ('ext_ragged', 'inj_ragged') for f in ('F2', 'F4')]


def _vah():
    import _vah
    return _vah


def _stream():
    return _vah().raw_stream(torch.device('cuda'))


def _nan(shape, dtype):
    return torch.full(tuple(shape), float('nan'), dtype=dtype, device='cuda')


def _nan_bytes(n):
    return torch.full((max(int(n), 1),), 255, dtype=torch.uint8, device='cuda')     # 0xFF..: NaN as fp32 and as bf16


def _call(name, *args):
    v = _vah()
    with v.on(torch.device('cuda')):
        rc = getattr(v.lib, name)(*args)
    v.check(rc, name)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _case(case, form, seed=0, backward=True):
    """(inputs, reference), computed once per (case, form, seed) and shared by the tests; never modified."""
    inp = mfo.inputs(case, form, seed)
    return inp, mfo.reference(inp, backward=backward and not inp.forward_only)


def _dev(inp):
    """The operands on the GPU.  off / logit: device pointers; os / ls: row strides as the ABI takes them."""
    N, M, D, P, Lq, L, S = inp.dims
    d = types.SimpleNamespace(value=inp.value.cuda(), gout=inp.grad_out.cuda(), ref=inp.ref.cuda().contiguous(),
                              shapes=inp.shapes.cuda(), lsi=inp.lsi.cuda())
    if inp.params is not None:
        d.params = inp.params.cuda()
        d.off = d.params.data_ptr()
        d.logit = d.off + 2 * L * P * d.params.element_size()
        d.os = d.ls = inp.stride
    else:
        d.offsets, d.logits = inp.offsets.cuda(), inp.logits.cuda()
        d.off, d.logit, d.os, d.ls = d.offsets.data_ptr(), d.logits.data_ptr(), 0, 0
    return d


def _forward(inp, d):
    N, M, D, P, Lq, L, S = inp.dims
    out = _nan((N, Lq, M * D), inp.f.value)
    _call('vah_msda_fused_forward', d.value.data_ptr(), _DT[inp.f.value], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit,
          _DT[inp.f.param], d.os, d.ls, d.ref.data_ptr(), inp.ref_levels, N, S, M, D, L, Lq, P, out.data_ptr(), _stream())
    return out


def _forward_win(inp, d, ws, holds_schedule):
    N, M, D, P, Lq, L, S = inp.dims
    out = _nan((N, Lq, M * D), inp.f.value)
    _call('vah_msda_fused_forward_win', d.value.data_ptr(), _DT[inp.f.value], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off,
          d.logit, _DT[inp.f.param], d.os, d.ls, d.ref.data_ptr(), N, S, M, D, Lq, P, HALO, ws.data_ptr(), ws.numel(),
          int(holds_schedule), out.data_ptr(), _stream())
    return out


def _win_ws(inp):
    N, M, D, P, Lq, L, S = inp.dims
    n = _vah().lib.vah_msda_win_ws_bytes(S, Lq)
    assert n > 0
    return _nan_bytes(n)


def _grad_outputs(inp):
    """NaN-filled d_offsets / d_logits in the layout of the form -> (holder, d_off ptr, d_logit ptr, dos, dls, views)."""
    N, M, D, P, Lq, L, S = inp.dims
    f = inp.f
    if f.interleaved:
        esz = 2 if f.gparam == torch.bfloat16 else 4
        g = _nan_bytes(N * Lq * M * inp.stride * esz).view(f.gparam).view(N, Lq, M, inp.stride)
        return g, g.data_ptr(), g.data_ptr() + 2 * L * P * esz, inp.stride, inp.stride, mfo.param_views(g, L)
    d_off, d_logit = _nan((N, Lq, M, L, P, 2), f.gparam), _nan((N, Lq, M, L * P), f.gparam)
    return None, d_off.data_ptr(), d_logit.data_ptr(), 0, 0, (d_off, d_logit)


def _backward_tiled(inp, d):
    N, M, D, P, Lq, L, S = inp.dims
    f = inp.f
    gv = _nan((N, S, M, D), f.gv)
    g, d_off_p, d_logit_p, dos, dls, (d_off, d_logit) = _grad_outputs(inp)
    ws_bytes = _vah().lib.vah_msda_tile_ws_bytes(N, S, M, L, Lq, P)
    assert ws_bytes > 0
    ws = _nan_bytes(ws_bytes)
    _call('vah_msda_fused_backward_tiled', d.value.data_ptr(), _DT[f.value], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit,
          _DT[f.param], d.os, d.ls, d.ref.data_ptr(), inp.ref_levels, d.gout.data_ptr(), N, S, M, D, L, Lq, P, gv.data_ptr(),
          _DT[f.gv], d_off_p, d_logit_p, _DT[f.gparam], dos, dls, ws.data_ptr(), ws_bytes, _stream())
    return gv, d_off, d_logit, g


def _check_backward(tag, inp, want, gv, d_off, d_logit, rules):
    mfo.check(tag + ' grad_value', gv, want.grad_value, rules['grad_value'], abs_gv=want.abs_gv)
    mfo.check(tag + ' d_logits', d_logit, want.d_logits, rules['d_logits'])
    mfo.check(tag + ' d_offsets', d_off, want.d_offsets, rules['d_offsets'], mask=mfo.smooth_mask(inp))


@pytest.mark.parametrize('case,form', FORWARD)
def test_forward(case, form):
    """vah_msda_fused_forward on every case; on the single-level ones vah_msda_fused_forward_win as well: once building
    its schedule, then with new offsets and logits on the untouched workspace."""
    inp, want = _case(case, form)
    d = _dev(inp)
    rule = mfo.bounds(form)['out']
    tag = '%s %s' % (case, form)
    mfo.check(tag + ' out (8-lane)', _forward(inp, d), want.out, rule)
    if len(inp.levels) > 1:
        return
    ws = _win_ws(inp)
    mfo.check(tag + ' out (windows)', _forward_win(inp, d, ws, False), want.out, rule)
    held = ws.clone()
    inp2, want2 = _case(case, form, 1, False)
    assert torch.equal(inp2.ref, inp.ref) and not torch.equal(inp2.logits, inp.logits)
    mfo.check(tag + ' out (windows, schedule reused)', _forward_win(inp2, _dev(inp2), ws, True), want2.out, rule)
    assert torch.equal(ws, held), 'the forward kernel wrote to its workspace'


@pytest.mark.parametrize('case,form', TILED)
def test_backward_tiled(case, form):
    inp, want = _case(case, form)
    d = _dev(inp)
    gv, d_off, d_logit, g = _backward_tiled(inp, d)
    _check_backward('%s %s tiled' % (case, form), inp, want, gv, d_off, d_logit, mfo.bounds(form))
    if inp.f.pad:
        gap = g[..., inp.stride - inp.f.pad:].contiguous().view(torch.int16)
        assert bool((gap == -1).all()), 'the gap words between the rows of the gradient matrix were written'
        assert bool(torch.isnan(d.params[..., inp.stride - inp.f.pad:]).all())


@pytest.mark.parametrize('case,form', ATOMICS)
def test_backward_atomics(case, form):
    """vah_msda_fused_backward, the fallback of the tile pass: fp32 grad_value, zero on entry, one float atomic per sample,
    corner and channel; d_offsets / d_logits in the parameter dtype."""
    inp, want = _case(case, form)
    d = _dev(inp)
    N, M, D, P, Lq, L, S = inp.dims
    f = inp.f
    gv = torch.zeros((N, S, M, D), dtype=torch.float32, device='cuda')
    d_off, d_logit = _nan((N, Lq, M, L, P, 2), f.param), _nan((N, Lq, M, L * P), f.param)
    _call('vah_msda_fused_backward', d.value.data_ptr(), _DT[f.value], d.shapes.data_ptr(), d.lsi.data_ptr(), d.off, d.logit,
          _DT[f.param], d.ref.data_ptr(), inp.ref_levels, d.gout.data_ptr(), N, S, M, D, L, Lq, P, gv.data_ptr(),
          d_off.data_ptr(), d_logit.data_ptr(), _stream())
    par = 'bf16' if f.param == torch.bfloat16 else 'f32'
    _check_backward('%s %s atomics' % (case, form), inp, want, gv, d_off, d_logit,
                    dict(grad_value='f32', d_offsets=par, d_logits=par))


@pytest.mark.parametrize('form,stride', [('F4', 12), ('F5', 16)])
def test_strided_gradients_of_fp32_values_are_refused(form, stride):
    """include/vitadapter_hip.h: with strides the gradient kernels of fp32 values are not available."""
    inp, _ = _case('ext_ragged', form)
    d = _dev(inp)
    N, M, D, P, Lq, L, S = inp.dims
    f = inp.f
    esz = 2 if f.param == torch.bfloat16 else 4
    par = torch.zeros((N, Lq, M, stride), dtype=f.param, device='cuda')
    g = _nan((N, Lq, M, stride), f.gparam)
    gv = _nan((N, S, M, D), f.gv)
    lib = _vah().lib
    ws_bytes = lib.vah_msda_tile_ws_bytes(N, S, M, L, Lq, P)
    ws = _nan_bytes(ws_bytes)
    rc = lib.vah_msda_fused_backward_tiled(
        d.value.data_ptr(), _DT[f.value], d.shapes.data_ptr(), d.lsi.data_ptr(), par.data_ptr(), par.data_ptr() + 2 * L * P * esz,
        _DT[f.param], stride, stride, d.ref.data_ptr(), 1, d.gout.data_ptr(), N, S, M, D, L, Lq, P, gv.data_ptr(), _DT[f.gv],
        g.data_ptr(), g.data_ptr() + 2 * L * P * esz, _DT[f.gparam], stride, stride, ws.data_ptr(), ws_bytes, _stream())
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED, (rc, lib.vah_last_error())
    assert bool(torch.isnan(gv).all()) and bool(torch.isnan(g).all())


@pytest.mark.parametrize('case', ['invalid_level_rows', 'invalid_level_h0'])
def test_invalid_level_contributes_nothing(case):
    """A level that is no window of the value rows (start + H*W > S; H = 0): both forward entry points return VAH_OK with
    out exactly zero - the window forward also on a workspace that holds such a schedule - and the tiled backward
    returns grad_value, d_offsets and d_logits exactly zero."""
    inp = mfo.inputs(case, 'F1')
    d = _dev(inp)

    def zero(name, t):
        assert bool((t == 0).all()), '%s: %d of %d elements are not zero' % (name, int((t != 0).sum()), t.numel())

    zero('out (8-lane)', _forward(inp, d))
    ws = _win_ws(inp)
    zero('out (windows)', _forward_win(inp, d, ws, False))
    zero('out (windows, schedule reused)', _forward_win(inp, d, ws, True))
    gv, d_off, d_logit, _ = _backward_tiled(inp, d)
    zero('grad_value', gv)
    zero('d_offsets', d_off)
    zero('d_logits', d_logit)


def test_python_layer_launches_the_same_call():
    """ops.functions.ms_deform_attn_fused.fused_forward on views of one interleaved matrix (what _MSDAPairCore hands it):
    the same bits as the direct call."""
    from ops.functions import ms_deform_attn_fused as mf
    assert mf.WIN_HALO == HALO
    inp, _ = _case('ext_ragged', 'F1')
    d = _dev(inp)
    N, M, D, P, Lq, L, S = inp.dims
    offsets, logits = mfo.param_views(d.params, L)
    assert mf.window_forward(L, P, inp.ref_levels, Lq)
    got = mf.fused_forward(d.value, d.shapes, d.lsi, offsets, logits, inp.stride, inp.stride, d.ref)
    torch.cuda.synchronize()
    want = _forward_win(inp, d, _win_ws(inp), False)
    assert torch.equal(got, want), '%d elements differ' % int((got != want).sum())
