"""CPU: the rules of the bias-partials registry (vitadapter/fused.py::_BiasPartials).  A kernel that writes the dY of a
Linear leaves the partial column sums of dY there; the Linear's backward may take them only when its gradient IS that
tensor - same storage, offset, element count, row width, contiguous, unchanged since - because a wrong hit is a wrong
bias gradient and a miss only costs the column-sum launch it would have saved.  No device is touched: the partial rows
are stand-in tensors."""
import pytest
import torch

import _vah
from vitadapter import fused


def _entry(reg, dz, nparts=3):
    bpart = torch.zeros(nparts, dz.shape[-1])
    reg.record(dz, bpart, nparts)
    return bpart


def test_hit_needs_the_same_bytes_cpu():
    reg = fused._BiasPartials()
    dz = torch.randn(2, 6, 8).to(torch.bfloat16)
    bpart = _entry(reg, dz)
    got = reg.take(dz.view(12, 8))                  # what _LinearBF16.backward makes of the incoming gradient
    assert got is not None and got[0] is bpart and got[1] == 3
    assert reg.take(dz.view(12, 8)) is None, 'an entry serves one Linear and is dropped'
    for name, other in (('clone', dz.clone().view(12, 8)),
                        ('other row width', dz.view(6, 16)),
                        ('part of the rows', dz.view(12, 8)[2:]),
                        ('not contiguous', dz.view(12, 8)[:, :4]),
                        ('another dtype', dz.view(12, 8).float())):
        _entry(reg, dz)
        assert reg.take(other) is None, name
    # the tensor itself still hits after all those misses: a miss leaves the entry alone
    assert reg.take(dz.view(-1, 8)) is not None


def test_square_transpose_made_contiguous_misses_cpu():
    reg = fused._BiasPartials()
    dz = torch.randn(8, 8).to(torch.bfloat16)
    _entry(reg, dz)
    assert reg.take(dz.t()) is None                       # same storage, offset, shape and count - other element order
    assert reg.take(dz.t().contiguous()) is None
    assert reg.take(dz) is not None


def test_in_place_edit_misses_cpu():
    reg = fused._BiasPartials()
    dz = torch.randn(4, 8).to(torch.bfloat16)
    _entry(reg, dz)
    dz.view(-1)[0] += 1                                   # through a view: the version counter is shared
    assert reg.take(dz) is None
    _entry(reg, dz)                                       # recorded again at the new version: a hit again
    assert reg.take(dz) is not None


def test_no_partials_is_a_miss_cpu():
    reg = fused._BiasPartials()
    dz = torch.randn(4, 8).to(torch.bfloat16)
    reg.record(dz, torch.zeros(0, 8), 0)                  # rows == 0 kernels report *nparts = 0
    assert reg.take(dz) is None


def test_a_live_entry_pins_the_address_cpu():
    """The key is an address: the entry keeps dz alive, so no other tensor can appear at it while the entry exists."""
    reg = fused._BiasPartials()
    dz = torch.randn(64, 8).to(torch.bfloat16)
    ptr = dz.data_ptr()
    _entry(reg, dz)
    del dz
    others = [torch.randn(64, 8).to(torch.bfloat16) for _ in range(8)]
    assert all(o.data_ptr() != ptr for o in others)
    assert all(reg.take(o) is None for o in others)


class _Producer(torch.autograd.Function):
    """Stands for a kernel that writes dz in a backward pass and records its partials."""

    @staticmethod
    def forward(ctx, x, reg, seen):
        ctx.reg, ctx.seen = reg, seen
        return x * 2

    @staticmethod
    def backward(ctx, g):
        dz = (g * 2).to(torch.bfloat16)
        ctx.reg.record(dz, torch.zeros(1, dz.shape[-1]), 1)
        ctx.seen.append(len(ctx.reg.passes[None]))
        return dz.float(), None, None


def test_entries_vanish_with_the_pass_and_the_epoch_cpu():
    reg, seen = fused._BiasPartials(), []
    x = torch.randn(4, 8, requires_grad=True)
    _Producer.apply(x, reg, seen).sum().backward()
    assert seen == [1], 'the entry existed inside the pass'
    assert reg.passes == {}, 'and the engine callback dropped it, unconsumed, at the end of the pass'
    _Producer.apply(x, reg, seen).sum().backward()        # a second pass arms its own callback
    assert seen == [1, 1] and reg.passes == {}
    # recorded outside any backward pass (no callback can be queued): the next epoch clears
    dz = torch.randn(4, 8).to(torch.bfloat16)
    _entry(reg, dz)
    assert reg.passes[None]
    reg.begin_epoch()
    assert reg.passes == {} and reg.take(dz) is None


def test_forward_epoch_clears_the_module_registry():
    """forward_epoch reaches begin_epoch only on the bf16 GPU path; begin_epoch itself is what it calls."""
    dz = torch.randn(4, 8).to(torch.bfloat16)
    _entry(fused.BIAS_PARTIALS, dz)
    try:
        assert fused.BIAS_PARTIALS.take(dz.clone()) is None
        fused.BIAS_PARTIALS.begin_epoch()
        assert fused.BIAS_PARTIALS.passes == {}
    finally:
        fused.BIAS_PARTIALS.begin_epoch()


def test_switch_turns_tagging_off_cpu():
    reg = fused.BIAS_PARTIALS
    lin = torch.nn.Linear(8, 8)
    assert fused.ENABLED['bias_partials'] is True
    y = torch.randn(3, 8).to(torch.bfloat16)
    assert not reg.wanted(y)
    assert reg.mark(y, lin.bias) is y and reg.wanted(y)
    assert not reg.wanted(reg.mark(torch.randn(3, 8), lin.bias)), 'bf16 only'
    assert not reg.wanted(reg.mark(torch.randn(3, 12).to(torch.bfloat16), lin.bias)), 'rows of 16-byte multiples only'
    assert not reg.wanted(reg.mark(torch.randn(3, 8).to(torch.bfloat16), None)), 'no bias: nothing to sum'
    frozen = torch.nn.Linear(8, 8)
    frozen.bias.requires_grad_(False)
    assert not reg.wanted(reg.mark(torch.randn(3, 8).to(torch.bfloat16), frozen.bias))
    with torch.no_grad():
        assert not reg.wanted(reg.mark(torch.randn(3, 8).to(torch.bfloat16), lin.bias))
    fused.ENABLED['bias_partials'] = False
    try:
        assert not reg.wanted(y), 'a mark made earlier is not honoured either'
        assert not reg.wanted(reg.mark(torch.randn(3, 8).to(torch.bfloat16), lin.bias))
    finally:
        fused.ENABLED['bias_partials'] = True


def test_cpu_tensors_take_the_torch_expressions():
    lin, act, norm = torch.nn.Linear(8, 16), torch.nn.GELU(), torch.nn.LayerNorm(8)
    x = torch.randn(2, 3, 8)
    y = fused.linear(lin, x)
    assert torch.equal(y, lin(x)) and not hasattr(y, fused._BiasPartials.ATTR)
    h = torch.randn(2, 3, 16, requires_grad=True)
    assert torch.equal(fused.gelu(act, h), act(h))
    # a marked bf16 tensor on the CPU still takes the module: the kernel path needs a device and bf16 autocast
    hb = fused.BIAS_PARTIALS.mark(torch.randn(2, 3, 16).to(torch.bfloat16).requires_grad_(True), lin.bias)
    out = fused.gelu(act, hb)
    assert torch.equal(out, act(hb)) and out.grad_fn.name().startswith('Gelu')
    assert torch.equal(fused.gelu(torch.nn.GELU(approximate='tanh'), h), torch.nn.functional.gelu(h, approximate='tanh'))
    assert torch.equal(fused.gelu(torch.nn.ReLU(), h), torch.relu(h))
    z = fused.BIAS_PARTIALS.mark(torch.randn(2, 3, 8).to(torch.bfloat16), lin.bias)
    t, hh = fused.residual_ln(x, z, None, None, norm)
    assert torch.equal(t, x + z) and torch.equal(hh, norm(x + z))
    assert torch.equal(fused.residual(x, z), x + z)
    assert fused.BIAS_PARTIALS.passes == {}


def test_new_entry_points_are_bf16_only_additions():
    new = ('vah_residual_layernorm_bwd_bsum', 'vah_scale_residual_bwd_bsum', 'vah_gelu_bwd_bsum_bf16')
    for n in new:
        assert n in _vah.EXPORTS and n not in _vah.FUSED_F16_TWINS and n + '_f16' not in _vah.EXPORTS
    assert len(_vah.FUSED_F16_TWINS) == 10 and _vah.lib.vah_abi_version() == 37


P = 4096           # a non-null, 16-byte aligned fake pointer: never dereferenced by a rejected call
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4


def _res_ln(fn, extra, t=P, gh=P, z=P, gamma=None, dgamma=None, batch=2, rpb=4, C=64, dz=P, dw=P):
    return fn(t, gh, P, P, P, None, z, gamma, None, batch, rpb, C, P, dz, dgamma, dw, P, P, *extra, None)


def _sr(fn, extra, g=P, z=P, gamma=None, batch=2, rpb=4, C=64, dz=P, dgamma=None, ws=None):
    return fn(g, z, gamma, None, batch, rpb, C, dz, dgamma, ws, *extra, None)


@pytest.mark.parametrize('call,parent,bsum,cases', [
    (_res_ln, 'vah_residual_layernorm_bwd', 'vah_residual_layernorm_bwd_bsum', [
        dict(rpb=-1), dict(z=None), dict(dz=None), dict(gamma=P), dict(dgamma=P), dict(dz=P + 2), dict(C=66),
        dict(dw=None), dict(gh=P + 4)]),
    (_sr, 'vah_scale_residual_bwd', 'vah_scale_residual_bwd_bsum', [
        dict(rpb=-1), dict(C=6), dict(dz=None), dict(gamma=P, dgamma=P), dict(dz=P + 4), dict(g=P + 8)]),
], ids=['residual_layernorm', 'scale_residual'])
def test_bsum_entries_reject_what_their_parents_reject(call, parent, bsum, cases):
    """Null and misaligned arguments fail as the parent entry's do: same code, same message, the name changed.  All are
    rejected before anything touches a device."""
    import ctypes
    lib = _vah.lib
    for kw in cases:
        n = ctypes.c_int64(-1)
        rc_p = call(getattr(lib, parent), (), **kw)
        msg_p = lib.vah_last_error().decode()
        rc_b = call(getattr(lib, bsum), (P, ctypes.byref(n)), **kw)
        msg_b = lib.vah_last_error().decode()
        assert rc_p != 0 and rc_b == rc_p, (kw, rc_p, rc_b, msg_b)
        assert msg_b == msg_p.replace(parent + ':', bsum + ':'), (kw, msg_p, msg_b)


def test_bsum_entries_own_argument_checks():
    import ctypes
    lib = _vah.lib
    n = ctypes.c_int64(-1)
    ok = (P, ctypes.byref(n))
    # a layer scale beside the LayerNorm form is refused with its own message
    rc = _res_ln(lib.vah_residual_layernorm_bwd_bsum, ok, gamma=P, dgamma=P)
    assert rc == E_SHAPE and b'vah_residual_layernorm_bwd_bsum' in lib.vah_last_error() and b'gamma' in lib.vah_last_error()
    for fn, call in ((lib.vah_residual_layernorm_bwd_bsum, _res_ln), (lib.vah_scale_residual_bwd_bsum, _sr)):
        assert call(fn, (None, ctypes.byref(n))) == E_NULL
        assert call(fn, (P, None)) == E_NULL
        assert call(fn, (P + 8, ctypes.byref(n))) == E_ALIGN
    # no rows: nothing is launched and no partial row is promised
    n.value = -1
    assert _sr(lib.vah_scale_residual_bwd_bsum, ok, g=None, z=None, dz=None, batch=0) == 0 and n.value == 0
    g = lib.vah_gelu_bwd_bsum_bf16
    n.value = -1
    assert g(None, None, 0, 64, None, P, ctypes.byref(n), None) == 0 and n.value == 0
    assert g(P, P, 4, 60, P, P, ctypes.byref(n), None) == E_SHAPE          # C % 8
    assert g(P, P, -1, 64, P, P, ctypes.byref(n), None) == E_SHAPE
    assert g(P, None, 4, 64, P, P, ctypes.byref(n), None) == E_NULL
    assert g(P, P, 4, 64, P, None, ctypes.byref(n), None) == E_NULL
    assert g(P, P, 4, 64, P, P, None, None) == E_NULL
    assert g(P + 8, P, 4, 64, P, P, ctypes.byref(n), None) == E_ALIGN
    assert g(P, P, 4, 64, P + 8, P, ctypes.byref(n), None) == E_ALIGN
