"""CPU: the two entry points of the fused MSDeformAttn core that take reference BOXES (include/vitadapter_hip_msda_box.h:
vah_msda_fused_forward_box, vah_msda_fused_backward_tiled_box - the *_nref signatures plus one int64 ref_comps directly
after ref_batch), their binding table (_vah.BOX_SIGNATURES) and the host gate ref_points_ok.

The prototypes are held to the binding with the method of tests/test_binding_table_cpu.py, applied to the second header
and the second table; the primary header's tables stay what they were (122 / 79 / 43, ABI version 37: adding symbols
does not move it).  Every call here is answered by the host-side validation before anything touches a device (fake,
aligned pointers that are never dereferenced), as in tests/test_abi_errors_cpu.py."""
import ctypes
import os
import re

import pytest
import torch

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_msda_box.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
N, S, M, D, L, LQ, PTS = 2, 64, 2, 32, 1, 8, 4
F32, BF16, F16 = 0, 1, 2
NAMES = ('vah_msda_fused_forward_box', 'vah_msda_fused_backward_tiled_box')
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}


def _err():
    return lib.vah_last_error().decode()


def _param(text):
    """One parameter of a prototype -> the ctypes types the binding may declare for it."""
    if '*' in text:
        base = text[:text.index('*')].replace('const', '').strip()
        if base == 'char':
            return (ctypes.c_char_p,)
        if base == 'int64_t':
            return (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64))
        return (ctypes.c_void_p,)
    words = text.replace('const', '').split()
    assert len(words) == 2 and words[0] in SCALARS, 'parameter the test cannot read: %r' % text
    return (SCALARS[words[0]],)


def _prototypes():
    """{name: (restype, [allowed argtypes per position], parameter text)} of every vah_* prototype of the box header."""
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)
    out = {}
    for ret, name, params in re.findall(r'\b(int64_t|int)\s*(vah_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        params = ' '.join(params.split())
        assert name not in out, name
        out[name] = (SCALARS[ret], [_param(p.strip()) for p in params.split(',')], params)
    return out


PROTOTYPES = _prototypes()


def _forward(comps=4, ref=P, N=N, D=D, L=L, Lq=LQ, pts=PTS, v=BF16, p=F32, value=P):
    return lib.vah_msda_fused_forward_box(value, v, P, P, P, P, p, 0, 0, ref, 1, 1, comps, N, S, M, D, L, Lq, pts, P, None)


def _tiled(comps=4, ref=P, N=N, D=D, L=L, Lq=LQ, pts=PTS, v=BF16, p=F32, gv=BF16, gp=BF16, ws_bytes=1 << 30, value=P, os_=0):
    return lib.vah_msda_fused_backward_tiled_box(value, v, P, P, P, P, p, os_, 0, ref, 1, 1, comps, P, N, S, M, D, L, Lq, pts,
                                                 P, gv, P, P, gp, 0, 0, P, ws_bytes, None)


CALLS = {'vah_msda_fused_forward_box': _forward, 'vah_msda_fused_backward_tiled_box': _tiled}


def test_every_box_signature_matches_its_prototype():
    assert set(PROTOTYPES) == set(_vah.BOX_SIGNATURES) == set(NAMES)
    for name, (restype, params, _) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        got = list(fn.argtypes or [])
        assert got == list(_vah.BOX_SIGNATURES[name][1])
        assert len(got) == len(params), (name, len(got), len(params))
        for i, (g, allowed) in enumerate(zip(got, params)):
            assert g in allowed, (name, i, g, allowed)


@pytest.mark.parametrize('name', NAMES)
def test_library_exports_the_symbol_with_ref_comps_after_ref_batch(name):
    raw = ctypes.CDLL(_vah.LIB_PATH)
    assert hasattr(raw, name), name
    assert re.search(r'int64_t ref_levels,\s*int64_t ref_batch,\s*int64_t ref_comps,', PROTOTYPES[name][2]), PROTOTYPES[name][2]
    # the *_nref signature plus that one argument
    twin = name.replace('_box', '_nref')
    want = list(_vah.SIGNATURES[twin][1])
    got = list(_vah.BOX_SIGNATURES[name][1])
    at = 12          # value, dtype, shapes, lsi, offsets, logits, dtype, 2 strides, ref, ref_levels, ref_batch | ref_comps
    assert got[:at] == want[:at] and got[at] is ctypes.c_int64 and got[at + 1:] == want[at:], name


def test_the_primary_tables_are_untouched():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION
    assert len(_vah.EXPORTS) == 122 and len(_vah.SIGNATURES) == 79 and len(_vah.F16_TWINS) == 43
    assert not set(_vah.BOX_SIGNATURES) & set(_vah.EXPORTS)
    primary = open(os.path.join(ROOT, 'include', 'vitadapter_hip.h')).read()
    assert not re.search(r'vah_msda_fused_\w+_box\s*\(', re.sub(r'/\*.*?\*/', '', primary, flags=re.S))


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('comps', [3, 0, 1, 8, -4])
def test_ref_comps_must_be_two_or_four(name, comps):
    assert CALLS[name](comps=comps) == E_SHAPE, _err()
    assert 'ref_comps' in _err() and name in _err(), _err()
    assert CALLS[name](comps=comps, Lq=0, ref=None) == E_SHAPE          # also where there is nothing to do


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('comps', [2, 4])
def test_null_pointers_and_empty_calls(name, comps):
    assert CALLS[name](comps=comps, ref=None) == E_NULL and 'null' in _err()
    assert CALLS[name](comps=comps, value=None) == E_NULL and 'null' in _err()
    # N * Lq * M == 0: nothing to do is not an error, and no pointer is read
    assert CALLS[name](comps=comps, Lq=0, ref=None, value=None) == OK
    assert CALLS[name](comps=comps, N=0, ref=None, value=None) == OK


@pytest.mark.parametrize('name', NAMES)
def test_boxes_must_be_16_byte_aligned(name):
    assert CALLS[name](comps=4, ref=P + 8) == E_ALIGN, _err()
    assert 'misaligned' in _err() and name in _err()
    assert CALLS[name](comps=4, ref=P + 4) == E_ALIGN
    # points keep the 8-byte rule of the *_nref entry points: P + 8 passes the alignment checks, and the call is stopped by a
    # later host-side one (a misaligned offsets stride)
    if name == 'vah_msda_fused_forward_box':
        assert lib.vah_msda_fused_forward_box(P, BF16, P, P, P, P, BF16, 18, 18, P + 8, 1, 1, 2, N, S, M, D, L, LQ, PTS, P, None) == E_ALIGN
    else:
        assert _tiled(comps=2, ref=P + 8, p=BF16, os_=20) == E_ALIGN
    assert 'strides' in _err(), _err()


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('comps', [2, 4])
def test_shapes_outside_the_fused_core_are_refused(name, comps):
    call = CALLS[name]
    assert call(comps=comps, D=48) == E_UNSUPPORTED, _err()
    assert 'D == 32 or D == 64' in _err()
    assert call(comps=comps, pts=8) == E_UNSUPPORTED, _err()
    assert call(comps=comps, L=5) == E_UNSUPPORTED, _err()
    for v, p in ((F16, BF16), (F16, F32), (BF16, F16), (F32, F16)):
        assert call(comps=comps, v=v, p=p) == E_UNSUPPORTED, ((v, p), _err())
        assert 'fp16' in _err()


@pytest.mark.parametrize('comps', [2, 4])
@pytest.mark.parametrize('D', [32, 64])
def test_workspace_one_byte_short(comps, D):
    need = lib.vah_msda_tile_ws_bytes(N, S, M * (D // 32), L, LQ, PTS)
    assert need > 0
    for v, p, gv, gp in ((F32, F32, F32, F32), (BF16, BF16, BF16, BF16), (BF16, F32, BF16, BF16), (F16, F16, F16, F16)):
        assert _tiled(comps=comps, D=D, v=v, p=p, gv=gv, gp=gp, ws_bytes=need - 1) == E_SHAPE, ((v, p), _err())
        assert 'workspace too small' in _err()


def _ref(shape, grad=False):
    return torch.zeros(shape, requires_grad=grad)


def test_ref_points_ok_takes_boxes_under_the_rules_of_points():
    from ops.functions.ms_deform_attn_fused import ref_points_ok
    n, lq, levels = 2, 5, 3
    for comps in (2, 4):
        for rl in (1, levels):
            assert ref_points_ok(_ref((1, lq, rl, comps)), n, levels)
            assert ref_points_ok(_ref((n, lq, rl, comps)), n, levels)
            assert ref_points_ok(_ref((1, lq, rl, comps), grad=True), n, levels)         # a shared grid never had a gradient
            assert not ref_points_ok(_ref((n, lq, rl, comps), grad=True), n, levels)     # learned per image: unfused
            with torch.no_grad():
                assert ref_points_ok(_ref((n, lq, rl, comps), grad=True), n, levels)
        assert not ref_points_ok(_ref((n, lq, 2, comps)), n, levels)                     # levels: 1 or L
        assert not ref_points_ok(_ref((3, lq, 1, comps)), n, levels)                     # batch: 1 or N
        assert not ref_points_ok(_ref((lq, 1, comps)), n, levels)
    for comps in (1, 3, 5, 8):
        assert not ref_points_ok(_ref((1, lq, 1, comps)), n, levels)


def test_module_still_raises_for_other_last_dimensions():
    """MSDeformAttn.forward on CPU tensors: a last dimension other than 2 or 4 reaches the module's own ValueError."""
    from ops.modules import MSDeformAttn
    mod = MSDeformAttn(d_model=64, n_levels=1, n_heads=2, n_points=4)
    shapes, lsi = torch.tensor([[2, 2]]), torch.tensor([0])
    with pytest.raises(ValueError, match='Last dim of reference_points must be 2 or 4'):
        mod(torch.zeros(1, 3, 64), torch.zeros(1, 3, 1, 3), torch.zeros(1, 4, 64), shapes, lsi)


def test_window_forward_is_never_chosen_for_boxes():
    from ops.functions.ms_deform_attn_fused import window_forward
    if os.environ.get('VAH_MSDA_FWD_WIN', '1') != '0':
        assert window_forward(1, 4, 1, 100, 1) and window_forward(1, 4, 1, 100, 1, 2)
    assert not window_forward(1, 4, 1, 100, 1, 4)
