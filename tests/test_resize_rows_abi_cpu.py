"""CPU: the resize entry points (include/vitadapter_hip_resize.h, csrc/resize_rows.hip), their binding table
(_vah.RESIZE_SIGNATURES) and the host-side argument checks.

The prototypes are held to the binding with the method of tests/test_group_norm_abi_cpu.py, applied to the fourth header
and the fourth table; the other tables stay what they were.  Every call here is answered by the host-side validation
before anything touches a device (fake or null pointers that are never dereferenced)."""
import ctypes
import os
import re

import pytest

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_resize.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
F32, BF16, F16 = 0, 1, 2
N, C, HI, WI, HO, WO = 2, 256, 10, 12, 20, 25
NAMES = ('vah_resize_rows_ws_bytes', 'vah_resize_rows_forward', 'vah_resize_rows_backward')
KERNELS = NAMES[1:]
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}


def _err():
    return lib.vah_last_error().decode()


def _param(text):
    if '*' in text:
        return (ctypes.c_void_p,)
    words = text.replace('const', '').split()
    assert len(words) == 2 and words[0] in SCALARS, 'parameter the test cannot read: %r' % text
    return (SCALARS[words[0]],)


def _prototypes():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r'\b(int64_t|int)\s*(vah_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        params = ' '.join(params.split())
        assert name not in out, name
        out[name] = (SCALARS[ret], [_param(p.strip()) for p in params.split(',')])
    return out


PROTOTYPES = _prototypes()


def _call(name, a=P, adt=F32, ars=None, ais=None, N=N, C=C, Hi=HI, Wi=WI, Ho=HO, Wo=WO, align=0, b=P, bdt=BF16, brs=None, bis=None,
          ws=P, ws_bytes=None):
    """a: the tensor read (x / dy), b: the one written (y / dx)"""
    fwd = name.endswith('forward')
    ta, tb = (Hi * Wi, Ho * Wo) if fwd else (Ho * Wo, Hi * Wi)
    ars = C if ars is None else ars
    brs = C if brs is None else brs
    ais = ta * C if ais is None else ais
    bis = tb * C if bis is None else bis
    ws_bytes = lib.vah_resize_rows_ws_bytes(Hi, Wi, Ho, Wo) if ws_bytes is None else ws_bytes
    return getattr(lib, name)(a, adt, ars, ais, N, C, Hi, Wi, Ho, Wo, align, b, bdt, brs, bis, ws, ws_bytes, None)


def test_every_signature_matches_its_prototype():
    assert set(PROTOTYPES) == set(_vah.RESIZE_SIGNATURES) == set(NAMES)
    for name, (restype, params) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        got = list(fn.argtypes or [])
        assert got == list(_vah.RESIZE_SIGNATURES[name][1])
        assert len(got) == len(params), (name, len(got), len(params))
        for i, (g, allowed) in enumerate(zip(got, params)):
            assert g in allowed, (name, i, g, allowed)


@pytest.mark.parametrize('name', NAMES)
def test_library_exports_the_symbol(name):
    assert hasattr(ctypes.CDLL(_vah.LIB_PATH), name), name


def test_the_other_tables_are_untouched():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION
    assert len(_vah.EXPORTS) == 122 and len(_vah.SIGNATURES) == 79 and len(_vah.F16_TWINS) == 43
    assert len(_vah.GN_SIGNATURES) == 6 and len(_vah.BOX_SIGNATURES) == 2
    assert not set(_vah.RESIZE_SIGNATURES) & (set(_vah.EXPORTS) | set(_vah.BOX_SIGNATURES) | set(_vah.GN_SIGNATURES))
    for header in ('vitadapter_hip.h', 'vitadapter_hip_msda_box.h', 'vitadapter_hip_group_norm.h'):
        text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        assert 'vah_resize' not in text, header


def test_workspace_size():
    # 16 bytes per output row and column, 8 per input row and column; nothing for an empty side
    assert lib.vah_resize_rows_ws_bytes(HI, WI, HO, WO) == 16 * (HO + WO) + 8 * (HI + WI)
    assert lib.vah_resize_rows_ws_bytes(1, 1, 1, 1) == 48
    for dims in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-1, 1, 1, 1)):
        assert lib.vah_resize_rows_ws_bytes(*dims) == 0


@pytest.mark.parametrize('name', KERNELS)
def test_bad_dims_and_unserved_shapes(name):
    for kw in (dict(N=-1), dict(C=0), dict(Hi=-1), dict(Wi=-2), dict(Ho=-1), dict(Wo=-1), dict(N=1 << 20), dict(Ho=1 << 31),
               dict(Ho=1 << 20, Wo=1 << 20)):
        assert _call(name, **kw) == E_SHAPE, (kw, _err())
        assert name in _err() and 'bad dims' in _err()
    # an empty source for a non-empty result
    empty_src = dict(Hi=0) if name.endswith('forward') else dict(Wo=0)
    assert _call(name, **empty_src) == E_SHAPE and 'bad dims' in _err()
    for c in (4, 12, 250, 257):
        assert _call(name, C=c) == E_UNSUPPORTED, (c, _err())
        assert 'multiple of 8' in _err()
    assert _call(name, C=12, N=0) == E_UNSUPPORTED                      # also where there is nothing to do
    assert _call(name, adt=3) == E_UNSUPPORTED and 'dtype codes' in _err()
    assert _call(name, bdt=-1) == E_UNSUPPORTED
    for adt, bdt in ((F16, BF16), (BF16, F16)):
        assert _call(name, adt=adt, bdt=bdt) == E_UNSUPPORTED and 'fp16 mixed with bf16' in _err()
    for adt, bdt in ((F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16), (BF16, F32), (F16, F32)):
        assert _call(name, adt=adt, bdt=bdt, ws=None) == E_NULL, (adt, bdt)    # passes every check up to the last


@pytest.mark.parametrize('name', KERNELS)
def test_null_pointers_and_empty_calls(name):
    assert _call(name, a=None) == E_NULL and 'null' in _err() and name in _err()
    assert _call(name, b=None) == E_NULL and 'null' in _err()
    assert _call(name, ws=None) == E_NULL and 'ws' in _err()
    # nothing to write is not an error, and no pointer is read
    assert _call(name, N=0, a=None, b=None, ws=None, ws_bytes=0) == OK and _err() == ''
    empty = (dict(Ho=0), dict(Wo=0)) if name.endswith('forward') else (dict(Hi=0), dict(Wi=0))
    for kw in empty:
        assert _call(name, a=None, b=None, ws=None, ws_bytes=0, **kw) == OK, (kw, _err())
        assert _call(name, a=P + 2, b=P + 2, ars=3, ws=None, ws_bytes=0, **kw) == OK


@pytest.mark.parametrize('name', KERNELS)
def test_alignment_strides_and_workspace(name):
    for kw in (dict(a=P + 8), dict(a=P + 2), dict(ars=C + 4), dict(ais=HI * WI * C * 4 + 2), dict(b=P + 8), dict(brs=C + 4),
               dict(bis=C + 4), dict(ws=P + 8)):
        assert _call(name, **kw) == E_ALIGN, (kw, _err())
        assert 'misaligned' in _err() and name in _err()
    assert _call(name, ars=C - 8) == E_SHAPE and 'strides' in _err()
    assert _call(name, brs=C - 8) == E_SHAPE and 'strides' in _err()
    need = lib.vah_resize_rows_ws_bytes(HI, WI, HO, WO)
    assert _call(name, ws_bytes=need - 1) == E_SHAPE and 'workspace too small' in _err()
    assert _call(name, ws_bytes=0) == E_SHAPE
    # the strided forms pass every check: a level's rows of an (Lq, N, C) buffer, on either side
    assert _call(name, ars=N * C, ais=C, ws=None) == E_NULL and 'ws' in _err()
    assert _call(name, brs=N * C, bis=C, ws=None) == E_NULL and 'ws' in _err()
