"""CPU: the GroupNorm entry points (include/vitadapter_hip_group_norm.h, csrc/group_norm.hip), their binding table
(_vah.GN_SIGNATURES) and the host-side argument checks.

The prototypes are held to the binding with the method of tests/test_binding_table_cpu.py, applied to the third header
and the third table; the primary header's tables and the box table stay what they were (122 / 79 / 43, ABI version 37:
adding symbols does not move it).  Every call here is answered by the host-side validation before anything touches a
device (fake, aligned pointers that are never dereferenced), as in tests/test_abi_errors_cpu.py."""
import ctypes
import os
import re

import pytest

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_group_norm.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
F32, BF16, F16 = 0, 1, 2
N, T, C, G = 2, 100, 256, 32
NAMES = ('vah_group_norm_supported', 'vah_group_norm_ws_floats', 'vah_group_norm_stats', 'vah_group_norm_apply',
         'vah_group_norm_bwd_stats', 'vah_group_norm_bwd_apply')
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


def _ws(N=N, T=T, C=C, G=G):
    return lib.vah_group_norm_ws_floats(N, T, C, G)


def _stats(x=P, dt=BF16, rs=C, is_=T * C, N=N, T=T, C=C, G=G, mean=P, rstd=P, ws=P, ws_floats=None, **_):
    return lib.vah_group_norm_stats(x, dt, rs, is_, N, T, C, G, 1e-5, mean, rstd, ws, _ws(N, T, C, G) if ws_floats is None else ws_floats, None)


def _apply(x=P, dt=BF16, rs=C, is_=T * C, N=N, T=T, C=C, G=G, mean=P, rstd=P, add=None, y=P, ydt=BF16, yrs=C, yis=T * C, **_):
    return lib.vah_group_norm_apply(x, dt, rs, is_, N, T, C, G, mean, rstd, P, P, 1, add, y, ydt, yrs, yis, None)


def _bwd_stats(x=P, dt=BF16, rs=C, is_=T * C, N=N, T=T, C=C, G=G, mean=P, rstd=P, ws=P, ws_floats=None, y=P, ydt=BF16, yrs=C,
               yis=T * C, gsums=P, **_):
    return lib.vah_group_norm_bwd_stats(x, dt, rs, is_, y, ydt, yrs, yis, N, T, C, G, mean, rstd, P, P, 1, gsums, P, P, ws,
                                        _ws(N, T, C, G) if ws_floats is None else ws_floats, None)


def _bwd_apply(x=P, dt=BF16, rs=C, is_=T * C, N=N, T=T, C=C, G=G, mean=P, rstd=P, y=P, ydt=BF16, yrs=C, yis=T * C, gsums=P, dx=P,
               dxdt=BF16, **_):
    return lib.vah_group_norm_bwd_apply(x, dt, rs, is_, y, ydt, yrs, yis, N, T, C, G, mean, rstd, P, P, 1, gsums, dx, dxdt, C, T * C, None)


CALLS = {'vah_group_norm_stats': _stats, 'vah_group_norm_apply': _apply, 'vah_group_norm_bwd_stats': _bwd_stats,
         'vah_group_norm_bwd_apply': _bwd_apply}
KERNELS = tuple(CALLS)


def test_every_signature_matches_its_prototype():
    assert set(PROTOTYPES) == set(_vah.GN_SIGNATURES) == set(NAMES)
    for name, (restype, params) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        got = list(fn.argtypes or [])
        assert got == list(_vah.GN_SIGNATURES[name][1])
        assert len(got) == len(params), (name, len(got), len(params))
        for i, (g, allowed) in enumerate(zip(got, params)):
            assert g in allowed, (name, i, g, allowed)


@pytest.mark.parametrize('name', NAMES)
def test_library_exports_the_symbol(name):
    assert hasattr(ctypes.CDLL(_vah.LIB_PATH), name), name


def test_the_other_tables_are_untouched():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION
    assert len(_vah.EXPORTS) == 122 and len(_vah.SIGNATURES) == 79 and len(_vah.F16_TWINS) == 43
    assert set(_vah.BOX_SIGNATURES) == {'vah_msda_fused_forward_box', 'vah_msda_fused_backward_tiled_box'}
    assert not set(_vah.GN_SIGNATURES) & (set(_vah.EXPORTS) | set(_vah.BOX_SIGNATURES))
    for header in ('vitadapter_hip.h', 'vitadapter_hip_msda_box.h'):
        text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        assert 'vah_group_norm' not in text, header


def test_supported_shapes():
    for c in (64, 128, 256, 512):
        for cpg in (1, 2, 4, 8):
            assert lib.vah_group_norm_supported(c, c // cpg) == 1, (c, cpg)
            assert lib.vah_group_norm_ws_floats(1, 1, c, c // cpg) > 0
    for c, g in ((32, 32), (1024, 128), (96, 12), (192, 24), (256, 16), (256, 8), (256, 0), (256, 3), (0, 1), (64, 128)):
        assert lib.vah_group_norm_supported(c, g) == 0, (c, g)
        assert lib.vah_group_norm_ws_floats(2, 100, c, g) == 0
    assert lib.vah_group_norm_ws_floats(0, 100, 256, 32) == 0 and lib.vah_group_norm_ws_floats(2, 0, 256, 32) == 0
    # the workspace grows with the rows of an image up to the cap on the partial rows, then stays
    assert _ws(1, 64) == 2 * C and _ws(1, 65) == 2 * 2 * C and _ws(1, 1 << 20) == _ws(1, 1 << 21) == 512 * 2 * C


@pytest.mark.parametrize('name', KERNELS)
def test_bad_dims_and_unserved_shapes(name):
    call = CALLS[name]
    for kw in (dict(N=-1), dict(T=-1), dict(C=0), dict(G=0), dict(N=1 << 20)):
        assert call(**kw) == E_SHAPE, (kw, _err())
        assert name in _err() and 'bad dims' in _err()
    for kw in (dict(C=256, G=16), dict(C=32, G=32), dict(C=1024, G=128), dict(C=192, G=24), dict(C=256, G=5)):
        assert call(**kw) == E_UNSUPPORTED, (kw, _err())
        assert 'C / G' in _err()
    assert call(T=0, C=256, G=16) == E_UNSUPPORTED                   # also where there is nothing to do
    assert call(dt=3) == E_UNSUPPORTED and 'dtype codes' in _err()
    if name != 'vah_group_norm_stats':
        assert call(dt=F16, ydt=BF16) == E_UNSUPPORTED and 'fp16 mixed with bf16' in _err()
    if name == 'vah_group_norm_bwd_apply':
        assert call(dt=F32, ydt=BF16, dxdt=F16) == E_UNSUPPORTED and 'fp16 mixed with bf16' in _err()


@pytest.mark.parametrize('name', KERNELS)
def test_null_pointers_and_empty_calls(name):
    call = CALLS[name]
    assert call(x=None) == E_NULL and 'null' in _err() and name in _err()
    assert call(mean=None) == E_NULL and 'null' in _err()
    assert call(rstd=None) == E_NULL
    if name != 'vah_group_norm_stats':
        assert call(y=None) == E_NULL and 'null' in _err()
    if 'stats' in name:
        assert call(ws=None) == E_NULL and 'ws' in _err()
    if 'bwd' in name:
        assert call(gsums=None) == E_NULL
    if name == 'vah_group_norm_bwd_apply':
        assert call(dx=None) == E_NULL
    # N * T == 0: nothing to do is not an error, and no pointer is read
    assert call(N=0, x=None, mean=None, rstd=None, y=None) == OK and _err() == ''
    assert call(T=0, x=None, mean=None, rstd=None, y=None) == OK


@pytest.mark.parametrize('name', KERNELS)
def test_alignment_and_strides(name):
    call = CALLS[name]
    for kw in (dict(x=P + 8), dict(x=P + 2), dict(rs=C + 4), dict(is_=T * C + 2)):
        assert call(**kw) == E_ALIGN, (kw, _err())
        assert 'misaligned' in _err() and name in _err()
    if name != 'vah_group_norm_stats':
        assert call(y=P + 8) == E_ALIGN and call(yrs=C + 4) == E_ALIGN and call(yis=T * C + 4) == E_ALIGN
    if name == 'vah_group_norm_apply':
        assert call(add=P + 8) == E_ALIGN and 'add' in _err()
    assert call(rs=C - 8) == E_SHAPE and 'strides' in _err()
    # the strided forms pass: a level's rows of an (Lq, N, C) buffer
    assert call(rs=N * C, is_=C, mean=None) == E_NULL


@pytest.mark.parametrize('name', ['vah_group_norm_stats', 'vah_group_norm_bwd_stats'])
@pytest.mark.parametrize('dims', [(1, 1), (1, 67200), (3, 65), (2, 100)])
def test_workspace_one_float_short(name, dims):
    n, t = dims
    need = _ws(n, t)
    assert need > 0
    kw = dict(N=n, T=t, is_=t * C, yis=t * C) if name.endswith('bwd_stats') else dict(N=n, T=t, is_=t * C)
    assert CALLS[name](ws_floats=need - 1, **kw) == E_SHAPE, _err()
    assert 'workspace too small' in _err()
