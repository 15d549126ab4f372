"""CPU: the point-sampling / match-cost entry points (include/vitadapter_hip_points.h, csrc/point_loss.hip), their binding table
(_vah.POINTS_SIGNATURES) and the host-side argument checks.

The prototypes are held to the binding with the method of tests/test_masked_attn_abi_cpu.py, applied to the sixth header and
the sixth table; the other tables stay what they were.  Every call here is answered by the host-side validation before
anything touches a device (fake or null pointers that are never dereferenced)."""
import ctypes
import os
import re

import pytest

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_points.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
A = 4096           # a non-null, 16-byte aligned fake pointer
F32, U8 = 0, 3
NAMES = ('vah_pts_sample', 'vah_pts_match_cost')
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}


def _err():
    return lib.vah_last_error().decode()


def _param(text):
    if '*' in text:
        return ctypes.c_void_p
    words = text.replace('const', '').split()
    assert len(words) == 2 and words[0] in SCALARS, 'parameter the test cannot read: %r' % text
    return SCALARS[words[0]]


def _prototypes():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r'\b(int64_t|int)\s*(vah_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        assert name not in out, name
        out[name] = (SCALARS[ret], [_param(p.strip()) for p in ' '.join(params.split()).split(',')])
    return out


def sample(maps=A, dt=F32, ms=160 * 160, rs=160, M=200, h=160, w=160, points=A, S=2, P=12544, map_idx=None, set_idx=A, R=200, out=A):
    return lib.vah_pts_sample(maps, dt, ms, rs, M, h, w, points, S, P, map_idx, set_idx, R, out, None)


def cost(xs=A, ts=A, off=A, cls=A, labels=A, N=2, Q=100, C1=151, G=24, Gmax=12, P=12544, out=A):
    return lib.vah_pts_match_cost(xs, ts, off, cls, labels, N, Q, C1, G, Gmax, P, 2.0, 5.0, 5.0, 1.0, out, None)


CALLS = {'vah_pts_sample': sample, 'vah_pts_match_cost': cost}
# every pointer argument of each call: (keyword, may be null)
POINTERS = {
    'vah_pts_sample': [('maps', False), ('points', False), ('map_idx', True), ('set_idx', True), ('out', False)],
    'vah_pts_match_cost': [(k, False) for k in ('xs', 'ts', 'off', 'cls', 'labels', 'out')],
}
EMPTY = {'vah_pts_sample': dict(R=0), 'vah_pts_match_cost': dict(Gmax=0, G=0)}


def test_every_signature_matches_its_prototype():
    protos = _prototypes()
    assert set(protos) == set(_vah.POINTS_SIGNATURES) == set(NAMES)
    for name, (restype, params) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        assert list(fn.argtypes) == list(_vah.POINTS_SIGNATURES[name][1]) == params, name


@pytest.mark.parametrize('name', NAMES)
def test_library_exports_the_symbol(name):
    assert hasattr(ctypes.CDLL(_vah.LIB_PATH), name), name


def test_the_other_tables_are_untouched():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION
    assert len(_vah.EXPORTS) == 122 and len(_vah.SIGNATURES) == 79 and len(_vah.F16_TWINS) == 43
    assert len(_vah.GN_SIGNATURES) == 6 and len(_vah.BOX_SIGNATURES) == 2 and len(_vah.RESIZE_SIGNATURES) == 3
    assert len(_vah.MCA_SIGNATURES) == 5
    others = (set(_vah.EXPORTS) | set(_vah.BOX_SIGNATURES) | set(_vah.GN_SIGNATURES) | set(_vah.RESIZE_SIGNATURES)
              | set(_vah.MCA_SIGNATURES))
    assert not set(_vah.POINTS_SIGNATURES) & others
    for header in ('vitadapter_hip.h', 'vitadapter_hip_msda_box.h', 'vitadapter_hip_group_norm.h', 'vitadapter_hip_resize.h',
                   'vitadapter_hip_masked_attn.h'):
        text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        assert 'vah_pts' not in text, header


def test_the_header_states_the_contracts():
    text = ' '.join(open(HEADER).read().split())
    for words in ('every element written', 'No atomics', 'the same inputs give the same bits', 'in ascending order',
                  '+inf', 'x first', 'not binary', '3 uint8'):
        assert ' '.join(words.split()) in text.replace('* ', ''), words


@pytest.mark.parametrize('name', NAMES)
def test_null_pointers_and_empty_calls(name):
    call = CALLS[name]
    for kw, optional in POINTERS[name]:
        if not optional:
            assert call(**{kw: None}) == E_NULL, (kw, _err())
            assert 'null' in _err() and name in _err()
    # nothing to write is not an error, and no pointer is read
    nothing = {kw: None for kw, _ in POINTERS[name]}
    assert call(**nothing, **EMPTY[name]) == OK and _err() == ''


@pytest.mark.parametrize('name', NAMES)
def test_p_must_be_positive_also_where_there_is_nothing_to_do(name):
    call = CALLS[name]
    for P in (0, -1):
        assert call(P=P) == E_SHAPE and 'P must be positive' in _err() and name in _err()
        assert call(P=P, **EMPTY[name]) == E_SHAPE
    assert call(P=1 << 31) == E_SHAPE and 'bad dims' in _err()


def test_sample_point_index_stays_in_int():
    """a thread of the sample kernel forms p + 3 * 256 in int: P is bounded so that it cannot wrap"""
    assert sample(P=(1 << 31) - 1023) == E_SHAPE and 'bad dims' in _err()
    assert sample(P=(1 << 31) - 1024, out=None) == E_NULL


def test_dtype_codes():
    for dt in (1, 2, 4, -1):
        assert sample(dt=dt) == E_UNSUPPORTED and 'dtype codes' in _err()
        assert sample(dt=dt, R=0) == E_UNSUPPORTED
    # a uint8 map asks no alignment, an fp32 map 4 bytes
    assert sample(dt=U8, maps=A + 1, out=None) == E_NULL and '(out)' in _err()
    assert sample(dt=F32, maps=A + 1) == E_ALIGN and 'maps' in _err()


def test_bad_dims():
    for kw in (dict(R=-1), dict(S=-1), dict(M=-1), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 16), dict(rs=159), dict(ms=-1),
               dict(h=1 << 20, rs=1 << 20, w=4)):
        assert sample(**kw) == E_SHAPE, (kw, _err())
    for kw in (dict(N=-1), dict(Q=-1), dict(C1=-1), dict(G=-1), dict(Gmax=-1), dict(Gmax=25), dict(C1=0), dict(N=1 << 20, Q=1 << 20)):
        assert cost(**kw) == E_SHAPE, (kw, _err())


def test_identity_rows_out_of_range_are_seen_on_the_host():
    assert sample(map_idx=None, R=201) == E_SHAPE and 'index out of range' in _err()
    assert sample(map_idx=A, set_idx=None, R=3) == E_SHAPE and 'index out of range' in _err()
    assert sample(map_idx=None, set_idx=None, R=2, out=None) == E_NULL                     # in range: passes up to the last check


@pytest.mark.parametrize('name', NAMES)
def test_alignment(name):
    call = CALLS[name]
    wide = {'points': 8, 'labels': 8}
    for kw, _ in POINTERS[name]:
        need = wide.get(kw, 4)
        for off in (1, 2) + ((4,) if need == 8 else ()):
            assert call(**{kw: A + off}) == E_ALIGN, (kw, off, _err())
            assert 'misaligned' in _err() and name in _err()
        last = [k for k, opt in POINTERS[name] if not opt and k != kw][-1]
        assert call(**{kw: A + need, last: None}) == E_NULL, (kw, _err())       # aligned enough: the call goes on to the null
