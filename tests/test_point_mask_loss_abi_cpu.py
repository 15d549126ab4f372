"""CPU: the sampled-mask-loss entry points (include/vitadapter_hip_point_mask_loss.h, csrc/point_mask_loss.hip), their binding
table (_vah.PML_SIGNATURES) and the host-side argument checks.

The method of tests/test_points_abi_cpu.py, applied to the eighth header and its table; the other tables stay what they were.
Every call here is answered by the host-side validation before anything touches a device (fake or null pointers that are
never dereferenced)."""
import ctypes
import os
import re

import pytest

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_point_mask_loss.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
A = 4096           # a non-null, 16-byte aligned fake pointer
F32, U8 = 0, 3
NAMES = ('vah_pml_ws_bytes', 'vah_pml_forward', 'vah_pml_backward')
CALLED = NAMES[1:]
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}
BIG = 1 << 40


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


def forward(pred=A, pms=160 * 160, prs=160, Mp=200, h=160, w=160, tgt=A, dt=U8, tms=640 * 640, trs=640, Mt=24, H=640, W=640, points=A,
            P=12544, rows=A, tgt_rows=A, K=24, bce=A, dice=A, xs=A, ts=A, sums=A, ws=A, ws_bytes=BIG):
    return lib.vah_pml_forward(pred, pms, prs, Mp, h, w, tgt, dt, tms, trs, Mt, H, W, points, P, rows, tgt_rows, K, 1.0, bce, dice, xs, ts,
                               sums, ws, ws_bytes, None)


def backward(points=A, xs=A, ts=A, sums=A, g_bce=A, g_dice=A, K=24, P=12544, h=160, w=160, dmaps=A, ws=A, ws_bytes=BIG):
    return lib.vah_pml_backward(points, xs, ts, sums, g_bce, g_dice, K, P, h, w, 1.0, dmaps, ws, ws_bytes, None)


CALLS = {'vah_pml_forward': forward, 'vah_pml_backward': backward}
# every pointer argument of each call: (keyword, may be null)
POINTERS = {
    'vah_pml_forward': [('pred', False), ('tgt', False), ('points', False), ('rows', True), ('tgt_rows', True), ('bce', False),
                        ('dice', False), ('xs', False), ('ts', False), ('sums', False), ('ws', False)],
    'vah_pml_backward': [(k, False) for k in ('points', 'xs', 'ts', 'sums', 'g_bce', 'g_dice', 'dmaps', 'ws')],
}


def test_every_signature_matches_its_prototype():
    protos = _prototypes()
    assert set(protos) == set(_vah.PML_SIGNATURES) == set(NAMES)
    for name, (restype, params) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        assert list(fn.argtypes) == list(_vah.PML_SIGNATURES[name][1]) == params, name


@pytest.mark.parametrize('name', NAMES)
def test_library_exports_the_symbol(name):
    assert hasattr(ctypes.CDLL(_vah.LIB_PATH), name), name


def test_the_other_tables_are_untouched():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION
    assert len(_vah.EXPORTS) == 122 and len(_vah.SIGNATURES) == 79 and len(_vah.F16_TWINS) == 43
    assert len(_vah.GN_SIGNATURES) == 6 and len(_vah.BOX_SIGNATURES) == 2 and len(_vah.RESIZE_SIGNATURES) == 3
    assert len(_vah.MCA_SIGNATURES) == 5 and len(_vah.POINTS_SIGNATURES) == 2 and len(_vah.SEG_SIGNATURES) == 3
    others = (set(_vah.EXPORTS) | set(_vah.BOX_SIGNATURES) | set(_vah.GN_SIGNATURES) | set(_vah.RESIZE_SIGNATURES)
              | set(_vah.MCA_SIGNATURES) | set(_vah.POINTS_SIGNATURES) | set(_vah.SEG_SIGNATURES))
    assert not set(_vah.PML_SIGNATURES) & others
    for header in ('vitadapter_hip.h', 'vitadapter_hip_msda_box.h', 'vitadapter_hip_group_norm.h', 'vitadapter_hip_resize.h',
                   'vitadapter_hip_masked_attn.h', 'vitadapter_hip_points.h', 'vitadapter_hip_seg.h'):
        text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
        assert 'vah_pml' not in text, header


def test_the_header_states_the_contracts():
    text = ' '.join(open(HEADER).read().split()).replace('* ', '')
    for words in ('every element written', 'No floating-point atomics', 'the same inputs give the same bits', 'in ascending order',
                  'exactly +0.0', 'x first', 'read in place', 'chunks in ascending order', 'ascending order of the point index',
                  'P <= 0 is VAH_E_SHAPE'):
        assert ' '.join(words.split()) in text, words


@pytest.mark.parametrize('name', CALLED)
def test_null_pointers_and_empty_calls(name):
    call = CALLS[name]
    for kw, optional in POINTERS[name]:
        if not optional:
            assert call(**{kw: None}) == E_NULL, (kw, _err())
            assert 'null' in _err() and name in _err()
    # nothing to write is not an error, and no pointer is read
    nothing = {kw: None for kw, _ in POINTERS[name]}
    assert call(**nothing, K=0, ws_bytes=0) == OK and _err() == ''


@pytest.mark.parametrize('name', CALLED)
def test_p_must_be_positive_also_where_there_is_nothing_to_do(name):
    call = CALLS[name]
    for P in (0, -1):
        assert call(P=P) == E_SHAPE and 'P must be positive' in _err() and name in _err()
        assert call(P=P, K=0) == E_SHAPE
    assert call(P=1 << 31) == E_SHAPE and 'bad dims' in _err()


def test_dtype_codes():
    for dt in (1, 2, 4, -1):
        assert forward(dt=dt) == E_UNSUPPORTED and 'dtype codes' in _err()
        assert forward(dt=dt, K=0) == E_UNSUPPORTED
    # a uint8 target asks no alignment, an fp32 target 4 bytes; the prediction is fp32
    assert forward(dt=U8, tgt=A + 1, ws=None) == E_NULL and '(ws)' in _err()
    assert forward(dt=F32, tgt=A + 1) == E_ALIGN and 'tgt' in _err()
    assert forward(pred=A + 2) == E_ALIGN and 'pred' in _err()


def test_bad_dims():
    for kw in (dict(K=-1), dict(Mp=-1), dict(Mt=-1), dict(h=0), dict(w=0), dict(H=0), dict(W=0), dict(h=1 << 16, w=1 << 16), dict(prs=159),
               dict(trs=639), dict(pms=-1), dict(tms=-1), dict(h=1 << 20, prs=1 << 20, w=4), dict(K=1 << 20, rows=A, Mp=1 << 21)):
        assert forward(**kw) == E_SHAPE, (kw, _err())
    for kw in (dict(K=-1), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 16), dict(K=1 << 20)):
        assert backward(**kw) == E_SHAPE, (kw, _err())


def test_identity_rows_out_of_range_are_seen_on_the_host():
    assert forward(rows=None, K=201, Mt=300) == E_SHAPE and 'index out of range' in _err()
    assert forward(tgt_rows=None, K=25) == E_SHAPE and 'index out of range' in _err()
    assert forward(rows=None, tgt_rows=None, K=24, ws=None) == E_NULL                     # in range: passes up to the last check


def test_workspace_size():
    """the query covers both calls, is 16-byte granular, 0 for an empty or bad shape, and a smaller workspace is refused"""
    need = lib.vah_pml_ws_bytes(24, 12544, 160, 160)
    assert need == 4 * 24 * (2 * 12544 + 161 * 161) and need % 16 == 0
    assert lib.vah_pml_ws_bytes(1, 1 << 20, 1, 1) >= 4 * 4 * 1024                        # the forward's chunks fit too
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-1, 1, 1, 1), (1 << 20, 12544, 160, 160), (1, 1, 1 << 16, 1 << 16)):
        assert lib.vah_pml_ws_bytes(*bad) == 0, bad
    for call in (forward, backward):
        assert call(ws_bytes=need - 1) == E_SHAPE and 'workspace too small' in _err()
    assert lib.vah_pml_ws_bytes(3, 5, 2, 3) % 16 == 0


@pytest.mark.parametrize('name', CALLED)
def test_alignment(name):
    call = CALLS[name]
    wide = {'points': 8, 'ws': 16}
    for kw, _ in POINTERS[name]:
        if kw == 'tgt':
            continue                                     # uint8 by default: test_dtype_codes
        need = wide.get(kw, 4)
        for off in (1, 2) + ((4,) if need >= 8 else ()) + ((8,) if need == 16 else ()):
            assert call(**{kw: A + off}) == E_ALIGN, (kw, off, _err())
            assert 'misaligned' in _err() and name in _err()
        last = [k for k, opt in POINTERS[name] if not opt and k != kw][-1]
        assert call(**{kw: A + need, last: None}) == E_NULL, (kw, _err())       # aligned enough: the call goes on to the null
