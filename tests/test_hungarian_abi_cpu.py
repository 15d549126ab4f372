"""CPU: the entry point of the assignment step of Mask2Former's matching (include/vitadapter_hip_assign.h, csrc/assign.hip), its
binding table (_vah.ASSIGN_SIGNATURES) and the host-side argument checks.

The prototype is held to the binding with the method of tests/test_seg_targets_abi_cpu.py, applied to the thirteenth header and
its table; the other tables stay what they were.  Every call here is answered by the host-side validation before anything
touches a device (fake or null pointers that are never dereferenced)."""
import ctypes
import os
import re

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_assign.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
NAMES = ('vah_assign_solve',)
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


def solve(cost=P, offsets=P, L=10, N=2, Q=100, Gmax=12, table=P, status=P):
    return lib.vah_assign_solve(cost, offsets, L, N, Q, Gmax, table, status, None)


def test_the_signature_matches_its_prototype():
    assert set(PROTOTYPES) == set(_vah.ASSIGN_SIGNATURES) == set(NAMES)
    for name, (restype, params) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        got = list(fn.argtypes or [])
        assert got == list(_vah.ASSIGN_SIGNATURES[name][1])
        assert len(got) == len(params) == 9, (name, len(got), len(params))
        for i, (g, allowed) in enumerate(zip(got, params)):
            assert g in allowed, (name, i, g, allowed)


def test_library_exports_the_symbol():
    assert hasattr(ctypes.CDLL(_vah.LIB_PATH), 'vah_assign_solve')


def test_the_other_tables_are_untouched():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION
    assert len(_vah.EXPORTS) == 122 and len(_vah.SEGTGT_SIGNATURES) == 3 and len(_vah.SEGEVAL_SIGNATURES) == 2
    others = (set(_vah.EXPORTS) | set(_vah.BOX_SIGNATURES) | set(_vah.GN_SIGNATURES) | set(_vah.RESIZE_SIGNATURES)
              | set(_vah.MCA_SIGNATURES) | set(_vah.POINTS_SIGNATURES) | set(_vah.PML_SIGNATURES) | set(_vah.SEG_SIGNATURES)
              | set(_vah.SCE_SIGNATURES) | set(_vah.EPOCH_SIGNATURES) | set(_vah.SEGEVAL_SIGNATURES) | set(_vah.SEGTGT_SIGNATURES))
    assert not set(_vah.ASSIGN_SIGNATURES) & others
    for header in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        if header != 'vitadapter_hip_assign.h':
            text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
            assert 'vah_assign' not in text, header


def test_limits_are_unsupported_before_any_pointer_is_read():
    for kw in (dict(Q=0), dict(Q=-1), dict(Q=257), dict(Gmax=-1), dict(Gmax=257), dict(Q=256, Gmax=200), dict(Q=129, Gmax=256),
               dict(Q=182, Gmax=182)):
        assert solve(**kw) == E_UNSUPPORTED, (kw, _err())
        assert 'vah_assign_solve' in _err() and 'Q * Gmax' in _err()
        assert solve(cost=None, offsets=None, table=None, status=None, **kw) == E_UNSUPPORTED
    # the largest problems pass that check: the next answer is about a pointer
    for kw in (dict(Q=256, Gmax=128), dict(Q=128, Gmax=256), dict(Q=181, Gmax=181), dict(Q=1, Gmax=256), dict(Q=256, Gmax=1)):
        assert solve(status=None, **kw) == E_NULL and 'status' in _err(), kw


def test_shape_errors():
    for kw in (dict(L=-1), dict(N=-1), dict(N=4097), dict(L=1 << 31), dict(L=1 << 20, N=4096)):
        assert solve(**kw) == E_SHAPE, (kw, _err())
        assert 'bad dims' in _err()
    assert solve(N=4096, status=None) == E_NULL


def test_pointer_errors():
    for kw in (dict(cost=None), dict(offsets=None), dict(table=None), dict(status=None)):
        assert solve(**kw) == E_NULL, kw
        assert {'offsets': 'gt_offsets'}.get(list(kw)[0], list(kw)[0]) in _err() and 'null' in _err()
    assert solve(cost=P + 2) == E_ALIGN and 'cost' in _err() and 'misaligned' in _err()
    assert solve(offsets=P + 1) == E_ALIGN and 'gt_offsets' in _err()
    assert solve(table=P + 4) == E_ALIGN and 'table' in _err()
    assert solve(status=P + 2) == E_ALIGN and 'status' in _err()


def test_empty_problems_read_no_pointer():
    # no problem (L * N == 0) or no target anywhere (Gmax == 0, so K == 0)
    for kw in (dict(L=0), dict(N=0), dict(Gmax=0), dict(L=0, N=0, Gmax=0)):
        assert solve(cost=None, offsets=None, table=None, status=None, **kw) == OK and _err() == '', kw
        assert solve(cost=P + 1, offsets=P + 1, table=P + 1, status=P + 1, **kw) == OK, kw
    assert solve(L=0, Q=0) == E_UNSUPPORTED and solve(N=0, L=-1) == E_SHAPE          # sizes are still checked
