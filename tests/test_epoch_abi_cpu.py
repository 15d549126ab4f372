"""CPU: the entry points of include/vitadapter_hip_epoch.h (csrc/epoch_copies.hip, the row-mapped weight-gradient GEMM of
csrc/gemm.hip, the BatchNorm finalize launch with bookkeeping of csrc/tail_ops.hip), their binding table
(_vah.EPOCH_SIGNATURES) and the host-side argument checks.

The prototypes are held to the binding with the method of tests/test_resize_rows_abi_cpu.py; the other tables and the ABI
version stay what they were.  Every call here is answered by the host-side validation before anything touches a device
(fake or null pointers that are never dereferenced)."""
import ctypes
import os
import re

import pytest

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_epoch.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
NAMES = ('vah_epoch_job_bytes', 'vah_epoch_chunk_elems', 'vah_epoch_copies', 'vah_gemm_bf16_fin_rowmap',
         'vah_gemm_f16_fin_rowmap', 'vah_bn_finalize_stats_book')
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}


def _err():
    return lib.vah_last_error().decode()


def _param(text):
    if '*' in text:
        if text.replace('const', '').split()[0] == 'int':          # a host int the call writes
            return (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int))
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
        out[name] = (SCALARS[ret], [] if params == 'void' else [_param(p.strip()) for p in params.split(',')])
    return out


PROTOTYPES = _prototypes()


def test_every_signature_matches_its_prototype():
    assert set(PROTOTYPES) == set(_vah.EPOCH_SIGNATURES) == set(NAMES)
    for name, (restype, params) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        got = list(fn.argtypes or [])
        assert got == list(_vah.EPOCH_SIGNATURES[name][1])
        assert len(got) == len(params), (name, len(got), len(params))
        for i, (g, allowed) in enumerate(zip(got, params)):
            assert g in allowed, (name, i, g, allowed)


@pytest.mark.parametrize('name', NAMES)
def test_library_exports_the_symbol(name):
    assert hasattr(ctypes.CDLL(_vah.LIB_PATH), name), name


def test_the_other_tables_are_untouched():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION
    assert len(_vah.EXPORTS) == 122 and len(_vah.SIGNATURES) == 79 and len(_vah.F16_TWINS) == 43
    others = set(_vah.EXPORTS)
    for table in ('BOX_SIGNATURES', 'GN_SIGNATURES', 'RESIZE_SIGNATURES', 'MCA_SIGNATURES', 'POINTS_SIGNATURES', 'PML_SIGNATURES',
                  'SEG_SIGNATURES', 'SCE_SIGNATURES'):
        others |= set(getattr(_vah, table))
    assert not set(_vah.EPOCH_SIGNATURES) & others
    for header in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        if header != 'vitadapter_hip_epoch.h':
            text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
            for name in NAMES:
                assert name not in text, (header, name)


def test_job_layout():
    assert lib.vah_epoch_job_bytes() == 128 and lib.vah_epoch_chunk_elems() == 2048


def _copies(jobs=P, njobs=3, chunks=P, nchunks=5, dt=1, out16=P, cap16=4096, out32=P, cap32=64):
    return lib.vah_epoch_copies(jobs, njobs, chunks, nchunks, dt, out16, cap16, out32, cap32, None)


def test_epoch_copies_argument_checks():
    for kw in (dict(njobs=-1), dict(nchunks=-1), dict(cap16=-1), dict(cap32=-1), dict(nchunks=1 << 31), dict(njobs=1 << 25)):
        assert _copies(**kw) == E_SHAPE and 'bad dims' in _err(), kw
    for dt in (0, 3, -1):
        assert _copies(dt=dt) == E_UNSUPPORTED and 'dtype16' in _err()
    assert _copies(nchunks=0, jobs=None, chunks=None, out16=None, out32=None) == OK and _err() == ''
    assert _copies(njobs=0) == E_SHAPE and 'without jobs' in _err()
    for kw in (dict(jobs=None), dict(chunks=None), dict(out16=None), dict(out32=None)):
        assert _copies(**kw) == E_NULL and 'null' in _err(), kw
    assert _copies(out32=None, cap32=0, out16=None, cap16=0, jobs=P + 4) == E_ALIGN        # empty buffers need no pointer
    for kw in (dict(jobs=P + 4), dict(chunks=P + 4), dict(out16=P + 8), dict(out32=P + 8)):
        assert _copies(**kw) == E_ALIGN and 'misaligned' in _err() and 'vah_epoch_copies' in _err(), kw


@pytest.mark.parametrize('name', ('vah_gemm_bf16_fin_rowmap', 'vah_gemm_f16_fin_rowmap'))
def test_fin_rowmap_argument_checks(name):
    fn = getattr(lib, name)
    M, N, K = 16, 8, 64
    applied = ctypes.c_int(7)

    def call(fin_part=P, nparts=2, fin_C=M, fin_out=P, row_map=P, K=K):
        return fn(1, 0, M, N, K, P, M, P, N, P, N, 1, P, 1 << 20, fin_part, nparts, fin_C, fin_out, row_map, ctypes.byref(applied), None)

    assert call(fin_part=None) == E_SHAPE and 'bad finalize job' in _err() and name in _err()
    assert applied.value == 0                                  # never left unset
    assert call(nparts=0) == E_SHAPE and call(fin_out=None) == E_SHAPE
    assert call(row_map=None) == E_NULL and 'row_map' in _err()
    assert call(fin_C=M - 1) == E_SHAPE and 'fin_C == M' in _err()
    assert call(row_map=P + 2) == E_SHAPE
    assert call(K=0) == E_SHAPE and 'K = 0' in _err()           # the dispatcher's own checks follow


def test_bn_finalize_book_argument_checks():
    fn = lib.vah_bn_finalize_stats_book
    name = 'vah_bn_finalize_stats_book'
    assert fn(P, 0, 8.0, 1e-5, 0.1, P, P, P, P, P, None) == E_SHAPE and 'bad C' in _err() and name in _err()
    for args in ((None, 8, 8.0, 1e-5, 0.1, P, P, P, P, P), (P, 8, 8.0, 1e-5, 0.1, P, P, None, P, P),
                 (P, 8, 8.0, 1e-5, 0.1, P, P, P, None, P), (P, 8, 8.0, 1e-5, 0.1, P, None, P, P, P),
                 (P, 8, 8.0, 1e-5, 0.1, None, P, P, P, None)):
        assert fn(*args, None) == E_NULL and 'null' in _err(), args
