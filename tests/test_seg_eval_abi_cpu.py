"""CPU: the class-count entry points of the mIoU evaluation (include/vitadapter_hip_seg_eval.h, csrc/seg_eval.hip), their
binding table (_vah.SEGEVAL_SIGNATURES) and the host-side argument checks.

The prototypes are held to the binding with the method of tests/test_seg_logits_abi_cpu.py, applied to the eleventh header
and its table; the other tables stay what they were.  Every call here is answered by the host-side validation before
anything touches a device (fake or null pointers that are never dereferenced)."""
import ctypes
import os
import re

import pytest

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_seg_eval.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
NAMES = ('vah_segeval_ws_bytes', 'vah_segeval_update')
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}
N, H, W, C = 2, 61, 67, 19


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


def update(pred=P, label=P, totals=P, ws=P, N=N, H=H, W=W, C=C, dtype=1, pis=None, prs=None, lis=None, lrs=None, ignore=255, rz=0,
           label_map=None, map_len=0, ws_bytes=None):
    prs = W if prs is None else prs
    pis = H * prs if pis is None else pis
    lrs = W if lrs is None else lrs
    lis = H * lrs if lis is None else lis
    if ws_bytes is None:
        ws_bytes = lib.vah_segeval_ws_bytes(N, H, W, C)
    return lib.vah_segeval_update(pred, pis, prs, label, dtype, lis, lrs, N, H, W, C, ignore, rz, label_map, map_len, totals, ws,
                                  ws_bytes, None)


def test_every_signature_matches_its_prototype():
    assert set(PROTOTYPES) == set(_vah.SEGEVAL_SIGNATURES) == set(NAMES)
    for name, (restype, params) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        got = list(fn.argtypes or [])
        assert got == list(_vah.SEGEVAL_SIGNATURES[name][1])
        assert len(got) == len(params), (name, len(got), len(params))
        for i, (g, allowed) in enumerate(zip(got, params)):
            assert g in allowed, (name, i, g, allowed)


@pytest.mark.parametrize('name', NAMES)
def test_library_exports_the_symbol(name):
    assert hasattr(ctypes.CDLL(_vah.LIB_PATH), name), name


def test_the_other_tables_are_untouched():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION
    assert len(_vah.EXPORTS) == 122 and len(_vah.SIGNATURES) == 79 and len(_vah.F16_TWINS) == 43
    assert len(_vah.GN_SIGNATURES) == 6 and len(_vah.BOX_SIGNATURES) == 2 and len(_vah.RESIZE_SIGNATURES) == 3
    assert len(_vah.MCA_SIGNATURES) == 5 and len(_vah.POINTS_SIGNATURES) == 2 and len(_vah.PML_SIGNATURES) == 3
    assert len(_vah.SEG_SIGNATURES) == 3 and len(_vah.SCE_SIGNATURES) == 3 and len(_vah.EPOCH_SIGNATURES) == 6
    others = (set(_vah.EXPORTS) | set(_vah.BOX_SIGNATURES) | set(_vah.GN_SIGNATURES) | set(_vah.RESIZE_SIGNATURES)
              | set(_vah.MCA_SIGNATURES) | set(_vah.POINTS_SIGNATURES) | set(_vah.PML_SIGNATURES) | set(_vah.SEG_SIGNATURES)
              | set(_vah.SCE_SIGNATURES) | set(_vah.EPOCH_SIGNATURES))
    assert not set(_vah.SEGEVAL_SIGNATURES) & others
    for header in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        if header != 'vitadapter_hip_seg_eval.h':
            text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
            assert 'vah_segeval' not in text, header


def test_ws_bytes():
    ws = lib.vah_segeval_ws_bytes
    assert ws(N, H, W, C) > 0 and ws(N, H, W, C) % (3 * C * 4) == 0
    assert ws(1, 1, 1, 1) == 12                                     # one workgroup, one class
    for args in ((0, H, W, C), (N, 0, W, C), (N, H, 0, C), (N, H, W, 0), (-1, H, W, C), (N, H, W, 4097), (65536, H, W, C),
                 (N, 1 << 16, 1 << 16, C), (N, 1 << 31, 1, C)):
        assert ws(*args) == 0, args
    assert ws(N, H, W, 4096) > 0
    # more pixels never need fewer workgroups, and their number is bounded
    rows = [ws(1, h, 2048, C) // (3 * C * 4) for h in (1, 2, 3, 64, 1024, 65536)]
    assert rows == sorted(rows) and rows[0] == 1 and rows[-1] <= 1024


def test_update_argument_errors():
    name = 'vah_segeval_update'
    for kw in (dict(N=-1), dict(H=-1), dict(W=-2), dict(C=-1), dict(C=0), dict(N=65536), dict(H=1 << 31), dict(H=1 << 16, W=1 << 16)):
        assert update(ws_bytes=1 << 40, **kw) == E_SHAPE, (kw, _err())
        assert name in _err() and 'bad dims' in _err()
    assert update(C=4097, ws_bytes=1 << 40) == E_UNSUPPORTED and '4096' in _err()
    assert update(C=4096, pred=None) == E_NULL                          # the largest C passes that check
    for dtype in (-1, 2, 7):
        assert update(dtype=dtype) == E_UNSUPPORTED and 'dtype' in _err()
    assert update(map_len=257, label_map=P) == E_SHAPE and 'label_map_len' in _err()
    assert update(map_len=-1, label_map=P) == E_SHAPE
    assert update(map_len=256, label_map=P, pred=None) == E_NULL
    assert update(pred=None) == E_NULL and 'pred' in _err() and name in _err()
    assert update(label=None) == E_NULL and 'label' in _err()
    assert update(totals=None) == E_NULL and 'totals' in _err()
    assert update(ws=None) == E_NULL and 'ws' in _err()
    assert update(pred=P + 4) == E_ALIGN and 'misaligned' in _err() and 'pred' in _err()
    assert update(totals=P + 4) == E_ALIGN and 'totals' in _err()
    assert update(ws=P + 8) == E_ALIGN and 'ws' in _err()
    assert update(label=P + 4, dtype=0) == E_ALIGN and 'label' in _err()
    assert update(label_map=P + 4, map_len=3) == E_ALIGN and 'label_map' in _err()
    assert update(label=P + 3, dtype=1, totals=None) == E_NULL and 'totals' in _err()     # uint8 labels: any alignment
    # a row stride smaller than the width, images that overlap
    for kw in (dict(prs=W - 1), dict(lrs=W - 1), dict(pis=H * W - 1), dict(lis=H * W - 1), dict(prs=-W), dict(lrs=0),
               dict(prs=W + 3, pis=(H - 1) * (W + 3) + W - 1), dict(lrs=W + 5, lis=H * W)):
        assert update(**kw) == E_SHAPE, (kw, _err())
        assert 'strides' in _err()
    assert update(prs=W + 3, pis=(H - 1) * (W + 3) + W, lrs=W + 5, lis=(H - 1) * (W + 5) + W, totals=None) == E_NULL
    need = lib.vah_segeval_ws_bytes(N, H, W, C)
    assert update(ws_bytes=need - 1) == E_SHAPE and 'workspace too small' in _err() and str(need) in _err()
    assert update(ws_bytes=0) == E_SHAPE


def test_empty_problems_read_no_pointer():
    for kw in (dict(N=0), dict(H=0), dict(W=0)):
        assert update(pred=None, label=None, totals=None, ws=None, ws_bytes=0, **kw) == OK and _err() == '', kw
        assert update(pred=P + 1, label=P + 3, totals=P + 1, ws=P + 1, prs=0, lrs=0, ws_bytes=0, **kw) == OK
    assert update(N=0, C=4097) == E_UNSUPPORTED and update(N=0, C=0) == E_SHAPE and update(N=0, dtype=3) == E_UNSUPPORTED
