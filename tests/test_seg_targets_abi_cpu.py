"""CPU: the entry points of Mask2Former's targets from a label map (include/vitadapter_hip_seg_target.h, csrc/seg_target.hip),
their binding table (_vah.SEGTGT_SIGNATURES) and the host-side argument checks.

The prototypes are held to the binding with the method of tests/test_seg_eval_abi_cpu.py, applied to the twelfth header and its
table; the other tables stay what they were.  Every call here is answered by the host-side validation before anything
touches a device (fake or null pointers that are never dereferenced)."""
import ctypes
import os
import re

import pytest

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_seg_target.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
NAMES = ('vah_segtgt_ws_bytes', 'vah_segtgt_scan', 'vah_segtgt_masks')
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}
N, H, W = 2, 61, 67


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


def scan(label=P, labels=P, slot=P, meta=P, ws=P, N=N, H=H, W=W, dtype=1, lis=None, lrs=None, ignore=255, remap=None, ws_bytes=None):
    lrs = W if lrs is None else lrs
    lis = H * lrs if lis is None else lis
    if ws_bytes is None:
        ws_bytes = lib.vah_segtgt_ws_bytes(N, H, W)
    return lib.vah_segtgt_scan(label, dtype, lis, lrs, N, H, W, ignore, remap, labels, slot, meta, ws, ws_bytes, None)


def masks(label=P, slot=P, labels=P, meta=P, out=P, image_of=P, labels_out=P, N=N, H=H, W=W, dtype=1, lis=None, lrs=None, remap=None,
          G=5):
    lrs = W if lrs is None else lrs
    lis = H * lrs if lis is None else lis
    return lib.vah_segtgt_masks(label, dtype, lis, lrs, N, H, W, remap, slot, labels, meta, G, out, image_of, labels_out, None)


def test_every_signature_matches_its_prototype():
    assert set(PROTOTYPES) == set(_vah.SEGTGT_SIGNATURES) == set(NAMES)
    for name, (restype, params) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        got = list(fn.argtypes or [])
        assert got == list(_vah.SEGTGT_SIGNATURES[name][1])
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
    assert len(_vah.SEGEVAL_SIGNATURES) == 2
    others = (set(_vah.EXPORTS) | set(_vah.BOX_SIGNATURES) | set(_vah.GN_SIGNATURES) | set(_vah.RESIZE_SIGNATURES)
              | set(_vah.MCA_SIGNATURES) | set(_vah.POINTS_SIGNATURES) | set(_vah.PML_SIGNATURES) | set(_vah.SEG_SIGNATURES)
              | set(_vah.SCE_SIGNATURES) | set(_vah.EPOCH_SIGNATURES) | set(_vah.SEGEVAL_SIGNATURES))
    assert not set(_vah.SEGTGT_SIGNATURES) & others
    for header in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        if header != 'vitadapter_hip_seg_target.h':
            text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
            assert 'vah_segtgt' not in text, header


def test_ws_bytes():
    ws = lib.vah_segtgt_ws_bytes
    assert ws(N, H, W) == N * 64                                    # 4087 pixels: one workgroup an image
    assert ws(1, 1, 1) == 64
    assert ws(2, 96, 131) == 2 * 4 * 64                             # 12576 pixels: four ranges of 4096
    for args in ((0, H, W), (N, 0, W), (N, H, 0), (-1, H, W), (4097, H, W), (N, 1 << 16, 1 << 16), (N, 1 << 31, 1)):
        assert ws(*args) == 0, args
    assert ws(4096, H, W) == 4096 * 64
    # more pixels never need fewer workgroups, and their number is bounded
    rows = [ws(1, h, 2048) // 64 for h in (1, 2, 3, 64, 1024, 65536)]
    assert rows == sorted(rows) and rows[0] == 1 and rows[2] == 2 and rows[-1] <= 256


@pytest.mark.parametrize('call,name', [(scan, 'vah_segtgt_scan'), (masks, 'vah_segtgt_masks')])
def test_shared_argument_errors(call, name):
    for kw in (dict(N=-1), dict(H=-1), dict(W=-2), dict(N=4097), dict(H=1 << 31), dict(H=1 << 16, W=1 << 16)):
        assert call(**kw) == E_SHAPE, (kw, _err())
        assert name in _err() and 'bad dims' in _err()
    for dtype in (-1, 2, 7):
        assert call(dtype=dtype) == E_UNSUPPORTED and 'dtype' in _err()
    assert call(label=None) == E_NULL and 'label' in _err() and name in _err()
    assert call(label=P + 4, dtype=0) == E_ALIGN and 'label' in _err() and 'misaligned' in _err()
    assert call(label=P + 3, dtype=1, meta=None) == E_NULL and 'meta' in _err()          # uint8 labels: any alignment
    assert call(remap=P + 3, meta=None) == E_NULL and 'meta' in _err()                   # the table too
    # a row stride smaller than the width, images that overlap
    for kw in (dict(lrs=W - 1), dict(lis=H * W - 1), dict(lrs=0), dict(lrs=-W), dict(lrs=W + 5, lis=H * W),
               dict(lrs=W + 3, lis=(H - 1) * (W + 3) + W - 1)):
        assert call(**kw) == E_SHAPE, (kw, _err())
        assert 'strides' in _err()
    assert call(lrs=W + 3, lis=(H - 1) * (W + 3) + W, meta=None) == E_NULL
    for kw in (dict(slot=None), dict(labels=None), dict(meta=None)):
        assert call(**kw) == E_NULL and list(kw)[0] in _err()
    assert call(slot=P + 2) == E_ALIGN and 'slot' in _err()
    assert call(labels=P + 4) == E_ALIGN and 'labels' in _err()
    assert call(meta=P + 1) == E_ALIGN and 'meta' in _err()


def test_scan_argument_errors():
    assert scan(ws=None) == E_NULL and 'ws' in _err()
    assert scan(ws=P + 8) == E_ALIGN and 'ws' in _err()
    need = lib.vah_segtgt_ws_bytes(N, H, W)
    assert scan(ws_bytes=need - 1) == E_SHAPE and 'workspace too small' in _err() and str(need) in _err()
    assert scan(ws_bytes=0) == E_SHAPE
    assert scan(N=4096, ws_bytes=0) == E_SHAPE and 'workspace' in _err()      # the largest N passes the size check


def test_masks_argument_errors():
    for G in (-1, N * 256 + 1):
        assert masks(G=G) == E_SHAPE and 'G_total' in _err()
    assert masks(G=N * 256, out=None) == E_NULL                                # the largest G_total passes that check
    assert masks(out=None) == E_NULL and 'masks' in _err()
    assert masks(image_of=None) == E_NULL and 'image_of' in _err()
    assert masks(labels_out=None) == E_NULL and 'labels_out' in _err()
    assert masks(out=P + 8) == E_ALIGN and 'masks' in _err()
    assert masks(image_of=P + 2) == E_ALIGN and 'image_of' in _err()
    assert masks(labels_out=P + 4) == E_ALIGN and 'labels_out' in _err()


def test_empty_problems_read_no_pointer():
    for kw in (dict(N=0), dict(H=0), dict(W=0)):
        assert scan(label=None, labels=None, slot=None, meta=None, ws=None, ws_bytes=0, **kw) == OK and _err() == '', kw
        assert scan(label=P + 1, labels=P + 1, slot=P + 1, meta=P + 1, ws=P + 1, lrs=0, ws_bytes=0, **kw) == OK
        assert masks(label=None, slot=None, labels=None, meta=None, out=None, image_of=None, labels_out=None, G=0, **kw) == OK
    assert masks(label=None, slot=None, labels=None, meta=None, out=None, image_of=None, labels_out=None, G=0) == OK and _err() == ''
    assert scan(N=0, dtype=3) == E_UNSUPPORTED and scan(N=0, H=-1) == E_SHAPE
    assert masks(N=0, G=0, dtype=3) == E_UNSUPPORTED and masks(N=0, G=1) == E_SHAPE
