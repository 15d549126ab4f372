"""CPU: the segmentor's logit-tail entry points (include/vitadapter_hip_seg.h, csrc/seg_logits.hip), their binding table
(_vah.SEG_SIGNATURES) and the host-side argument checks.

The prototypes are held to the binding with the method of tests/test_resize_rows_abi_cpu.py, applied to the seventh header
and its table; the other tables stay what they were.  Every call here is answered by the host-side validation before
anything touches a device (fake or null pointers that are never dereferenced)."""
import ctypes
import os
import re

import pytest

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_seg.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
NAMES = ('vah_seg_resize_add', 'vah_seg_finish', 'vah_seg_argmax')
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}
N, C = 2, 19


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


def _planes(C, H, W, ptr=P, rs=None, ps=None, is_=None):
    rs = W if rs is None else rs
    ps = H * rs if ps is None else ps
    is_ = C * ps if is_ is None else is_
    return ptr, is_, ps, rs


def resize_add(src=P, dst=P, N=N, C=C, hs=12, ws=13, Hc=48, Wc=52, Hd=61, Wd=67, y0=5, x0=7, align=0, accumulate=1, src_kw={},
               dst_kw={}):
    return lib.vah_seg_resize_add(*_planes(C, hs, ws, src, **src_kw), N, C, hs, ws, Hc, Wc, align,
                                  *_planes(C, Hd, Wd, dst, **dst_kw), Hd, Wd, y0, x0, accumulate, None)


def finish(acc=P, cy=P, cx=P, prob=P, labels=P, N=N, C=C, Hs=48, Ws=52, Ha=61, Wa=67, resize=1, Ho=31, Wo=45, align=0, flip=0,
           accumulate=0, acc_kw={}, prob_kw={}, lis=None, lrs=None):
    lrs = Wo if lrs is None else lrs
    lis = Ho * lrs if lis is None else lis
    return lib.vah_seg_finish(*_planes(C, Ha, Wa, acc, **acc_kw), N, C, Hs, Ws, cy, cx, resize, Ho, Wo, align, flip,
                              *_planes(C, Ho, Wo, prob, **prob_kw), accumulate, labels, lis, lrs, None)


def argmax(total=P, labels=P, N=N, C=C, H=31, W=45, divisor=3.0, kw={}, lis=None, lrs=None):
    lrs = W if lrs is None else lrs
    lis = H * lrs if lis is None else lis
    return lib.vah_seg_argmax(*_planes(C, H, W, total, **kw), N, C, H, W, divisor, labels, lis, lrs, None)


def test_every_signature_matches_its_prototype():
    assert set(PROTOTYPES) == set(_vah.SEG_SIGNATURES) == set(NAMES)
    for name, (restype, params) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        got = list(fn.argtypes or [])
        assert got == list(_vah.SEG_SIGNATURES[name][1])
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
    assert len(_vah.MCA_SIGNATURES) == 5 and len(_vah.POINTS_SIGNATURES) == 2
    others = (set(_vah.EXPORTS) | set(_vah.BOX_SIGNATURES) | set(_vah.GN_SIGNATURES) | set(_vah.RESIZE_SIGNATURES)
              | set(_vah.MCA_SIGNATURES) | set(_vah.POINTS_SIGNATURES))
    assert not set(_vah.SEG_SIGNATURES) & others
    for header in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        if header != 'vitadapter_hip_seg.h':
            text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
            assert 'vah_seg_' not in text, header


def test_resize_add_argument_errors():
    name = 'vah_seg_resize_add'
    for kw in (dict(N=-1), dict(C=-1), dict(hs=-1), dict(ws=-2), dict(Hc=-1), dict(Wc=-1), dict(Hd=-1), dict(Wd=-1), dict(N=1 << 20),
               dict(Hd=1 << 31)):
        assert resize_add(**kw) == E_SHAPE, (kw, _err())
        assert name in _err() and 'bad dims' in _err()
    # a window that leaves dst
    for kw in (dict(y0=-1), dict(x0=-1), dict(y0=14), dict(x0=16), dict(Hc=57), dict(Wc=61), dict(Hd=52), dict(Wd=58)):
        assert resize_add(**kw) == E_SHAPE, (kw, _err())
        assert 'leaves dst' in _err()
    assert resize_add(y0=13, x0=15, src=None) == E_NULL                # the last window that fits passes that check
    assert resize_add(hs=0) == E_SHAPE and 'empty source' in _err()
    assert resize_add(ws=0) == E_SHAPE
    assert resize_add(src=None) == E_NULL and 'src' in _err() and name in _err()
    assert resize_add(dst=None) == E_NULL and 'dst' in _err()
    assert resize_add(src=P + 2) == E_ALIGN and 'misaligned' in _err()
    assert resize_add(dst=P + 1) == E_ALIGN
    # a row stride smaller than the width, planes and images that overlap
    for kw in (dict(src_kw=dict(rs=12)), dict(dst_kw=dict(rs=66)), dict(src_kw=dict(ps=12 * 13 - 1)), dict(dst_kw=dict(ps=0)),
               dict(dst_kw=dict(is_=61 * 67 * (C - 1))), dict(src_kw=dict(rs=-13))):
        assert resize_add(**kw) == E_SHAPE, (kw, _err())
        assert 'strides' in _err()


def test_finish_argument_errors():
    name = 'vah_seg_finish'
    for kw in (dict(N=-1), dict(C=-1), dict(Hs=-1), dict(Ws=-1), dict(Ho=-1), dict(Wo=-1), dict(N=65536), dict(Wo=1 << 31)):
        assert finish(**kw) == E_SHAPE, (kw, _err())
        assert name in _err() and 'bad dims' in _err()
    assert finish(Ho=1 << 16, Wo=1 << 16) == E_SHAPE and '2^31' in _err()
    for flip in (-1, 3, 7):
        assert finish(flip=flip) == E_SHAPE and 'flip' in _err()
    for flip in (0, 1, 2):
        assert finish(flip=flip, acc=None) == E_NULL
    assert finish(resize=0) == E_SHAPE and 'resize == 0' in _err()
    assert finish(resize=0, Ho=48, Wo=52, acc=None) == E_NULL
    assert finish(Hs=0) == E_SHAPE and 'empty source' in _err()
    assert finish(acc=None) == E_NULL and 'acc' in _err()
    assert finish(cy=None) == E_NULL and 'cy' in _err()
    assert finish(cx=None) == E_NULL
    assert finish(prob=None, labels=None) == E_NULL and 'nothing to write' in _err()
    assert finish(acc=P + 2) == E_ALIGN and finish(cy=P + 2) == E_ALIGN and finish(prob=P + 2) == E_ALIGN
    assert finish(labels=P + 4) == E_ALIGN and 'labels' in _err()
    for kw in (dict(acc_kw=dict(rs=51)), dict(Ws=68), dict(prob_kw=dict(rs=44)), dict(prob_kw=dict(ps=31 * 45 - 1)), dict(lrs=44),
               dict(lis=31 * 45 - 1)):
        assert finish(**kw) == E_SHAPE, (kw, _err())
        assert 'strides' in _err()
    # the read region may be smaller than its buffer, and an absent output's strides are not read
    assert finish(acc_kw=dict(rs=67), prob=None, prob_kw=dict(rs=1), labels=P + 4) == E_ALIGN
    assert finish(labels=None, lrs=0, lis=0, prob=P + 2) == E_ALIGN


def test_argmax_argument_errors():
    name = 'vah_seg_argmax'
    for kw in (dict(N=-1), dict(C=-1), dict(H=-1), dict(W=-1), dict(N=65536), dict(H=1 << 16, W=1 << 16)):
        assert argmax(**kw) == E_SHAPE, (kw, _err())
        assert name in _err() and 'bad dims' in _err()
    assert argmax(total=None) == E_NULL and 'sum' in _err()
    assert argmax(labels=None) == E_NULL and 'labels' in _err()
    assert argmax(total=P + 2) == E_ALIGN and argmax(labels=P + 4) == E_ALIGN
    for kw in (dict(kw=dict(rs=44)), dict(kw=dict(ps=100)), dict(lrs=44), dict(lis=10)):
        assert argmax(**kw) == E_SHAPE, (kw, _err())
        assert 'strides' in _err()


def test_empty_problems_read_no_pointer():
    for kw in (dict(N=0), dict(C=0), dict(Hc=0), dict(Wc=0)):
        assert resize_add(src=None, dst=None, **kw) == OK and _err() == '', kw
        assert resize_add(src=P + 1, dst=P + 3, src_kw=dict(rs=0), **kw) == OK
    assert resize_add(N=0, hs=0, ws=0) == OK
    assert resize_add(N=0, y0=20) == E_SHAPE                                       # the window is checked first
    for kw in (dict(N=0), dict(C=0), dict(Ho=0), dict(Wo=0)):
        assert finish(acc=None, cy=None, cx=None, prob=None, labels=None, **kw) == OK and _err() == '', kw
    assert finish(N=0, flip=5) == E_SHAPE
    for kw in (dict(N=0), dict(C=0), dict(H=0), dict(W=0)):
        assert argmax(total=None, labels=None, **kw) == OK and _err() == '', kw
