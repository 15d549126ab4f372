"""CPU: the entry points of the UperNet training loss (include/vitadapter_hip_seg_loss.h, csrc/seg_ce_loss.hip), their binding
table (_vah.SCE_SIGNATURES) and the host-side argument checks.

The prototypes are held to the binding with the method of tests/test_seg_logits_abi_cpu.py, applied to the ninth header and
its table; the other tables stay what they were.  Every call here is answered by the host-side validation before anything
touches a device (fake or null pointers that are never dereferenced)."""
import ctypes
import os
import re

import pytest

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vitadapter_hip_seg_loss.h')
lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
NAMES = ('vah_sce_ws_bytes', 'vah_sce_forward', 'vah_sce_backward')
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}
N, C, h, w, H, W = 2, 19, 12, 13, 48, 52


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


def _head(kw):
    """the arguments the two calls share, from keyword overrides"""
    g = dict(logits=P, dtype=0, N=N, C=C, h=h, w=w, H=H, W=W, labels=P, align=0, ignore=255, cw=P, rs=None, ps=None, is_=None,
             lrs=None, lis=None)
    g.update(kw)
    rs = g['w'] if g['rs'] is None else g['rs']
    ps = g['h'] * rs if g['ps'] is None else g['ps']
    is_ = g['C'] * ps if g['is_'] is None else g['is_']
    lrs = g['W'] if g['lrs'] is None else g['lrs']
    lis = g['H'] * lrs if g['lis'] is None else g['lis']
    return (g['logits'], g['dtype'], is_, ps, rs, g['N'], g['C'], g['h'], g['w'], g['labels'], lis, lrs, g['H'], g['W'], g['align'],
            g['ignore'], g['cw'])


def _need(**kw):
    g = dict(N=N, C=C, h=h, w=w, H=H, W=W)
    g.update({k: v for k, v in kw.items() if k in g})
    return lib.vah_sce_ws_bytes(g['N'], g['C'], g['h'], g['w'], g['H'], g['W'])


def forward(lse=P, loss_sum=P, counts=P, ws=P, ws_bytes=None, **kw):
    ws_bytes = max(_need(**kw), 16) if ws_bytes is None else ws_bytes
    return lib.vah_sce_forward(*_head(kw), lse, loss_sum, counts, ws, ws_bytes, None)


def backward(lse=P, scale=P, dlogits=P, ws=P, ws_bytes=None, drs=None, dps=None, dis=None, **kw):
    ws_bytes = max(_need(**kw), 16) if ws_bytes is None else ws_bytes
    hh, ww, CC = kw.get('h', h), kw.get('w', w), kw.get('C', C)
    drs = ww if drs is None else drs
    dps = hh * drs if dps is None else dps
    dis = CC * dps if dis is None else dis
    return lib.vah_sce_backward(*_head(kw), lse, scale, dlogits, dis, dps, drs, ws, ws_bytes, None)


CALLS = (('vah_sce_forward', forward), ('vah_sce_backward', backward))


def test_every_signature_matches_its_prototype():
    assert set(PROTOTYPES) == set(_vah.SCE_SIGNATURES) == set(NAMES)
    for name, (restype, params) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        got = list(fn.argtypes or [])
        assert got == list(_vah.SCE_SIGNATURES[name][1])
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
    assert len(_vah.SEG_SIGNATURES) == 3
    others = (set(_vah.EXPORTS) | set(_vah.BOX_SIGNATURES) | set(_vah.GN_SIGNATURES) | set(_vah.RESIZE_SIGNATURES)
              | set(_vah.MCA_SIGNATURES) | set(_vah.POINTS_SIGNATURES) | set(_vah.PML_SIGNATURES) | set(_vah.SEG_SIGNATURES))
    assert not set(_vah.SCE_SIGNATURES) & others
    for header in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        if header != 'vitadapter_hip_seg_loss.h':
            text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
            assert 'vah_sce_' not in text, header


def test_workspace_size():
    """partials of 12 bytes per 256 output pixels, 16 bytes per output row / column, 8 per source row / column: no term in C"""
    assert _need() >= 12 * N * ((H * W + 255) // 256) + 16 * (H + W) + 8 * (h + w)
    assert _need() % 16 == 0 and _need(C=150) == _need(C=1)
    assert _need(N=2, h=128, w=128, H=512, W=512) < 64 * 1024
    for kw in (dict(N=0), dict(C=0), dict(h=0), dict(W=0), dict(N=65536), dict(H=1 << 16, W=1 << 16), dict(h=-1)):
        assert _need(**kw) == 0, kw


@pytest.mark.parametrize('name,call', CALLS)
def test_argument_errors(name, call):
    for kw in (dict(N=-1), dict(C=-1), dict(h=-1), dict(w=-2), dict(H=-1), dict(W=-1), dict(N=1 << 20), dict(N=65536), dict(W=1 << 31)):
        assert call(**kw) == E_SHAPE, (kw, _err())
        assert name in _err() and 'bad dims' in _err()
    assert call(H=1 << 16, W=1 << 16) == E_SHAPE and '2^31' in _err()
    assert call(dtype=3) == E_UNSUPPORTED and 'dtype' in _err() and name in _err()
    assert call(dtype=-1) == E_UNSUPPORTED
    assert call(h=0) == E_SHAPE and 'empty source' in _err()                 # an empty source for a non-empty result
    assert call(w=0) == E_SHAPE
    for operand in ('logits', 'labels'):
        assert call(**{operand: None}) == E_NULL and operand in _err() and name in _err()
    assert call(lse=None) == E_NULL and 'lse' in _err()
    assert call(ws=None) == E_NULL and 'ws' in _err()
    assert call(cw=None, logits=None) == E_NULL and 'logits' in _err()       # class_weight is optional
    assert call(cw=None, ws=P + 8) == E_ALIGN
    # misalignment per operand: fp32 logits 4 bytes, 16-bit logits 2, labels 8, fp32 vectors 4, the workspace 16
    assert call(logits=P + 2) == E_ALIGN and 'misaligned' in _err() and 'logits' in _err()
    assert call(logits=P + 1, dtype=1) == E_ALIGN and call(logits=P + 1, dtype=2) == E_ALIGN
    assert call(logits=P + 2, dtype=1, ws=None) == E_NULL                    # 2-byte alignment is enough for 16-bit logits
    assert call(labels=P + 4) == E_ALIGN and 'labels' in _err()
    assert call(cw=P + 2) == E_ALIGN and 'class_weight' in _err()
    assert call(lse=P + 2) == E_ALIGN and 'lse' in _err()
    assert call(ws=P + 8) == E_ALIGN and 'ws' in _err()
    # a row stride smaller than the width, planes and images that overlap
    for kw in (dict(rs=w - 1), dict(ps=h * w - 1), dict(is_=h * w * (C - 1)), dict(ps=0), dict(rs=-w), dict(lrs=W - 1),
               dict(lis=H * W - 1)):
        assert call(**kw) == E_SHAPE, (kw, _err())
        assert 'strides' in _err()
    assert call(ws_bytes=_need() - 1) == E_SHAPE and 'workspace too small' in _err()
    assert call(ws_bytes=0) == E_SHAPE


def test_forward_outputs_and_backward_operands():
    assert forward(loss_sum=None) == E_NULL and 'loss_sum' in _err()
    assert forward(counts=None) == E_NULL and 'counts' in _err()
    assert forward(loss_sum=P + 2) == E_ALIGN and forward(counts=P + 4) == E_ALIGN and 'counts' in _err()
    assert backward(scale=None) == E_NULL and 'scale' in _err()
    assert backward(dlogits=None) == E_NULL and 'dlogits' in _err()
    assert backward(scale=P + 2) == E_ALIGN and backward(dlogits=P + 2) == E_ALIGN
    assert backward(dlogits=P + 2, dtype=2, ws=None) == E_NULL
    for kw in (dict(drs=w - 1), dict(dps=h * w - 1), dict(dis=h * w * (C - 1))):
        assert backward(**kw) == E_SHAPE, (kw, _err())
        assert 'strides' in _err() and 'dlogits' in _err()


@pytest.mark.parametrize('name,call', CALLS)
def test_empty_problems_read_no_pointer(name, call):
    nothing = dict(logits=None, labels=None, cw=None, lse=None, ws=None, ws_bytes=0)
    more = dict(loss_sum=None, counts=None) if call is forward else dict(scale=None, dlogits=None)
    for kw in (dict(N=0), dict(C=0), dict(H=0), dict(W=0)):
        assert call(**nothing, **more, **kw) == OK and _err() == '', kw
        assert call(logits=P + 1, labels=P + 3, rs=0, **kw) == OK
    assert call(N=0, h=0, w=0) == OK
    assert call(N=0, dtype=3) == E_UNSUPPORTED                               # the dtype code is checked first
