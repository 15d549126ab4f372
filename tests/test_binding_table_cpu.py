"""CPU: the ctypes binding (_vah.SIGNATURES, the fp16 twin table, sym / call) against include/vitadapter_hip.h, and the
two autocast-type questions of vitadapter/fused.py.  Nothing here launches GPU work: the entry points are only looked
at, or called with arguments they reject before touching a device."""
import contextlib
import ctypes
import itertools
import os
import re

import pytest
import torch

import _vah

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = _vah.lib
GROUPS = {'attn': _vah.ATTN_F16_TWINS, 'fused': _vah.FUSED_F16_TWINS, 'linear': _vah.LINEAR_F16_TWINS,
          'spm': _vah.SPM_F16_TWINS, 'tail': _vah.TAIL_F16_TWINS}
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}
RETURNS = dict(SCALARS, **{'const char *': ctypes.c_char_p})


def _param(text):
    """One parameter of a prototype -> the ctypes types the binding may declare for it."""
    if '*' in text:
        base = text[:text.index('*')].replace('const', '').strip()
        if base == 'char':                 # text in (const) or a host buffer the library writes text to
            return (ctypes.c_char_p,)
        if base == 'int64_t':
            return (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64))
        return (ctypes.c_void_p,)
    words = text.replace('const', '').split()
    assert len(words) == 2 and words[0] in SCALARS, 'parameter the test cannot read: %r' % text
    return (SCALARS[words[0]],)


def _prototypes():
    """{name: (restype, [allowed argtypes per position])} of every vah_* prototype of the header."""
    src = open(os.path.join(ROOT, 'include', 'vitadapter_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)
    out = {}
    for ret, name, params in re.findall(r'\b(int64_t|int|const char \*)\s*(vah_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        params = ' '.join(params.split())
        assert name not in out, name
        out[name] = (RETURNS[ret], [] if params == 'void' else [_param(p.strip()) for p in params.split(',')])
    return out


PROTOTYPES = _prototypes()


def test_every_signature_matches_its_prototype():
    assert len(PROTOTYPES) == len(_vah.EXPORTS) == 122 and set(PROTOTYPES) == set(_vah.EXPORTS)
    assert len(_vah.SIGNATURES) == 79 and not set(_vah.SIGNATURES) & set(_vah.F16_TWINS.values())
    for name, (restype, params) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype, restype)
        got = list(fn.argtypes or [])
        assert len(got) == len(params), (name, len(got), len(params))
        for i, (g, allowed) in enumerate(zip(got, params)):
            assert g in allowed, (name, i, g, allowed)
    for name, (restype, argtypes) in _vah.SIGNATURES.items():       # every entry states both, none leans on a ctypes default
        assert restype is not None and isinstance(argtypes, list), name


def test_twin_table():
    for (ka, a), (kb, b) in itertools.combinations(GROUPS.items(), 2):
        assert not set(a) & set(b) and not set(a.values()) & set(b.values()), (ka, kb)
    union = {}
    for g in GROUPS.values():
        union.update(g)
    assert union == _vah.F16_TWINS and len(_vah.F16_TWINS) == 43
    assert [len(g) for g in GROUPS.values()] == [8, 10, 7, 10, 8]
    assert sorted(_vah.F16_TWINS.values()) == sorted(n for n in PROTOTYPES if '_f16' in n)
    assert len(set(_vah.F16_TWINS.values())) == 43 and set(_vah.F16_TWINS) <= set(_vah.SIGNATURES)
    for b16, f16 in _vah.F16_TWINS.items():
        assert getattr(lib, f16).argtypes == getattr(lib, b16).argtypes and getattr(lib, f16).restype is getattr(lib, b16).restype
    assert _vah.F16_TWINS['vah_residual_layernorm_bwd_bsum'] == 'vah_residual_layernorm_bwd_f16_bsum'      # irregular, kept


def test_resolver():
    for b16, f16 in _vah.F16_TWINS.items():
        assert _vah.sym(b16, torch.bfloat16) is getattr(lib, b16)
        assert _vah.sym(b16, torch.float16) is getattr(lib, f16)
        assert _vah.sym(b16, torch.float16).__name__ == f16
        with pytest.raises(ValueError, match=b16 + '.*float32'):
            _vah.sym(b16, torch.float32)
    assert _vah.sym('vah_colsum_f32', torch.bfloat16) is lib.vah_colsum_f32
    with pytest.raises(ValueError, match='vah_colsum_f32.*float16'):
        _vah.sym('vah_colsum_f32', torch.float16)
    with pytest.raises(ValueError, match='vah_gemm_f16.*bfloat16'):       # asked for by the bf16 spelling only
        _vah.sym('vah_gemm_f16', torch.bfloat16)


def test_call_raises_under_the_name_of_the_symbol_that_ran():
    P = 4096            # a non-null, aligned fake pointer: the call is rejected (C % 4) before anything is dereferenced
    args = (P, P, P, 8, 66, 1e-6, P, P, P, None)
    for dtype, name in ((torch.bfloat16, 'vah_layernorm_fwd_f32_bf16'), (torch.float16, 'vah_layernorm_fwd_f32_f16')):
        with pytest.raises(RuntimeError, match=r'^%s failed \(code -2\): %s:' % (name, name)):
            _vah.call('vah_layernorm_fwd_f32_bf16', dtype, *args)
    assert _vah.call('vah_layernorm_fwd_f32_bf16', torch.float16, None, P, P, 0, 64, 1e-6, None, P, P, None) is None     # zero rows


@contextlib.contextmanager
def _cuda_autocast(dtype):
    """The state torch.autocast('cuda', dtype=dtype) sets; the context manager itself switches autocast off on a host
    without a device."""
    prev = (torch.is_autocast_enabled('cuda'), torch.get_autocast_dtype('cuda'))
    torch.set_autocast_enabled('cuda', dtype is not None)
    if dtype is not None:
        torch.set_autocast_dtype('cuda', dtype)
    try:
        yield
    finally:
        torch.set_autocast_enabled('cuda', prev[0])
        torch.set_autocast_dtype('cuda', prev[1])


@pytest.mark.parametrize('switch', ['fp16_rows', 'fp16_linear', 'fp16_tail', 'fp16_spm'])
def test_autocast_helper(switch):
    from vitadapter import fused, spm_nhwc
    bf16, f16 = torch.bfloat16, torch.float16
    wrappers = {'fp16_tail': [fused.tail_dtype], 'fp16_spm': [spm_nhwc.autocast_dtype]}.get(switch, [])
    asks = [lambda: fused.autocast_16(switch)] + wrappers
    assert fused.ENABLED[switch] is True
    for ask in asks:
        with _cuda_autocast(None):
            assert ask() is None
        with _cuda_autocast(bf16):
            assert ask() == bf16
        with _cuda_autocast(f16):
            assert ask() == f16
        with _cuda_autocast(torch.float32):
            assert ask() is None
    assert fused.takes_16(bf16, switch) and fused.takes_16(f16, switch) and not fused.takes_16(torch.float32, switch)
    fused.ENABLED[switch] = False
    try:
        for ask in asks:
            with _cuda_autocast(f16):
                assert ask() is None
            with _cuda_autocast(bf16):
                assert ask() == bf16
            with _cuda_autocast(None):
                assert ask() is None
        assert fused.takes_16(bf16, switch) and not fused.takes_16(f16, switch) and not fused.takes_16(torch.float32, switch)
        others = [s for s in ('fp16_rows', 'fp16_linear', 'fp16_tail', 'fp16_spm') if s != switch]
        with _cuda_autocast(f16):
            assert all(fused.autocast_16(s) == f16 for s in others)          # a switch governs its own family only
            assert fused._maps_dtype() == (bf16 if switch == 'fp16_tail' else f16)
    finally:
        fused.ENABLED[switch] = True
    with _cuda_autocast(bf16):
        assert fused._bf16_autocast() and fused._maps_dtype() == bf16
    with _cuda_autocast(f16):
        assert not fused._bf16_autocast()
    assert not torch.is_autocast_enabled('cuda')
