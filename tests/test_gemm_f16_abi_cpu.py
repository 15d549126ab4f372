"""CPU: the fp16 entry points of the Linear path (include/vitadapter_hip.h): vah_gemm_f16 / vah_gemm_f16_fin of
csrc/gemm.hip and the fp16 twins of the column-sum, GELU-backward and `_bsum` residual kernels of csrc/fused_ops.hip.
Each is its bf16 entry point's twin: for the argument sets the bf16 entry rejects before anything touches a device it
returns the same VAH_E_* code with the same message, the function name changed.  (The dispatcher checks no alignment
and sizes the workspace only once it holds a hipBLASLt handle, which needs a device: the workspace cases here are the
ones refused before that - a negative size, a size without a pointer.)  The table text takes `f16 ` lines beside the
bf16 ones."""
import ctypes

import pytest

import _vah

lib = _vah.lib
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
P = 4096           # a non-null, 16-byte aligned fake pointer: never dereferenced by a rejected call


def _gemm(ta=0, tb=0, M=8, N=8, K=8, A=P, lda=8, B=P, ldb=8, D=P, ldd=8, d32=0, epi=0, bias=None, bias32=0, ws=P, ws_bytes=1024):
    return (ta, tb, M, N, K, A, lda, B, ldb, D, ldd, d32, epi, bias, bias32, ws, ws_bytes, None)


def _gemm_fin(ta=1, tb=0, M=8, N=8, K=8, A=P, lda=8, B=P, ldb=8, D=P, ldd=8, d32=1, ws=P, ws_bytes=1024, part=P, nparts=2,
              C=8, out=P):
    return (ta, tb, M, N, K, A, lda, B, ldb, D, ldd, d32, ws, ws_bytes, part, nparts, C, out, None)


def _colsum(g=P, rows=4, C=64, out=P, ws=P):
    return (g, rows, C, out, ws, None)


def _colsum_partials(g=P, rows=4, C=64, ws=P, n=True):
    return (g, rows, C, ws, ctypes.byref(ctypes.c_int64(-1)) if n else None, None)


def _gelu(da=P, h=P, rows=4, C=64, dh=P, bpart=P, n=True):
    return (da, h, rows, C, dh, bpart, ctypes.byref(ctypes.c_int64(-1)) if n else None, None)


def _res_ln(t=P, gh=P, z=P, gamma=None, dgamma=None, batch=2, rpb=4, C=64, dz=P, dw=P, bpart=P, n=True):
    return (t, gh, P, P, P, None, z, gamma, None, batch, rpb, C, P, dz, dgamma, dw, P, P, bpart,
            ctypes.byref(ctypes.c_int64(-1)) if n else None, None)


def _sr(g=P, z=P, gamma=None, batch=2, rpb=4, C=64, dz=P, dgamma=None, ws=None, bpart=P, n=True):
    return (g, z, gamma, None, batch, rpb, C, dz, dgamma, ws, bpart, ctypes.byref(ctypes.c_int64(-1)) if n else None, None)


# (bf16 entry, argument builder, [(case, kwargs, expected rc)])
CASES = [
    ('vah_gemm_bf16', _gemm, [
        ('negative M', dict(M=-1), E_SHAPE), ('negative K', dict(K=-1), E_SHAPE), ('K = 0', dict(K=0), E_SHAPE),
        ('null A', dict(A=None), E_NULL), ('null B', dict(B=None), E_NULL), ('null D', dict(D=None), E_NULL),
        ('lda too small', dict(lda=7), E_SHAPE), ('lda too small, transposed', dict(ta=1, M=16, lda=8), E_SHAPE),
        ('ldb too small', dict(tb=1, K=16, lda=16, ldb=8), E_SHAPE), ('ldd too small', dict(ldd=4), E_SHAPE),
        ('unknown epilogue', dict(epi=7), E_SHAPE), ('bias epilogue without bias', dict(epi=1), E_NULL),
        ('bias without its epilogue', dict(bias=P), E_NULL), ('negative workspace', dict(ws_bytes=-1), E_NULL),
        ('workspace size without pointer', dict(ws=None), E_NULL),
        ('no rows', dict(M=0, A=None, D=None), 0), ('no columns', dict(N=0, B=None, D=None), 0)]),
    ('vah_gemm_bf16_fin', _gemm_fin, [
        ('null partials', dict(part=None), E_SHAPE), ('null finalize output', dict(out=None), E_SHAPE),
        ('no partial rows', dict(nparts=0), E_SHAPE), ('no columns to sum', dict(C=0), E_SHAPE),
        ('too many partial rows', dict(nparts=(1 << 20) + 1), E_SHAPE), ('negative N', dict(N=-1), E_SHAPE),
        ('K = 0', dict(K=0), E_SHAPE), ('null A', dict(A=None), E_NULL), ('lda too small', dict(lda=4), E_SHAPE),
        ('negative workspace', dict(ws_bytes=-8), E_NULL), ('workspace size without pointer', dict(ws=None), E_NULL)]),
    ('vah_colsum_bf16', _colsum, [
        ('C % 8', dict(C=60), E_SHAPE), ('bad rows', dict(rows=-1), E_SHAPE), ('null out', dict(out=None), E_NULL),
        ('null ws', dict(ws=None), E_NULL), ('null g', dict(g=None), E_NULL), ('misaligned g', dict(g=P + 8), E_ALIGN)]),
    ('vah_colsum_bf16_partials', _colsum_partials, [
        ('no rows', dict(rows=0), E_SHAPE), ('C % 8', dict(C=4), E_SHAPE), ('C too large', dict(C=(1 << 20) + 8), E_SHAPE),
        ('null g', dict(g=None), E_NULL), ('null count', dict(n=False), E_NULL), ('misaligned g', dict(g=P + 2), E_ALIGN)]),
    ('vah_gelu_bwd_bsum_bf16', _gelu, [
        ('C % 8', dict(C=60), E_SHAPE), ('bad rows', dict(rows=-1), E_SHAPE), ('null h', dict(h=None), E_NULL),
        ('null partials', dict(bpart=None), E_NULL), ('null count', dict(n=False), E_NULL),
        ('misaligned da', dict(da=P + 8), E_ALIGN), ('misaligned dh', dict(dh=P + 8), E_ALIGN),
        ('no rows', dict(da=None, h=None, dh=None, rows=0), 0)]),
    ('vah_residual_layernorm_bwd_bsum', _res_ln, [
        ('bad dims', dict(rpb=-1), E_SHAPE), ('null z', dict(z=None), E_NULL), ('null dz', dict(dz=None), E_NULL),
        ('gamma without dgamma', dict(gamma=P), E_NULL), ('dgamma without gamma', dict(dgamma=P), E_NULL),
        ('a layer scale', dict(gamma=P, dgamma=P), E_SHAPE), ('misaligned dz', dict(dz=P + 2), E_ALIGN),
        ('C % 4', dict(C=66), E_SHAPE), ('null dw', dict(dw=None), E_NULL), ('misaligned gh', dict(gh=P + 4), E_ALIGN),
        ('null partials', dict(bpart=None), E_NULL), ('null count', dict(n=False), E_NULL),
        ('misaligned partials', dict(bpart=P + 8), E_ALIGN)]),
    ('vah_scale_residual_bwd_bsum', _sr, [
        ('bad dims', dict(rpb=-1), E_SHAPE), ('C % 4', dict(C=6), E_SHAPE), ('null dz', dict(dz=None), E_NULL),
        ('dgamma without ws', dict(gamma=P, dgamma=P), E_NULL), ('misaligned dz', dict(dz=P + 4), E_ALIGN),
        ('misaligned g', dict(g=P + 8), E_ALIGN), ('null partials', dict(bpart=None), E_NULL),
        ('null count', dict(n=False), E_NULL), ('misaligned partials', dict(bpart=P + 8), E_ALIGN),
        ('zero rows', dict(g=None, z=None, dz=None, batch=0), 0)]),
]


def test_the_table_covers_every_linear_twin():
    assert sorted(c[0] for c in CASES) == sorted(_vah.LINEAR_F16_TWINS)
    assert not set(_vah.LINEAR_F16_TWINS) & set(_vah.FUSED_F16_TWINS)
    for f16 in _vah.LINEAR_F16_TWINS.values():
        assert f16 in _vah.EXPORTS and 'f16' in f16 and 'bf16' not in f16, f16


@pytest.mark.parametrize('name,build,cases', CASES, ids=[c[0] for c in CASES])
def test_f16_entry_checks_arguments_like_its_bf16_twin(name, build, cases):
    f16 = _vah.LINEAR_F16_TWINS[name]
    assert getattr(lib, f16).argtypes == getattr(lib, name).argtypes
    for case, kw, want in cases:
        rc16 = getattr(lib, f16)(*build(**kw))
        msg16 = lib.vah_last_error().decode()
        rcb = getattr(lib, name)(*build(**kw))
        msgb = lib.vah_last_error().decode()
        assert rcb == want, (name, case, rcb, msgb)
        assert rc16 == want, (f16, case, rc16, msg16)
        if want:
            assert msg16.startswith(f16 + ':') or msg16.startswith(f16 + '_partials:'), (case, msg16)
            assert msg16 == msgb.replace(name, f16), (case, msg16, msgb)
        else:
            assert msg16 == '', (case, msg16)


def test_host_picks_the_entry_by_type_cpu():
    import torch
    from vitadapter import fused
    assert fused.ENABLED['fp16_linear'] is True and fused.autocast_16('fp16_linear') is None         # no autocast here
    assert fused.takes_16(torch.bfloat16, 'fp16_linear') and fused.takes_16(torch.float16, 'fp16_linear') and not fused.takes_16(torch.float32, 'fp16_linear')
    fused.ENABLED['fp16_linear'] = False
    try:
        assert fused.takes_16(torch.bfloat16, 'fp16_linear') and not fused.takes_16(torch.float16, 'fp16_linear')
    finally:
        fused.ENABLED['fp16_linear'] = True
    for b16, f16 in _vah.LINEAR_F16_TWINS.items():
        assert _vah.sym(b16, torch.bfloat16) is getattr(lib, b16)
        assert _vah.sym(b16, torch.float16) is getattr(lib, f16)
    assert fused.gemm_bf16 is fused.gemm_16
    lin = torch.nn.Linear(8, 16)
    x = torch.randn(2, 3, 8)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        y = fused.linear(lin, x)                  # a CPU tensor takes the module
    assert not hasattr(y, fused._BiasPartials.ATTR)
    # a copy is looked up by (parameter, type): never the other type's
    copies = fused._Bf16Copies()
    assert copies.get(lin.weight, torch.float16).dtype == torch.float16 and copies.get(lin.weight).dtype == torch.bfloat16
    copies.begin([lin.weight], torch.float16)
    try:
        assert copies.get(lin.weight, torch.float16) is copies.get(lin.weight, torch.float16)
        assert copies.get(lin.weight, torch.bfloat16).dtype == torch.bfloat16
        assert torch.equal(copies.get(lin.weight, torch.float16), lin.weight.detach().half())
    finally:
        copies.end()
    pair = fused._PairCopies()
    a, b = torch.nn.Linear(8, 8), torch.nn.Linear(8, 16)
    assert pair.get(a, b, torch.float16)[0].dtype == torch.float16 and pair.get(a, b)[0].dtype == torch.bfloat16


# shapes no model or test runs: the table is the process's, and an entry that is never used is never resolved
BF16_LINES = ('1 0 1 0 0 7 9 11 7 9 9 1234 8 57.5\n'
              '0 1 0 1 1 13 17 19 19 19 17 77 1 101.25\n')


def _dump():
    n = lib.vah_gemm_table_dump(None, 0)
    buf = ctypes.create_string_buffer(int(n))
    lib.vah_gemm_table_dump(buf, n)
    return buf.value.decode()


def test_table_text_takes_f16_lines():
    """The raw C entry points (the Python wrapper's version line needs a device).  A bf16-only text counts as before; an
    `f16 ` line is an entry of its own even where the rest of the line equals a bf16 one, no fp16 line starts like a
    bf16 line, the dump loads back, and a malformed `f16` line is refused."""
    before = _dump()
    base = len(before.splitlines())
    assert lib.vah_gemm_table_load(BF16_LINES.encode()) == 2
    assert len(_dump().splitlines()) == base + 2
    f16 = ''.join('f16 ' + ln + '\n' for ln in BF16_LINES.splitlines())
    assert lib.vah_gemm_table_load(('# a comment\n' + BF16_LINES + f16).encode()) == 4
    text = _dump()
    lines = text.splitlines()
    assert len(lines) == base + 4
    for ln in BF16_LINES.splitlines():
        key = ' '.join(ln.split()[:11]) + ' '
        assert len([t for t in lines if t.startswith(key)]) == 1, 'an fp16 line does not match a bf16 prefix'
        got = [t for t in lines if t.startswith('f16 ' + key)]
        assert len(got) == 1 and got[0].split()[12:14] == ln.split()[11:13], got
    for t in lines:
        assert len(t.split()) == (15 if t.startswith('f16 ') else 14), t
    assert lib.vah_gemm_table_load(text.encode()) == len(lines)
    assert _dump() == text
    for bad in ('f16 1 0 1 0 0 768 768\n', 'f16\n', 'f16 x 0 1 0 0 1 1 1 1 1 1 1 1 1\n', 'f16 f16 ' + BF16_LINES):
        assert lib.vah_gemm_table_load(bad.encode()) == E_SHAPE, bad
        assert b'vah_gemm_table_load: malformed line' in lib.vah_last_error()
