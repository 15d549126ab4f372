"""GPU: the masked cross-attention kernels (csrc/masked_attn.hip) by direct C calls against the fp64 reference of
tests/masked_attn_ref.py, in bf16 and fp16, every output and the workspace NaN-filled first.

Pack: the words equal the reference's exactly.  Attention: o, lse, dq, dk, dv are checked with oracle.attention.check against
oracle.attention.budget, unchanged - every element within its budget and ||err|| <= 0.5 ||budget|| - because the kernels'
numerics contract is that of the other attention kernels.  The reference starts from the 16-bit operands the
kernel saw and from the reference's own keep mask.

Mask regimes (on a random-half base, each on every shape that can hold it): 'half'; 'all' (nothing excluded); 'norow' (one row
of logits all negative: the pack rule keeps every key); 'lastkey' (one row keeps only the last key: its output is that v row);
'lastchunk' (one row's kept keys all lie in the last chunk, every earlier chunk is empty for it); 'nochunk' (one whole chunk
excluded for every row).

Worst measured ratios on an MI355X ((a) max err / budget, (b) ||err|| / ||budget||, all 268 runs of
test_attention_against_fp64; the table MEASURED below repeats them):
    bf16   o 0.45 / 0.16   lse 0.26 / 0.08   dq 0.14 / 0.03   dk 0.27 / 0.04   dv 0.61 / 0.18
    fp16   o 0.40 / 0.16   lse 0.28 / 0.08   dq 0.15 / 0.03   dk 0.28 / 0.04   dv 0.62 / 0.17
"""
import math

import pytest
import torch

import _vah
import masked_attn_ref as mref
from oracle import attention as oa
from vitadapter import fused

pytestmark = pytest.mark.gpu

lib = _vah.lib
SCALE = 1.0 / math.sqrt(32)
CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
DTYPES = (torch.bfloat16, torch.float16)

# worst ratios over all cases of test_attention_against_fp64, copied from the RATIO lines of a run on an MI355X
MEASURED = {
    'bf16': 'o 0.45 / 0.16   lse 0.26 / 0.08   dq 0.14 / 0.03   dk 0.27 / 0.04   dv 0.61 / 0.18',
    'fp16': 'o 0.40 / 0.16   lse 0.28 / 0.08   dq 0.15 / 0.03   dk 0.28 / 0.04   dv 0.62 / 0.17',
}


def _rule(Lk):
    """(splits, keys per chunk) by the rule of include/vitadapter_hip_masked_attn.h"""
    tiles = -(-Lk // 64)
    per = -(-tiles // min(16, tiles))
    return -(-tiles // per), 64 * per


C = 1024 // lib.vah_mca_splits(1024)                 # keys per chunk where a chunk is one tile
SHAPES = [(2, 2, 1, 1), (2, 2, 31, 63), (2, 2, 32, 64), (2, 2, 33, 65), (1, 2, 100, 400), (2, 8, 100, 1600), (1, 2, 128, 1000),
          (1, 2, 100, C - 1), (1, 2, 100, C), (1, 2, 100, C + 1), (1, 2, 100, 2 * C + 1),
          (1, 2, 100, 1601),                          # two-tile chunks, the last one ending in a tile of one key
          (1, 8, 100, 6400)]
MASKS = ('half', 'all', 'norow', 'lastkey', 'lastchunk', 'nochunk')


def _dev():
    return torch.device('cuda:0')


def _logits(N, Lq, Lk, regime, seed):
    """fp32 logits (N, Lq, Lk) of a mask regime, or None where the shape cannot hold it"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, Lq, Lk), generator=g)
    x[x == 0] = 1.0
    S, chunk = _rule(Lk)
    row = min(Lq - 1, 37 if Lq > 37 else Lq // 2)       # a row of wave 1 where there is one
    if regime == 'half':
        return x
    if regime == 'all':
        return x.abs()
    if regime == 'norow':
        x[N - 1, row] = -x[N - 1, row].abs()
        return x
    if regime == 'lastkey':
        if Lk < 2:
            return None
        x[N - 1, row] = -x[N - 1, row].abs()
        x[N - 1, row, Lk - 1] = 1.0
        return x
    if regime == 'lastchunk':
        if S < 2:
            return None
        x[0, row, :(S - 1) * chunk] = -x[0, row, :(S - 1) * chunk].abs()
        x[0, row, (S - 1) * chunk:] = x[0, row, (S - 1) * chunk:].abs()
        return x
    if regime == 'nochunk':
        if S < 2:
            return None
        c = S // 2
        x[:, :, c * chunk:(c + 1) * chunk] = -x[:, :, c * chunk:(c + 1) * chunk].abs()
        return x
    raise ValueError(regime)


def _bits_of(keep, dev):
    return torch.from_numpy(mref.pack_bits(keep).astype('uint32').view('int32')).to(dev)


def _nan(shape, dtype, dev):
    return torch.full(shape, float('nan'), dtype=dtype, device=dev)


def _arg(t):
    return t.data_ptr(), CODES[t.dtype], t.stride(0), t.stride(1)


def _direct(q, k, v, do, bits, H):
    """forward + backward by direct C calls; q, do (Lq, N, E), k, v (Lk, N, E) 16-bit (any served strides)"""
    Lq, N, E = q.shape
    Lk = k.shape[0]
    dev, dt = q.device, q.dtype
    st = _vah.raw_stream(dev)
    nws = lib.vah_mca_ws_bytes(N, H, Lq, Lk)
    assert nws % 16 == 0
    ws = _nan((nws // 4,), torch.float32, dev)
    out, lse = _nan((Lq, N, E), dt, dev), _nan((N, H, Lq), torch.float32, dev)
    _vah.check(lib.vah_mca_forward(*_arg(q), *_arg(k), *_arg(v), bits.data_ptr(), N, H, Lq, Lk, 32, SCALE, *_arg(out), lse.data_ptr(),
                                   ws.data_ptr(), nws, st), 'vah_mca_forward')
    ws.fill_(float('nan'))
    dq, dk, dv = _nan((Lq, N, E), dt, dev), _nan((Lk, N, E), dt, dev), _nan((Lk, N, E), dt, dev)
    _vah.check(lib.vah_mca_backward(*_arg(q), *_arg(k), *_arg(v), bits.data_ptr(), *_arg(out), *_arg(do), lse.data_ptr(), N, H, Lq, Lk,
                                    32, SCALE, *_arg(dq), *_arg(dk), *_arg(dv), ws.data_ptr(), nws, st), 'vah_mca_backward')
    torch.cuda.synchronize()
    return dict(o=out, lse=lse, dq=dq, dk=dk, dv=dv)


def _operands(N, H, Lq, Lk, regime, seed, dt):
    return [t.to(_dev(), dt) for t in mref.make_inputs(N, H, Lq, Lk, regime, seed)]


# ----------------------------------------------------------------------------------------------------------------------
# pack
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16, torch.float16], ids=['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('Lk', [1, 31, 32, 33, 400, 1601])
def test_pack_equals_the_reference(Lk, dt):
    dev = _dev()
    N, Q = 2, 7
    g = torch.Generator().manual_seed(Lk)
    # strided rows: the logits are columns 3 .. 3 + Lk of a wider buffer
    buf = torch.randn((N, Q, Lk + 5), generator=g).to(dt)
    x = buf[:, :, 3:3 + Lk]
    specials = [0.0, -0.0, float('nan'), float('inf'), float('-inf'), -1e-30 if dt != torch.float16 else -6e-8, 1e-30]
    for i, s in enumerate(specials):
        if i < Lk:
            x[0, 0, (i * 5) % Lk] = s
    x[0, 1] = -x[0, 1].abs() - 1.0                       # keeps nothing: keeps everything
    x[1, 2] = -x[1, 2].abs() - 1.0                       # keeps one key, the last
    x[1, 2, Lk - 1] = 0.0
    x[1, 3] = float('-inf')                              # keeps nothing
    x[1, 4] = float('nan')                               # keeps everything
    want = mref.pack_bits(mref.keep_rule(x.float()))
    W = (Lk + 31) // 32
    xd = buf.to(dev)[:, :, 3:3 + Lk]
    assert xd.stride(1) == Lk + 5
    bits = torch.full((N, Q, W), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    _vah.check(lib.vah_mca_pack_mask(xd.data_ptr(), CODES[dt], xd.stride(1), xd.stride(0), N, Q, Lk, bits.data_ptr(),
                                     _vah.raw_stream(dev)), 'vah_mca_pack_mask')
    torch.cuda.synchronize()
    got = mref.words_of(bits)
    assert (got == want).all(), (Lk, dt)
    full = [0xFFFFFFFF] * (Lk // 32) + ([(1 << (Lk % 32)) - 1] if Lk % 32 else [])
    assert got[0, 1].tolist() == full and got[1, 3].tolist() == full and got[1, 4].tolist() == full
    assert int(got[:, :, -1].max()) < (1 << ((Lk - 1) % 32 + 1))                 # pad bits are zero
    # the glue's wrapper gives the same words
    assert (mref.words_of(fused.mca_pack_mask(xd)) == want).all()


# ----------------------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_attention_against_fp64(shape, dt):
    N, H, Lq, Lk = shape
    dev = _dev()
    assert lib.vah_mca_splits(Lk) == _rule(Lk)[0]
    worst = {}
    ran = 0
    for mi, mask in enumerate(MASKS):
        x = _logits(N, Lq, Lk, mask, 11 + mi)
        if x is None:
            continue
        keep = mref.keep_rule(x)
        bits = _bits_of(keep, dev)
        for ri, regime in enumerate(('peaked', 'flat')):
            q, k, v, do = _operands(N, H, Lq, Lk, regime, 7 * mi + ri, dt)
            got = _direct(q, k, v, do, bits, H)
            ref = mref.reference(*(mref.heads(t, H) for t in (q, k, v, do)), keep.to(dev), SCALE)
            for name in ('o', 'lse', 'dq', 'dk', 'dv'):
                g = got[name] if name == 'lse' else mref.heads(got[name], H)
                a, b = oa.ratios(g, ref[name], oa.budget(ref, name, dt))
                print('RATIO %s %s %s %s %s: %.3f %.3f' % ('x'.join(map(str, shape)), str(dt)[6:], mask, regime, name, a, b))
                wa, wb = worst.get(name, (0.0, 0.0))
                worst[name] = (max(wa, a), max(wb, b))
                oa.check('%s %s %s %s' % (shape, mask, regime, name), g, ref[name], oa.budget(ref, name, dt))
            if mask == 'lastkey':
                row = min(Lq - 1, 37 if Lq > 37 else Lq // 2)
                o_row, v_row = got['o'][row, N - 1].double(), v[Lk - 1, N - 1].double()
                assert bool(((o_row - v_row).abs() <= oa.UNIT[dt] * v_row.abs()).all()), 'the only kept key: o is its v row'
            ran += 1
    assert ran >= 6
    print('WORST %s %s: %s' % ('x'.join(map(str, shape)), str(dt)[6:],
                               '   '.join('%s %.2f / %.2f' % (n, a, b) for n, (a, b) in worst.items())))


@pytest.mark.parametrize('dt', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape', [(2, 2, 33, 65), (2, 8, 100, 1600)], ids=lambda s: 'x'.join(map(str, s)))
def test_two_runs_the_function_and_strided_operands_give_the_same_bits(shape, dt):
    N, H, Lq, Lk = shape
    dev = _dev()
    E = H * 32
    x = _logits(N, Lq, Lk, 'norow', 5)
    bits = _bits_of(mref.keep_rule(x), dev)
    q, k, v, do = _operands(N, H, Lq, Lk, 'peaked', 3, dt)
    first = _direct(q, k, v, do, bits, H)
    for t in first.values():
        assert bool(torch.isfinite(t.float()).all())
    again = _direct(q, k, v, do, bits, H)
    for name in first:
        assert torch.equal(first[name], again[name]), name
    # k and v as column slices of a packed (Lk, N, 2E) projection, q and dO as slices of wider buffers
    kv = torch.cat([k, v], dim=2)
    qq = torch.cat([do, q, do], dim=2)
    strided = _direct(qq[:, :, E:2 * E], kv[:, :, :E], kv[:, :, E:], qq[:, :, 2 * E:], bits, H)
    for name in first:
        assert torch.equal(first[name], strided[name]), name
    # the autograd.Function around the same calls (the pack kernel's words for the same logits)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, kv[:, :, :E], kv[:, :, E:]))
    out = fused._MaskedCrossAttention.apply(qa, ka, va, fused.mca_pack_mask(x.to(dev)), H, SCALE)
    dq, dk, dv = torch.autograd.grad(out, (qa, ka, va), do)
    torch.cuda.synchronize()
    for name, t in (('o', out.detach()), ('dq', dq), ('dk', dk), ('dv', dv)):
        assert torch.equal(first[name], t), name
    # and masked_cross_attention under autocast from fp32 operands that round to the same 16-bit values
    with torch.autocast('cuda', dtype=dt):
        qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
        out2 = fused.masked_cross_attention(qf, kf, vf, x.to(dev), H)
    dq2, dk2, dv2 = torch.autograd.grad(out2, (qf, kf, vf), do)
    for name, t in (('o', out2.detach()), ('dq', dq2), ('dk', dk2), ('dv', dv2)):
        assert torch.equal(first[name].float(), t.float()), name
