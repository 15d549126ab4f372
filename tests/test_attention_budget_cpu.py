"""CPU: the error budgets of oracle/attention.py against a CPU emulation of the attention kernels' numerics.

The emulation follows DESIGN 4.4: scores, max, sum, lse, delta and every accumulator in fp32, P and dS rounded to the
16-bit type once each, every output rounded once.  The normaliser is the sum of the T-rounded P (whole-sequence
kernels) or of the fp32 P (resident window kernels).  An honest kernel must use at most half of every budget, in both
checks: else the budgets are too tight for the GPU to pass reliably.  Emulated bugs must fail the checks: else the
budgets are too loose to be worth having.  Raising oracle.attention.C to 64 makes the mutant cases here pass their
check, so this file fails."""
import pytest
import torch

from oracle import attention as oa

SCALE = 64 ** -0.5
DTYPES = [torch.bfloat16, torch.float16]


def _operands(B, N, H, regime, seed, dtype):
    qkv, dout = oa.make_inputs(B, N, H, regime, seed, SCALE)
    q, k, v = (t.to(dtype).transpose(1, 2).contiguous() for t in qkv.unbind(2))      # (B, H, N, 64)
    return q, k, v, dout.to(dtype).transpose(1, 2).contiguous()


def _emulate(q, k, v, do, scale, bias2=None, fp32_sum=False, mutant=None):
    """Kernel numerics on the CPU.  bias2: the 16-bit (H, N, N) bias * log2(e) operand.  Mutants: 'extra_keys' (keys padded
    to a multiple of 32 with zero rows join the forward softmax), 'drop_tile' (the forward drops the last 64-key tile),
    'dkdv_short' (dK, dV leave out the last 32 queries)."""
    T = q.dtype
    qf, kf, vf, gf = (t.float() for t in (q, k, v, do))
    N = q.shape[2]
    sl2 = scale * oa.LOG2E
    s = (qf @ kf.transpose(-1, -2)) * sl2
    if bias2 is not None:
        s = s + bias2.float()
    sf, vff = s, vf
    if mutant == 'extra_keys':
        extra = -N % 32
        sf = torch.cat((s, s.new_zeros(s.shape[:-1] + (extra,))), -1)
        vff = torch.cat((vf, vf.new_zeros(vf.shape[:-2] + (extra, 64))), -2)
    elif mutant == 'drop_tile':
        keep = (N - 1) // 64 * 64
        sf, vff = s[..., :keep], vf[..., :keep, :]
    m = sf.amax(-1, keepdim=True)
    p = torch.exp2(sf - m)
    pt = p.to(T).float()
    l = (p if fp32_sum else pt).sum(-1, keepdim=True)
    o = ((pt @ vff) / l).to(T)
    lse = (m + torch.log2(l)).squeeze(-1)

    delta = (o.float() * gf).sum(-1, keepdim=True)
    p = torch.exp2(s - lse[..., None])
    ds = p * (gf @ vf.transpose(-1, -2) - delta)
    dst, pt = ds.to(T).float(), p.to(T).float()
    dq = (dst @ kf * scale).to(T)
    nq = N - 32 if mutant == 'dkdv_short' else N
    dk = (dst[..., :nq, :].transpose(-1, -2) @ qf[..., :nq, :] * scale).to(T)
    dv = (pt[..., :nq, :].transpose(-1, -2) @ gf[..., :nq, :]).to(T)
    got = {'o': o, 'lse': lse, 'dq': dq, 'dk': dk, 'dv': dv}
    if bias2 is not None:
        got['dbias'] = ds.to(T).double().sum(0)
    return got


def _ratios(got, ref, dtype):
    return {n: oa.ratios(g, ref[n], oa.budget(ref, n, dtype)) for n, g in got.items()}


def _case(B, N, H, regime, seed, dtype, bias=False, fp32_sum=False, mutant=None):
    q, k, v, do = _operands(B, N, H, regime, seed, dtype)
    bias2 = None
    if bias:
        g = torch.Generator().manual_seed(seed + 1)
        bias2 = (torch.randn((H, N, N), generator=g) * oa.LOG2E).to(dtype)
    got = _emulate(q, k, v, do, SCALE, bias2, fp32_sum, mutant)
    ref = oa.reference(q, k, v, do, SCALE, None if bias2 is None else bias2.double() / oa.LOG2E)
    return got, ref


HONEST = [(2, 1, 2, False), (2, 63, 2, False), (2, 65, 2, False), (2, 196, 2, True), (2, 333, 2, False),
          (1, 1024, 2, False), (2, 197, 2, False)]


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('regime', ['peaked', 'flat', 'late'])
@pytest.mark.parametrize('B,N,H,fp32_sum', HONEST)
def test_honest_emulation_uses_under_half_the_budget(B, N, H, fp32_sum, regime, dtype):
    got, ref = _case(B, N, H, regime, N + 7, dtype, fp32_sum=fp32_sum)
    for n, (a, b) in _ratios(got, ref, dtype).items():
        assert a < 0.5 and b < 0.5 * oa.L2_FRACTION, (n, a, b)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('regime', ['peaked', 'flat'])
def test_honest_emulation_with_bias(regime, dtype):
    got, ref = _case(2, 197, 2, regime, 11, dtype, bias=True)
    r = _ratios(got, ref, dtype)
    assert set(r) == {'o', 'lse', 'dq', 'dk', 'dv', 'dbias'}
    for n, (a, b) in r.items():
        assert a < 0.5 and b < 0.5 * oa.L2_FRACTION, (n, a, b)


def _fails(got, ref, dtype, names):
    """True when at least one of `names` fails oracle.attention.check."""
    for n in names:
        try:
            oa.check(n, got[n], ref[n], oa.budget(ref, n, dtype))
        except AssertionError:
            return True
    return False


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('N', [196, 100, 33])
def test_extra_zero_keys_fail(N, dtype):
    """The window forward's mask at 32 NB instead of N: zero keys join the softmax.  Flat inputs: every output moves."""
    got, ref = _case(2, N, 2, 'flat', N, dtype, fp32_sum=True, mutant='extra_keys')
    assert _fails(got, ref, dtype, ['o'])


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('regime', ['peaked', 'flat'])
@pytest.mark.parametrize('N', [65, 333, 1024])
def test_dropped_last_key_tile_fails(N, regime, dtype):
    got, ref = _case(1, N, 2, regime, N, dtype, mutant='drop_tile')
    assert _fails(got, ref, dtype, ['o'])


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('regime', ['peaked', 'flat'])
@pytest.mark.parametrize('N', [64, 196, 1024])
def test_dkdv_missing_last_queries_fail(N, regime, dtype):
    got, ref = _case(1, N, 2, regime, N, dtype, fp32_sum=True, mutant='dkdv_short')
    assert _fails(got, ref, dtype, ['dk', 'dv'])
