"""A toy model with one module of every kind vitadapter/fused.py::_EpochCopies writes jobs for, the torch expressions the
code uses for their 16-bit copies when ENABLED['epoch_copies'] is off (``expected``), and the copies an open forward epoch
serves (``served``).  Shared by tests/test_epoch_table_cpu.py and tests/test_epoch_copies_gpu.py."""
import torch
import torch.nn.functional as F


class Pair(torch.nn.Module):
    """what fused.msda_pair_core and the job table read of an MSDeformAttn module"""

    def __init__(self, M, L, P, K):
        super().__init__()
        self.n_heads, self.n_levels, self.n_points = M, L, P
        self.sampling_offsets = torch.nn.Linear(K, M * L * P * 2)
        self.attention_weights = torch.nn.Linear(K, M * L * P)


class Toy(torch.nn.Module):
    """``width``: channels of the 3x3 convolutions - 16 for the copies alone, 64 (the narrowest the 3x3 kernels take) where
    the model runs."""

    def __init__(self, width=16):
        super().__init__()
        nn = torch.nn
        self.lin1, self.lin2 = nn.Linear(24, 16), nn.Linear(16, 5)        # a 5-element bias: a tail that is no multiple of 4
        self.pair1, self.pair2 = Pair(2, 1, 4, 16), Pair(3, 3, 4, 24)
        self.conv_a = nn.Conv2d(3, width, 3, padding=1, bias=False)
        self.conv_b = nn.Conv2d(width, width, 3, padding=1, bias=False)
        self.fc = nn.Conv2d(width, 24, 1)
        self.up = nn.ConvTranspose2d(16, 8, 2, 2)
        self.patch = nn.Conv2d(3, 16, 8, 8)


def specials():
    """fp32 values whose cast has a case of its own: +-inf, NaN, beyond fp16's range (65520 is the first value that rounds
    to inf), fp16 / bf16 / fp32 subnormals, and ties between two bf16 (8 mantissa bits) or fp16 (11 bits) neighbours, to
    even and to odd."""
    inf, nan = float('inf'), float('nan')
    return torch.tensor([inf, -inf, nan, 65520.0, 65519.996, -65520.0, 1e38, -3e38, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -14 * 0.75,
                         2.0 ** -133, -2.0 ** -140, 2.0 ** -149, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8),
                         1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -11 - 2.0 ** -23, 0.0, -0.0],
                        dtype=torch.float32)


def plant(model, seed=0, special=True):
    """Seeded weights, with the special values written over the first and the last elements of every weight matrix."""
    g = torch.Generator().manual_seed(seed)
    sp = specials()
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
            if special and p.dim() > 1:
                flat = p.view(-1)
                n = min(sp.numel(), flat.numel() // 2)
                flat[:n] = sp[:n].to(p.device)
                flat[-n:] = sp[:n].flip(0).to(p.device)
    return model


def _pair_rows(pair):
    M = pair.n_heads
    na, nb = pair.sampling_offsets.weight.shape[0], pair.attention_weights.weight.shape[0]
    po, pl = na // M, nb // M
    return torch.cat([torch.cat((torch.arange(m * po, (m + 1) * po), na + torch.arange(m * pl, (m + 1) * pl))) for m in range(M)])


def expected(model, t16):
    """name -> the copy as the per-use code makes it (fused._Bf16Copies.get, _PairCoreCopies.get, spm_nhwc._Conv3x3 with
    conv.forward_weight / dgrad_weight, fused._UpFromTokens)."""
    from vitadapter import conv
    out = {}
    with torch.no_grad():
        for name in ('lin1', 'lin2') + (('fc', 'patch') if t16 == torch.bfloat16 else ()):
            m = getattr(model, name)
            out[name + '.weight'] = m.weight.detach().to(t16)
        for name in ('lin1', 'lin2'):
            out[name + '.bias'] = getattr(model, name).bias.detach().to(t16)
        for name in ('pair1', 'pair2'):
            pair = getattr(model, name)
            a, b = pair.sampling_offsets, pair.attention_weights
            for lin, tag in ((a, '.a'), (b, '.b')):
                out[name + tag + '.weight'] = lin.weight.detach().to(t16)
                out[name + tag + '.bias'] = lin.bias.detach().to(t16)
            if t16 == torch.bfloat16:
                rows = _pair_rows(pair).to(a.weight.device)
                out[name + '.core_w'] = torch.cat([a.weight.detach(), b.weight.detach()], 0).index_select(0, rows).to(torch.bfloat16)
                out[name + '.core_b'] = torch.cat([a.bias.detach(), b.bias.detach()], 0).float().index_select(0, rows)
        for name in ('conv_a', 'conv_b'):
            w = getattr(model, name).weight.detach()
            cin = (w.shape[1] + 15) // 16 * 16
            if w.shape[1] != cin:
                w = F.pad(w, (0, 0, 0, 0, 0, cin - w.shape[1]))
            wb = w.to(t16)
            out[name + '.w9'] = conv.forward_weight(wb, t16)
            out[name + '.wt9'] = conv.dgrad_weight(wb, t16)
        w = model.up.weight
        out['up'] = w.detach().to(t16).permute(2, 3, 1, 0).reshape(4 * w.shape[1], w.shape[0]).contiguous()
    return out


def served(model, t16):
    """name -> the copy the open epoch serves (None: not served - the per-use expression would run)."""
    from vitadapter import fused
    cp = fused.BF16_COPIES
    out = {}
    for name in ('lin1', 'lin2') + (('fc', 'patch') if t16 == torch.bfloat16 else ()):
        out[name + '.weight'] = cp._hit(getattr(model, name).weight, t16)
    for name in ('lin1', 'lin2'):
        out[name + '.bias'] = cp._hit(getattr(model, name).bias, t16)
    for name in ('pair1', 'pair2'):
        pair = getattr(model, name)
        a, b = pair.sampling_offsets, pair.attention_weights
        for lin, tag in ((a, '.a'), (b, '.b')):
            out[name + tag + '.weight'] = cp._hit(lin.weight, t16)
            out[name + tag + '.bias'] = cp._hit(lin.bias, t16)
        if t16 == torch.bfloat16:
            e = fused.PAIR_CORE_COPIES.entries.get((id(a.weight), id(b.weight)))
            hit = e is not None and e[0] == cp.epoch and (cp.epoch & 1) and e[4]() is a.weight
            out[name + '.core_w'], out[name + '.core_b'] = (e[1], e[2]) if hit else (None, None)
    for name in ('conv_a', 'conv_b'):
        made = cp.layout('conv9', getattr(model, name).weight, t16)
        out[name + '.w9'], out[name + '.wt9'] = made if made is not None else (None, None)
    out['up'] = cp.layout('up', model.up.weight, t16)
    return out


def assert_same_bits(got, want, what):
    """Bit-equal (compared as integers) except that a NaN only has to be a NaN in the same place."""
    assert got is not None, '%s: not served' % what
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), '%s: NaN positions differ' % what
    itype = torch.int16 if want.element_size() == 2 else torch.int32
    g, w = got.contiguous().view(itype), want.contiguous().view(itype)
    bad = (g != w) & ~nan
    assert not bool(bad.any()), '%s: %d of %d elements differ in their bits' % (what, int(bad.sum()), want.numel())
