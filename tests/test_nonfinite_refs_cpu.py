"""CPU: the case table of the non-finite propagation contract, and the proof that it is not vacuous.

The contract ("GradScaler has to see it"): an inf or NaN that ARRIVES at a kernel comes out non-finite
wherever torch's own operator would produce one.  A case starts from small finite inputs, sets ONE element of ONE
floating-point operand (an activation, an incoming gradient, or a saved activation the backward rereads) to a poison and
evaluates the call.  The reference is torch's own fp64 evaluation, on the CPU, of the expression the wrapper's docstring
says it equals, on the same poisoned operands widened to fp64; tests/test_nonfinite_gpu.py imports this table, runs the
kernels through the Python wrappers and asserts inclusion: every element that is non-finite in the reference is
non-finite in the kernel's output (the kind need not match, and the kernel may spread a NaN further).

A case whose reference is all finite asserts nothing.  This file runs only the references: the set of non-finite
reference elements (the union over the call's outputs) is non-empty for every (case, operand, poison) outside ALLOW_FINITE
and empty for every one inside, at every position; ALLOW_FINITE holds no +inf or NaN triple; and the unpoisoned inputs
give an all-finite reference.

Positions: the first, the last and one interior element of the operand's logical extent.  Under a fused ReLU these three
lie where the ReLU is open on the finite baseline (the inputs are planted so: see _plant), and 'closed' is one more
position where it is closed.  No exact zero multiplies a poison: weights and scales are drawn away from zero.  Parameters
(weights, gamma, beta) and integer operands are never poisoned.

Needs no GPU, but the built tree, as the project's other *_cpu tests: the deformable-attention reference is
ops.functions.ms_deform_attn_func.ms_deform_attn_core_pytorch (the statement the issue names), and importing that module
loads libvitadapter_hip.so; oracle.msda_fused loads the C oracle."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

INF, NAN = float('inf'), float('nan')
POISONS = {'+inf': INF, 'nan': NAN, '-inf': -INF}
BF16, F16, F32, f64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
DTYPES = {'bf16': BF16, 'f16': F16, 'f32': F32}
SENTINEL = 7.0            # finite: an element the kernel never wrote must not pass as "non-finite"
EPS, MOMENTUM = 1e-5, 0.1
OPEN, CLOSED = 2.5, -2.5  # planted pre-activations (in units of the channel's standard deviation)

# (case, operand, poison) whose fp64 torch result really is finite, at every position of the table:
ALLOW_FINITE = {
    # -inf into a 3 x 3 / stride 2 / padding 1 max-pool window: every window of the maps used here holds at least one
    # more (finite, larger) element, so the maximum and the gradient routing do not see it
    ('spm_maxpool', 'x', '-inf'),
    ('tail_max_pool', 'x', '-inf'),
    # -inf into an attention logit: the softmax gives that key the weight 0 and every other key of the row is finite
    # (a table entry serves at most one key per query row), so the output and every gradient stay finite
    ('attn_bias', 'bias', '-inf'),
    ('attn_relpos', 'table', '-inf'),
    # -inf into a deformable-attention logit: the softmax over the L * P samples gives that sample the weight 0
    ('msda_plain', 'logits', '-inf'),
    ('msda_fused_ext', 'logits', '-inf'),
    ('msda_fused_ext_gather', 'logits', '-inf'),
    ('msda_fused_inj', 'logits', '-inf'),
}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, shape, dtype, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _away(g, shape, lo=0.5, hi=1.5, signed=False):
    """parameters away from zero: |v| in [lo, hi]"""
    v = lo + (hi - lo) * torch.rand(shape, generator=g)
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    return v


def _flat(shape, idx):
    i = 0
    for n, k in zip(shape, idx):
        i = i * n + (k if k >= 0 else n + k)
    return i


def _three(shape, mid):
    """first, last and one interior element of a contiguous tensor, as flat indices"""
    return {'first': 0, 'last': _flat(shape, [-1] * len(shape)), 'mid': _flat(shape, mid)}


def _plant(t, positions, closed=None):
    """Write OPEN at ``positions`` (flat indices) and CLOSED at ``closed``: with channel statistics near (0, 1), a positive
    gamma and a small beta the fused ReLU is open / closed there on the finite baseline (asserted by the baseline check of
    the CPU test through the reference's own pre-activation)."""
    flat = t.view(-1)
    for i in positions:
        flat[i] = OPEN
    if closed is not None:
        flat[closed] = CLOSED
    return t


class Case:
    """name; dtypes: the 16-bit types the kernels are instantiated on; build(dtype) -> dict of CPU tensors (finite) with
    '_pos': {operand: {label: flat index}}; poisons: {operand: [poison names]}; ref(ins) -> {output: fp64 tensor}; run:
    the name of the GPU runner in tests/test_nonfinite_gpu.py (same output names)."""

    def __init__(self, name, build, ref, poisons, dtypes=('bf16', 'f16'), **kw):
        # one set of inputs per dtype: poisoned() and the runners copy, nothing writes into them
        self.name, self.build, self.ref, self.poisons, self.dtypes, self.kw = name, functools.lru_cache(None)(build), ref, poisons, dtypes, kw

    def triples(self):
        ins = self.build(DTYPES[self.dtypes[0]])
        for op, names in self.poisons.items():
            for label in ins['_pos'][op]:
                for p in names:
                    if label == 'closed' and p == '-inf':
                        continue
                    yield op, label, p


def poisoned(ins, op, label, poison):
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ins.items()}
    out[op].view(-1)[ins['_pos'][op][label]] = POISONS[poison]
    return out


def d(t):
    return None if t is None else t.detach().to(f64)


def leaf(t):
    return d(t).requires_grad_(True)


def nonfinite_count(outs):
    return sum(int((~torch.isfinite(v)).sum()) for v in outs.values() if v is not None)


# ---------------------------------------------------------------------------------------------------------------------
# SpatialPriorModule, NHWC (vitadapter/spm_nhwc.py, vitadapter/conv.py)
# ---------------------------------------------------------------------------------------------------------------------
def _image_build(dtype):
    x = _rand(_gen(1), (2, 3, 8, 32), F32)
    return {'x': x, '_pos': {'x': _three(x.shape, (1, 1, 3, 17))}}


def _image_ref(ins):
    """spm_nhwc.image_to_nhwc16: (N, 3, H, W) -> (N, H, W, 16), channels 3..15 zero"""
    return {'y': F.pad(d(ins['x']).permute(0, 2, 3, 1), (0, 13))}


def _conv_build(cin, cout, stride):
    def build(dtype):
        g = _gen(2 + cin + stride)
        N, H, W = 2, 8, 32
        OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
        x = _rand(g, (N, H, W, cin), dtype)
        w = _away(g, (cout, cin, 3, 3), 0.02, 0.06, signed=True).to(dtype)
        gy = _rand(g, (N, OH, OW, cout), dtype)
        # no input gradient at cin = 16: vah_conv3x3_dgrad_nhwc_* take cin % 64 == 0 only (csrc/conv.hip conv_dgrad_entry;
        # the 16-channel convolution reads the image, a leaf), so conv3x3_input_grad runs at (64, 64, 1)
        return {'x': x, 'w': w, 'gy': gy, 'stride': stride, 'dgrad': cin != 16,
                '_pos': {'x': _three(x.shape, (1, 3, 17, cin // 2 + 1)), 'gy': _three(gy.shape, (1, 2, 9, cout // 2 + 1))}}
    return build


def _conv_ref(ins):
    """conv.conv3x3_forward / conv3x3_input_grad / conv3x3_weight_grad: nn.Conv2d(k=3, padding=1, bias=False) and its
    autograd, NHWC"""
    x, w = leaf(ins['x'].permute(0, 3, 1, 2)), leaf(ins['w'])
    y = F.conv2d(x, w, stride=ins['stride'], padding=1)
    gx, gw = torch.autograd.grad(y, (x, w), d(ins['gy']).permute(0, 3, 1, 2))
    out = {'y': y.detach().permute(0, 2, 3, 1), 'gw': gw.permute(0, 2, 3, 1)}
    if ins['dgrad']:
        out['gx'] = gx.permute(0, 2, 3, 1)
    return out


def _bn_params(g, C):
    return {'gamma': _away(g, (C,), 0.5, 1.5), 'beta': _rand(g, (C,), F32, 0.1),
            'rm': _rand(g, (C,), F32, 0.05), 'rv': _away(g, (C,), 0.9, 1.1)}


def _spm_bn_build(relu, training):
    def build(dtype):
        g = _gen(11)
        shape = (2, 8, 32, 64)
        x, dy = _rand(g, shape, dtype), _rand(g, shape, dtype)
        pos = _three(shape, (1, 3, 17, 37))
        xpos = dict(pos, closed=_flat(shape, (0, 5, 9, 21))) if relu else pos
        _plant(x, pos.values(), xpos.get('closed'))
        return dict(_bn_params(g, 64), x=x, dy=dy, relu=relu, training=training, _pos={'x': xpos, 'dy': pos})
    return build


def _bn_ref(t, ins):
    """[relu] BatchNorm over dim 1 of the fp64 leaf ``t`` -> y and the running statistics after the call"""
    rm, rv = d(ins['rm']).clone(), d(ins['rv']).clone()
    y = F.batch_norm(t, rm, rv, ins['_w'], ins['_b'], ins['training'], MOMENTUM, EPS)
    return (F.relu(y) if ins['relu'] else y), rm, rv


def _spm_bn_ref(ins):
    """spm_nhwc._BNRelu: relu(BatchNorm(x)) over the rows of an NHWC tensor, and its autograd"""
    x = leaf(ins['x'])
    ins = dict(ins, _w=leaf(ins['gamma']), _b=leaf(ins['beta']))
    y, rm, rv = _bn_ref(x.view(-1, x.shape[-1]), ins)
    dx, dw, db = torch.autograd.grad(y, (x, ins['_w'], ins['_b']), d(ins['dy']).view(y.shape))
    return {'y': y.detach().view(x.shape), 'dx': dx, 'dweight': dw, 'dbias': db, 'running_mean': rm, 'running_var': rv}


def _pool_build(nhwc):
    def build(dtype):
        g = _gen(17)
        N, C, H, W = 2, 16, 7, 10          # odd height: the last window row is cut short by the border
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        if nhwc:
            x, gy = _rand(g, (N, H, W, C), dtype), _rand(g, (N, OH, OW, C), dtype)
            pos = {'x': _three(x.shape, (1, 3, 4, 9)), 'gy': _three(gy.shape, (1, 2, 3, 9))}
        else:
            x, gy = _rand(g, (N, C, H, W), dtype), _rand(g, (N, C, OH, OW), dtype)
            pos = {'x': _three(x.shape, (1, 9, 3, 4)), 'gy': _three(gy.shape, (1, 9, 2, 3))}
        return {'x': x, 'gy': gy, 'nhwc': nhwc, '_pos': pos}
    return build


def _pool_ref(ins):
    """F.max_pool2d(x, 3, 2, 1) and its autograd (spm_nhwc._MaxPool on NHWC, fused.max_pool on NCHW)"""
    x = leaf(ins['x'].permute(0, 3, 1, 2) if ins['nhwc'] else ins['x'])
    gy = d(ins['gy'])
    y = F.max_pool2d(x, 3, 2, 1)
    gx, = torch.autograd.grad(y, x, gy.permute(0, 3, 1, 2) if ins['nhwc'] else gy)
    y = y.detach()
    return {'y': y.permute(0, 2, 3, 1), 'gx': gx.permute(0, 2, 3, 1)} if ins['nhwc'] else {'y': y, 'gx': gx}


# ---------------------------------------------------------------------------------------------------------------------
# output tail (fused.bn_tail, bn_relu, tokens_to_maps, maps_to_tokens, max_pool, halve)
# ---------------------------------------------------------------------------------------------------------------------
def _tail_build(scale, relu, training):
    def build(dtype):
        g = _gen(23 + scale)
        N, C, H, W = 2, 8, 16, 16
        shape = (N, C, H, W)
        pos = _three(shape, (1, 3, 9, 6))
        out = dict(_bn_params(g, C), scale=scale, relu=relu, training=training)
        if relu:            # fused.bn_relu(norm, a): output and gradient in a's dtype
            a, dy = _rand(g, shape, dtype), _rand(g, shape, dtype)
            apos = dict(pos, closed=_flat(shape, (0, 5, 3, 10)))
            _plant(a, pos.values(), apos['closed'])
            return dict(out, a=a, dy=dy, _pos={'a': apos, 'dy': pos})
        lshape = (N, C, H // scale, W // scale)
        a, b = _rand(g, shape, dtype, 0.6), _rand(g, shape, dtype, 0.6)
        x, dy = _rand(g, lshape, F32, 0.6), _rand(g, shape, F32)
        # interior of the low-res map, away from row / column 1: bilinear interpolation reads those with weight exactly 0
        # for the border pixels of the output (zero-multiplier semantics are not part of this contract)
        xpos = _three(lshape, (1, 3, H // scale // 2, W // scale // 2))
        return dict(out, a=a, b=b, x=x, shift=_rand(g, (C,), F32, 0.2), dy=dy, _pos={'a': pos, 'b': pos, 'x': xpos, 'dy': pos})
    return build


def _tail_ref(ins):
    """fused.bn_tail: norm(a + b + shift + F.interpolate(x, scale_factor=scale, mode='bilinear', align_corners=False));
    fused.bn_relu: relu(norm(a)); and their autograd"""
    ins = dict(ins, _w=leaf(ins['gamma']), _b=leaf(ins['beta']))
    a = leaf(ins['a'])
    leaves, names = [a, ins['_w'], ins['_b']], ['da', 'dweight', 'dbias']
    t = a
    if not ins['relu']:
        b, x = leaf(ins['b']), leaf(ins['x'])
        up = x if ins['scale'] == 1 else F.interpolate(x, scale_factor=ins['scale'], mode='bilinear', align_corners=False)
        t = a + b + d(ins['shift']).view(1, -1, 1, 1) + up
        leaves += [b, x]
        names += ['db', 'dx']
    y, rm, rv = _bn_ref(t, ins)
    out = dict(zip(names, torch.autograd.grad(y, leaves, d(ins['dy']))))
    out.update(y=y.detach())
    if ins['training']:
        out.update(running_mean=rm, running_var=rv)
    return out


MAP_HW = ((4, 8), (2, 4))


def _t2m_build(dtype):
    g = _gen(31)
    B, C = 2, 40
    T = sum(h * w for h, w in MAP_HW)
    tokens = _rand(g, (B, T, C), F32)
    gs = [_rand(g, (B, C, h, w), F32) for h, w in MAP_HW]
    return {'tokens': tokens, 'g0': gs[0], 'g1': gs[1],
            '_pos': {'tokens': _three(tokens.shape, (1, 33, 21)), 'g0': _three(gs[0].shape, (1, 21, 2, 5)),
                     'g1': _three(gs[1].shape, (1, 21, 1, 2))}}


def _t2m_ref(ins):
    """fused.tokens_to_maps: [tokens[:, a:b].transpose(1, 2).reshape(B, C, h, w) for the consecutive ranges]"""
    tok = leaf(ins['tokens'])
    B, _, C = tok.shape
    outs, t0 = [], 0
    for h, w in MAP_HW:
        outs.append(tok[:, t0:t0 + h * w].transpose(1, 2).reshape(B, C, h, w))
        t0 += h * w
    gt, = torch.autograd.grad(outs, tok, [d(ins['g0']), d(ins['g1'])])
    return {'m0': outs[0].detach(), 'm1': outs[1].detach(), 'gtokens': gt}


def _m2t_build(dtype):
    g = _gen(37)
    B, C = 2, 40
    T = sum(h * w for h, w in MAP_HW)
    m0, m1 = _rand(g, (B, C) + MAP_HW[0], dtype), _rand(g, (B, C) + MAP_HW[1], F32)
    gout = _rand(g, (B, T, C), F32)
    return {'m0': m0, 'm1': m1, 'v0': _rand(g, (C,), F32), 'v1': _rand(g, (C,), F32), 'g': gout,
            '_pos': {'m0': _three(m0.shape, (1, 21, 2, 5)), 'm1': _three(m1.shape, (1, 21, 1, 2)),
                     'g': _three(gout.shape, (1, 33, 21))}}


def _m2t_ref(ins):
    """fused.maps_to_tokens: cat([m.flatten(2).transpose(1, 2) + v for m, v in zip(maps, vecs)], dim=1)"""
    ms, vs = [leaf(ins['m0']), leaf(ins['m1'])], [leaf(ins['v0']), leaf(ins['v1'])]
    out = torch.cat([m.flatten(2).transpose(1, 2) + v for m, v in zip(ms, vs)], dim=1)
    g = torch.autograd.grad(out, ms + vs, d(ins['g']))
    return {'tokens': out.detach(), 'gm0': g[0], 'gm1': g[1], 'gv0': g[2], 'gv1': g[3]}


def _halve_build(dtype):
    g = _gen(41)
    x, gy = _rand(g, (2, 5, 8, 12), F32), _rand(g, (2, 5, 4, 6), F32)
    return {'x': x, 'gy': gy, '_pos': {'x': _three(x.shape, (1, 3, 5, 7)), 'gy': _three(gy.shape, (1, 3, 2, 3))}}


def _halve_ref(ins):
    """fused.halve: F.interpolate(x, scale_factor=0.5, mode='bilinear', align_corners=False)"""
    x = leaf(ins['x'])
    y = F.interpolate(x, scale_factor=0.5, mode='bilinear', align_corners=False)
    gx, = torch.autograd.grad(y, x, d(ins['gy']))
    return {'y': y.detach(), 'gx': gx}


# ---------------------------------------------------------------------------------------------------------------------
# row kernels (csrc/fused_ops.hip) through fused.layer_norm, layer_norm_dual_keep, residual_ln, residual, gelu,
# dwconv_tokens
# ---------------------------------------------------------------------------------------------------------------------
ROWS, C_ROW = 13, 200
DROP_SCALE = 1.0 / 0.7          # the drop-path scale of a kept sample (never zero: a dropped sample is out of scope)


def _ln_params(g, C, tag=''):
    return {'lnw' + tag: _away(g, (C,), 0.5, 1.5), 'lnb' + tag: _rand(g, (C,), F32, 0.1)}


def _ln_build(dtype):
    g = _gen(43)
    x, gy = _rand(g, (ROWS, C_ROW), F32), _rand(g, (ROWS, C_ROW), dtype)
    pos = _three(x.shape, (6, 101))
    return dict(_ln_params(g, C_ROW), x=x, g=gy, _pos={'x': pos, 'g': pos})


def _ln(t, ins, tag=''):
    return F.layer_norm(t, (t.shape[-1],), ins['_lnw' + tag], ins['_lnb' + tag], EPS)


def _ln_ref(ins):
    """fused.layer_norm: norm(x)"""
    ins = dict(ins, _lnw=leaf(ins['lnw']), _lnb=leaf(ins['lnb']))
    x = leaf(ins['x'])
    y = _ln(x, ins)
    dx, dw, db = torch.autograd.grad(y, (x, ins['_lnw'], ins['_lnb']), d(ins['g']))
    return {'y': y.detach(), 'dx': dx, 'dw': dw, 'db': db}


def _ln_dual_build(dtype):
    g = _gen(47)
    x = _rand(g, (ROWS, C_ROW), F32)
    pos = _three(x.shape, (6, 101))
    out = dict(_ln_params(g, C_ROW, 'a'), x=x, gres=_rand(g, x.shape, F32), ga=_rand(g, x.shape, dtype), gb=_rand(g, x.shape, dtype))
    out.update(_ln_params(g, C_ROW, 'b'))
    return dict(out, _pos={k: pos for k in ('x', 'gres', 'ga', 'gb')})


def _ln_dual_ref(ins):
    """fused.layer_norm_dual_keep: (x, norm_a(x), norm_b(x))"""
    ps = {k: leaf(ins[k]) for k in ('lnwa', 'lnba', 'lnwb', 'lnbb')}
    ins = dict(ins, **{'_' + k: v for k, v in ps.items()})
    x = leaf(ins['x'])
    xk, ya, yb = x * 1.0, _ln(x, ins, 'a'), _ln(x, ins, 'b')
    g = torch.autograd.grad([xk, ya, yb], [x] + list(ps.values()), [d(ins['gres']), d(ins['ga']), d(ins['gb'])])
    return {'x': xk.detach(), 'ya': ya.detach(), 'yb': yb.detach(), 'dx': g[0], 'dwa': g[1], 'dba': g[2], 'dwb': g[3], 'dbb': g[4]}


def _res_build(with_gamma, with_ln):
    def build(dtype):
        g = _gen(53 + with_gamma)
        shape = (1, ROWS, C_ROW)
        pos = _three(shape, (0, 6, 101))
        out = {'x': _rand(g, shape, F32), 'z': _rand(g, shape, dtype), 'gt': _rand(g, shape, F32),
               'gamma': _away(g, (C_ROW,), 0.5, 1.5) if with_gamma else None, 'scale': torch.full((1,), DROP_SCALE),
               'with_ln': with_ln, '_pos': {'x': pos, 'z': pos, 'gt': pos}}
        if with_ln:
            out.update(_ln_params(g, C_ROW), gh=_rand(g, shape, dtype))
            out['_pos']['gh'] = pos
        return out
    return build


def _res_ref(ins):
    """fused.residual: x + drop_path(gamma * z); fused.residual_ln: t = x + drop_path(gamma * z); return t, norm(t)"""
    x, z = leaf(ins['x']), leaf(ins['z'])
    gamma = leaf(ins['gamma']) if ins['gamma'] is not None else None
    leaves, names = [x, z] + ([gamma] if gamma is not None else []), ['dx', 'dz'] + (['dgamma'] if gamma is not None else [])
    br = gamma * z if gamma is not None else z
    t = x + d(ins['scale']).view(-1, 1, 1) * br
    if not ins['with_ln']:
        return dict(zip(names, torch.autograd.grad(t, leaves, d(ins['gt']))), y=t.detach())
    ins = dict(ins, _lnw=leaf(ins['lnw']), _lnb=leaf(ins['lnb']))
    h = _ln(t, ins)
    g = torch.autograd.grad([t, h], leaves + [ins['_lnw'], ins['_lnb']], [d(ins['gt']), d(ins['gh'])])
    return dict(zip(names + ['dw', 'db'], g), t=t.detach(), h=h.detach())


def _gelu_build(dtype):
    g = _gen(59)
    h, da = _rand(g, (ROWS, 264), dtype), _rand(g, (ROWS, 264), dtype)
    pos = _three(h.shape, (6, 133))
    return {'h': h, 'da': da, '_pos': {'h': pos, 'da': pos}}


def _gelu_ref(ins):
    """fused.gelu: act(h) for an exact nn.GELU"""
    h = leaf(ins['h'])
    a = F.gelu(h)
    dh, = torch.autograd.grad(a, h, d(ins['da']))
    return {'a': a.detach(), 'dh': dh}


DW_H = DW_W = 8
DW_C = 48


def _dw_levels():
    return [(2 * DW_H, 2 * DW_W), (DW_H, DW_W), (DW_H // 2, DW_W // 2)]


def _dwconv_build(dtype):
    g = _gen(61)
    N = 21 * (DW_H // 2) * (DW_W // 2)
    x, gy = _rand(g, (1, N, DW_C), dtype), _rand(g, (1, N, DW_C), dtype)
    pos = _three(x.shape, (0, 256 + 27, 25))         # interior: a pixel of the middle map
    # The weight gradient multiplies g at a border pixel with the zero padding of x (torch: inf * 0 = NaN; the kernel skips
    # the taps that fall outside).  Zero multipliers are not part of this contract, so the first and last positions of g
    # are the first channel of pixel (1, 1) of the first map and the last channel of pixel (2, 2) of the last (4 x 4) map.
    gpos = dict(pos, first=_flat(x.shape, (0, 2 * DW_W + 1, 0)), last=_flat(x.shape, (0, N - 16 + 2 * 4 + 2, DW_C - 1)))
    return {'x': x, 'g': gy, 'w': _away(g, (DW_C, 1, 3, 3), 0.1, 0.4, signed=True), 'b': _rand(g, (DW_C,), F32, 0.1),
            '_pos': {'x': pos, 'g': gpos}}


def _dwconv_ref(ins):
    """fused.dwconv_tokens: ConvFFN's DWConv - the token row holds three maps (2H x 2W, H x W, H/2 x W/2), each goes
    through the same depthwise 3 x 3 convolution (adapter_modules.py DWConv)"""
    x, w, b = leaf(ins['x']), leaf(ins['w']), leaf(ins['b'])
    B, _, C = x.shape
    outs, t0 = [], 0
    for h, wd in _dw_levels():
        m = x[:, t0:t0 + h * wd].transpose(1, 2).reshape(B, C, h, wd)
        outs.append(F.conv2d(m, w, b, 1, 1, groups=C).flatten(2).transpose(1, 2))
        t0 += h * wd
    y = torch.cat(outs, dim=1)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), d(ins['g']))
    return {'y': y.detach(), 'dx': dx, 'dw': dw, 'db': db}


# ---------------------------------------------------------------------------------------------------------------------
# Linear layers (csrc/gemm.hip and the glue): fused.linear, linear_pair, conv1x1, patch_embed, up_from_tokens
# ---------------------------------------------------------------------------------------------------------------------
def _lin_params(g, n_out, n_in, tag=''):
    return {'w' + tag: _away(g, (n_out, n_in), 0.05, 0.2, signed=True), 'b' + tag: _rand(g, (n_out,), F32, 0.1)}


def _linear_build(dtype):
    g = _gen(67)
    x, gy = _rand(g, (ROWS, 40), dtype), _rand(g, (ROWS, 72), dtype)
    return dict(_lin_params(g, 72, 40), x=x, g=gy, _pos={'x': _three(x.shape, (6, 21)), 'g': _three(gy.shape, (6, 37))})


def _linear_ref(ins):
    """fused.linear: lin(x); dW and db come from fused._wgrad_bgrad with a column-sum launch"""
    x, w, b = leaf(ins['x']), leaf(ins['w']), leaf(ins['b'])
    y = F.linear(x, w, b)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), d(ins['g']))
    return {'y': y.detach(), 'dx': dx, 'dw': dw, 'db': db}


def _mlp_build(dtype):
    g = _gen(71)
    shape = (1, ROWS, 40)
    pos = _three(shape, (0, 6, 21))
    out = dict(_lin_params(g, 72, 40, '1'), x=_rand(g, shape, dtype), x0=_rand(g, shape, F32), gt=_rand(g, shape, F32),
               gh=_rand(g, shape, dtype), scale=torch.full((1,), DROP_SCALE))
    out.update(_lin_params(g, 40, 72, '2'))
    out.update(_ln_params(g, 40))
    return dict(out, _pos={k: pos for k in ('x', 'x0', 'gt', 'gh')})


def _mlp_ref(ins):
    """z = fc2(gelu(fc1(x))); t = x0 + drop_path(z); return t, norm(t) - fused.linear, fused.gelu, fused.linear,
    fused.residual_ln: both Linears take their bias gradient from the partial column sums that the GELU backward and the
    residual + LayerNorm backward leave"""
    names = ('w1', 'b1', 'w2', 'b2', 'lnw', 'lnb')
    ps = {k: leaf(ins[k]) for k in names}
    ins = dict(ins, _lnw=ps['lnw'], _lnb=ps['lnb'])
    x, x0 = leaf(ins['x']), leaf(ins['x0'])
    z = F.linear(F.gelu(F.linear(x, ps['w1'], ps['b1'])), ps['w2'], ps['b2'])
    t = x0 + d(ins['scale']).view(-1, 1, 1) * z
    h = _ln(t, ins)
    g = torch.autograd.grad([t, h], [x, x0] + list(ps.values()), [d(ins['gt']), d(ins['gh'])])
    return dict(zip(('dx', 'dx0') + tuple('d' + k for k in names), g), t=t.detach(), h=h.detach())


def _pair_build(dtype):
    g = _gen(73)
    x = _rand(g, (ROWS, 40), dtype)
    ga, gb = _rand(g, (ROWS, 48), dtype), _rand(g, (ROWS, 24), dtype)
    out = dict(_lin_params(g, 48, 40, 'a'), x=x, ga=ga, gb=gb)
    out.update(_lin_params(g, 24, 40, 'b'))
    return dict(out, _pos={'x': _three(x.shape, (6, 21)), 'ga': _three(ga.shape, (6, 25)), 'gb': _three(gb.shape, (6, 13))})


def _pair_ref(ins):
    """fused.linear_pair: (lin_a(x), lin_b(x))"""
    names = ('wa', 'ba', 'wb', 'bb')
    ps = {k: leaf(ins[k]) for k in names}
    x = leaf(ins['x'])
    ya, yb = F.linear(x, ps['wa'], ps['ba']), F.linear(x, ps['wb'], ps['bb'])
    g = torch.autograd.grad([ya, yb], [x] + list(ps.values()), [d(ins['ga']), d(ins['gb'])])
    return dict(zip(('dx',) + tuple('d' + k for k in names), g), ya=ya.detach(), yb=yb.detach())


def _conv1x1_build(dtype):
    g = _gen(79)
    x, gy = _rand(g, (2, 16, 4, 10), dtype), _rand(g, (2, 24, 4, 10), dtype)
    return {'x': x, 'g': gy, 'w': _away(g, (24, 16, 1, 1), 0.05, 0.2, signed=True),
            '_pos': {'x': _three(x.shape, (1, 9, 2, 5)), 'g': _three(gy.shape, (1, 13, 2, 5))}}


def _conv1x1_ref(ins):
    """fused.conv1x1: F.conv2d(x, conv.weight, None)"""
    x, w = leaf(ins['x']), leaf(ins['w'])
    y = F.conv2d(x, w, None)
    dx, dw = torch.autograd.grad(y, (x, w), d(ins['g']))
    return {'y': y.detach(), 'dx': dx, 'dw': dw}


def _patch_build(dtype):
    g = _gen(83)
    x, gy = _rand(g, (1, 3, 32, 32), F32), _rand(g, (1, 4, 24), dtype)
    return {'x': x, 'g': gy, 'w': _away(g, (24, 3, 16, 16), 0.02, 0.06, signed=True), 'b': _rand(g, (24,), F32, 0.1),
            '_pos': {'x': _three(x.shape, (0, 1, 17, 21)), 'g': _three(gy.shape, (0, 2, 13))}}


def _patch_ref(ins):
    """fused.patch_embed: conv(x).flatten(2).transpose(1, 2) for a Conv2d with kernel = stride = 16 (no input gradient:
    the image is a leaf)"""
    x, w, b = d(ins['x']), leaf(ins['w']), leaf(ins['b'])
    y = F.conv2d(x, w, b, stride=16).flatten(2).transpose(1, 2)
    dw, db = torch.autograd.grad(y, (w, b), d(ins['g']))
    return {'y': y.detach(), 'dw': dw, 'db': db}


def _up_build(dtype):
    g = _gen(89)
    rows, add = _rand(g, (2, 64, 16), dtype), _rand(g, (2, 16, 16, 16), dtype)
    gy = _rand(g, (2, 16, 16, 16), dtype)
    pos = _three(add.shape, (1, 9, 7, 11))
    return {'rows': rows, 'addend': add, 'g': gy, 'w': _away(g, (16, 16, 2, 2), 0.05, 0.2, signed=True),
            '_pos': {'rows': _three(rows.shape, (1, 37, 9)), 'addend': pos, 'g': pos}}


def _up_ref(ins):
    """fused.up_from_tokens: F.conv_transpose2d(rows.transpose(1, 2).view(B, C, h, w), up.weight, None, stride=2) + addend"""
    rows, add, w = leaf(ins['rows']), leaf(ins['addend']), leaf(ins['w'])
    B, _, C = rows.shape
    y = F.conv_transpose2d(rows.transpose(1, 2).reshape(B, C, 8, 8), w, None, stride=2) + add
    g = torch.autograd.grad(y, (rows, add, w), d(ins['g']))
    return {'y': y.detach(), 'drows': g[0], 'daddend': g[1], 'dw': g[2]}


# ---------------------------------------------------------------------------------------------------------------------
# attention (csrc/attn_*.hip, relpos.hip) through vitadapter/kernels.py
# ---------------------------------------------------------------------------------------------------------------------
ATTN_SCALE = 0.125


def window_relative_position_index(w):
    """(w*w, w*w) index into the (2w-1)^2-row bias table (vitadapter/backbones/beit_det.py)"""
    ys, xs = torch.meshgrid(torch.arange(w), torch.arange(w), indexing='ij')
    coords = torch.stack([ys.flatten(), xs.flatten()])
    rel = coords[:, :, None] - coords[:, None, :]
    return (rel[0] + w - 1) * (2 * w - 1) + (rel[1] + w - 1)


def _attn_build(kind, B, N, H, grid=None, win=None, seed=97):
    def build(dtype):
        g = _gen(seed + N)
        qkv, dout = _rand(g, (B, N, 3, H, 64), dtype), _rand(g, (B, N, H, 64), dtype)
        pos = {}
        for i, nm in enumerate('qkv'):
            pos[nm + '-first'] = _flat(qkv.shape, (0, 0, i, 0, 0))
            pos[nm + '-last'] = _flat(qkv.shape, (-1, -1, i, -1, -1))
            pos[nm + '-mid'] = _flat(qkv.shape, (B // 2, N // 2 + 3, i, H // 2, 37))
            if grid is not None and (grid[0] % win or grid[1] % win):      # a token of a window that the grid cuts short
                pos[nm + '-cut'] = _flat(qkv.shape, (0, (grid[0] - 1) * grid[1] + 1, i, 0, 5))
        out = {'qkv': qkv, 'dout': dout, 'kind': kind, 'grid': grid, 'win': win,
               '_pos': {'qkv': pos, 'dout': _three(dout.shape, (B // 2, N // 2 + 3, H // 2, 37))}}
        if kind == 'bias':
            out['bias'] = _rand(g, (H, N, N), F32)
            out['_pos']['bias'] = _three(out['bias'].shape, (H // 2, N // 2, N // 2 + 5))
        if kind == 'relpos':
            w = int(round(N ** 0.5))
            out['index'] = window_relative_position_index(w)
            out['table'] = _rand(g, ((2 * w - 1) ** 2, H), F32, 1.5)
            out['_pos']['table'] = _three(out['table'].shape, ((2 * w - 1) ** 2 // 2 + 3, H // 2))
        return out
    return build


def _attention_math(q, k, v, scale, bias=None):
    """kernels._attention_math on (.., heads, N, hd) operands, with the additive bias of attention_bias"""
    attn = (q @ k.transpose(-2, -1)) * scale
    if bias is not None:
        attn = attn + bias
    return attn.softmax(dim=-1) @ v


def _attn_ref(ins):
    """kernels.attention: softmax(q k^T scale) v; attention_bias: + bias (heads, N, N); attention_relpos:
    bias[h][i][j] = table[index[i][j]][h]; window_attention: the reference's sequence - pad the (gh, gw) grid with zero
    tokens to multiples of win, partition into win x win windows, attention inside each window, merge, crop"""
    qkv = leaf(ins['qkv'])
    B, N, _, H, hd = qkv.shape
    leaves, names, bias = [qkv], ['dqkv'], None
    if ins['kind'] == 'bias':
        bias = leaf(ins['bias'])
        leaves, names = leaves + [bias], names + ['dbias']
    if ins['kind'] == 'relpos':
        table = leaf(ins['table'])
        bias = table[ins['index'].reshape(-1)].view(N, N, H).permute(2, 0, 1)
        leaves, names = leaves + [table], names + ['dtable']
    if ins['kind'] == 'window':
        (gh, gw), win = ins['grid'], ins['win']
        ph, pw = -gh % win, -gw % win
        x = F.pad(qkv.view(B, gh, gw, 3 * H * hd), (0, 0, 0, pw, 0, ph))
        nh, nw = (gh + ph) // win, (gw + pw) // win
        x = x.view(B, nh, win, nw, win, 3, H, hd).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B * nh * nw, H, win * win, hd)
        o = _attention_math(x[0], x[1], x[2], ATTN_SCALE)                      # (Z, H, win * win, hd)
        o = o.view(B, nh, nw, H, win, win, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, gh + ph, gw + pw, H, hd)
        out = o[:, :gh, :gw].reshape(B, N, H, hd)
    else:
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
        out = _attention_math(q, k, v, ATTN_SCALE, bias).transpose(1, 2)
    g = torch.autograd.grad(out, leaves, d(ins['dout']))
    return dict(zip(names, g), out=out.detach())


# ---------------------------------------------------------------------------------------------------------------------
# deformable attention (csrc/msda*.hip): the plain fp32 Function, the fused Function (bf16, fp16) and the pair core
# ---------------------------------------------------------------------------------------------------------------------
MSDA_D, MSDA_P, PAIR_K = 32, 4, 48


def _msda_geometry(name):
    """(levels, query grids, N, M): the smallest 'adapter' entry of oracle.cases.PARITY_CASES for the plain Function,
    ext_ragged (one level) and inj_ragged (three levels) of oracle/msda_fused.py for the fused forms"""
    if name == 'plain':
        from oracle import cases
        c = cases.PARITY_CASES['inj128_adapter']
        return c['shapes'], c['query_shapes'], c['N'], c['M']
    from oracle import msda_fused
    c = msda_fused.CASES[name]
    return c['levels'], c['qgrids'], c['N'], c['M']


def _msda_core(value, levels, ref, offsets, logits):
    """softmax and the location arithmetic of ops/modules/ms_deform_attn.py:137-144 around ms_deform_attn_core_pytorch"""
    from ops.functions.ms_deform_attn_func import ms_deform_attn_core_pytorch
    N, Lq, M, L, P, _ = offsets.shape
    norm = torch.tensor([[w, h] for h, w in levels], dtype=offsets.dtype)
    loc = ref[:, :, None, :, None, :] + offsets / norm[None, None, None, :, None, :]
    attn = torch.softmax(logits, -1).view(N, Lq, M, L, P)
    return ms_deform_attn_core_pytorch(value, torch.tensor(levels), loc, attn)


def _ref_px(ref, levels):
    """(Lq, L, 2) pixel coordinates (x, y) of the reference points on every level"""
    wh = torch.tensor([[w, h] for h, w in levels], dtype=torch.float32)
    return ref[0, :, 0, None, :] * wh[None] - 0.5


def _msda_build(geometry, pair=False, seed=101, **kw):
    """Zero multipliers are not part of the contract, and a sample outside the map (or with a corner outside it) is one:
    its d(out)/d(location) is an exact 0 that torch multiplies with the poison.  So every (n, q) row that holds a poisoned
    logit or incoming-gradient element has all its samples planted inside the map, both corners included: the offsets
    directly, or - pair core, where the Linears make them - through column 0 of the query, which the offsets' weight
    matrix passes on with weight 1."""
    def build(dtype):
        from oracle import cases
        levels, qgrids, N, M = _msda_geometry(geometry)
        g = _gen(seed + len(levels))
        L, S, Lq = len(levels), sum(h * w for h, w in levels), sum(h * w for h, w in qgrids)
        ref = cases.reference_grid(qgrids)                                      # (1, Lq, 1, 2) pixel centres
        px = _ref_px(ref, levels)
        hi = torch.tensor([[w - 1.0, h - 1.0] for h, w in levels])             # (L, 2): the last pixel column / row
        value, gout = _rand(g, (N, S, M, MSDA_D), dtype), _rand(g, (N, Lq, M * MSDA_D), dtype)
        qmid = Lq // 2 + 1
        planted = (0, qmid, Lq - 1)
        out = dict(kw, value=value, gout=gout, ref=ref, levels=levels, pair=pair,
                   _pos={'gout': _three(gout.shape, (N // 2, qmid, 37))})
        if pair:
            query = _rand(g, (N, Lq, PAIR_K), F32)
            wa = _away(g, (M * L * MSDA_P * 2, PAIR_K), 0.001, 0.004, signed=True)
            wa[:, 0] = 1.0
            for q in planted:       # one shift for both coordinates of every level: the middle of what keeps them inside
                lo, up = float((0.4 - px[q]).max()), float((hi - 0.4 - px[q]).min()) - 0.2
                assert up - lo > 0.3, (geometry, q, lo, up)
                query[:, q, 0] = 0.5 * (lo + up)
            out['query'], out['wa'] = query.to(dtype), wa
            out['ba'] = _away(g, (M * L * MSDA_P * 2,), 0.05, 0.15)
            out['wb'] = _away(g, (M * L * MSDA_P, PAIR_K), 0.05, 0.2, signed=True)
            out['bb'] = _rand(g, (M * L * MSDA_P,), F32, 0.1)
            out['_pos']['query'] = _three(query.shape, (N // 2, qmid, 25))
            offsets = F.linear(d(out['query']), d(out['wa']), d(out['ba'])).view(N, Lq, M, L, MSDA_P, 2)
            logits = F.linear(d(out['query']), d(out['wb']), d(out['bb'])).view(N, Lq, M, L * MSDA_P)
        else:
            off = _rand(g, (N, Lq, M, L, MSDA_P, 2), F32) + cases.ring_offsets(M, L, MSDA_P)[None, None]
            for q in planted:       # the reference pixel pulled into [1.2, last - 1.2], a jitter of +-0.2 px per sample
                pull = torch.minimum(torch.maximum(px[q], torch.full_like(hi, 1.2)), hi - 1.2) - px[q]      # (L, 2)
                off[:, q] = pull[None, None, :, None, :] + 0.4 * torch.rand((N, M, L, MSDA_P, 2), generator=g) - 0.2
            out['offsets'], out['logits'] = off.to(dtype), _rand(g, (N, Lq, M, L * MSDA_P), dtype)
            out['_pos']['offsets'] = _three(off.shape, (N // 2, qmid, M // 2, L - 1, 2, 1))
            out['_pos']['logits'] = _three(out['logits'].shape, (N // 2, qmid, M // 2, L * MSDA_P - 3))
            offsets, logits = d(out['offsets']), d(out['logits'])
        # the planted rows really are inside: pixel coordinates within [0, last] on every level
        loc = px[None, :, None, :, None, :].double() + offsets
        for q in planted:
            assert bool(((loc[:, q] >= 0.05) & (loc[:, q] <= hi[None, None, :, None, :] - 0.05)).all()), (geometry, q)
        # value: the first, the last and a middle one of the elements that a sample touches with non-zero bilinear weight
        # on the finite inputs (d sum(out) / d value != 0 in the fp64 reference)
        v = leaf(value)
        touched, = torch.autograd.grad(_msda_core(v, levels, d(ref), offsets, logits).sum(), v)
        idx = torch.nonzero(touched.reshape(-1)).reshape(-1)
        out['_pos']['value'] = {'first': int(idx[0]), 'last': int(idx[-1]), 'mid': int(idx[idx.numel() // 2 + 5])}
        return out
    return build


def _msda_ref(ins):
    """MSDeformAttnFunction / MSDeformAttnFusedFunction: the core on value, offsets, logits; fused.msda_pair_core: the
    module's sampling_offsets / attention_weights Linears on the query, then the core"""
    value, ref = leaf(ins['value']), d(ins['ref'])
    if ins['pair']:
        names = ('query', 'wa', 'ba', 'wb', 'bb')
        ps = {k: leaf(ins[k]) for k in names}
        N, Lq, _ = ps['query'].shape
        L, M = len(ins['levels']), value.shape[2]
        offsets = F.linear(ps['query'], ps['wa'], ps['ba']).view(N, Lq, M, L, MSDA_P, 2)
        logits = F.linear(ps['query'], ps['wb'], ps['bb']).view(N, Lq, M, L * MSDA_P)
        leaves, gnames = [value] + list(ps.values()), ['grad_value'] + ['d' + k for k in names]
    else:
        offsets, logits = leaf(ins['offsets']), leaf(ins['logits'])
        leaves, gnames = [value, offsets, logits], ['grad_value', 'd_offsets', 'd_logits']
    out = _msda_core(value, ins['levels'], ref, offsets, logits)
    return dict(zip(gnames, torch.autograd.grad(out, leaves, d(ins['gout']))), out=out.detach())


PN = ['+inf', 'nan']
PNM = ['+inf', 'nan', '-inf']

MSDA_OPS = {'value': PN, 'logits': PNM, 'offsets': PNM, 'gout': PN}
MSDA_PAIR_OPS = {'value': PN, 'query': PN, 'gout': PN}     # the pair core makes offsets and logits from the query

CASES = [
    Case('spm_image', _image_build, _image_ref, {'x': PN}),
    Case('spm_conv_16_64_s2', _conv_build(16, 64, 2), _conv_ref, {'x': PN, 'gy': PN}, run='spm_conv'),
    Case('spm_conv_64_64_s1', _conv_build(64, 64, 1), _conv_ref, {'x': PN, 'gy': PN}, run='spm_conv'),
    Case('spm_bn_relu', _spm_bn_build(True, True), _spm_bn_ref, {'x': PN, 'dy': PN}, run='spm_bn'),
    Case('spm_bn', _spm_bn_build(False, True), _spm_bn_ref, {'x': PN, 'dy': PN}, run='spm_bn'),
    Case('spm_bn_relu_eval', _spm_bn_build(True, False), _spm_bn_ref, {'x': PN, 'dy': PN}, run='spm_bn'),
    Case('spm_maxpool', _pool_build(True), _pool_ref, {'x': PNM, 'gy': PN}),
    Case('tail_bn_s1', _tail_build(1, False, True), _tail_ref, {'a': PN, 'b': PN, 'x': PN, 'dy': PN}, run='tail_bn'),
    Case('tail_bn_s2', _tail_build(2, False, True), _tail_ref, {'a': PN, 'b': PN, 'x': PN, 'dy': PN}, run='tail_bn'),
    Case('tail_bn_s2_eval', _tail_build(2, False, False), _tail_ref, {'a': PN, 'b': PN, 'x': PN, 'dy': PN}, run='tail_bn'),
    Case('tail_bn_relu', _tail_build(1, True, True), _tail_ref, {'a': PN, 'dy': PN}, run='tail_bn'),
    Case('tail_bn_relu_eval', _tail_build(1, True, False), _tail_ref, {'a': PN, 'dy': PN}, run='tail_bn'),
    Case('tail_tokens_to_maps', _t2m_build, _t2m_ref, {'tokens': PN, 'g0': PN, 'g1': PN}),
    Case('tail_maps_to_tokens', _m2t_build, _m2t_ref, {'m0': PN, 'm1': PN, 'g': PN}),
    Case('tail_max_pool', _pool_build(False), _pool_ref, {'x': PNM, 'gy': PN}),
    Case('tail_halve', _halve_build, _halve_ref, {'x': PN, 'gy': PN}),
    Case('rows_layer_norm', _ln_build, _ln_ref, {'x': PN, 'g': PN}),
    Case('rows_layer_norm_dual_keep', _ln_dual_build, _ln_dual_ref, {'x': PN, 'gres': PN, 'ga': PN, 'gb': PN}),
    Case('rows_residual_ln_gamma', _res_build(True, True), _res_ref, {'x': PN, 'z': PN, 'gt': PN, 'gh': PN}, run='rows_residual'),
    Case('rows_residual_ln', _res_build(False, True), _res_ref, {'x': PN, 'z': PN, 'gt': PN, 'gh': PN}, run='rows_residual'),
    Case('rows_residual_gamma', _res_build(True, False), _res_ref, {'x': PN, 'z': PN, 'gt': PN}, run='rows_residual'),
    Case('rows_residual', _res_build(False, False), _res_ref, {'x': PN, 'z': PN, 'gt': PN}, run='rows_residual'),
    Case('rows_gelu', _gelu_build, _gelu_ref, {'h': PN, 'da': PN}),
    Case('rows_dwconv_tokens', _dwconv_build, _dwconv_ref, {'x': PN, 'g': PN}),
    Case('lin_linear', _linear_build, _linear_ref, {'x': PN, 'g': PN}),
    Case('lin_mlp_bias_partials', _mlp_build, _mlp_ref, {'x': PN, 'x0': PN, 'gt': PN, 'gh': PN}),
    Case('lin_linear_pair', _pair_build, _pair_ref, {'x': PN, 'ga': PN, 'gb': PN}),
    Case('lin_conv1x1', _conv1x1_build, _conv1x1_ref, {'x': PN, 'g': PN}, dtypes=('bf16',)),
    Case('lin_patch_embed', _patch_build, _patch_ref, {'x': PN, 'g': PN}, dtypes=('bf16',)),
    Case('lin_up_from_tokens', _up_build, _up_ref, {'rows': PN, 'addend': PN, 'g': PN}),
    # two key blocks of 64, the second nearly all padding
    Case('attn_seq', _attn_build('seq', 1, 65, 2), _attn_ref, {'qkv': PN, 'dout': PN}, run='attn'),
    Case('attn_bias', _attn_build('bias', 1, 65, 2), _attn_ref, {'qkv': PN, 'dout': PN, 'bias': PNM}, run='attn'),
    Case('attn_relpos', _attn_build('relpos', 1, 196, 2), _attn_ref, {'qkv': PN, 'dout': PN, 'table': PNM}, run='attn'),
    # tests/test_attention_fp64_gpu.py WIN_CASES: the smallest resident case, the smallest resident case whose windows the
    # grid cuts short, and the smallest case of the general path (win * win = 225 > 224)
    Case('attn_win1', _attn_build('window', 2, 12, 2, (3, 4), 1), _attn_ref, {'qkv': PN, 'dout': PN}, run='attn'),
    Case('attn_win5', _attn_build('window', 2, 84, 2, (12, 7), 5), _attn_ref, {'qkv': PN, 'dout': PN}, run='attn'),
    Case('attn_win15', _attn_build('window', 2, 527, 2, (17, 31), 15), _attn_ref, {'qkv': PN, 'dout': PN}, run='attn'),
    Case('msda_plain', _msda_build('plain'), _msda_ref, MSDA_OPS, dtypes=('f32',), run='msda'),
    # one level: the LDS-window forward, and (VAH_MSDA_FWD_WIN=0) the gather forward; three levels: the gather forward
    Case('msda_fused_ext', _msda_build('ext_ragged'), _msda_ref, MSDA_OPS, run='msda'),
    Case('msda_fused_ext_gather', _msda_build('ext_ragged', env={'VAH_MSDA_FWD_WIN': '0'}), _msda_ref, MSDA_OPS, run='msda'),
    Case('msda_fused_inj', _msda_build('inj_ragged'), _msda_ref, MSDA_OPS, run='msda'),
    Case('msda_pair_ext', _msda_build('ext_ragged', pair=True), _msda_ref, MSDA_PAIR_OPS, dtypes=('bf16',), run='msda'),
    Case('msda_pair_inj', _msda_build('inj_ragged', pair=True), _msda_ref, MSDA_PAIR_OPS, dtypes=('bf16',), run='msda'),
]
BY_NAME = {c.name: c for c in CASES}


def params():
    """one pytest.param per (case, dtype, operand, position, poison); the id names the poisoned operand, position and
    poison"""
    out = []
    for c in CASES:
        for dt in c.dtypes:
            for op, label, p in c.triples():
                out.append(pytest.param(c.name, dt, op, label, p, id='%s-%s-%s-%s-%s' % (c.name, dt, op, label, p)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the CPU checks
# ---------------------------------------------------------------------------------------------------------------------
def test_allow_list_holds_no_inf_or_nan_triple():
    names = {c.name: c for c in CASES}
    for case, op, poison in ALLOW_FINITE:
        assert poison == '-inf', (case, op, poison)
        assert case in names and op in names[case].poisons and poison in names[case].poisons[op], (case, op, poison)


@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_reference_sets(name):
    """baseline all finite; fused ReLU open / closed where the table says; the reference's non-finite set non-empty exactly
    outside ALLOW_FINITE"""
    case = BY_NAME[name]
    for dt in case.dtypes:
        ins = case.build(DTYPES[dt])
        base = case.ref(ins)
        assert nonfinite_count(base) == 0, (name, dt, 'the finite baseline is not finite')
        if ins.get('relu'):
            op = 'x' if 'x' in ins else 'a'
            y = base['y'].reshape(-1)
            for label, i in ins['_pos'][op].items():
                assert (float(y[i]) > 0) == (label != 'closed'), (name, dt, label, float(y[i]))
        for op, label, p in case.triples():
            n = nonfinite_count(case.ref(poisoned(ins, op, label, p)))
            if (name, op, p) in ALLOW_FINITE:
                assert n == 0, '%s %s %s %s %s: allow-listed, but torch gives %d non-finite elements' % (name, dt, op, label, p, n)
            else:
                assert n > 0, '%s %s %s %s %s: torch is finite everywhere, the case would assert nothing' % (name, dt, op, label, p)


@contextlib.contextmanager
def sentinel_alloc():
    """torch.empty / torch.empty_like hand out SENTINEL-filled floating-point buffers while active: the outputs and
    gradients that the wrappers allocate start finite, so an element no kernel wrote cannot pass as non-finite"""
    real_empty, real_like = torch.empty, torch.empty_like

    def empty(*a, **k):
        t = real_empty(*a, **k)
        return t.fill_(SENTINEL) if t.is_floating_point() else t

    def empty_like(*a, **k):
        t = real_like(*a, **k)
        return t.fill_(SENTINEL) if t.is_floating_point() else t

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_like
