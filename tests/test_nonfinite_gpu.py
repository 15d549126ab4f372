"""GPU: no kernel may turn an inf or NaN into a finite value ("GradScaler has to see it").

The case table, the fp64 torch references and the allow-list are those of tests/test_nonfinite_refs_cpu.py (which proves,
without a GPU, that every case outside the allow-list has a non-empty reference set).  Per case, dtype, operand, position
and poison this file
  1. runs the call on the finite inputs, through the Python wrapper, and asserts an all-finite result (the baseline);
  2. sets one element of one operand to the poison and runs the call again, with every buffer the wrapper allocates
     (torch.empty / torch.empty_like) pre-filled with a finite sentinel;
  3. asserts inclusion: every element that is non-finite in torch's fp64 evaluation of the wrapper's documented expression
     is non-finite in the kernel's output - for the result and for every gradient the call returns.
The converse is not asserted (a kernel may spread a NaN further than torch does), and the kind need not match.  Each
runner asserts the autograd node (or calls the kernel wrapper directly), so a fall-back to torch cannot pass."""
import pytest
import torch

from test_nonfinite_refs_cpu import BY_NAME, DTYPES, EPS, F32, MOMENTUM, params, poisoned, sentinel_alloc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _no_live_tuning():
    """the GEMM dispatcher in mode 0 (hipBLASLt's first heuristic answer, no timing, no candidate runs), as
    tests/test_gemm_f16_fp64_gpu.py; the baseline run of a case resolves each problem on finite operands"""
    import _vah
    from test_gemm_f16_fp64_gpu import _env_tuning
    _vah.check(_vah.lib.vah_gemm_set_tuning(0, 32), 'gemm_set_tuning')
    yield
    _vah.check(_vah.lib.vah_gemm_set_tuning(*_env_tuning()), 'gemm_set_tuning')


def _g(t):
    return None if t is None else t.detach().cuda()


def _leaf(t):
    return None if t is None else t.detach().cuda().requires_grad_(True)


def _node(t, prefix):
    fn = t.grad_fn
    if fn is not None and type(fn).__name__ == 'ViewBackward0':      # a reshape of the fused call's result
        fn = fn.next_functions[0][0]
    assert fn is not None and type(fn).__name__.startswith(prefix), 'the fused path did not run: %s' % type(fn).__name__


def _norm(ins, C):
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM, affine=True).cuda()
    with torch.no_grad():
        bn.weight.copy_(ins['gamma'])
        bn.bias.copy_(ins['beta'])
        bn.running_mean.copy_(ins['rm'])
        bn.running_var.copy_(ins['rv'])
    return bn.train(ins['training'])


# ---------------------------------------------------------------------------------------------------------------------
# runners: ins (CPU tensors) -> {output name: GPU tensor}, the names of the case's reference
# ---------------------------------------------------------------------------------------------------------------------
def run_spm_image(ins, dtype, monkeypatch):
    from vitadapter import spm_nhwc
    return {'y': spm_nhwc.image_to_nhwc16(_g(ins['x']), dtype)}


def run_spm_conv(ins, dtype, monkeypatch):
    from vitadapter import conv
    x, w, gy, s = _g(ins['x']), _g(ins['w']), _g(ins['gy']), ins['stride']
    out = {'y': conv.conv3x3_forward(x, conv.forward_weight(w, dtype), s), 'gw': conv.conv3x3_weight_grad(x, gy, s)}
    if ins['dgrad']:
        out['gx'] = conv.conv3x3_input_grad(gy, conv.dgrad_weight(w, dtype), s, x.shape[1:3])
    return out


def run_spm_bn(ins, dtype, monkeypatch):
    from vitadapter import spm_nhwc
    bn = _norm(ins, ins['x'].shape[-1])
    x = _leaf(ins['x'])
    y = spm_nhwc._BNRelu.apply(x, bn.weight, bn.bias, bn, ins['relu'])
    _node(y, '_BNRelu')
    y.backward(_g(ins['dy']))
    return {'y': y.detach(), 'dx': x.grad, 'dweight': bn.weight.grad, 'dbias': bn.bias.grad,
            'running_mean': bn.running_mean, 'running_var': bn.running_var}


def run_spm_maxpool(ins, dtype, monkeypatch):
    from vitadapter import spm_nhwc
    x = _leaf(ins['x'])
    y = spm_nhwc._MaxPool.apply(x)
    _node(y, '_MaxPool')
    y.backward(_g(ins['gy']))
    return {'y': y.detach(), 'gx': x.grad}


def run_tail_bn(ins, dtype, monkeypatch):
    from vitadapter import fused
    bn = _norm(ins, ins['a'].shape[1])
    a = _leaf(ins['a'])
    with torch.autocast('cuda', dtype=dtype):
        if ins['relu']:
            monkeypatch.setattr(fused, 'BN_RELU_MIN_NUMEL', 0)      # the gate is a tuning constant (8M elements)
            y = fused.bn_relu(bn, a)
        else:
            b, x = _leaf(ins['b']), _leaf(ins['x'])
            y = fused.bn_tail(bn, a, b, x, ins['scale'], _g(ins['shift']))
    _node(y, '_BNTail')
    y.backward(_g(ins['dy']))
    out = {'y': y.detach(), 'da': a.grad, 'dweight': bn.weight.grad, 'dbias': bn.bias.grad,
           'running_mean': bn.running_mean, 'running_var': bn.running_var}
    if not ins['relu']:
        out.update(db=b.grad, dx=x.grad)
    return out


def run_tail_tokens_to_maps(ins, dtype, monkeypatch):
    from vitadapter import fused
    from test_nonfinite_refs_cpu import MAP_HW
    tok = _leaf(ins['tokens'])
    with torch.autocast('cuda', dtype=dtype):
        m0, m1 = fused.tokens_to_maps(tok, MAP_HW)
    _node(m0, '_TokensToMaps')
    torch.autograd.backward([m0, m1], [_g(ins['g0']), _g(ins['g1'])])
    return {'m0': m0.detach(), 'm1': m1.detach(), 'gtokens': tok.grad}


def run_tail_maps_to_tokens(ins, dtype, monkeypatch):
    from vitadapter import fused
    m0, m1, v0, v1 = _leaf(ins['m0']), _leaf(ins['m1']), _leaf(ins['v0']), _leaf(ins['v1'])
    with torch.autocast('cuda', dtype=dtype):
        tok = fused.maps_to_tokens([m0, m1], [v0, v1])
    _node(tok, '_MapsToTokens')
    tok.backward(_g(ins['g']))
    return {'tokens': tok.detach(), 'gm0': m0.grad, 'gm1': m1.grad, 'gv0': v0.grad, 'gv1': v1.grad}


def run_tail_max_pool(ins, dtype, monkeypatch):
    from vitadapter import fused
    x = _leaf(ins['x'])
    with torch.autocast('cuda', dtype=dtype):
        y = fused.max_pool(torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1), x)
    _node(y, '_MaxPool3s2')
    y.backward(_g(ins['gy']))
    return {'y': y.detach(), 'gx': x.grad}


def run_tail_halve(ins, dtype, monkeypatch):
    from vitadapter import fused
    x = _leaf(ins['x'])
    with torch.autocast('cuda', dtype=dtype):
        y = fused.halve(x)
    _node(y, 'AvgPool')
    y.backward(_g(ins['gy']))
    return {'y': y.detach(), 'gx': x.grad}


class _Drop:
    drop_prob, training = 0.3, True


class _fixed_drop:
    """fused.DROP_POOL.take answers with the given per-image scales (stands in for the pooled drop-path draw)"""

    def __init__(self, sc):
        self.sc = sc

    def __enter__(self):
        from vitadapter import fused
        self.take = fused.DROP_POOL.take
        fused.DROP_POOL.take = lambda x_, keep: self.sc

    def __exit__(self, *exc):
        from vitadapter import fused
        fused.DROP_POOL.take = self.take
        return False


def _layer_norm(ins, C, tag=''):
    ln = torch.nn.LayerNorm(C, eps=EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(ins['lnw' + tag])
        ln.bias.copy_(ins['lnb' + tag])
    return ln


def _linear(ins, tag=''):
    w = ins['w' + tag]
    lin = torch.nn.Linear(w.shape[1], w.shape[0]).cuda()
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(ins['b' + tag])
    return lin


def run_rows_layer_norm(ins, dtype, monkeypatch):
    from vitadapter import fused
    ln, x = _layer_norm(ins, ins['x'].shape[-1]), _leaf(ins['x'])
    with torch.autocast('cuda', dtype=dtype):
        y = fused.layer_norm(ln, x)
    _node(y, '_LayerNormBF16')
    y.backward(_g(ins['g']))
    return {'y': y.detach(), 'dx': x.grad, 'dw': ln.weight.grad, 'db': ln.bias.grad}


def run_rows_layer_norm_dual_keep(ins, dtype, monkeypatch):
    from vitadapter import fused
    C = ins['x'].shape[-1]
    na, nb, x = _layer_norm(ins, C, 'a'), _layer_norm(ins, C, 'b'), _leaf(ins['x'])
    with torch.autocast('cuda', dtype=dtype):
        xk, ya, yb = fused.layer_norm_dual_keep(na, nb, x * 1.0)
    _node(ya, '_LayerNormDualBF16')
    torch.autograd.backward([xk, ya, yb], [_g(ins['gres']), _g(ins['ga']), _g(ins['gb'])])
    return {'x': xk.detach(), 'ya': ya.detach(), 'yb': yb.detach(), 'dx': x.grad, 'dwa': na.weight.grad, 'dba': na.bias.grad,
            'dwb': nb.weight.grad, 'dbb': nb.bias.grad}


def run_rows_residual(ins, dtype, monkeypatch):
    from vitadapter import fused
    x, z, gamma = _leaf(ins['x']), _leaf(ins['z']), _leaf(ins['gamma'])
    out = {}
    with _fixed_drop(_g(ins['scale'])), torch.autocast('cuda', dtype=dtype):
        if ins['with_ln']:
            ln = _layer_norm(ins, x.shape[-1])
            t, h = fused.residual_ln(x, z, gamma, _Drop(), ln)
            _node(h, '_ResidualLN')
            torch.autograd.backward([t, h], [_g(ins['gt']), _g(ins['gh'])])
            out.update(t=t.detach(), h=h.detach(), dw=ln.weight.grad, db=ln.bias.grad)
        else:
            y = fused.residual(x, z, gamma, _Drop())
            _node(y, '_ScaleResidual')
            y.backward(_g(ins['gt']))
            out.update(y=y.detach())
    out.update(dx=x.grad, dz=z.grad)
    if gamma is not None:
        out.update(dgamma=gamma.grad)
    return out


def run_rows_gelu(ins, dtype, monkeypatch):
    from vitadapter import fused
    h = _leaf(ins['h'])
    setattr(h, fused._BiasPartials.ATTR, True)          # as fused.linear marks its output: the GELU sums fc1's bias gradient
    with torch.autocast('cuda', dtype=dtype):
        a = fused.gelu(torch.nn.GELU(), h)
    _node(a, '_GeluBF16')
    a.backward(_g(ins['da']))
    return {'a': a.detach(), 'dh': h.grad}


def run_rows_dwconv_tokens(ins, dtype, monkeypatch):
    from vitadapter import fused
    from test_nonfinite_refs_cpu import DW_C, DW_H, DW_W
    conv = torch.nn.Conv2d(DW_C, DW_C, 3, 1, 1, groups=DW_C).cuda()
    with torch.no_grad():
        conv.weight.copy_(ins['w'])
        conv.bias.copy_(ins['b'])
    x = _leaf(ins['x'])
    with torch.autocast('cuda', dtype=dtype):
        y = fused.dwconv_tokens(conv, x, DW_H, DW_W)
    assert y is not None
    _node(y, '_DWConvTokens')
    y.backward(_g(ins['g']))
    return {'y': y.detach(), 'dx': x.grad, 'dw': conv.weight.grad, 'db': conv.bias.grad}


def run_lin_linear(ins, dtype, monkeypatch):
    from vitadapter import fused
    lin, x = _linear(ins), _leaf(ins['x'])
    with torch.autocast('cuda', dtype=dtype):
        y = fused.linear(lin, x)
    _node(y, '_LinearBF16')
    y.backward(_g(ins['g']))
    return {'y': y.detach(), 'dx': x.grad, 'dw': lin.weight.grad, 'db': lin.bias.grad}


def run_lin_mlp_bias_partials(ins, dtype, monkeypatch):
    from vitadapter import fused
    fc1, fc2, ln = _linear(ins, '1'), _linear(ins, '2'), _layer_norm(ins, 40)
    x, x0 = _leaf(ins['x']), _leaf(ins['x0'])
    seen, real = [], fused._wgrad_bgrad

    def wgrad_bgrad(g2, x2, partials=None):
        seen.append(partials is not None)
        return real(g2, x2, partials)

    monkeypatch.setattr(fused, '_wgrad_bgrad', wgrad_bgrad)
    with _fixed_drop(_g(ins['scale'])), torch.autocast('cuda', dtype=dtype):
        a = fused.gelu(torch.nn.GELU(), fused.linear(fc1, x))
        _node(a, '_GeluBF16')
        t, h = fused.residual_ln(x0, fused.linear(fc2, a), None, _Drop(), ln)
        _node(h, '_ResidualLN')
        torch.autograd.backward([t, h], [_g(ins['gt']), _g(ins['gh'])])
    assert seen == [True, True], 'the Linears did not take the bias partials of the GELU / residual + LayerNorm backward: %r' % seen
    return {'t': t.detach(), 'h': h.detach(), 'dx': x.grad, 'dx0': x0.grad, 'dw1': fc1.weight.grad, 'db1': fc1.bias.grad,
            'dw2': fc2.weight.grad, 'db2': fc2.bias.grad, 'dlnw': ln.weight.grad, 'dlnb': ln.bias.grad}


def run_lin_linear_pair(ins, dtype, monkeypatch):
    from vitadapter import fused
    la, lb, x = _linear(ins, 'a'), _linear(ins, 'b'), _leaf(ins['x'])
    with torch.autocast('cuda', dtype=dtype):
        ya, yb = fused.linear_pair(la, lb, x)
    _node(ya, '_LinearPairBF16')
    torch.autograd.backward([ya, yb], [_g(ins['ga']), _g(ins['gb'])])
    return {'ya': ya.detach(), 'yb': yb.detach(), 'dx': x.grad, 'dwa': la.weight.grad, 'dba': la.bias.grad,
            'dwb': lb.weight.grad, 'dbb': lb.bias.grad}


def run_lin_conv1x1(ins, dtype, monkeypatch):
    from vitadapter import fused
    conv = torch.nn.Conv2d(16, 24, 1, bias=False).cuda()
    with torch.no_grad():
        conv.weight.copy_(ins['w'])
    x = _leaf(ins['x'])
    with torch.autocast('cuda', dtype=dtype):
        y = fused.conv1x1(conv, x)
    _node(y, '_Conv1x1BF16')
    y.backward(_g(ins['g']))
    return {'y': y.detach(), 'dx': x.grad, 'dw': conv.weight.grad}


def run_lin_patch_embed(ins, dtype, monkeypatch):
    from vitadapter import fused
    conv = torch.nn.Conv2d(3, 24, 16, 16).cuda()
    with torch.no_grad():
        conv.weight.copy_(ins['w'])
        conv.bias.copy_(ins['b'])
    with torch.autocast('cuda', dtype=dtype):
        got = fused.patch_embed(conv, _g(ins['x']))
    assert got is not None and got[1:] == (2, 2)
    _node(got[0], '_LinearBF16')
    got[0].backward(_g(ins['g']))
    return {'y': got[0].detach(), 'dw': conv.weight.grad, 'db': conv.bias.grad}


def run_lin_up_from_tokens(ins, dtype, monkeypatch):
    from vitadapter import fused
    up = torch.nn.ConvTranspose2d(16, 16, 2, 2).cuda()
    with torch.no_grad():
        up.weight.copy_(ins['w'])
    rows, add = _leaf(ins['rows']), _leaf(ins['addend'])
    with torch.autocast('cuda', dtype=dtype):
        y = fused.up_from_tokens(up, rows, 8, 8, add)
    assert y is not None
    _node(y, '_UpFromTokens')
    y.backward(_g(ins['g']))
    return {'y': y.detach(), 'drows': rows.grad, 'daddend': add.grad, 'dw': up.weight.grad}


def run_attn(ins, dtype, monkeypatch):
    from vitadapter import kernels
    from test_nonfinite_refs_cpu import ATTN_SCALE
    qkv = _leaf(ins['qkv'])
    out = {}
    if ins['kind'] == 'seq':
        o = kernels.attention(qkv, ATTN_SCALE)
        _node(o, '_FlashAttention')
    elif ins['kind'] == 'bias':
        bias = _leaf(ins['bias'])
        o = kernels.attention_bias(qkv, bias, ATTN_SCALE)
    elif ins['kind'] == 'relpos':
        table = _leaf(ins['table'])
        o = kernels.attention_relpos(qkv, table, _g(ins['index']), ATTN_SCALE)
    else:
        o = kernels.window_attention(qkv, ATTN_SCALE, ins['grid'][0], ins['grid'][1], ins['win'])
    assert o is not None, 'the MFMA path did not take the call'
    o.backward(_g(ins['dout']))
    out.update(out=o.detach(), dqkv=qkv.grad)
    if ins['kind'] == 'bias':
        out.update(dbias=bias.grad)
    if ins['kind'] == 'relpos':
        out.update(dtable=table.grad)
    return out


class _PairModule:
    """what fused.msda_pair_core reads of an MSDeformAttn module"""

    def __init__(self, ins, M, L):
        from test_nonfinite_refs_cpu import MSDA_P
        self.n_heads, self.n_levels, self.n_points = M, L, MSDA_P
        self.sampling_offsets, self.attention_weights = _linear(ins, 'a'), _linear(ins, 'b')


def run_msda(ins, dtype, monkeypatch):
    """The plain fp32 Function behind the module's torch glue, the fused Function (bf16 / fp16 operands) and the pair core.

    Poisoned: value, logits, offsets and the incoming gradient (pair core: value, query, incoming gradient - its Linears
    make offsets and logits from the query).  A sample whose location is NaN or +-inf is not dropped as one outside the
    map is: the kernels put it on pixel (0, 0) with NaN fractions, so its weights, the output and the gradients it feeds
    are NaN, as torch's grid_sample makes them.

    Why a NaN or +-inf sampling coordinate cannot form an out-of-range address or list index in any kernel a location
    reaches - established by reading the code before the first such case ran:
      * every kernel turns a location into pixel coordinates with the same arithmetic and the same gate,
        `gate = h_im > -1 && w_im > -1 && h_im < H && w_im < W`: csrc/msda_common.h make_tap (the only location code of
        msda.hip and of msda_fused.hip), the inline copy in csrc/msda_fwd_win.hip and make_base in csrc/msda_tile.hip
        (binning and tile pass).  A NaN fails every comparison; +inf fails `< H`, -inf fails `> -1`; `ref + off / W` of a
        non-finite offset is non-finite, never a large finite number.
      * the float -> int conversions see `gate ? h_im : 0`, never the coordinate itself: a sample that fails the gate has
        the base pixel (0, 0), which exists in every valid level (H, W >= 1); its other corners are used only under the
        in-map checks (h_high <= H - 1, w_high <= W - 1) that every sample passes through.
      * a non-finite sample is then an ordinary in-map sample at (0, 0) for all addressing - rows, atomics, the LDS
        window or the global fetch beyond the halo, the bin of tile (0, 0) and its list - and only its fractions
        (lh, lw = NaN) differ; a finite sample outside the gate is dropped as before (ok[] false, rows 0, no tile).
      * the binning clamps tile rows / columns to the map, names tiles only for samples with in[p] = inside; the tile pass
        clamps its list reads and the window cell, gates the weight columns by unsigned range checks and the gradient
        stores by on[p] = live && inside.
    Reference points are geometry, not activations, and are never poisoned: the window schedule of
    msda_fwd_win.hip:82-83 - the one place that converts an ungated coordinate - only sees finite values."""
    from oracle import cases
    from ops.functions.ms_deform_attn_func import MSDeformAttnFunction
    from ops.functions import ms_deform_attn_fused as mf
    for k, v in ins.get('env', {}).items():
        monkeypatch.setenv(k, v)
    levels = ins['levels']
    L = len(levels)
    shapes, lsi = torch.tensor(levels).cuda(), cases.level_start_index(levels).cuda()
    value, ref = _leaf(ins['value']), _g(ins['ref'])
    M = value.shape[2]
    if ins['pair']:
        from vitadapter import fused
        mod, query = _PairModule(ins, M, L), _leaf(ins['query'])
        with torch.autocast('cuda', dtype=dtype):
            assert fused.msda_pair_core_ok(mod, query, value, ref)
            out = fused.msda_pair_core(mod, query, value, shapes, lsi, ref)
        _node(out, '_MSDAPairCore')
        out.backward(_g(ins['gout']))
        a, b = mod.sampling_offsets, mod.attention_weights
        return {'out': out.detach(), 'grad_value': value.grad, 'dquery': query.grad, 'dwa': a.weight.grad, 'dba': a.bias.grad,
                'dwb': b.weight.grad, 'dbb': b.bias.grad}
    offsets, logits = _leaf(ins['offsets']), _leaf(ins['logits'])
    N, Lq = offsets.shape[:2]
    if dtype == F32:        # the module's glue in torch (ms_deform_attn.py:137-144), the plain Function on locations / weights
        norm = torch.tensor([[w, h] for h, w in levels], dtype=F32).cuda()
        loc = ref[:, :, None, :, None, :] + offsets / norm[None, None, None, :, None, :]
        attn = torch.softmax(logits, -1).view(N, Lq, M, L, -1)
        out = MSDeformAttnFunction.apply(value, shapes, lsi, loc, attn, 64)
        _node(out, 'MSDeformAttnFunction')
    else:
        assert mf.fused_supported(value, offsets, logits, ref, L, offsets.shape[4])
        out = mf.MSDeformAttnFusedFunction.apply(value, shapes, lsi, offsets, logits, ref)
        _node(out, 'MSDeformAttnFusedFunction')
    out.backward(_g(ins['gout']))
    return {'out': out.detach(), 'grad_value': value.grad, 'd_offsets': offsets.grad, 'd_logits': logits.grad}


def _runner(case):
    return globals()['run_' + case.kw.get('run', case.name)]


def _finite_where_torch_is_not(got, ref):
    """-> list of 'output: n of m ... first at flat i' for the outputs that break inclusion"""
    bad = []
    for name, r in ref.items():
        assert name in got and got[name] is not None, 'the call returned no %s' % name
        g = got[name].detach().cpu()
        assert tuple(g.shape) == tuple(r.shape), (name, tuple(g.shape), tuple(r.shape))
        want = ~torch.isfinite(r).reshape(-1)
        miss = want & torch.isfinite(g.double()).reshape(-1)
        if bool(miss.any()):
            i = int(torch.nonzero(miss)[0])
            bad.append('%s: %d of the %d elements that are non-finite in torch came out finite; first at flat %d: got %r, torch %r'
                       % (name, int(miss.sum()), int(want.sum()), i, g.reshape(-1)[i].item(), r.reshape(-1)[i].item()))
    return bad


@pytest.mark.parametrize('name,dt,op,label,poison', params())
def test_nonfinite_in_nonfinite_out(name, dt, op, label, poison, monkeypatch):
    case, dtype = BY_NAME[name], DTYPES[dt]
    run = _runner(case)
    ins = case.build(dtype)
    base = run(ins, dtype, monkeypatch)
    torch.cuda.synchronize()
    for k, v in base.items():
        assert v is not None and bool(torch.isfinite(v).all()), '%s: the finite baseline gives a non-finite %s' % (name, k)
    bad_ins = poisoned(ins, op, label, poison)
    with sentinel_alloc():
        got = run(bad_ins, dtype, monkeypatch)
        torch.cuda.synchronize()
    bad = _finite_where_torch_is_not(got, case.ref(bad_ins))
    assert not bad, '%s, %s at %s of %s:\n  %s' % (name, poison, label, op, '\n  '.join(bad))
