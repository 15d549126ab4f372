"""MSDeformAttnPixelDecoder (vitadapter/pixel_decoder.py) against the golden produced by the
reference's own class (tools/gen_golden_pixel_decoder.py -> tests/golden/pixel_decoder.npz): state-dict layout,
mask_feature, the three multi-scale maps, the position term and reference points handed to the encoder, the four input
gradients (every 23rd element + a digest of the whole) and digests of every parameter gradient (sum, weighted sum,
largest magnitude, sum of magnitudes), for two cases (the
second with a 33 x 49 stride-4 map over 16 x 24).

PARITY UNPINNED against mmcv for the ConvModule and the encoder class (stand-ins in the tool: conv -> gn -> ReLU, and the
arithmetic of tests/test_pixel_decoder.py::_expected); the forward composition, the sine term, the points, the level
order and the FPN tail are the reference's own code.

CPU tier: the gather inside ops.modules is patched with the oracle (the product has no CPU kernel).  GPU tier: the HIP
kernels - fp32 against the golden, then bf16 / fp16 autocast against a yardstick, torch's own autocast evaluation of the
same module (ENABLED group_norm, linear, spm_nhwc off): both are independent roundings of the same arithmetic, so the
kernel path may show at most 2 x the yardstick's error in each quantity.  Measured on MI355X (kernel path / yardstick,
relative L2 error; outputs against the golden, parameter gradients against the module's own fp32 GPU run, which
test_gpu_fp32_matches_golden holds to the golden):
    see MEASURED below."""
import json
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pixel_decoder.npz')
CASES = ('base', 'odd')
# measured pairs (kernel path, yardstick), relative L2: worst output, worst input gradient, median and worst parameter
# gradient.  A record of one run, not a bound: the bound is 2 x the yardstick of the same run.
MEASURED = {
    # dtype: {case: {quantity: (kernel path, yardstick)}}
    'bf16': {'base': dict(out=(0.0045, 0.0047), gfeat=(0.062, 0.050), gp_median=(0.041, 0.042), gp_worst=(0.088, 0.098)),
             'odd': dict(out=(0.0046, 0.0048), gfeat=(0.061, 0.050), gp_median=(0.042, 0.045), gp_worst=(0.092, 0.118))},
    'fp16': {'base': dict(out=(0.00058, 0.00074), gfeat=(0.062, 0.062), gp_median=(0.0145, 0.0160), gp_worst=(0.103, 0.105)),
             'odd': dict(out=(0.00058, 0.00074), gfeat=(0.065, 0.066), gp_median=(0.0156, 0.0178), gp_worst=(0.127, 0.129))},
}


@pytest.fixture(scope='module')
def gold():
    g = np.load(GOLD)
    return g, json.loads(str(g['meta']))


def _digest(t):
    a = t.detach().to(torch.float64).flatten().cpu().numpy()
    return np.array([a.sum(), (a * np.cos(np.arange(a.size, dtype=np.float64) * 0.61803398875)).sum()], dtype=np.float64)


def _check_digest(what, t, want, tol):
    """want = [sum, weighted sum, largest magnitude, sum of magnitudes] of the golden's tensor.  An element-wise relative
    error of tol moves either sum (weights of magnitude <= 1) by at most tol * sum of magnitudes; the floor of 1 is the
    absolute floor of the per-element bounds of tests/test_pixel_decoder.py.  The largest magnitude is held to the
    per-element bound itself."""
    got = _digest(t)
    bound = tol * max(1.0, want[3])
    assert np.abs(got - want[:2]).max() <= bound, (what, got, want, bound)
    assert abs(float(t.detach().abs().max()) - want[2]) <= tol * max(1.0, want[2]), (what, float(t.detach().abs().max()), want[2])
    assert abs(float(t.detach().double().abs().sum()) - want[3]) <= bound, (what, float(t.detach().double().abs().sum()), want[3])


def _named(outs, gfeats, gparams):
    d = dict(zip(('mask_feature', 'ms0', 'ms1', 'ms2'), outs))
    d.update(('gfeat%d' % i, t) for i, t in enumerate(gfeats))
    d.update(('grad:' + k, t) for k, t in gparams.items())
    return d


# What two runs of the module may NOT be asked to agree on bit for bit, by data flow.  Everything else is asserted, so a
# new source of run-to-run differences anywhere else fails the test.
#  * Under autocast every operator of the tail is this repository's and ordered (GEMMs, csrc/group_norm.hip, csrc/conv.hip).
#    The gradient reaches the encoder through the adjoint of F.interpolate (upsample_bilinear2d_backward accumulates with
#    float atomics: torch lists it as non-deterministic), and inside the encoder through the MSDA tile pass, which orders a
#    tile's list by atomics.  Behind them: every encoder parameter, the input convs, the level embedding and
#    the three coarse input gradients.  Seen on the GPU: in the 33 x 49 case all of these differ, down to the last layer's
#    norms.1.bias (behind the upsample adjoint alone); in the 32 x 48 case, where every coarse pixel receives the same four
#    weights, only value_proj (behind the tile pass) and what follows it.
BEHIND_ATOMICS = ('grad:encoder.', 'grad:input_convs.', 'grad:level_encoding.', 'gfeat1', 'gfeat2', 'gfeat3')
#  * In plain fp32 the 3 x 3 output_conv is torch's (MIOpen), whose result was seen to change bits between calls of one
#    process.  mask_feature is computed from it, and so is every gradient: the backward of the GroupNorm behind the
#    convolution reads the convolution's output.  In front of it stand the three encoder maps.
BEHIND_TORCH_FP32_CONV = ('mask_feature', 'gfeat', 'grad:')


def _assert_same_bits(what, first, second, may_differ):
    differ = [k for k in first if not torch.equal(first[k], second[k])]
    assert [k for k in differ if not k.startswith(may_differ)] == [], (what, differ)
    assert len([k for k in first if not k.startswith(may_differ)]) >= 3


def _grid(g, key):
    return torch.from_numpy(g[key + '_q'].astype(np.float32)) * float(g[key + '_scale'])


def _model(g, meta, dev):
    from vitadapter.pixel_decoder import MSDeformAttnPixelDecoder
    m = MSDeformAttnPixelDecoder(**meta['config'])
    sd = {}
    for k, shape in meta['state_dict'].items():
        v = _grid(g, 'w_' + k)
        sd[k] = 1.0 + v if (v.dim() == 1 and not k.endswith('bias')) else v
        assert list(v.shape) == shape
    m.load_state_dict(sd)
    return m.to(dev)


def _io(g, case, dev):
    feats = [_grid(g, '%s_feat%d' % (case if i == 0 else 'base', i)).to(dev).requires_grad_(True) for i in range(4)]
    gouts = [_grid(g, '%s_gout%d' % (case if j == 0 else 'base', j)).to(dev) for j in range(4)]
    return feats, gouts


def _run(m, feats, gouts, autocast=None):
    m.zero_grad(set_to_none=True)
    for f in feats:
        f.grad = None
    if autocast is None:
        mf, ms = m(feats)
    else:
        with torch.autocast('cuda', dtype=autocast):
            mf, ms = m(feats)
    outs = [mf] + list(ms)
    sum((o.float() * go).sum() for o, go in zip(outs, gouts)).backward()
    return [o.detach().float() for o in outs], [f.grad.detach().float() for f in feats], {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _check_against_golden(g, meta, case, outs, gfeats, gparams, tol_out, tol_g, tol_gp):
    want = [g[case + '_mask_feature']] + [g['base_ms%d' % j] for j in range(3)]
    for j, (o, w) in enumerate(zip(outs, want)):
        assert tuple(o.shape) == w.shape, (j, o.shape, w.shape)
        assert np.abs(o.cpu().numpy() - w).max() <= tol_out, (case, j, np.abs(o.cpu().numpy() - w).max())
    step = meta['step']
    for i, gf in enumerate(gfeats):
        w = g['%s_gfeat%d_sample' % (case, i)]
        got = gf.cpu().flatten()[::step].numpy()
        assert np.abs(got - w).max() <= tol_g * max(1.0, np.abs(w).max()), (case, i, np.abs(got - w).max())
        _check_digest((case, 'gfeat', i), gf, g['%s_gfeat%d_digest' % (case, i)], tol_g)
    n = 0
    for k, gr in gparams.items():
        _check_digest((case, k), gr, g['%s_gp_%s' % (case, k)], tol_gp)
        n += 1
    assert n == len(meta['state_dict'])


def _patch_oracle(monkeypatch):
    import ops.modules.ms_deform_attn as mod
    from oracle import msda as oracle_msda

    class _OracleFunction:
        @staticmethod
        def apply(value, shapes, lsi, loc, attn, step):
            return oracle_msda.core_torch(value, shapes, loc, attn)
    monkeypatch.setattr(mod, 'MSDeformAttnFunction', _OracleFunction)


def test_state_dict_table_equals_the_goldens(gold):
    from vitadapter.pixel_decoder import MSDeformAttnPixelDecoder
    g, meta = gold
    m = MSDeformAttnPixelDecoder(**meta['config'])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == meta['state_dict']
    keys = [k for k in meta['state_dict'] if not k.startswith('encoder.')]
    want = (['input_convs.%d.%s' % (i, s) for i in range(3) for s in ('conv.weight', 'conv.bias', 'gn.weight', 'gn.bias')]
            + ['lateral_convs.0.conv.weight', 'lateral_convs.0.gn.weight', 'lateral_convs.0.gn.bias', 'output_convs.0.conv.weight',
               'output_convs.0.gn.weight', 'output_convs.0.gn.bias', 'mask_feature.weight', 'mask_feature.bias', 'level_encoding.weight'])
    assert sorted(keys) == sorted(want)
    # the defaults are the reference's: 256 channels, 6 layers, 8 heads, 3 levels, 4 points, FFN 1024
    d = MSDeformAttnPixelDecoder()
    assert d.input_convs[0].conv.weight.shape == (256, 2048, 1, 1) and d.lateral_convs[0].conv.weight.shape == (256, 256, 1, 1)
    assert len(d.encoder.layers) == 6 and d.encoder.layers[0].attentions[0].sampling_offsets.weight.shape == (8 * 3 * 4 * 2, 256)
    assert d.encoder.layers[0].ffns[0].layers[0][0].weight.shape == (1024, 256) and d.level_encoding.weight.shape == (3, 256)


def test_constructor_refuses_what_it_does_not_build(gold):
    from vitadapter.pixel_decoder import MSDeformAttnPixelDecoder
    cfg = gold[1]['config']
    for bad in (dict(norm_cfg=None), dict(norm_cfg=dict(type='BN')), dict(norm_cfg=dict(type='GN')),
                dict(positional_encoding=dict(type='LearnedPositionalEncoding', num_feats=32)), dict(positional_encoding=None)):
        with pytest.raises(ValueError):
            MSDeformAttnPixelDecoder(**dict(cfg, **bad))


def _reference_pixel_decoder_cfg(**ffn):
    """the ``pixel_decoder`` dict of the reference's configs/_base_/models/mask2former_beit.py:31-63, key for key"""
    return dict(
        type='MSDeformAttnPixelDecoder', num_outs=3, norm_cfg=dict(type='GN', num_groups=32), act_cfg=dict(type='ReLU'),
        encoder=dict(type='DetrTransformerEncoder', num_layers=6, transformerlayers=dict(
            type='BaseTransformerLayer',
            attn_cfgs=dict(type='MultiScaleDeformableAttention', embed_dims=256, num_heads=8, num_levels=3, num_points=4,
                           im2col_step=64, dropout=0.0, batch_first=False, norm_cfg=None, init_cfg=None),
            ffn_cfgs=dict(dict(type='FFN', embed_dims=256, feedforward_channels=1024, num_fcs=2, ffn_drop=0.0,
                               act_cfg=dict(type='ReLU', inplace=True)), **ffn),
            operation_order=('self_attn', 'norm', 'ffn', 'norm')), init_cfg=None),
        positional_encoding=dict(type='SinePositionalEncoding', num_feats=128, normalize=True), init_cfg=None)


def test_constructor_reads_ffn_cfgs_as_the_reference_configs_give_them():
    from vitadapter.pixel_decoder import MSDeformAttnPixelDecoder

    def build(cfg, **kw):
        cfg = dict(cfg, **kw)
        assert cfg.pop('type') == 'MSDeformAttnPixelDecoder'
        return MSDeformAttnPixelDecoder(in_channels=[1024] * 4, strides=[4, 8, 16, 32], feat_channels=256, out_channels=256, **cfg)

    def ffn(m):
        f = m.encoder.layers[-1].ffns[0]
        return tuple(f.layers[0][0].weight.shape), tuple(f.layers[1].weight.shape), f.layers[0][2].p, f.layers[2].p
    m = build(_reference_pixel_decoder_cfg())
    assert len(m.encoder.layers) == 6 and ffn(m) == ((1024, 256), (256, 1024), 0.0, 0.0)
    assert m.input_convs[0].conv.weight.shape == (256, 1024, 1, 1)
    m = build(_reference_pixel_decoder_cfg(feedforward_channels=2048, ffn_drop=0.1))        # not this class's defaults
    assert ffn(m) == ((2048, 256), (256, 2048), 0.1, 0.1)

    def layers(**kw):
        cfg = _reference_pixel_decoder_cfg()
        tl = cfg['encoder']['transformerlayers']
        for k, v in kw.items():
            if v is None:
                tl.pop(k)
            else:
                tl[k] = v
        return cfg
    # the deprecated top-level keys (the class's own default encoder) where ffn_cfgs is silent or absent
    assert ffn(build(layers(ffn_cfgs=None, feedforward_channels=512, ffn_dropout=0.2))) == ((512, 256), (256, 512), 0.2, 0.2)
    assert ffn(build(layers(ffn_cfgs=dict(type='FFN', num_fcs=2), feedforward_channels=512))) == ((512, 256), (256, 512), 0.0, 0.0)
    assert ffn(build(layers(feedforward_channels=1024, ffn_dropout=0.0))) == ((1024, 256), (256, 1024), 0.0, 0.0)      # both, agreeing
    assert ffn(MSDeformAttnPixelDecoder()) == ((1024, 256), (256, 1024), 0.0, 0.0)
    for bad in (layers(feedforward_channels=512), layers(ffn_dropout=0.3),                       # the two forms disagree
                _reference_pixel_decoder_cfg(num_fcs=3), _reference_pixel_decoder_cfg(act_cfg=dict(type='GELU')),
                _reference_pixel_decoder_cfg(embed_dims=128), _reference_pixel_decoder_cfg(add_identity=False),
                _reference_pixel_decoder_cfg(type='MLP'), layers(operation_order=('norm', 'self_attn', 'norm', 'ffn'))):
        with pytest.raises(ValueError):
            build(bad)


@torch.no_grad()
def test_init_weights(gold):
    from vitadapter.pixel_decoder import MSDeformAttnPixelDecoder
    torch.manual_seed(0)
    m = MSDeformAttnPixelDecoder(**dict(gold[1]['config'], feat_channels=256, out_channels=256, in_channels=[256] * 4,
                                        positional_encoding=dict(type='SinePositionalEncoding', num_feats=128, normalize=True),
                                        encoder=None))
    with torch.no_grad():
        for p in m.parameters():
            p.fill_(7.0)
    m.init_weights()
    for c in m.input_convs:
        assert float(c.conv.bias.abs().max()) == 0
        bound = (6.0 / (256 + 256)) ** 0.5                             # Xavier uniform, gain 1
        assert float(c.conv.weight.abs().max()) <= bound and float(c.conv.weight.std()) > 0.5 * bound
        assert float((c.gn.weight - 7.0).abs().max()) == 0             # norms are not touched
    assert float(m.mask_feature.bias.abs().max()) == 0
    for conv, fan_in in ((m.lateral_convs[0].conv, 256), (m.output_convs[0].conv, 256 * 9), (m.mask_feature, 256)):
        bound = (3.0 / fan_in) ** 0.5                                  # Kaiming uniform, a = 1: gain 1
        assert float(conv.weight.abs().max()) <= bound and float(conv.weight.std()) > 0.5 * bound, fan_in
    le = m.level_encoding.weight
    assert abs(float(le.mean())) < 0.15 and abs(float(le.std()) - 1.0) < 0.15
    a = m.encoder.layers[0].attentions[0]
    assert float(a.sampling_offsets.weight.abs().max()) == 0 and float(a.attention_weights.weight.abs().max()) == 0     # runs last
    assert float(m.encoder.layers[0].ffns[0].layers[0][0].weight.std()) > 0


def test_registers_under_the_references_name():
    from vitadapter.pixel_decoder import MSDeformAttnPixelDecoder, register_pixel_decoder

    class _Registry:
        def __init__(self):
            self.seen = {}

        def register_module(self, name=None, force=False, module=None):
            self.seen[name] = module
    r = _Registry()
    assert register_pixel_decoder(r) is MSDeformAttnPixelDecoder and r.seen == {'MSDeformAttnPixelDecoder': MSDeformAttnPixelDecoder}


@pytest.mark.parametrize('case', CASES)
def test_forward_backward_cpu(gold, case, monkeypatch):
    g, meta = gold
    _patch_oracle(monkeypatch)
    m = _model(g, meta, 'cpu')
    feats, gouts = _io(g, case, 'cpu')
    query, pos, ref, ss, lsi, shapes = m.encoder_inputs(feats)
    assert ref.shape == (1, 504, 3, 2) and np.abs(ref[0].numpy() - g['reference_points']).max() <= 1e-6
    assert pos.shape == query.shape == (504, 2, 64)
    assert np.abs(pos[:, 0].detach().numpy() - g['query_pos']).max() <= 2e-5
    assert ss.tolist() == [[4, 6], [8, 12], [16, 24]] and lsi.tolist() == [0, 24, 120]
    outs, gfeats, gparams = _run(m, feats, gouts)
    _check_against_golden(g, meta, case, outs, gfeats, gparams, 2e-5, 2e-5, 2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_gpu_fp32_matches_golden(gold, case):
    """fp32 on the HIP kernels (GroupNorm fp32 -> fp32, the MSDA core; torch's conv / linear) against the golden, bounds of
    tests/test_pixel_decoder.py::test_stack_matches_oracle_on_gpu; twice with identical bits in front of torch's fp32 convolution; and the same results within
    the same bounds with the GroupNorm kernels switched off."""
    from vitadapter import fused
    g, meta = gold
    m = _model(g, meta, 'cuda')
    feats, gouts = _io(g, case, 'cuda')
    assert fused.ENABLED['group_norm']
    outs, gfeats, gparams = _run(m, feats, gouts)
    assert outs[0].shape == (2, 8) + tuple(meta['cases'][case][0])
    _check_against_golden(g, meta, case, outs, gfeats, gparams, 2e-4, 2e-4, 3e-4)
    # twice more (the first run chose library algorithms): identical bits for everything in front of torch's fp32 convolution
    _assert_same_bits(case, _named(*_run(m, feats, gouts)), _named(*_run(m, feats, gouts)), BEHIND_TORCH_FP32_CONV)
    fused.ENABLED['group_norm'] = False
    try:
        outs3, gfeats3, gparams3 = _run(m, feats, gouts)
    finally:
        fused.ENABLED['group_norm'] = True
    _check_against_golden(g, meta, case, outs3, gfeats3, gparams3, 2e-4, 2e-4, 3e-4)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_gpu_autocast_against_torchs_autocast(gold, dtype):
    from vitadapter import fused
    g, meta = gold
    m = _model(g, meta, 'cuda')
    worst = {}
    for case in CASES:
        feats, gouts = _io(g, case, 'cuda')
        want = [torch.from_numpy(g[case + '_mask_feature']).cuda()] + [torch.from_numpy(g['base_ms%d' % j]).cuda() for j in range(3)]
        _, gf32, gp32 = _run(m, feats, gouts)
        sides = {}
        for side, off in (('kernels', ()), ('torch', ('group_norm', 'linear', 'spm_nhwc'))):
            was = {k: fused.ENABLED[k] for k in off}
            for k in off:
                fused.ENABLED[k] = False
            try:
                outs, gf, gp = _run(m, feats, gouts, autocast=dtype)
            finally:
                fused.ENABLED.update(was)
            assert all(bool(torch.isfinite(o).all()) for o in outs)
            if side == 'kernels':
                # identical bits from run to run (after the first, which chose GEMM algorithms): the forward, the stride-4
                # input gradient and every gradient of the tail
                _assert_same_bits((dtype, case), _named(*_run(m, feats, gouts, autocast=dtype)),
                                  _named(*_run(m, feats, gouts, autocast=dtype)), BEHIND_ATOMICS)
            rel_p = sorted(_rel(gp[k], gp32[k]) for k in gp32 if float(gp32[k].norm()) > 0)
            sides[side] = dict(out=max(_rel(o, w) for o, w in zip(outs, want)), gfeat=max(_rel(a, b) for a, b in zip(gf, gf32)),
                               gp_median=rel_p[len(rel_p) // 2], gp_worst=rel_p[-1])
        print('pixel decoder %s autocast, case %s: %s' % (dtype, case, sides))
        worst[case] = sides
    for case, sides in worst.items():
        for q, v in sides['kernels'].items():
            assert v <= 2.0 * sides['torch'][q], (case, q, v, sides['torch'][q])
