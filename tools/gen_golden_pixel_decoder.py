"""MSDeformAttnPixelDecoder golden from the reference's own class.  Container only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_pixel_decoder.py

Imports /root/reference/segmentation/mmseg_custom/{models/plugins/msdeformattn_pixel_decoder.py,
models/utils/positional_encoding.py, core/anchor/point_generator.py} under in-memory stand-ins for mmcv (written here,
with tools/gen_golden.py::_mod) and stores inputs and expected OUTPUTS in tests/golden/pixel_decoder.npz.  The
stand-ins: a ConvModule of ``conv``, an optional ``gn`` and an optional ReLU; registries that do nothing; an
attribute-dict for the ``encoder`` config; an encoder that evaluates the arithmetic of tests/test_pixel_decoder.py::
_expected on oracle.msda.core_torch, with its parameters under mmcv's names.  So the ConvModule and the encoder are NOT
pinned against mmcv; the class's forward composition, the sine term, the points, the level order and the tail are the
reference's own code.

What the file holds (the tests need nothing from oracle/):
  * inputs: the feature maps and every parameter, drawn on small grids (int8 numerators over a power of two, so that they
    are exact in fp32, bf16 and fp16 and compress) - ``<case>_feat<i>_q`` / ``w_<key>_q`` with ``*_scale``;
  * ``meta``: JSON with the state-dict key -> shape table, the cases, the sampling step;
  * per case: ``mask_feature``; the three ``multi_scale_features`` (case 'odd' differs from 'base' only in its stride-4
    map, which the encoder never sees: its three maps are the base case's and stored once); the query position term and
    the reference points the encoder received (batch-independent: image 0); every ``STEP``-th element (flat order) of the
    four input gradients together with a digest of the whole gradient; digests of every parameter gradient (a digest:
    sum, cosine-weighted sum, largest magnitude, sum of magnitudes).
The loss is sum(out * gout) over mask_feature and the three maps with seeded gouts, stored the same way as the inputs.
"""
import importlib
import json
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn as nn

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import gen_golden as gg                                   # noqa: E402
from oracle import msda as oracle_msda                    # noqa: E402

REF = os.path.join(gg.REF, 'segmentation', 'mmseg_custom')
E, HEADS, LAYERS, GROUPS, OUT = 64, 2, 2, 32, 8
STEP = 23                                                 # sampling step of the stored input gradients
CASES = {'base': ((32, 48), (16, 24), (8, 12), (4, 6)), 'odd': ((33, 49), (16, 24), (8, 12), (4, 6))}
BATCH = 2


def grid(key, shape, sigma, denom):
    """seeded normal values on the grid k / denom (|k| <= 127): int8 numerators and the scale"""
    g = torch.Generator(device='cpu').manual_seed(zlib.crc32(key.encode()) % (2 ** 31 - 1))
    q = (torch.randn(tuple(shape), generator=g) * sigma * denom).round().clamp_(-127, 127).to(torch.int8)
    return q.numpy(), 1.0 / denom


def digest(t):
    """[sum, cosine-weighted sum, largest magnitude, sum of magnitudes]: the last two scale the bounds a test may hold
    the sums to"""
    a = t.detach().to(torch.float64).flatten().numpy()
    return np.array([a.sum(), (a * np.cos(np.arange(a.size, dtype=np.float64) * 0.61803398875)).sum(), np.abs(a).max(), np.abs(a).sum()],
                    dtype=np.float64)


class AttrDict(dict):
    __getattr__ = dict.__getitem__


def _attr(d):
    return AttrDict({k: _attr(v) if isinstance(v, dict) else v for k, v in d.items()})


class ConvModule(nn.Module):
    def __init__(self, cin, cout, kernel_size, stride=1, padding=0, bias=True, norm_cfg=None, act_cfg=None):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=padding, bias=bias)
        self.gn = nn.GroupNorm(norm_cfg['num_groups'], cout) if norm_cfg is not None else None
        self.relu = act_cfg is not None

    def forward(self, x):
        x = self.conv(x)
        if self.gn is not None:
            x = self.gn(x)
        return torch.relu(x) if self.relu else x


class Attention(nn.Module):                     # mmcv's parameter names
    def __init__(self, embed_dims, num_heads, num_levels, num_points, **_):
        super().__init__()
        self.num_heads, self.num_levels, self.num_points = num_heads, num_levels, num_points
        self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = nn.Linear(embed_dims, num_heads * num_levels * num_points)
        self.value_proj = nn.Linear(embed_dims, embed_dims)
        self.output_proj = nn.Linear(embed_dims, embed_dims)

    def init_weights(self):
        pass


class FFN(nn.Module):
    def __init__(self, e, f):
        super().__init__()
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(e, f), nn.ReLU(), nn.Dropout(0.)), nn.Linear(f, e), nn.Dropout(0.))


class Layer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        a = cfg.attn_cfgs
        self.attentions = nn.ModuleList([Attention(**{k: v for k, v in a.items() if k != 'type'})])
        self.ffns = nn.ModuleList([FFN(a.embed_dims, cfg.ffn_cfgs.feedforward_channels)])
        self.norms = nn.ModuleList([nn.LayerNorm(a.embed_dims), nn.LayerNorm(a.embed_dims)])


class Encoder(nn.Module):
    """post-norm layers (attention with its own identity, norm, FFN with identity, norm) on the MSDA oracle"""

    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([Layer(cfg.transformerlayers) for _ in range(cfg.num_layers)])
        self.seen = {}

    def forward(self, query, query_pos, spatial_shapes, reference_points, query_key_padding_mask=None, **kwargs):
        assert query_key_padding_mask is None or not bool(query_key_padding_mask.any())
        assert bool((kwargs['valid_radios'] == 1).all())
        self.seen = dict(query_pos=query_pos.detach(), reference_points=reference_points.detach())
        ss, ref, pos = spatial_shapes, reference_points, query_pos
        shapes = [tuple(x) for x in ss.tolist()]
        for layer in self.layers:
            a = layer.attentions[0]
            M, L, P = a.num_heads, a.num_levels, a.num_points
            q = (query + pos).permute(1, 0, 2)
            v = query.permute(1, 0, 2)
            N, Lq, C = q.shape
            value = a.value_proj(v).view(N, -1, M, C // M)
            off = a.sampling_offsets(q).view(N, Lq, M, L, P, 2)
            w = a.attention_weights(q).view(N, Lq, M, L * P).softmax(-1).view(N, Lq, M, L, P)
            norm = torch.stack([ss[..., 1], ss[..., 0]], -1).to(q.dtype)
            loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
            out = oracle_msda.core_torch(value, shapes, loc, w)
            x = layer.norms[0](a.output_proj(out).permute(1, 0, 2) + query)
            query = layer.norms[1](x + layer.ffns[0].layers(x))
        return query


class Registry:
    def __init__(self, *a, **k):
        pass

    def register_module(self, *a, **k):
        return lambda cls: cls


class BaseModule(nn.Module):
    def __init__(self, init_cfg=None):
        super().__init__()


def load_reference():
    pe = {}

    def build_positional_encoding(cfg):
        return pe['cls'](**{k: v for k, v in cfg.items() if k != 'type'})
    nothing = lambda *a, **k: None                                         # noqa: E731
    gg._mod('mmcv'), gg._mod('mmcv.cnn.bricks')
    gg._mod('mmcv.cnn', PLUGIN_LAYERS=Registry(), Conv2d=nn.Conv2d, ConvModule=ConvModule, caffe2_xavier_init=nothing,
            normal_init=nothing, xavier_init=nothing)
    gg._mod('mmcv.cnn.bricks.transformer', POSITIONAL_ENCODING=Registry(), build_positional_encoding=build_positional_encoding,
            build_transformer_layer_sequence=lambda cfg: Encoder(cfg))
    gg._mod('mmcv.runner', BaseModule=BaseModule, ModuleList=nn.ModuleList)
    gg._mod('mmcv.utils', Registry=Registry, build_from_cfg=nothing)
    for name, sub in (('ref_pd', ''), ('ref_pd.core', 'core'), ('ref_pd.core.anchor', 'core/anchor'), ('ref_pd.models', 'models'),
                      ('ref_pd.models.plugins', 'models/plugins'), ('ref_pd.models.utils', 'models/utils')):
        gg._mod(name).__path__ = [os.path.join(REF, sub)]
    gg._mod('ref_pd.models.utils.transformer', MultiScaleDeformableAttention=Attention)
    pe['cls'] = importlib.import_module('ref_pd.models.utils.positional_encoding').SinePositionalEncoding
    sys.modules['ref_pd.core.anchor'].MlvlPointGenerator = importlib.import_module('ref_pd.core.anchor.point_generator').MlvlPointGenerator
    return importlib.import_module('ref_pd.models.plugins.msdeformattn_pixel_decoder').MSDeformAttnPixelDecoder


def config():
    return dict(
        in_channels=[E] * 4, strides=[4, 8, 16, 32], feat_channels=E, out_channels=OUT, num_outs=3,
        norm_cfg=dict(type='GN', num_groups=GROUPS), act_cfg=dict(type='ReLU'),
        encoder=dict(type='DetrTransformerEncoder', num_layers=LAYERS, transformerlayers=dict(
            type='BaseTransformerLayer', attn_cfgs=dict(type='MultiScaleDeformableAttention', embed_dims=E, num_heads=HEADS,
                                                        num_levels=3, num_points=4, im2col_step=64, dropout=0.0,
                                                        batch_first=False, norm_cfg=None, init_cfg=None),
            ffn_cfgs=dict(type='FFN', embed_dims=E, feedforward_channels=4 * E, num_fcs=2, ffn_drop=0.0, act_cfg=dict(type='ReLU', inplace=True)),
            operation_order=('self_attn', 'norm', 'ffn', 'norm')), init_cfg=None),
        positional_encoding=dict(type='SinePositionalEncoding', num_feats=E // 2, normalize=True), init_cfg=None)


def seeded_weight(key, shape):
    """-> (int8 numerators, scale).  Matrices ~ N(0, 1 / fan_in) (offsets half of that), norm scales around 1, biases
    small, offset biases in pixels: non-zero offsets and logits, as in the existing tests."""
    leaf = key.rsplit('.', 1)[-1]
    if leaf == 'bias':
        return grid(key, shape, 1.5, 16) if 'sampling_offsets' in key else grid(key, shape, 0.06, 256)
    if len(shape) == 1:                                   # GroupNorm / LayerNorm scale: 1 + N(0, 0.1), stored as the deviation
        return grid(key, shape, 0.1, 128)
    if key == 'level_encoding.weight':
        return grid(key, shape, 0.25, 64)
    fan_in = int(np.prod(shape[1:]))
    denom = 2 ** int(np.ceil(np.log2(16 * np.sqrt(fan_in))))
    return grid(key, shape, (0.5 if 'sampling_offsets' in key else 1.0) / np.sqrt(fan_in), denom)


def weight_value(key, q, scale):
    v = torch.from_numpy(q.astype(np.float32)) * scale
    return 1.0 + v if (v.dim() == 1 and not key.endswith('bias')) else v


def main():
    cls = load_reference()
    cfg = config()
    model = cls(**dict(cfg, encoder=_attr(cfg['encoder'])))
    g = {}
    meta = {'state_dict': {k: list(v.shape) for k, v in model.state_dict().items()}, 'cases': {k: [list(s) for s in v] for k, v in CASES.items()},
            'batch': BATCH, 'step': STEP, 'config': cfg}
    sd = {}
    for k, shape in meta['state_dict'].items():
        q, scale = seeded_weight(k, shape)
        g['w_' + k + '_q'], g['w_' + k + '_scale'] = q, np.float64(scale)
        sd[k] = weight_value(k, q, scale)
    model.load_state_dict(sd)
    shared = {}
    for name, sizes in CASES.items():
        model.zero_grad(set_to_none=True)
        feats = []
        for i, (h, w) in enumerate(sizes):
            key = 'feat%d_%dx%d' % (i, h, w)
            if key not in shared:
                shared[key] = grid(key, (BATCH, E, h, w), 1.0, 2)
            q, scale = shared[key]
            if i == 0 or name == 'base':
                g['%s_feat%d_q' % (name, i)], g['%s_feat%d_scale' % (name, i)] = q, np.float64(scale)
            feats.append((torch.from_numpy(q.astype(np.float32)) * scale).requires_grad_(True))
        mask_feature, ms = model(feats)
        outs = [mask_feature] + list(ms)
        gouts = []
        for j, o in enumerate(outs):
            key = 'gout%d_%s' % (j, 'x'.join(map(str, o.shape)))
            if key not in shared:
                shared[key] = grid(key, o.shape, 1.0, 2)
            q, scale = shared[key]
            if j == 0 or name == 'base':
                g['%s_gout%d_q' % (name, j)], g['%s_gout%d_scale' % (name, j)] = q, np.float64(scale)
            gouts.append(torch.from_numpy(q.astype(np.float32)) * scale)
        params = list(model.named_parameters())
        grads = torch.autograd.grad(sum((o * go).sum() for o, go in zip(outs, gouts)), feats + [p for _, p in params])
        g[name + '_mask_feature'] = mask_feature.detach().numpy()
        if name == 'base':
            for j, o in enumerate(ms):
                g['base_ms%d' % j] = o.detach().numpy()
            seen = model.encoder.seen
            assert all(bool((seen[k][i] == seen[k][0]).all()) for k in ('reference_points',) for i in range(BATCH))
            assert bool((seen['query_pos'] == seen['query_pos'][:, :1]).all())
            g['query_pos'] = seen['query_pos'][:, 0].numpy()                 # (Lq, C)
            g['reference_points'] = seen['reference_points'][0].numpy()      # (Lq, L, 2)
        else:
            assert all(np.array_equal(o.detach().numpy(), g['base_ms%d' % j]) for j, o in enumerate(ms))
        for i in range(4):
            g['%s_gfeat%d_sample' % (name, i)] = grads[i].flatten()[::STEP].numpy()
            g['%s_gfeat%d_digest' % (name, i)] = digest(grads[i])
        for (pn, _), gr in zip(params, grads[4:]):
            g['%s_gp_%s' % (name, pn)] = digest(gr)
    g['meta'] = np.array(json.dumps(meta))
    dst = os.path.join(ROOT, 'tests', 'golden', 'pixel_decoder.npz')
    np.savez_compressed(dst, **g)
    print(dst, os.path.getsize(dst), 'bytes,', len(g), 'arrays')


if __name__ == '__main__':
    main()
