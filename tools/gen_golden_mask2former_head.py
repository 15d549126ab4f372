"""Mask2FormerHead golden from the reference's own class.  Container only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_mask2former_head.py

Imports /root/reference/segmentation/mmseg_custom/models/decode_heads/mask2former_head.py under in-memory stand-ins for mmcv
and mmseg, on top of the ones tools/gen_golden_pixel_decoder.py has for the pixel decoder: a ``BaseDecodeHead`` that is a
bare nn.Module, registries and loss / assigner / sampler builders that do nothing, and the query decoder restated on
nn.MultiheadAttention with mmcv's parameter names (``DetrTransformerDecoder`` of ``DetrTransformerDecoderLayer``s,
post-norm, ``operation_order=('cross_attn', 'norm', 'self_attn', 'norm', 'ffn', 'norm')``; the attention wrapper adds the
position terms and its own identity).  So the mmcv layer classes are NOT pinned against mmcv (as for the encoder); the head's
own composition - decoder inputs, level embedding, position terms, ``forward_head``, the sigmoid test, the all-background
rule, the order of levels - is the reference's code.

Case: the 'base' case of tests/golden/pixel_decoder.npz (E = 64, 2 heads of 32 channels, batch 2, maps (32, 48), (16, 24),
(8, 12), (4, 6)); the feature maps and every ``pixel_decoder.*`` parameter are that file's and are not stored again.  8 queries,
3 decoder layers, 3 + 2 classes.  The head's own parameters are drawn on int8 grids as there.

Mask guard.  The reference's ``sigmoid() < 0.5`` is a sign test, which is discontinuous: the case is also run in fp64, and for
every mask a layer consumes d = the largest |fp32 - fp64| logit is recorded.  Seeds are walked in order until the smallest
|fp64 logit| of every consumed mask is at least 16 d AND some consumed row excludes every key (so that the reference's
"all background -> all False" rule is exercised).  ``meta`` holds the seed, d and the minima per consumed mask, and names the
all-excluded rows.  The issue's wording was to scale ``mask_embed``'s last bias until a row keeps no key; that bias is per
channel, not per query, so the seeds are walked for such a row instead.  What this costs: at the seed found (3) the case is
far from balanced - 95 / 90 / 94 % of the logits the three layers consume are negative, a row keeps 0 to a handful of keys
(median 0.5 / 6 / 4 of 24 / 96 / 384), and 13 consumed rows keep none.  So the module tests see sparse masks and the
all-background rule often; dense and half-full masks at every chunk edge are held to fp64 at kernel level
(tests/test_masked_attn_fp64_gpu.py: 'half', 'all'), not here.

What the file holds (everything from the fp64 run, stored as fp32, unless said otherwise):
  * ``w_<key>_q`` / ``_scale`` of the head's own parameters; ``meta`` (JSON): config, state-dict key -> shape, seed, guard;
  * ``cls_pred<i>``, ``mask_pred<i>`` for i = 0 .. layers;
  * per layer ``l<i>_query`` (the query going in), ``l<i>_logits`` (the interpolated mask logits it consumes, (N, Q, h * w)),
    ``l<i>_out``, and for the loss sum(out * gout(out.shape, 100 + i)) of that layer alone ``l<i>_gquery`` and every STEP-th
    element of the gradient of its memory rows, ``l<i>_gmem_sample``, with ``l<i>_gmem_digest``;
  * for the loss sum over all predictions of sum(pred * gout(pred.shape, j)): every STEP-th element and the digest of the
    four input gradients, and the digest of every parameter gradient.
gout(shape, j) = cos(0.37 k + j) over the flat index k: not stored.
"""
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import gen_golden as gg                                   # noqa: E402
import gen_golden_pixel_decoder as gpd                    # noqa: E402

E, HEADS, QUERIES, LAYERS, THINGS, STUFF = gpd.E, gpd.HEADS, 8, 3, 3, 2
STEP = gpd.STEP
GUARD = 16.0
PD_GOLD = os.path.join(ROOT, 'tests', 'golden', 'pixel_decoder.npz')


class AttrDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


def _attr(d):
    return AttrDict({k: _attr(v) if isinstance(v, dict) else v for k, v in d.items()})


def gout(shape, j, dtype):
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.37 + j).reshape(shape).to(dtype)


class MHA(nn.Module):                           # mmcv's MultiheadAttention wrapper, batch_first=False, no dropout
    def __init__(self, embed_dims, num_heads, **_):
        super().__init__()
        self.attn = nn.MultiheadAttention(embed_dims, num_heads, dropout=0.0)

    def forward(self, query, key, value, query_pos, key_pos, attn_mask):
        out = self.attn(query + query_pos, key + key_pos, value, attn_mask=attn_mask, key_padding_mask=None, need_weights=False)[0]
        return query + out


class DecoderLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        a = cfg.attn_cfgs
        assert tuple(cfg.operation_order) == ('cross_attn', 'norm', 'self_attn', 'norm', 'ffn', 'norm')
        self.attentions = nn.ModuleList([MHA(a.embed_dims, a.num_heads), MHA(a.embed_dims, a.num_heads)])
        self.ffns = nn.ModuleList([gpd.FFN(a.embed_dims, cfg.ffn_cfgs.feedforward_channels)])
        self.norms = nn.ModuleList([nn.LayerNorm(a.embed_dims) for _ in range(3)])
        self.seen = None

    def forward(self, query, key, value, query_pos, key_pos, attn_masks, query_key_padding_mask=None, key_padding_mask=None):
        assert query_key_padding_mask is None and key_padding_mask is None and attn_masks[1] is None
        self.seen = dict(query=query.detach(), key=key.detach(), key_pos=key_pos.detach(), query_pos=query_pos.detach())
        query = self.norms[0](self.attentions[0](query, key, value, query_pos, key_pos, attn_masks[0]))
        query = self.norms[1](self.attentions[1](query, query, query, query_pos, query_pos, None))
        return self.norms[2](query + self.ffns[0].layers(query))


class Decoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([DecoderLayer(cfg.transformerlayers) for _ in range(cfg.num_layers)])
        self.embed_dims = cfg.transformerlayers.attn_cfgs.embed_dims
        self.post_norm = nn.LayerNorm(self.embed_dims)


class BaseDecodeHead(nn.Module):
    def __init__(self, in_channels, channels, num_classes, init_cfg=None, input_transform=None, **kwargs):
        super().__init__()


class FProxy:
    """torch.nn.functional for the head's module, recording what F.interpolate returns: the mask logits"""

    def __init__(self):
        self.logits = []

    def __getattr__(self, name):
        return getattr(F, name)

    def interpolate(self, *a, **k):
        out = F.interpolate(*a, **k)
        self.logits.append(out.detach().flatten(2))
        return out


def load_reference():
    pixel_decoder = gpd.load_reference()
    nothing = lambda *a, **k: None                                         # noqa: E731
    tr = sys.modules['mmcv.cnn.bricks.transformer']
    tr.build_transformer_layer_sequence = lambda cfg: (Decoder if cfg.type == 'DetrTransformerDecoder' else gpd.Encoder)(cfg)

    def build_plugin_layer(cfg):
        cfg = dict(cfg)
        assert cfg.pop('type') == 'MSDeformAttnPixelDecoder'
        return 'pixel_decoder', pixel_decoder(**cfg)
    sys.modules['mmcv.cnn'].build_plugin_layer = build_plugin_layer
    gg._mod('mmcv.ops', point_sample=nothing)
    sys.modules['mmcv.runner'].force_fp32 = lambda *a, **k: (lambda f: f)
    gg._mod('mmseg'), gg._mod('mmseg.models'), gg._mod('mmseg.models.decode_heads')
    gg._mod('mmseg.models.builder', HEADS=gpd.Registry(), build_loss=nothing)
    gg._mod('mmseg.models.decode_heads.decode_head', BaseDecodeHead=BaseDecodeHead)
    core = sys.modules['ref_pd.core']
    core.build_sampler, core.multi_apply, core.reduce_mean = nothing, nothing, nothing
    gg._mod('ref_pd.models.builder', build_assigner=nothing)
    sys.modules['ref_pd.models.utils'].get_uncertain_point_coords_with_randomness = nothing
    gg._mod('ref_pd.models.decode_heads').__path__ = [os.path.join(gpd.REF, 'models', 'decode_heads')]
    mod = importlib.import_module('ref_pd.models.decode_heads.mask2former_head')
    mod.F = FProxy()
    return mod


def config(pd_cfg):
    pd = dict(pd_cfg, type='MSDeformAttnPixelDecoder')
    for k in ('in_channels', 'feat_channels', 'out_channels'):
        pd.pop(k)
    return dict(
        in_channels=[E] * 4, feat_channels=E, out_channels=gpd.OUT, num_things_classes=THINGS, num_stuff_classes=STUFF,
        num_queries=QUERIES, num_transformer_feat_level=3, pixel_decoder=pd, enforce_decoder_input_project=False,
        positional_encoding=dict(type='SinePositionalEncoding', num_feats=E // 2, normalize=True),
        transformer_decoder=dict(type='DetrTransformerDecoder', return_intermediate=True, num_layers=LAYERS, transformerlayers=dict(
            type='DetrTransformerDecoderLayer',
            attn_cfgs=dict(type='MultiheadAttention', embed_dims=E, num_heads=HEADS, attn_drop=0.0, proj_drop=0.0, dropout_layer=None,
                           batch_first=False),
            ffn_cfgs=dict(embed_dims=E, feedforward_channels=4 * E, num_fcs=2, act_cfg=dict(type='ReLU', inplace=True), ffn_drop=0.0,
                          dropout_layer=None, add_identity=True),
            feedforward_channels=4 * E, operation_order=('cross_attn', 'norm', 'self_attn', 'norm', 'ffn', 'norm')), init_cfg=None),
        loss_cls=dict(type='CrossEntropyLoss', class_weight=[1.0] * (THINGS + STUFF) + [0.1]), loss_mask=None, loss_dice=None,
        train_cfg=None, test_cfg=None, init_cfg=None)


def seeded_weight(key, shape, seed):
    """the head's own parameters: embeddings ~ N(0, 1) on a grid of 1/32, the rest as the pixel decoder's"""
    if key in ('query_embed.weight', 'query_feat.weight'):
        return gpd.grid('%s#%d' % (key, seed), shape, 1.0, 32)
    if key == 'level_embed.weight':
        return gpd.grid('%s#%d' % (key, seed), shape, 0.25, 64)
    skey = '%s#%d' % (key, seed)
    if key.endswith('bias'):
        return gpd.grid(skey, shape, 0.06, 256)
    if len(shape) == 1:                                   # LayerNorm scale: 1 + N(0, 0.1), stored as the deviation
        return gpd.grid(skey, shape, 0.1, 128)
    fan_in = int(np.prod(shape[1:]))
    return gpd.grid(skey, shape, 1.0 / np.sqrt(fan_in), 2 ** int(np.ceil(np.log2(16 * np.sqrt(fan_in)))))


def build(mod, cfg, pdg, seed, dtype):
    c = dict(cfg, pixel_decoder=_attr(cfg['pixel_decoder']), transformer_decoder=_attr(cfg['transformer_decoder']),
             loss_cls=_attr(cfg['loss_cls']))
    model = mod.Mask2FormerHead(**c)
    own, sd = {}, {}
    for k, v in model.state_dict().items():
        if k.startswith('pixel_decoder.'):
            pk = k[len('pixel_decoder.'):]
            sd[k] = gpd.weight_value(pk, pdg['w_' + pk + '_q'], float(pdg['w_' + pk + '_scale']))
        else:
            q, scale = seeded_weight(k, tuple(v.shape), seed)
            own[k] = (q, scale)
            sd[k] = gpd.weight_value(k, q, scale)
    model.load_state_dict(sd)
    return model.to(dtype), own


def run(mod, model, pdg, dtype):
    feats = [(torch.from_numpy(pdg['base_feat%d_q' % i].astype(np.float64)) * float(pdg['base_feat%d_scale' % i])).to(dtype)
             .requires_grad_(True) for i in range(4)]
    mod.F.logits = []
    cls_preds, mask_preds = model(feats, [None] * gpd.BATCH)
    return feats, cls_preds, mask_preds, list(mod.F.logits)


def main():
    mod = load_reference()
    pdg = np.load(PD_GOLD)
    pd_meta = json.loads(str(pdg['meta']))
    cfg = config(pd_meta['config'])
    for seed in range(2000):
        m32, own = build(mod, cfg, pdg, seed, torch.float32)
        with torch.no_grad():
            _, _, _, lg32 = run(mod, m32, pdg, torch.float32)
        m64, _ = build(mod, cfg, pdg, seed, torch.float64)
        feats, cls_preds, mask_preds, lg64 = run(mod, m64, pdg, torch.float64)
        d = [float((a.double() - b).abs().max()) for a, b in zip(lg32[:LAYERS], lg64[:LAYERS])]
        least = [float(b.abs().min()) for b in lg64[:LAYERS]]
        empty = [[i, n, q] for i, b in enumerate(lg64[:LAYERS]) for n in range(b.shape[0]) for q in range(b.shape[1])
                 if bool((b[n, q] < 0).all())]
        ok = all(m >= GUARD * x for m, x in zip(least, d)) and all(bool(((a < 0) == (b < 0)).all()) for a, b in zip(lg32, lg64))
        print('seed %d: d %s least %s all-excluded rows %s -> %s' % (seed, d, least, empty, ok and bool(empty)), flush=True)
        if ok and empty:
            break
    else:
        raise SystemExit('no seed passes the mask guard')
    g = {}
    for k, (q, scale) in own.items():
        g['w_' + k + '_q'], g['w_' + k + '_scale'] = q, np.float64(scale)
    f32 = lambda t: t.detach().to(torch.float32).numpy()                   # noqa: E731
    for i, (c, m) in enumerate(zip(cls_preds, mask_preds)):
        g['cls_pred%d' % i], g['mask_pred%d' % i] = f32(c), f32(m)
    params = list(m64.named_parameters())
    outs = list(cls_preds) + list(mask_preds)
    loss = sum((o * gout(o.shape, j, torch.float64)).sum() for j, o in enumerate(outs))
    grads = torch.autograd.grad(loss, feats + [p for _, p in params], allow_unused=True)
    for i in range(4):
        g['gfeat%d_sample' % i] = f32(grads[i].flatten()[::STEP])
        g['gfeat%d_digest' % i] = gpd.digest(grads[i])
    for (pn, p), gr in zip(params, grads[4:]):
        g['gp_' + pn] = gpd.digest(gr if gr is not None else torch.zeros_like(p))
    for i, layer in enumerate(m64.transformer_decoder.layers):
        seen = layer.seen
        q_in, mem = seen['query'].clone().requires_grad_(True), seen['key'].clone().requires_grad_(True)
        mask = (lg64[i].unsqueeze(1).repeat(1, HEADS, 1, 1).flatten(0, 1).sigmoid() < 0.5)
        mask[torch.where(mask.sum(-1) == mask.shape[-1])] = False
        out = layer(query=q_in, key=mem, value=mem, query_pos=seen['query_pos'], key_pos=seen['key_pos'], attn_masks=[mask, None])
        gq, gm = torch.autograd.grad((out * gout(out.shape, 100 + i, torch.float64)).sum(), (q_in, mem))
        g['l%d_query' % i], g['l%d_logits' % i], g['l%d_out' % i], g['l%d_gquery' % i] = f32(q_in), f32(lg64[i]), f32(out), f32(gq)
        g['l%d_gmem_sample' % i], g['l%d_gmem_digest' % i] = f32(gm.flatten()[::STEP]), gpd.digest(gm)
    meta = {'config': cfg, 'state_dict': {k: list(v.shape) for k, v in m64.state_dict().items()}, 'seed': seed, 'guard': GUARD,
            'd': d, 'least': least, 'all_excluded_rows': empty, 'step': STEP, 'layers': LAYERS, 'pixel_decoder_case': 'base'}
    g['meta'] = np.array(json.dumps(meta))
    dst = os.path.join(ROOT, 'tests', 'golden', 'mask2former_head.npz')
    np.savez_compressed(dst, **g)
    print(dst, os.path.getsize(dst), 'bytes,', len(g), 'arrays')


if __name__ == '__main__':
    main()
