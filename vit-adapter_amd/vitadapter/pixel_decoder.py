"""The deformable encoder of Mask2Former's pixel decoder on the gfx950 MSDA kernels (SURVEY.md section 8 f-3,
BASELINE configs[4]).

The reference builds it from mmcv / mmdet registry entries (``DetrTransformerEncoder`` of 6 ``BaseTransformerLayer``s,
``operation_order=('self_attn', 'norm', 'ffn', 'norm')``, attention ``MultiScaleDeformableAttention`` 256 ch / 8 heads /
3 levels / 4 points, ``FFN`` 256 -> 1024 -> 256 with ReLU, no dropout:
/root/reference/segmentation/configs/_base_/models/mask2former_beit.py:36-60) and drives it from
``MSDeformAttnPixelDecoder.forward`` (/root/reference/segmentation/mmseg_custom/models/plugins/
msdeformattn_pixel_decoder.py:160-242): the three coarsest backbone maps, projected to 256 channels and flattened from
low to high resolution, are the queries AND the values (Lq = S); ``query_pos`` = sine position + level embedding;
reference points = pixel centres of every level, repeated over the levels and multiplied by the valid ratios of every
image: an (N, Lq, L, 2) tensor (:224-240).  At every batch size the attention of all six layers runs on the fused MSDA
kernels, which read one grid per image (csrc/msda_fused.hip); under bf16 autocast that is the one-node
pair core of vitadapter/fused.py.

mmcv and mmdet are not part of the reference tree: the layer is restated from those call sites and mmcv 1.4's published
``BaseTransformerLayer`` / ``FFN`` (post-norm: ``x = norm(attn(x) + x)``, ``x = norm(x + ffn(x))``; the attention adds its
own identity, see mmcv_attention.py).  PARITY UNPINNED against mmcv; tests hold the stack to a plain PyTorch evaluation
of the same arithmetic on this repo's MSDA oracle.  Parameter names are mmcv's (``layers.{i}.attentions.0.*``,
``layers.{i}.ffns.0.layers.0.0.weight``, ``layers.{i}.ffns.0.layers.1.weight``, ``layers.{i}.norms.{0,1}.*``).
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import fused
from .mmcv_attention import MultiScaleDeformableAttention


class FFN(nn.Module):
    """mmcv ``FFN(embed_dims, feedforward_channels, num_fcs=2, act ReLU, ffn_drop, add_identity=True)``."""

    def __init__(self, embed_dims=256, feedforward_channels=1024, ffn_drop=0.0):
        super().__init__()
        self.layers = nn.Sequential(
            nn.Sequential(nn.Linear(embed_dims, feedforward_channels), nn.ReLU(inplace=True), nn.Dropout(ffn_drop)),
            nn.Linear(feedforward_channels, embed_dims), nn.Dropout(ffn_drop))

    def forward(self, x, identity=None):
        h = fused.linear(self.layers[0][0], x)
        h = self.layers[0][2](torch.relu(h))
        h = self.layers[2](fused.linear(self.layers[1], h))
        return (x if identity is None else identity) + h


class DeformableEncoderLayer(nn.Module):
    """One ``BaseTransformerLayer`` with ``operation_order=('self_attn', 'norm', 'ffn', 'norm')``."""

    def __init__(self, embed_dims=256, num_heads=8, num_levels=3, num_points=4, feedforward_channels=1024, dropout=0.0,
                 ffn_dropout=None):
        super().__init__()
        self.attentions = nn.ModuleList([MultiScaleDeformableAttention(
            embed_dims=embed_dims, num_heads=num_heads, num_levels=num_levels, num_points=num_points, dropout=dropout,
            batch_first=False)])
        self.ffns = nn.ModuleList([FFN(embed_dims, feedforward_channels, dropout if ffn_dropout is None else ffn_dropout)])
        self.norms = nn.ModuleList([nn.LayerNorm(embed_dims), nn.LayerNorm(embed_dims)])

    def forward(self, query, query_pos=None, query_key_padding_mask=None, spatial_shapes=None, reference_points=None,
                level_start_index=None):
        query = self.attentions[0](query, query, query, identity=None, query_pos=query_pos,
                                   key_padding_mask=query_key_padding_mask, reference_points=reference_points,
                                   spatial_shapes=spatial_shapes, level_start_index=level_start_index)
        query = fused.layer_norm(self.norms[0], query)
        query = self.ffns[0](query)
        return fused.layer_norm(self.norms[1], query)


class MSDeformAttnEncoder(nn.Module):
    """``DetrTransformerEncoder(num_layers=6, transformerlayers=...)`` of the pixel decoder: (Lq, N, E) in and out."""

    def __init__(self, num_layers=6, embed_dims=256, num_heads=8, num_levels=3, num_points=4, feedforward_channels=1024,
                 dropout=0.0, ffn_dropout=None):
        super().__init__()
        self.layers = nn.ModuleList([DeformableEncoderLayer(embed_dims, num_heads, num_levels, num_points,
                                                            feedforward_channels, dropout, ffn_dropout) for _ in range(num_layers)])
        self.embed_dims = embed_dims
        self.init_weights()

    def init_weights(self):
        """msdeformattn_pixel_decoder.py:143-158: Xavier on every matrix, then the attention's own init."""
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_normal_(p)
        for layer in self.layers:
            layer.attentions[0].init_weights()

    def forward(self, query, query_pos=None, query_key_padding_mask=None, spatial_shapes=None, reference_points=None,
                level_start_index=None, **kwargs):
        with fused.forward_epoch(self):
            for layer in self.layers:
                query = layer(query, query_pos, query_key_padding_mask, spatial_shapes, reference_points, level_start_index)
        return query


def encoder_inputs(level_shapes, batch, embed_dims, device, seed=0, dtype=torch.float32):
    """Synthetic inputs of the encoder as MSDeformAttnPixelDecoder.forward builds them (:176-228): levels from low to high
    resolution, queries (Lq, N, E), query_pos (Lq, N, E), pixel-centre reference points (N, Lq, L, 2), int64 geometry."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    L = len(level_shapes)
    Lq = sum(h * w for h, w in level_shapes)
    query = torch.randn(Lq, batch, embed_dims, generator=g).to(device=device, dtype=dtype)
    pos = torch.randn(Lq, batch, embed_dims, generator=g).to(device=device, dtype=dtype)
    pts = []
    for h, w in level_shapes:
        ys = (torch.arange(h, dtype=torch.float32) + 0.5) / h
        xs = (torch.arange(w, dtype=torch.float32) + 0.5) / w
        gy, gx = torch.meshgrid(ys, xs, indexing='ij')
        pts.append(torch.stack((gx.reshape(-1), gy.reshape(-1)), -1))
    ref = torch.cat(pts, 0)[None, :, None].repeat(batch, 1, L, 1).to(device)
    shapes = torch.as_tensor(level_shapes, dtype=torch.long, device=device)
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    return query, pos, ref, shapes, lsi


class ConvModule(nn.Module):
    """mmcv ``ConvModule(cin, cout, k, padding=k // 2, bias=..., norm_cfg=dict(type='GN', num_groups=G), act_cfg=...)``:
    ``conv`` -> ``gn`` -> ReLU, with mmcv's parameter names (``conv.weight``, ``conv.bias``, ``gn.weight``, ``gn.bias``).
    mmcv is not part of the reference tree: PARITY UNPINNED against it.  The pixel decoder calls the three parts itself,
    on channels-last rows; ``forward`` is the plain NCHW expression."""

    def __init__(self, in_channels, out_channels, kernel_size, bias, num_groups, relu):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=kernel_size // 2, bias=bias)
        self.gn = nn.GroupNorm(num_groups, out_channels)
        self.with_relu = relu

    def forward(self, x):
        x = self.gn(self.conv(x))
        return torch.relu(x) if self.with_relu else x


def _get(cfg, key, default=None):
    return cfg.get(key, default) if cfg is not None else default


def _ffn_settings(layer, embed_dims):
    """(feedforward_channels, ffn_drop) of a ``transformerlayers`` config, read as mmcv's BaseTransformerLayer reads them:
    from ``ffn_cfgs`` (the reference's configs, mask2former_beit.py:52-58), with the deprecated top-level keys
    ``feedforward_channels`` / ``ffn_dropout`` (the class's own default, msdeformattn_pixel_decoder.py:63-64) taken where
    ``ffn_cfgs`` does not name the value; both forms naming different values, or an FFN this repository does not build
    (``num_fcs`` other than 2, an activation other than ReLU, no identity, another ``embed_dims``), raise ValueError."""
    ffn = _get(layer, 'ffn_cfgs') or {}
    if isinstance(ffn, (list, tuple)):
        if len(ffn) != 1:
            raise ValueError('one ffn_cfgs per layer, got %d' % len(ffn))
        ffn = ffn[0]
    if ffn.get('type', 'FFN') != 'FFN' or ffn.get('num_fcs', 2) != 2 or (ffn.get('act_cfg') or {'type': 'ReLU'}).get('type') != 'ReLU' \
            or not ffn.get('add_identity', True) or ffn.get('embed_dims', embed_dims) != embed_dims:
        raise ValueError('ffn_cfgs must describe FFN(embed_dims=%d, num_fcs=2, ReLU, add_identity), got %r' % (embed_dims, ffn))
    out = []
    for new, old, default in (('feedforward_channels', 'feedforward_channels', 1024), ('ffn_drop', 'ffn_dropout', 0.0)):
        a, b = ffn.get(new), _get(layer, old)
        if a is not None and b is not None and a != b:
            raise ValueError('ffn_cfgs.%s = %r but the deprecated %s = %r' % (new, a, old, b))
        out.append(a if a is not None else (b if b is not None else default))
    return tuple(out)


def _rows(x):
    """NCHW-shaped (N, C, H, W) -> channels-last rows (N, H * W, C); a view when x is channels-last in memory"""
    N, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(N, H * W, C)


def _maps(rows, hw):
    """rows (N, H * W, C) -> the NCHW-shaped view (N, C, H, W)"""
    N, _, C = rows.shape
    return rows.reshape(N, hw[0], hw[1], C).permute(0, 3, 1, 2)


def _conv1x1_rows(conv, rows):
    """a 1 x 1 nn.Conv2d as a matrix product on channels-last rows, with its bias: the GEMM dispatcher under 16-bit
    autocast (fused._LinearBF16, as fused.linear), F.linear otherwise"""
    w = conv.weight.view(conv.weight.shape[0], -1)
    t16 = fused.autocast_16('fp16_linear')
    if (fused.ENABLED['linear'] and rows.is_cuda and t16 is not None and w.dtype == torch.float32
            and rows.dtype in (t16, torch.float32) and w.shape[0] % 8 == 0 and w.shape[1] % 8 == 0 and rows.numel() > 0):
        return fused._LinearBF16.apply(rows, w, conv.bias, t16)
    return F.linear(rows, w, conv.bias)


def _conv3x3_rows(conv, rows, hw):
    """a 3 x 3 / padding 1 nn.Conv2d without bias on channels-last rows: vitadapter.conv on NHWC under 16-bit autocast
    (channel counts in multiples of 64), F.conv2d on the NCHW-shaped view otherwise"""
    N, _, C = rows.shape
    w = conv.weight
    if (fused.ENABLED['spm_nhwc'] and rows.is_cuda and torch.is_autocast_enabled() and fused.takes_16(rows.dtype, 'fp16_spm')
            and rows.dtype == torch.get_autocast_dtype('cuda') and conv.bias is None and C % 64 == 0 and w.shape[0] % 64 == 0
            and w.dtype == torch.float32 and rows.numel() > 0):
        from .spm_nhwc import _Conv3x3
        return _Conv3x3.apply(rows.contiguous().view(N, hw[0], hw[1], C), w, 1).view(N, hw[0] * hw[1], w.shape[0])
    return _rows(F.conv2d(_maps(rows, hw), w, conv.bias, padding=1))


def sine_rows(s, h, w, device):
    """positional_encoding.py:55-92 for an all-valid (h, w) mask, as rows: (h * w, 2 * num_feats) fp32.  ``s``: the settings
    of a SinePositionalEncoding (num_feats, temperature, normalize, scale, eps, offset)"""
    y = torch.arange(1, h + 1, dtype=torch.float32, device=device)
    x = torch.arange(1, w + 1, dtype=torch.float32, device=device)
    if s['normalize']:
        y = (y + s['offset']) / (y[-1:] + s['eps']) * s['scale']
        x = (x + s['offset']) / (x[-1:] + s['eps']) * s['scale']
    k = torch.arange(s['num_feats'], dtype=torch.float32, device=device)
    dim_t = s['temperature'] ** (2 * torch.div(k, 2, rounding_mode='floor') / s['num_feats'])

    def enc(v):                                   # (len,) -> (len, num_feats): sin on even, cos on odd channels
        p = v[:, None] / dim_t
        return torch.stack((p[:, 0::2].sin(), p[:, 1::2].cos()), dim=2).flatten(1)
    py = enc(y)[:, None, :].expand(h, w, -1)
    px = enc(x)[None, :, :].expand(h, w, -1)
    return torch.cat((py, px), dim=2).reshape(h * w, -1)


class MSDeformAttnPixelDecoder(nn.Module):
    """Mask2Former's pixel decoder (/root/reference/segmentation/mmseg_custom/models/plugins/msdeformattn_pixel_decoder.py:
    16-268): the constructor arguments, defaults, state-dict layout, ``init_weights`` and ``forward(feats) ->
    (mask_feature, multi_scale_features)`` of the reference's class; the config dicts may be plain dicts.

    ``forward`` works on channels-last rows.  The three coarsest maps go through their 1 x 1 product (with bias, on the GEMM
    dispatcher under 16-bit autocast) and a GroupNorm (csrc/group_norm.hip) that writes straight into the level's rows of
    one fp32 (Lq, N, C) query buffer, low to high resolution: no concatenation.  The position term (sine encoding of an
    all-valid mask + level embedding), the pixel-centre reference points - one (1, Lq, L, 2) grid shared by the batch,
    valid ratios being one - and the level geometry are constants of (h, w, device) and cached; the reference's all-False
    padding mask is not built.  After the encoder the stride-4 tail runs lateral 1 x 1 -> GroupNorm + bilinear upsample of
    the finest encoder level (fused.resize_bilinear_rows, summed in by the GroupNorm kernel) -> 3 x 3 conv (vitadapter.conv on
    NHWC under 16-bit autocast) -> GroupNorm + ReLU -> ``mask_feature`` as a product on the rows.  Under 16-bit autocast
    the intermediate maps are 16-bit, the query buffer and the statistics fp32; without autocast everything is fp32; on
    the CPU the torch expressions run throughout.

    With more than one tail level (more input maps than encoder levels + 1) the loop indexes ``lateral_convs[i]`` /
    ``output_convs[i]`` by the MAP's index, as the reference does (:254-264), while the lists are filled from the finest
    remaining map down: as there, that is consistent only for one tail level, which is all the reference's configs use.

    The outputs have the reference's NCHW SHAPES; their memory format is free: they are channels-last views
    (``multi_scale_features`` of the encoder's output buffer).  ``.contiguous()`` gives NCHW memory where it is needed.
    The ConvModule and the encoder class are restated (mmcv is not in the reference tree); the forward composition, the
    sine term, the points, the level order and the tail are pinned by tests/golden/pixel_decoder.npz."""

    def __init__(self, in_channels=(256, 512, 1024, 2048), strides=(4, 8, 16, 32), feat_channels=256, out_channels=256,
                 num_outs=3, norm_cfg=dict(type='GN', num_groups=32), act_cfg=dict(type='ReLU'), encoder=None,
                 positional_encoding=dict(type='SinePositionalEncoding', num_feats=128, normalize=True), init_cfg=None):
        super().__init__()
        if norm_cfg is None or norm_cfg.get('type') != 'GN' or 'num_groups' not in norm_cfg:
            raise ValueError("norm_cfg must be dict(type='GN', num_groups=...), got %r" % (norm_cfg,))
        if positional_encoding is None or positional_encoding.get('type') != 'SinePositionalEncoding':
            raise ValueError("positional_encoding must be a SinePositionalEncoding config, got %r" % (positional_encoding,))
        if act_cfg is not None and act_cfg.get('type') != 'ReLU':
            raise ValueError("act_cfg must be None or dict(type='ReLU'), got %r" % (act_cfg,))
        encoder = encoder or {}
        layer = _get(encoder, 'transformerlayers') or {}
        attn = _get(layer, 'attn_cfgs') or {}
        if isinstance(attn, (list, tuple)):
            attn = attn[0]
        embed_dims = _get(attn, 'embed_dims', 256)
        if embed_dims != feat_channels:
            raise ValueError('the attention\'s embed_dims (%d) must equal feat_channels (%d)' % (embed_dims, feat_channels))
        if 2 * positional_encoding.get('num_feats', 128) != feat_channels:
            raise ValueError('positional_encoding.num_feats must be feat_channels / 2')
        ffn_width, ffn_drop = _ffn_settings(layer, embed_dims)
        order = _get(layer, 'operation_order')
        if order is not None and tuple(order) != ('self_attn', 'norm', 'ffn', 'norm'):
            raise ValueError("operation_order must be ('self_attn', 'norm', 'ffn', 'norm'), got %r" % (order,))
        self.strides = list(strides)
        self.num_input_levels = len(in_channels)
        self.num_encoder_levels = _get(attn, 'num_levels', 3)
        assert self.num_encoder_levels >= 1, 'num_levels in attn_cfgs must be at least one'
        G = norm_cfg['num_groups']
        self.input_convs = nn.ModuleList(
            ConvModule(in_channels[i], feat_channels, 1, True, G, False)
            for i in range(self.num_input_levels - 1, self.num_input_levels - self.num_encoder_levels - 1, -1))
        self.encoder = MSDeformAttnEncoder(
            num_layers=_get(encoder, 'num_layers', 6), embed_dims=embed_dims, num_heads=_get(attn, 'num_heads', 8),
            num_levels=self.num_encoder_levels, num_points=_get(attn, 'num_points', 4),
            feedforward_channels=ffn_width, dropout=_get(attn, 'dropout', 0.0), ffn_dropout=ffn_drop)
        pe = positional_encoding
        self.sine = dict(num_feats=pe.get('num_feats', 128), temperature=pe.get('temperature', 10000),
                         normalize=pe.get('normalize', False), scale=pe.get('scale', 2 * math.pi), eps=pe.get('eps', 1e-6),
                         offset=pe.get('offset', 0.))
        self.level_encoding = nn.Embedding(self.num_encoder_levels, feat_channels)
        self.lateral_convs = nn.ModuleList()
        self.output_convs = nn.ModuleList()
        self.use_bias = False                         # norm_cfg is never None here
        for i in range(self.num_input_levels - self.num_encoder_levels - 1, -1, -1):
            self.lateral_convs.append(ConvModule(in_channels[i], feat_channels, 1, False, G, False))
            self.output_convs.append(ConvModule(feat_channels, feat_channels, 3, False, G, act_cfg is not None))
        self.mask_feature = nn.Conv2d(feat_channels, out_channels, kernel_size=1, stride=1, padding=0)
        self.num_outs = num_outs
        self.point_offset = 0.5                       # MlvlPointGenerator's default
        self._geometry = {}

    def init_weights(self):
        """:134-158, with mmcv's xavier_init (uniform, gain 1), caffe2_xavier_init (Kaiming uniform, a = 1, fan_in,
        leaky_relu) and normal_init restated; the attention's own init runs last."""
        for m in self.input_convs:
            nn.init.xavier_uniform_(m.conv.weight, gain=1)
            nn.init.constant_(m.conv.bias, 0)
        for conv in [m.conv for m in self.lateral_convs] + [m.conv for m in self.output_convs] + [self.mask_feature]:
            nn.init.kaiming_uniform_(conv.weight, a=1, mode='fan_in', nonlinearity='leaky_relu')
            if conv.bias is not None:
                nn.init.constant_(conv.bias, 0)
        nn.init.normal_(self.level_encoding.weight, 0, 1)
        self.encoder.init_weights()

    def _sine(self, h, w, device):
        return sine_rows(self.sine, h, w, device)

    def _constants(self, shapes, device):
        """per geometry: spatial_shapes, level_start_index, the (1, Lq, L, 2) reference grid, the sine rows (Lq, C)"""
        key = (tuple(shapes), str(device))
        c = self._geometry.get(key)
        if c is None:
            if len(self._geometry) > 16:
                self._geometry.clear()
            L = self.num_encoder_levels
            ss = torch.as_tensor(shapes, dtype=torch.long, device=device)
            lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
            pts, sine = [], []
            for i, (h, w) in enumerate(shapes):
                stride = self.strides[self.num_input_levels - i - 1]
                xs = (torch.arange(0, w, device=device) + self.point_offset) * stride
                ys = (torch.arange(0, h, device=device) + self.point_offset) * stride
                xx = xs.to(torch.float32).repeat(h)
                yy = ys.to(torch.float32).view(-1, 1).repeat(1, w).view(-1)
                factor = torch.tensor([[w, h]], dtype=torch.float32, device=device) * stride
                pts.append(torch.stack([xx, yy], dim=-1) / factor)
                sine.append(self._sine(h, w, device))
            ref = torch.cat(pts, 0)[None, :, None].repeat(1, 1, L, 1)
            c = self._geometry[key] = (ss, lsi, ref, torch.cat(sine, 0))
        return c

    def encoder_inputs(self, feats):
        """-> query (Lq, N, C) fp32, query_pos (Lq, N, C) (a broadcast view), reference_points (1, Lq, L, 2),
        spatial_shapes, level_start_index, [(h, w)] - what ``forward`` hands to the encoder"""
        N = feats[0].shape[0]
        L = self.num_encoder_levels
        levels = [feats[self.num_input_levels - i - 1] for i in range(L)]
        shapes = [tuple(f.shape[-2:]) for f in levels]
        ss, lsi, ref, sine = self._constants(shapes, feats[0].device)
        C = self.level_encoding.weight.shape[1]
        Lq = sum(h * w for h, w in shapes)
        query = torch.empty((Lq, N, C), dtype=torch.float32, device=feats[0].device)
        start = 0
        for m, f, (h, w) in zip(self.input_convs, levels, shapes):
            proj = _conv1x1_rows(m.conv, _rows(f))
            fused.group_norm(m.gn, proj, out=query[start:start + h * w].permute(1, 0, 2))
            start += h * w
        level = torch.cat([self.level_encoding.weight[i].expand(h * w, C) for i, (h, w) in enumerate(shapes)], 0)
        pos = (sine + level)[:, None, :].expand(Lq, N, C)
        return query, pos, ref, ss, lsi, shapes

    def forward(self, feats):
        N = feats[0].shape[0]
        query, pos, ref, ss, lsi, shapes = self.encoder_inputs(feats)
        memory = self.encoder(query=query, key=None, value=None, query_pos=pos, query_key_padding_mask=None,
                              spatial_shapes=ss, reference_points=ref, level_start_index=lsi)
        outs, start = [], 0
        for h, w in shapes:                             # (h * w, N, C) rows of the buffer -> NCHW-shaped views
            top, top_hw = memory[start:start + h * w].permute(1, 0, 2), (h, w)      # the same rows as (N, h * w, C), in place
            outs.append(memory[start:start + h * w].permute(1, 2, 0).reshape(N, -1, h, w))
            start += h * w
        t16 = fused.autocast_16('fp16_rows') if feats[0].is_cuda else None
        rows = None
        for i in range(self.num_input_levels - self.num_encoder_levels - 1, -1, -1):
            x = feats[i]
            hw = tuple(x.shape[-2:])
            lat = _conv1x1_rows(self.lateral_convs[i].conv, _rows(x))
            # the finest map so far, resized to this level: 16-bit rows straight from the encoder's buffer
            up = fused.resize_bilinear_rows(top, top_hw, hw, align_corners=False, out_dtype=t16 or torch.float32)
            rows = fused.group_norm(self.lateral_convs[i].gn, lat, add=up, out_dtype=t16)
            rows = _conv3x3_rows(self.output_convs[i].conv, rows, hw)
            rows = fused.group_norm(self.output_convs[i].gn, rows, relu=self.output_convs[i].with_relu, out_dtype=t16)
            top, top_hw = rows, hw
            outs.append(_maps(rows, hw))
        last = rows if rows is not None else _rows(outs[-1])
        hw = tuple(outs[-1].shape[-2:])
        return _maps(_conv1x1_rows(self.mask_feature, last), hw), outs[:self.num_outs]


def register_pixel_decoder(registry=None, force=True):
    """Register under the reference's name so ``pixel_decoder=dict(type='MSDeformAttnPixelDecoder', ...)`` of its configs
    (configs/_base_/models/mask2former_beit.py) builds this class.  ``registry`` defaults to mmcv's PLUGIN_LAYERS."""
    if registry is None:
        from mmcv.cnn import PLUGIN_LAYERS as registry
    registry.register_module(name='MSDeformAttnPixelDecoder', force=force, module=MSDeformAttnPixelDecoder)
    return MSDeformAttnPixelDecoder
