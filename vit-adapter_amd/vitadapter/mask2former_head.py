"""Mask2Former's head: pixel decoder, query decoder on the masked cross-attention kernels, class and mask heads, and the
training losses with their matching on the point-sampling kernels (BASELINE configs[4]).

The reference is /root/reference/segmentation/mmseg_custom/models/decode_heads/mask2former_head.py (constructor :57-141,
``init_weights`` :143-152, ``forward_head`` :404-444, ``forward`` :446-525) with the config
configs/_base_/models/mask2former_beit.py:20-111.  ``Mask2FormerHead`` here takes its constructor arguments and defaults,
keeps its state-dict layout, and returns what its ``forward`` returns: ``(cls_pred_list, mask_pred_list)``.  ``loss``
(:154-402), ``forward_train`` and ``forward_test`` (:527-579) are the reference's too: signatures, dict keys and arithmetic.
mmseg's builders are not here, so the losses, the assigner and the sampler are restated from their config dicts (which stay
attributes: ``loss_*``, ``train_cfg``, ``test_cfg``): CrossEntropyLoss (softmax, class weights) for the classes,
CrossEntropyLoss(use_sigmoid=True) and DiceLoss(naive_dice=True) on sampled points for the masks, MaskHungarianAssigner with
ClassificationCost / CrossEntropyLossCost / DiceCost(pred_act=True) and MaskPseudoSampler.  Anything else is a ValueError.

The query decoder is mmcv's ``DetrTransformerDecoder`` of ``DetrTransformerDecoderLayer``s with
``operation_order=('cross_attn', 'norm', 'self_attn', 'norm', 'ffn', 'norm')`` around ``MultiheadAttention`` (a wrapper of
nn.MultiheadAttention that adds the position terms and its own identity) and ``FFN``.  mmcv is not part of the reference tree:
those layer classes are restated from mmcv 1.4's published code with its parameter names, PARITY UNPINNED against mmcv; the
head's own composition is pinned by tests/golden/mask2former_head.npz, which is computed by the reference's class.

Differences from the reference's expression, none in the arithmetic it defines:
  * the decoder inputs are the level rows of the pixel decoder's (Lq, N, C) buffer, read in place, plus the level embedding;
    the key position term is the sine encoding of an all-valid mask, built once per (h, w, device) by the pixel decoder's
    ``_sine`` and shared by the batch;
  * ``forward_head`` returns the interpolated mask logits as (N, Q, h * w) in fp32 (also under autocast) instead of a
    head-repeated bool tensor; the layer hands them to ``fused.masked_cross_attention``, which excludes key j where the logit
    is < 0 and keeps every key of a row that would keep none - the reference's ``sigmoid() < 0.5`` and its
    ``attn_mask[torch.where(...)] = False``, without the copy per head and without the host synchronisation.  The sign test
    differs from torch's rounded sigmoid in a thin band below zero (include/vitadapter_hip_masked_attn.h);
  * ``loss`` makes NO host round trip for the matching on the device path, where the reference makes one per (decoder
    output, image): the matching points, sampled predictions and cost matrices of every decoder output and image are computed
    first (fused.point_sample, fused.match_costs), then fused.hungarian_match solves every problem in one launch of
    csrc/assign.hip - scipy's method, fp64 duals - and leaves the table of matched pairs on the device.  With the targets a
    fused.SegTargets, ``loss`` contains no host synchronisation at all after a first call (small constants are cached per
    device); with per-image lists the upload of the offsets remains.  On the CPU, with ENABLED['hungarian'] off or beyond the
    kernel's limits it is ONE round trip: all costs go to the host in one copy, scipy's linear_sum_assignment runs per
    (output, image), and the table goes back in one copy.  The one difference in behaviour: where the reference's assigner
    raises at once (a cost matrix with a NaN or -inf, or an infeasible one), the device path adds NaN to every loss of the step,
    on the device - a GradScaler skips such a step - and ``check_last_match()`` raises scipy's error on request.
    ``last_assignment`` keeps its meaning and type; on the device path it is built, with a copy to the host, when it is read.
    Ground-truth masks are concatenated once per step as uint8
    and sampled at their own resolution without a float copy.  Every random draw goes through ``_draw``: the ORDER of the
    draws therefore differs from the reference's (all 'match' draws come first, then per decoder output the 'oversample' and
    the 'random' draw), their distribution does not;
  * ``max(num_total_masks, 1)`` is a clamp on the device when a process group is initialised and host arithmetic
    otherwise, not a comparison that synchronises.  The sampled BCE and dice of the matched masks
    (fused.point_mask_losses) are the kernels of csrc/point_mask_loss.hip on the GPU, with an ordered backward into mask_pred:
    two backward passes of the same step give the same bits; on the CPU, or with the switch off, torch's F.grid_sample.
"""
import copy
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import fused
from .pixel_decoder import FFN, MSDeformAttnPixelDecoder, _conv1x1_rows, _ffn_settings, _get, sine_rows

ORDER = ('cross_attn', 'norm', 'self_attn', 'norm', 'ffn', 'norm')


def _linear_rows(w, b, x):
    """``F.linear(x, w, b)`` for a weight that is a parameter or a row slice of one (the three parts of ``in_proj_weight``): the
    GEMM dispatcher under 16-bit autocast (fused._LinearBF16, as fused.linear and pixel_decoder._conv1x1_rows), F.linear
    otherwise.  A slice is no leaf, so its gradient goes back through autograd into the parameter's."""
    t16 = fused.autocast_16('fp16_linear')
    if (fused.ENABLED['linear'] and x.is_cuda and t16 is not None and w.dtype == torch.float32 and x.dtype in (t16, torch.float32)
            and w.shape[0] % 8 == 0 and w.shape[1] % 8 == 0 and x.numel() > 0):
        return fused._LinearBF16.apply(x, w, b, t16)
    return F.linear(x, w, b)


class MultiheadAttention(nn.Module):
    """mmcv ``MultiheadAttention(embed_dims, num_heads, attn_drop=0, proj_drop=0, batch_first=False)``: the parameters live in
    ``attn`` (an nn.MultiheadAttention, never called), the arithmetic is written out so that the cross-attention can take
    the masked kernels.  ``forward`` returns ``identity + proj_drop(attention(query + query_pos, key + key_pos, value))``."""

    def __init__(self, embed_dims, num_heads, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        if attn_drop:
            raise ValueError('attn_drop must be 0 (the attention kernels have no dropout), got %r' % (attn_drop,))
        self.embed_dims, self.num_heads = embed_dims, num_heads
        self.attn = nn.MultiheadAttention(embed_dims, num_heads, dropout=0.0)
        self.proj_drop = nn.Dropout(proj_drop)

    def _project(self, x, part):
        E = self.embed_dims
        return _linear_rows(self.attn.in_proj_weight[part * E:(part + 1) * E], self.attn.in_proj_bias[part * E:(part + 1) * E], x)

    def forward(self, query, key, value, query_pos=None, key_pos=None, mask_logits=None):
        identity = query
        q = self._project(query if query_pos is None else query + query_pos, 0)
        k = self._project(key if key_pos is None else key + key_pos, 1)
        v = self._project(value, 2)
        Lq, N, E = q.shape
        H = self.num_heads
        if mask_logits is not None:
            out = fused.masked_cross_attention(q, k, v, mask_logits, H)
        else:
            qh, kh, vh = (t.reshape(t.shape[0], N, H, E // H).permute(1, 2, 0, 3) for t in (q, k, v))
            out = F.scaled_dot_product_attention(qh, kh, vh).permute(2, 0, 1, 3).reshape(Lq, N, E)
        return identity + self.proj_drop(_linear_rows(self.attn.out_proj.weight, self.attn.out_proj.bias, out))


class Mask2FormerDecoderLayer(nn.Module):
    """One ``DetrTransformerDecoderLayer``: masked cross-attention to one level's rows, self-attention among the queries,
    FFN; post-norm.  ``forward(query, memory_rows, query_pos, key_pos, mask_logits)``: query, query_pos (Q, N, E);
    memory_rows (Lk, N, E) - keys and values; key_pos broadcastable to it; mask_logits (N, Q, Lk) - see the module docstring."""

    def __init__(self, embed_dims=256, num_heads=8, feedforward_channels=2048, attn_drop=0.0, proj_drop=0.0, ffn_drop=0.0):
        super().__init__()
        self.attentions = nn.ModuleList([MultiheadAttention(embed_dims, num_heads, attn_drop, proj_drop) for _ in range(2)])
        self.ffns = nn.ModuleList([FFN(embed_dims, feedforward_channels, ffn_drop)])
        self.norms = nn.ModuleList([nn.LayerNorm(embed_dims) for _ in range(3)])

    def forward(self, query, memory_rows, query_pos, key_pos, mask_logits):
        query = self.attentions[0](query, memory_rows, memory_rows, query_pos, key_pos, mask_logits)
        # post-norm: a norm's output is the fp32 residual stream itself, not only a GEMM operand, so it is not rounded to the
        # autocast's type (fused.layer_norm would); torch's LayerNorm answers in fp32 under autocast
        query = self.norms[0](query)
        query = self.attentions[1](query, query, query, query_pos, query_pos)
        query = self.norms[1](query)
        query = self.ffns[0](query)
        return self.norms[2](query)


class Mask2FormerTransformerDecoder(nn.Module):
    """``DetrTransformerDecoder(num_layers, transformerlayers, return_intermediate=True)``: the layers and ``post_norm``; the
    head drives the layers one by one (mask2former_head.py:499-520)."""

    def __init__(self, num_layers, embed_dims, num_heads, feedforward_channels, attn_drop=0.0, proj_drop=0.0, ffn_drop=0.0):
        super().__init__()
        self.layers = nn.ModuleList([Mask2FormerDecoderLayer(embed_dims, num_heads, feedforward_channels, attn_drop, proj_drop,
                                                             ffn_drop) for _ in range(num_layers)])
        self.post_norm = nn.LayerNorm(embed_dims)
        self.embed_dims = embed_dims


class Mask2FormerHead(nn.Module):
    """The reference's ``Mask2FormerHead`` (see the module docstring).  ``forward(feats, img_metas=None)`` ->
    ``(cls_pred_list, mask_pred_list)``: per decoder layer (and once before the first) class logits (N, Q, classes + 1) and mask
    logits (N, Q, h, w) at the stride of ``mask_feature``, the latter in fp32.  ``decode`` is everything after the pixel
    decoder."""

    def __init__(self, in_channels, feat_channels, out_channels, num_things_classes=80, num_stuff_classes=53, num_queries=100,
                 num_transformer_feat_level=3, pixel_decoder=None, enforce_decoder_input_project=False, transformer_decoder=None,
                 positional_encoding=None, loss_cls=None, loss_mask=None, loss_dice=None, train_cfg=None, test_cfg=None,
                 init_cfg=None, **kwargs):
        super().__init__()
        self.in_channels, self.channels = in_channels, feat_channels
        self.num_things_classes, self.num_stuff_classes = num_things_classes, num_stuff_classes
        self.num_classes = num_things_classes + num_stuff_classes
        self.num_queries = num_queries
        self.num_transformer_feat_level = num_transformer_feat_level
        layer = _get(transformer_decoder, 'transformerlayers') or {}
        attn = _get(layer, 'attn_cfgs') or {}
        if isinstance(attn, (list, tuple)):
            if any(a != attn[0] for a in attn):
                raise ValueError('the two attentions of a layer must share one config')
            attn = attn[0]
        order = _get(layer, 'operation_order')
        if order is None or tuple(order) != ORDER:
            raise ValueError('operation_order must be %r, got %r' % (ORDER, order))
        if attn.get('type', 'MultiheadAttention') != 'MultiheadAttention' or attn.get('batch_first', False):
            raise ValueError('attn_cfgs must describe MultiheadAttention(batch_first=False), got %r' % (attn,))
        if positional_encoding is None or positional_encoding.get('type') != 'SinePositionalEncoding':
            raise ValueError('positional_encoding must be a SinePositionalEncoding config, got %r' % (positional_encoding,))
        embed_dims = attn.get('embed_dims', 256)
        if embed_dims != feat_channels and not enforce_decoder_input_project:
            raise ValueError('embed_dims (%d) != feat_channels (%d) needs enforce_decoder_input_project' % (embed_dims, feat_channels))
        if 2 * positional_encoding.get('num_feats', 128) != embed_dims:
            raise ValueError('positional_encoding.num_feats must be embed_dims / 2')
        ffn_width, ffn_drop = _ffn_settings(layer, embed_dims)          # ValueError for an FFN that is not (ReLU, 2 fcs, identity)
        self.num_heads = attn.get('num_heads', 8)
        self.num_transformer_decoder_layers = _get(transformer_decoder, 'num_layers', 9)
        enc_attn = _get(_get(_get(pixel_decoder, 'encoder'), 'transformerlayers'), 'attn_cfgs') or {}
        if isinstance(enc_attn, (list, tuple)):
            enc_attn = enc_attn[0]
        assert enc_attn.get('num_levels', 3) == num_transformer_feat_level
        pd = {k: v for k, v in copy.deepcopy(dict(pixel_decoder)).items() if k != 'type'}
        pd.update(in_channels=in_channels, feat_channels=feat_channels, out_channels=out_channels)
        self.pixel_decoder = MSDeformAttnPixelDecoder(**pd)
        self.transformer_decoder = Mask2FormerTransformerDecoder(
            self.num_transformer_decoder_layers, embed_dims, self.num_heads, ffn_width, attn.get('attn_drop', 0.0),
            attn.get('proj_drop', 0.0), ffn_drop)
        self.decoder_embed_dims = embed_dims
        self.decoder_input_projs = nn.ModuleList(
            nn.Conv2d(feat_channels, embed_dims, kernel_size=1) if (embed_dims != feat_channels or enforce_decoder_input_project)
            else nn.Identity() for _ in range(num_transformer_feat_level))
        pe = positional_encoding
        self.sine = dict(num_feats=pe.get('num_feats', 128), temperature=pe.get('temperature', 10000),
                         normalize=pe.get('normalize', False), scale=pe.get('scale', 2 * math.pi), eps=pe.get('eps', 1e-6),
                         offset=pe.get('offset', 0.))
        self.query_embed = nn.Embedding(num_queries, feat_channels)
        self.query_feat = nn.Embedding(num_queries, feat_channels)
        self.level_embed = nn.Embedding(num_transformer_feat_level, feat_channels)
        self.cls_embed = nn.Linear(feat_channels, self.num_classes + 1)
        self.mask_embed = nn.Sequential(nn.Linear(feat_channels, feat_channels), nn.ReLU(inplace=True),
                                        nn.Linear(feat_channels, feat_channels), nn.ReLU(inplace=True),
                                        nn.Linear(feat_channels, out_channels))
        self.conv_seg = None
        self.loss_cls, self.loss_mask, self.loss_dice = loss_cls, loss_mask, loss_dice
        self.train_cfg, self.test_cfg, self.init_cfg = train_cfg, test_cfg, init_cfg
        self.class_weight = _get(loss_cls, 'class_weight')
        self.extra_cfg = kwargs                       # BaseDecodeHead's arguments (in_index, ...): kept, not used
        self._key_pos = {}
        self._loss_settings()

    def init_weights(self):
        """:143-152, with mmcv's caffe2_xavier_init restated (Kaiming uniform, a = 1, fan_in, leaky_relu)"""
        for m in self.decoder_input_projs:
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1, mode='fan_in', nonlinearity='leaky_relu')
                nn.init.constant_(m.bias, 0)
        self.pixel_decoder.init_weights()
        for p in self.transformer_decoder.parameters():
            if p.dim() > 1:
                nn.init.xavier_normal_(p)

    def key_pos(self, h, w, device):
        """the decoder's key position term for an (h, w) level: (h * w, 1, E) fp32, cached"""
        key = (h, w, str(device))
        pos = self._key_pos.get(key)
        if pos is None:
            if len(self._key_pos) > 16:
                self._key_pos.clear()
            pos = self._key_pos[key] = sine_rows(self.sine, h, w, device)[:, None, :]     # the head's own settings
        return pos

    def forward_head(self, decoder_out, mask_feature, size):
        """decoder_out (Q, N, C), mask_feature (N, C, h, w) -> cls_pred (N, Q, classes + 1), mask_pred (N, Q, h, w) fp32 and the
        mask logits of the next cross-attention: mask_pred resized to ``size``, (N, Q, size[0] * size[1]) fp32, no gradient."""
        x = fused.layer_norm(self.transformer_decoder.post_norm, decoder_out).transpose(0, 1)
        cls_pred = self.cls_embed(x)
        m = x
        for part in self.mask_embed:
            m = fused.linear(part, m) if isinstance(part, nn.Linear) else torch.relu(m)
        N, C, h, w = mask_feature.shape
        with torch.autocast(mask_feature.device.type, enabled=False):
            mask_pred = torch.matmul(m.float(), mask_feature.float().flatten(2)).view(N, -1, h, w)
            logits = F.interpolate(mask_pred, size, mode='bilinear', align_corners=False).flatten(2).detach()
        return cls_pred, mask_pred, logits

    def decode(self, mask_feature, multi_scale_memorys):
        """everything after the pixel decoder: -> (cls_pred_list, mask_pred_list)"""
        N = mask_feature.shape[0]
        inputs, positions, sizes = [], [], []
        for i in range(self.num_transformer_feat_level):
            mem = multi_scale_memorys[i]
            h, w = mem.shape[-2:]
            rows = mem.flatten(2).permute(2, 0, 1)                # (h * w, N, C): the buffer's own rows when mem is a view of it
            proj = self.decoder_input_projs[i]
            if isinstance(proj, nn.Conv2d):
                rows = _conv1x1_rows(proj, rows).float()
            inputs.append(rows + self.level_embed.weight[i].view(1, 1, -1))
            positions.append(self.key_pos(h, w, mem.device))
            sizes.append((h, w))
        query = self.query_feat.weight.unsqueeze(1).repeat(1, N, 1)
        query_pos = self.query_embed.weight.unsqueeze(1).expand(-1, N, -1)
        cls_preds, mask_preds = [], []
        cls_pred, mask_pred, logits = self.forward_head(query, mask_feature, sizes[0])
        cls_preds.append(cls_pred)
        mask_preds.append(mask_pred)
        L = self.num_transformer_feat_level
        for i, layer in enumerate(self.transformer_decoder.layers):
            query = layer(query, inputs[i % L], query_pos, positions[i % L], logits)
            cls_pred, mask_pred, logits = self.forward_head(query, mask_feature, sizes[(i + 1) % L])
            cls_preds.append(cls_pred)
            mask_preds.append(mask_pred)
        return cls_preds, mask_preds

    def forward(self, feats, img_metas=None):
        mask_feature, multi_scale_memorys = self.pixel_decoder(feats)
        return self.decode(mask_feature, multi_scale_memorys)

    # ------------------------------------------------------------------------------------------------------------------
    # training losses (the reference's :154-402) and the two entry points of mmseg's decode heads (:527-579)
    # ------------------------------------------------------------------------------------------------------------------
    def _loss_settings(self):
        """the loss / assigner configs this repository builds, read as mmseg's builders and the classes' defaults read them;
        a config that is given and asks for anything else is a ValueError.  With ``train_cfg`` None the training settings
        stay unset and ``loss`` raises."""
        lc, lm, ld = self.loss_cls, self.loss_mask, self.loss_dice
        if lc is not None and (lc.get('type', 'CrossEntropyLoss') != 'CrossEntropyLoss' or lc.get('use_sigmoid', False)
                               or lc.get('use_mask', False) or lc.get('reduction', 'mean') != 'mean'):
            raise ValueError("loss_cls must describe CrossEntropyLoss(use_sigmoid=False, reduction='mean'), got %r" % (lc,))
        if lm is not None and (lm.get('type') != 'CrossEntropyLoss' or not lm.get('use_sigmoid', False)
                               or lm.get('reduction', 'mean') != 'mean' or lm.get('class_weight') is not None):
            raise ValueError("loss_mask must describe CrossEntropyLoss(use_sigmoid=True, reduction='mean'), got %r" % (lm,))
        if ld is not None and (ld.get('type') != 'DiceLoss' or not ld.get('use_sigmoid', True) or not ld.get('activate', True)
                               or not ld.get('naive_dice', False) or ld.get('reduction', 'mean') != 'mean'):
            raise ValueError("loss_dice must describe DiceLoss(use_sigmoid=True, activate=True, naive_dice=True, "
                             "reduction='mean'), got %r" % (ld,))
        self.cls_loss_weight = _get(lc, 'loss_weight', 1.0)
        self.mask_loss_weight = _get(lm, 'loss_weight', 1.0)
        self.dice_loss_weight, self.dice_loss_eps = _get(ld, 'loss_weight', 1.0), _get(ld, 'eps', 1e-3)
        self.num_points = self.oversample_ratio = self.importance_sample_ratio = self.match_weights = self.dice_cost_eps = None
        tc = self.train_cfg
        if not tc:
            return
        a = _get(tc, 'assigner') or {}
        cc = a.get('cls_cost', dict(type='ClassificationCost', weight=1.0))
        mc, dc = a.get('mask_cost'), a.get('dice_cost', dict(type='DiceCost', weight=1.0))
        if (a.get('type') != 'MaskHungarianAssigner' or cc.get('type') != 'ClassificationCost' or mc is None
                or mc.get('type') != 'CrossEntropyLossCost' or not mc.get('use_sigmoid', True) or dc.get('type') != 'DiceCost'
                or not dc.get('pred_act', False)):
            raise ValueError('train_cfg.assigner must describe MaskHungarianAssigner(ClassificationCost, CrossEntropyLossCost('
                             'use_sigmoid=True), DiceCost(pred_act=True)), got %r' % (a,))
        sampler = _get(tc, 'sampler') or {}
        if sampler.get('type', 'MaskPseudoSampler') != 'MaskPseudoSampler':
            raise ValueError('train_cfg.sampler must be a MaskPseudoSampler config, got %r' % (sampler,))
        self.match_weights = (cc.get('weight', 1.0), mc.get('weight', 1.0), dc.get('weight', 1.0))
        self.dice_cost_eps = dc.get('eps', 1e-3)
        self.num_points = tc.get('num_points', 12544)
        self.oversample_ratio = tc.get('oversample_ratio', 3.0)
        self.importance_sample_ratio = tc.get('importance_sample_ratio', 0.75)
        if self.oversample_ratio < 1 or not 0 <= self.importance_sample_ratio <= 1 or self.num_points < 1:
            raise ValueError('train_cfg: num_points >= 1, oversample_ratio >= 1 and 0 <= importance_sample_ratio <= 1')

    def _draw(self, kind, layer, image, shape, device):
        """Every random draw of ``loss``: ``kind`` is 'match' (the matching points of decoder output ``layer`` and image
        ``image``, :234), 'oversample' or 'random' (the two draws of get_uncertain_point_coords_with_randomness for decoder
        output ``layer``, point_sample.py:61 and :84; ``image`` is None).  Uniform on [0, 1), as the reference's torch.rand.
        Tests replace this method to replay recorded points."""
        return torch.rand(shape, device=device)

    def _constant(self, key, device, make):
        """a small device tensor that ``loss`` would otherwise upload on every call (an upload waits for the device): built
        once per (key, device) by ``make``; the key carries everything the value depends on"""
        cache = self.__dict__.setdefault('_constants', {})
        key = key + (str(device),)
        if key not in cache:
            if len(cache) > 32:
                cache.clear()
            cache[key] = make()
        return cache[key]

    @property
    def last_assignment(self):
        """[output][image] -> (queries, gts), int64 tensors on the host, queries ascending: what the last ``loss`` matched.
        Built on first read from the step's table; on the device path that read copies the table to the host and so
        synchronises - a step that never reads it never waits."""
        if self.__dict__.get('_last_assignment') is None:
            match = self.__dict__.get('_last_match')
            if match is None:
                raise AttributeError('last_assignment: no loss has run yet')
            table, _, counts, Q = match
            host = table.detach().cpu()
            sizes = [min(Q, c) for c in counts]
            firsts = [sum(counts[:n]) for n in range(len(counts))]
            assign = []
            for i in range(host.shape[0]):
                rows, tgts = host[i, 0].split(sizes), host[i, 1].split(sizes)
                assign.append([(r - n * Q, t - firsts[n]) for n, (r, t) in enumerate(zip(rows, tgts))])
            self._last_assignment = assign
        return self._last_assignment

    @last_assignment.setter
    def last_assignment(self, value):
        self._last_assignment = value

    def check_last_match(self):
        """Raise what the reference raises inside its assigner, for the last ``loss``: ValueError with scipy's message when a
        cost matrix of that step held a NaN or -inf ('matrix contains invalid numeric entries') or allowed no complete
        assignment ('cost matrix is infeasible').  Reads the step's status from the device, so it synchronises; the step itself
        does not - its losses are NaN in that case.  Silent after a clean step, and on the host path, where scipy raised
        already."""
        match = self.__dict__.get('_last_match')
        if match is None or match[1] is None:
            return
        status = match[1].cpu()
        for code, message in fused.ASSIGN_ERRORS.items():
            hit = (status == code).nonzero()
            if hit.numel():
                raise ValueError('%s (decoder output %d, image %d)' % (message, int(hit[0, 0]), int(hit[0, 1])))

    def _gt_groups(self, gt_masks_list, device):
        """the ground-truth masks as ([(masks (G, H, W) uint8, image index per mask, first global gt index)], counts): one
        group when every image's masks share a size (the usual case: one concatenation per step), else one group per image"""
        masks = [m if isinstance(m, torch.Tensor) else torch.as_tensor(m.to_ndarray() if hasattr(m, 'to_ndarray') else m)
                 for m in gt_masks_list]
        masks = [(m if m.dtype in (torch.uint8, torch.bool) else (m != 0)).to(device) for m in masks]
        masks = [m.view(torch.uint8) if m.dtype == torch.bool else m for m in masks]
        counts = [int(m.shape[0]) for m in masks]
        image_of = [torch.full((c,), n, dtype=torch.int32, device=device) for n, c in enumerate(counts)]
        if len({tuple(m.shape[1:]) for m in masks}) == 1:
            return [(torch.cat(masks, 0), torch.cat(image_of), 0)], counts
        firsts = [sum(counts[:n]) for n in range(len(counts))]
        return [(m, i, f) for m, i, f in zip(masks, image_of, firsts)], counts

    def loss(self, all_cls_scores, all_mask_preds, gt_labels_list, gt_masks_list, img_metas):
        """The reference's ``loss`` (:360-402 over ``loss_single`` :269-358 and ``_get_target_single`` :199-267):
        all_cls_scores / all_mask_preds per decoder output (N, Q, classes + 1) / (N, Q, h, w); gt_labels_list / gt_masks_list
        per image (G_n,) / (G_n, H, W), masks 0 / 1 - or a fused.SegTargets in place of the first list (the second is then
        not read): its masks, image_of, labels, counts and offsets are the single group, used as they are.  -> {'loss_cls', 'loss_mask', 'loss_dice', 'd<i>.loss_*'}: the last
        output's losses under the plain names.  No host synchronisation for the matching on the device path, one on the
        fallback (see the module docstring; ``check_last_match`` for a step whose match was invalid).  ``last_assignment``
        ([output][image] -> (queries, gts)) and ``last_points`` ([output] -> (K, P, 2) or None) keep what the step chose."""
        if self.num_points is None or None in (self.loss_cls, self.loss_mask, self.loss_dice):
            raise ValueError('loss needs train_cfg (num_points, ratios, assigner) and the loss_cls / loss_mask / loss_dice configs')
        cls = [c.float() for c in all_cls_scores]                     # force_fp32
        preds = [m.float() for m in all_mask_preds]
        L = len(cls)
        N, Q, h, w = preds[0].shape
        dev = preds[0].device
        P = self.num_points
        targets = gt_labels_list if isinstance(gt_labels_list, fused.SegTargets) else None
        if targets is not None:                                         # built on the device: the one group, as it is
            groups, counts = [(targets.masks, targets.image_of, 0)], targets.counts
            labels_all = targets.labels
        else:
            groups, counts = self._gt_groups(gt_masks_list, dev)
            labels_all = torch.cat([torch.as_tensor(lab).to(dev).long().reshape(-1) for lab in gt_labels_list])
        counts = [int(c) for c in counts]
        G_total = sum(counts)
        class_weight = None
        if self.class_weight is not None:
            class_weight = self._constant(('class_weight', tuple(float(v) for v in self.class_weight)), dev,
                                          lambda: torch.tensor([float(v) for v in self.class_weight], dtype=torch.float32, device=dev))

        # 1. matching: points, sampled predictions and costs of every decoder output, then the assignment of all of them
        K = sum(min(Q, c) for c in counts)
        status = None
        if G_total > 0:
            offsets = (targets.offsets if targets is not None
                       else torch.tensor([sum(counts[:n]) for n in range(N + 1)], dtype=torch.int32, device=dev))
            image_of_query = self._constant(('image_of_query', N, Q), dev,
                                            lambda: torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(Q))
            costs = []
            with torch.no_grad():
                for i in range(L):
                    pts = torch.cat([self._draw('match', i, n, (1, P, 2), dev) for n in range(N)], 0)
                    xs = fused.point_sample(preds[i].flatten(0, 1), pts, set_idx=image_of_query)
                    ts = torch.cat([fused.point_sample(m, pts, set_idx=image_of) for m, image_of, _ in groups if m.shape[0]], 0)
                    costs.append(fused.match_costs(xs, ts, cls[i], labels_all, counts, self.match_weights, self.dice_cost_eps,
                                                   gt_offsets=offsets))
                # (L, 2, K): query row, global gt index.  On the device path nothing comes back; else the step's one round trip
                table, status = fused.hungarian_match(costs, counts, gt_offsets=offsets)
        else:
            table = torch.zeros((L, 2, 0), dtype=torch.long, device=dev)
        self._last_match = (table, status, counts, Q)
        self._last_assignment = None
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            total = cls[0].new_tensor([float(K)]) / torch.distributed.get_world_size()
            torch.distributed.all_reduce(total)
            num_total_masks = total.clamp(min=1)[0]
        else:
            num_total_masks = max(float(K), 1.0)

        # 2. the losses of each decoder output
        self.last_points = []
        losses = []
        for i in range(L):
            rows, tgts = table[i, 0], table[i, 1]
            target = torch.full((N * Q,), self.num_classes, dtype=torch.long, device=dev)
            target[rows] = labels_all[tgts]
            ce = F.cross_entropy(cls[i].flatten(0, 1), target, weight=class_weight, reduction='none')
            avg = class_weight[target].sum() if class_weight is not None else float(N * Q)
            loss_cls = self.cls_loss_weight * (ce.sum() / avg)
            if K == 0:
                zero = preds[i].flatten(0, 1)[:0].sum()                 # :327-331
                self.last_points.append(None)
                losses.append((loss_cls, zero, zero))
                continue
            with torch.no_grad():                                       # point_sample.py:32-87
                n_over = int(P * self.oversample_ratio)
                n_unc = int(self.importance_sample_ratio * P)
                over = self._draw('oversample', i, None, (K, n_over, 2), dev)
                logits = fused.point_sample(preds[i].flatten(0, 1), over, map_idx=rows)
                idx = torch.topk(-logits.abs(), k=n_unc, dim=1)[1]
                points = torch.gather(over, 1, idx[:, :, None].expand(-1, -1, 2))
                if P - n_unc > 0:
                    points = torch.cat((points, self._draw('random', i, None, (K, P - n_unc, 2), dev)), 1)
            self.last_points.append(points)
            bce, dice = [], []
            for m, _, first in groups:
                if len(groups) == 1:
                    b, d = fused.point_mask_losses(preds[i], rows, m, tgts, points, self.dice_loss_eps)
                else:
                    # images of different mask sizes: one call per image; the boolean index synchronises
                    sel = (tgts >= first) & (tgts < first + m.shape[0])
                    if m.shape[0] == 0 or not bool(sel.any()):
                        continue
                    b, d = fused.point_mask_losses(preds[i], rows[sel], m, tgts[sel] - first, points[sel], self.dice_loss_eps)
                bce.append(b)
                dice.append(d)
            loss_mask = self.mask_loss_weight * (torch.cat(bce).sum() / (num_total_masks * P))
            loss_dice = self.dice_loss_weight * (torch.cat(dice).sum() / num_total_masks)
            losses.append((loss_cls, loss_mask, loss_dice))
        if status is not None:
            # a problem the solver could not solve (its pairs are then the identity pairing): NaN into every loss, on the
            # device, where the reference raises at once - see check_last_match
            poison = torch.where(status.ne(0).any(), float('nan'), 0.0)
            losses = [tuple(v + poison for v in three) for three in losses]
        out = dict(loss_cls=losses[-1][0], loss_mask=losses[-1][1], loss_dice=losses[-1][2])
        for i, (lc, lm, ld) in enumerate(losses[:-1]):
            out['d%d.loss_cls' % i], out['d%d.loss_mask' % i], out['d%d.loss_dice' % i] = lc, lm, ld
        return out

    def prepare_targets(self, gt_semantic_seg):
        """Start building the step's targets from the label map ((N, H, W) or (N, 1, H, W)): the reference's ToMask step
        with the head's ``ignore_index`` (255 where it has none), fused.seg_targets_begin.  -> the pending handle that
        ``forward_train`` takes as ``gt_targets``; called before the backbone, its launches and its small copy to the host
        are done when the head asks for the result."""
        ignore = getattr(self, 'ignore_index', None)
        return fused.seg_targets_begin(gt_semantic_seg, 255 if ignore is None else ignore)

    def forward_train(self, x, img_metas, gt_semantic_seg, gt_labels=None, gt_masks=None, gt_targets=None):
        """:527-555: the loss dict of a training step.  The targets come, in this order, from ``gt_labels`` / ``gt_masks``
        (per-image lists, what the reference's pipeline delivers; ``gt_semantic_seg`` is then not used, as in the reference),
        from ``gt_targets`` (a fused.SegTargets or the handle of ``prepare_targets``), or from ``gt_semantic_seg`` itself."""
        if (gt_labels is None) != (gt_masks is None):
            raise ValueError('forward_train: gt_labels and gt_masks go together')
        if gt_masks is None and gt_targets is None and gt_semantic_seg is None:
            raise ValueError('forward_train needs the targets: gt_labels and gt_masks (per-image lists), gt_targets (a SegTargets '
                             'or the handle of prepare_targets), or gt_semantic_seg (the label map to derive them from)')
        if gt_masks is None and gt_targets is None:
            gt_targets = self.prepare_targets(gt_semantic_seg)
        all_cls_scores, all_mask_preds = self(x, img_metas)
        if gt_masks is not None:
            return self.loss(all_cls_scores, all_mask_preds, gt_labels, gt_masks, img_metas)
        return self.loss(all_cls_scores, all_mask_preds, gt_targets.finish(), None, img_metas)

    def forward_test(self, inputs, img_metas, test_cfg):
        """:557-579: semantic logits (N, classes, h, w) of the last decoder output, in fp32.  The reference also reads
        ``img_metas[0]['ori_shape']`` into two names it never uses (and so raises without metas); that read is left out."""
        all_cls_scores, all_mask_preds = self(inputs, img_metas)
        return self.semantic_inference(all_cls_scores[-1], all_mask_preds[-1])

    @staticmethod
    def semantic_inference(cls_score, mask_pred):
        """``einsum('bqc,bqhw->bchw', softmax(cls_score)[..., :-1], sigmoid(mask_pred))`` as one matmul, in fp32"""
        with torch.autocast(mask_pred.device.type, enabled=False):
            N, Q, h, w = mask_pred.shape
            prob = F.softmax(cls_score.float(), dim=-1)[..., :-1]
            return torch.matmul(prob.transpose(1, 2), mask_pred.float().sigmoid().flatten(2)).view(N, -1, h, w)
