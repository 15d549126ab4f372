"""Fused memory-bound operators of the blocks (csrc/fused_ops.hip) with their autograd glue.

Each helper computes exactly what the reference's module code computes (cited at the call sites);
it takes the fused HIP path when the tensors are what bf16 autocast produces on the GPU (fp32
residual stream, bf16 branch outputs) and otherwise evaluates the same expression with torch ops
(fp32 runs, CPU host-logic tests).

The row-streaming operators - LayerNorm (plain, keep, dual), residual, residual + LayerNorm, the token
DWConv - also take fp16 autocast (the reference's AMP mode): the same kernels instantiated on fp16
(`*_f16` entry points), fp32 math, fp32 -> fp16 rounded to nearest even with overflow to inf and
subnormals kept.  So does the output tail (csrc/tail_ops.hip: the BatchNorm tail, bn_relu, halve, the token <-> plane
transposes, the NCHW max-pool and up_from_tokens, whose two products are torch's fp16 library GEMMs).

The Linear layers (linear, linear_pair with 16-bit outputs, the GELU between two Linears, forward_epoch's weight copies)
run on the tuned GEMM dispatcher (csrc/gemm.hip) under bf16 autocast and, with ENABLED['fp16_linear'], under fp16
autocast: fp16 operands, fp32 accumulation, dX an fp16 GEMM output that overflows to inf as torch's does, dW and db in
fp32 straight from the accumulators (torch rounds dW to fp16 first), the same side-stream deferral, `fin` path and bias
partials as for bf16.  conv1x1, patch embedding and the MSDA pair core stay bf16-only; under fp16 autocast they are
torch's - the deformable attention itself is not: MSDeformAttn's fp16 value / offsets / logits go to the fp16
instantiation of the fused MSDA kernels (ops/functions/ms_deform_attn_fused.py; ENABLED['fp16_msda']).

group_norm (csrc/group_norm.hip, ENABLED['group_norm']) is the GroupNorm of the pixel decoder's ConvModules on
channels-last rows: fp32 without autocast, bf16 / fp16 (fp16 under ENABLED['fp16_rows']) maps with fp32 statistics under it.
resize_bilinear_rows (csrc/resize_rows.hip, ENABLED['bilinear_rows']) is F.interpolate(mode='bilinear', size=...) on the same
rows, with a gather-form adjoint that has no atomics: the upsample of the pixel decoder's FPN tail.
masked_cross_attention (csrc/masked_attn.hip, ENABLED['masked_attn']) is the cross-attention of Mask2Former's query decoder:
the mask packed to one bit per (image, query, key) by a sign test, heads of 32 channels, bf16 or fp16 autocast.
point_sample and match_costs (csrc/point_loss.hip, ENABLED['point_loss']) are mmcv's point_sample without a gradient and the costs
of MaskHungarianAssigner of Mask2Former's training head, in fp32; point_mask_losses (csrc/point_mask_loss.hip,
ENABLED['point_mask_loss'] and ENABLED['point_loss']) is the sampled BCE / dice of the matched masks with an ordered backward into mask_pred.
seg_resize_add, seg_finish and seg_argmax (csrc/seg_logits.hip, ENABLED['seg_logits']) are the logit tail of the Mask2Former segmentor
(vitadapter/segmentor.py): window upsample-and-add, then count division, rescale, softmax, flip, view sum and argmax, fp32 NCHW.
seg_cross_entropy (csrc/seg_ce_loss.hip, ENABLED['seg_ce_loss']) is the training loss of the UperNet heads (vitadapter/heads.py):
bilinear resize to the label map, cross-entropy with an ignore index and the top-1 count, with an ordered backward into the logits.
seg_eval_update (csrc/seg_eval.hip, ENABLED['seg_eval']) is the counting pass of the mIoU evaluation (vitadapter/evaluation.py):
predicted labels and ground truth in, 3 x num_classes int64 totals added to on the device, nothing read back.
seg_targets / seg_targets_begin (csrc/seg_target.hip, ENABLED['seg_targets']) are the training targets of Mask2Former from the label
map: the reference's ToMask step (labels and binary masks per image) on the device, the counts reaching the host in one small copy.
hungarian_match (csrc/assign.hip, ENABLED['hungarian']) is the assignment step of the matching: every (decoder output, image) cost block
of a step solved exactly in one launch, the matched pairs left on the device as the table the losses index with; off, scipy on the host.
"""
import math
import os

import torch
import torch.nn.functional as F

import _vah

ENABLED = {'pair_core': True, 'layer_norm': True, 'residual': True, 'residual_ln': True, 'dwconv': True, 'linear': True, 'bn_tail': True,
           'bn_relu': True, 'bias_fold': True, 'keep_feat': True, 'maps': True, 'maps_in': True, 'linear_pair': True, 'maxpool': True, 'conv1x1': True, 'ln_dual': True, 'wgrad_fin': True, 'spm_nhwc': True, 'up_gemm': True, 'patch_gemm': True, 'wgrad_overlap': True, 'drop_pool': True,
           'fp16_rows': True, 'fp16_spm': True, 'fp16_tail': True, 'bias_partials': True,
           'fp16_linear': True,
           'fp16_msda': True,        # fp16_msda: read by ops.functions.ms_deform_attn_fused.fused_supported
           'group_norm': True,
           'bilinear_rows': True,
           'masked_attn': True,
           'point_loss': True,
           'point_mask_loss': True,   # needs point_loss as well: the sampled BCE / dice of the matched masks on kernels
           'seg_logits': True,
           'seg_ce_loss': True,
           'seg_eval': True,
           'seg_targets': True,
           'hungarian': True,         # the matching's assignment step on the device (csrc/assign.hip); off: scipy on the host
           # the per-step parameter work on kernels of its own (include/vitadapter_hip_epoch.h): one launch for all 16-bit
           # parameter copies and layouts of a forward (_EpochCopies), pair-core weight gradients stored in parameter
           # order by the reduction launch, BatchNorm bookkeeping inside the finalize launch.  Off: the torch expressions
           'epoch_copies': True}
for _k in os.environ.get('VAH_FUSED_DISABLE', '').split(','):      # e.g. VAH_FUSED_DISABLE=residual_ln,bn_tail (A/B runs)
    if _k:
        ENABLED[_k.strip()] = False


def _stream(t):
    return _vah.raw_stream(t.device)


def _scratch(K, device):
    """Partial-sum scratch for the column reductions (stream-ordered: allocated per call from
    torch's caching allocator, so concurrent streams never share it)."""
    return torch.empty(_vah.lib.vah_reduce_ws_floats(K), dtype=torch.float32, device=device)


def _bf16_autocast():
    return torch.is_autocast_enabled() and torch.get_autocast_dtype('cuda') == torch.bfloat16


def takes_16(dtype, switch):
    """Is ``dtype`` a 16-bit type that the operator family behind ``switch`` is instantiated on?  bf16 always; fp16 unless
    ENABLED[switch] is off (VAH_FUSED_DISABLE=<switch>: the torch expressions under fp16 autocast, for A/B runs).  The
    switches: 'fp16_rows' (row-streaming kernels), 'fp16_linear' (GEMM dispatcher, weight copies, GELU backward, bias
    partials), 'fp16_tail' (csrc/tail_ops.hip), 'fp16_spm' (the NHWC SpatialPriorModule)."""
    return dtype == torch.bfloat16 or (dtype == torch.float16 and ENABLED[switch])


def autocast_16(switch):
    """The 16-bit type the family behind ``switch`` runs in under the active autocast: torch.bfloat16, torch.float16, or
    None (no autocast, another autocast type, or fp16 with the switch off)."""
    if not torch.is_autocast_enabled():
        return None
    dtype = torch.get_autocast_dtype('cuda')
    return dtype if takes_16(dtype, switch) else None


def tail_dtype():
    """For the backbones: the dtype of a ``c1`` that up_from_tokens can sum in."""
    return autocast_16('fp16_tail')


_tail_dtype = tail_dtype        # the name tests/test_tail_f16_fp64_gpu.py asks by


class _LayerNormBF16(torch.autograd.Function):
    """LayerNorm of the fp32 residual stream with 16-bit output (``dtype``: bf16, or fp16 under fp16
    autocast).  With ``keep`` the stream itself is
    returned next to the normalised copy, so the gradient of the residual branch and the LayerNorm
    gradient meet in ONE backward call and are summed inside the kernel (otherwise autograd adds
    them with a separate fp32 add per LayerNorm)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, keep, dtype=torch.bfloat16):
        C = x.shape[-1]
        xc = x.contiguous()
        x2 = xc.view(-1, C)
        rows = x2.shape[0]
        y = torch.empty(x.shape, dtype=dtype, device=x.device)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        w, b = weight.contiguous(), bias.contiguous()
        with _vah.on(x.device):
            _vah.call('vah_layernorm_fwd_f32_bf16', dtype, x2.data_ptr(), w.data_ptr(), b.data_ptr(), rows, C, float(eps), y.data_ptr(),
                      mean.data_ptr(), rstd.data_ptr(), _stream(x))
        ctx.save_for_backward(x2, w, mean, rstd)
        ctx.shape, ctx.dtype = x.shape, dtype
        ctx.set_materialize_grads(False)
        if keep:
            return xc, y
        return y

    @staticmethod
    def backward(ctx, *grads):
        gres, g = grads if len(grads) == 2 else (None, grads[0])
        x2, w, mean, rstd = ctx.saved_tensors
        rows, C = x2.shape
        if g is None:                      # the normalised copy was not used
            return (gres, None, None, None, None, None)
        g = g.contiguous().to(ctx.dtype)
        if gres is not None:
            gres = gres.contiguous().float()
        dx = torch.empty_like(x2)
        dwb = torch.empty(2, C, dtype=torch.float32, device=x2.device)
        ws = _scratch(2 * C, x2.device)
        with _vah.on(x2.device):
            _vah.call('vah_layernorm_bwd_f32_bf16', ctx.dtype, x2.data_ptr(), g.data_ptr(), w.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                      gres.data_ptr() if gres is not None else None, rows, C, dx.data_ptr(), dwb[0].data_ptr(), dwb[1].data_ptr(), ws.data_ptr(),
                      _stream(x2))
        return dx.view(ctx.shape), dwb[0], dwb[1], None, None, None


def _ln_fusable(norm, x):
    return (ENABLED['layer_norm'] and x.is_cuda and x.dtype == torch.float32 and autocast_16('fp16_rows') is not None
            and isinstance(norm, torch.nn.LayerNorm) and norm.elementwise_affine
            and x.shape[-1] % 4 == 0 and x.shape[-1] <= 2048 and x.numel() > 0)


class _LayerNormDualBF16(torch.autograd.Function):
    """(x, norm_a(x), norm_b(x)) for two LayerNorms of the same fp32 tensor (equal eps): statistics
    shared, x read once; the backward sums the residual-branch gradient and both LayerNorm gradients in
    one pass."""

    @staticmethod
    def forward(ctx, x, wa, ba, wb, bb, eps, dtype=torch.bfloat16):
        C = x.shape[-1]
        xc = x.contiguous()
        x2 = xc.view(-1, C)
        rows = x2.shape[0]
        ya = torch.empty(x.shape, dtype=dtype, device=x.device)
        yb = torch.empty(x.shape, dtype=dtype, device=x.device)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        wa, ba, wb, bb = (t.contiguous() for t in (wa, ba, wb, bb))
        with _vah.on(x.device):
            _vah.call('vah_layernorm_dual_fwd', dtype, x2.data_ptr(), wa.data_ptr(), ba.data_ptr(), wb.data_ptr(), bb.data_ptr(), rows, C,
                      float(eps), ya.data_ptr(), yb.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _stream(x))
        ctx.save_for_backward(x2, wa, wb, mean, rstd)
        ctx.shape, ctx.dtype = x.shape, dtype
        ctx.set_materialize_grads(False)
        return xc, ya, yb

    @staticmethod
    def backward(ctx, gres, ga, gb):
        x2, wa, wb, mean, rstd = ctx.saved_tensors
        rows, C = x2.shape
        if ga is None and gb is None:
            return (gres, None, None, None, None, None, None)
        ga = ga.contiguous().to(ctx.dtype) if ga is not None else None
        gb = gb.contiguous().to(ctx.dtype) if gb is not None else None
        if gres is not None:
            gres = gres.contiguous().float()
        dx = torch.empty_like(x2)
        dp = torch.empty(4, C, dtype=torch.float32, device=x2.device)
        ws = _scratch(2 * C, x2.device)
        with _vah.on(x2.device):
            _vah.call('vah_layernorm_dual_bwd', ctx.dtype, x2.data_ptr(), ga.data_ptr() if ga is not None else None,
                      gb.data_ptr() if gb is not None else None, wa.data_ptr(), wb.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                      gres.data_ptr() if gres is not None else None, rows, C, dx.data_ptr(), dp.data_ptr(), ws.data_ptr(), _stream(x2))
        return dx.view(ctx.shape), dp[0], dp[1], dp[2], dp[3], None, None


def layer_norm_dual_ok(norm_a, norm_b, x):
    return (ENABLED['ln_dual'] and _ln_fusable(norm_a, x) and _ln_fusable(norm_b, x) and norm_a.eps == norm_b.eps
            and x.shape[-1] <= 1024)


def layer_norm_dual_keep(norm_a, norm_b, x):
    """``(x, norm_a(x), norm_b(x))``; use the returned x downstream (see layer_norm_keep)."""
    if layer_norm_dual_ok(norm_a, norm_b, x):
        return _LayerNormDualBF16.apply(x, norm_a.weight, norm_a.bias, norm_b.weight, norm_b.bias, norm_a.eps, autocast_16('fp16_rows'))
    x, ya = layer_norm_keep(norm_a, x, fan_out=True)
    x, yb = layer_norm_keep(norm_b, x)
    return x, ya, yb


def layer_norm(norm, x):
    """``norm(x)`` for an nn.LayerNorm; output in the autocast type (bf16 / fp16) when the consumer is a 16-bit GEMM."""
    if _ln_fusable(norm, x):
        return _LayerNormBF16.apply(x, norm.weight, norm.bias, norm.eps, False, autocast_16('fp16_rows'))
    return norm(x)


def layer_norm_keep(norm, x, fan_out=False):
    """``(x, norm(x))`` for the pattern ``x + branch(norm(x))``: use the returned ``x`` for the
    residual update so both gradients of ``x`` are summed inside the LayerNorm backward kernel.
    ``fan_out``: the kept tensor is not a residual of this sub-block but goes on to other consumers
    (switchable for A/B runs: VAH_FUSED_DISABLE=keep_feat)."""
    if fan_out and not ENABLED['keep_feat']:
        return x, layer_norm(norm, x)
    if _ln_fusable(norm, x):
        return _LayerNormBF16.apply(x, norm.weight, norm.bias, norm.eps, True, autocast_16('fp16_rows'))
    return x, norm(x)


# ---------------------------------------------------------------------------------------
# nn.Linear under bf16 / fp16 autocast
# ---------------------------------------------------------------------------------------
class _Bf16Copies:
    """16-bit (bf16, or fp16 under fp16 autocast) working copies of fp32 parameters.  autocast makes the same copies, but one tiny cast
    kernel per parameter per use (and one more per gradient on the way back).  Here a model's forward
    opens an EPOCH (``begin_forward``): ONE multi-tensor cast writes fresh copies of all its Linear
    parameters into one new flat buffer, and those copies serve every use until the forward ends
    (``forward_epoch`` is the context manager around both).  Outside an epoch every use makes its own cast.

    Nothing is keyed on ``Tensor._version``: in-place writes through ``.data`` (legacy optimizers,
    EMA / fp16 hooks, ``weight.data.normal_()``) do not bump it, and a cached copy would silently go
    stale.  Copies are never rewritten in place either, so a backward that saved one still sees the
    values of its own forward whatever ran in between.  An entry is keyed by the copy's type as well: a model run under
    bf16 and then under fp16 (or a Linear reached under another autocast type inside one forward) is never served the
    other type's copy."""

    def __init__(self):
        self.entries = {}          # (id(param), dtype) -> (weakref(param), copy, epoch)
        self.layouts = {}          # (kind, id(param), dtype) -> (weakref(param), re-laid-out copies, epoch): _EpochCopies
        self.epoch = 0             # even: no forward open; odd: the open forward's epoch

    def _hit(self, p, dtype):
        e = self.entries.get((id(p), dtype))
        if (e is not None and e[2] == self.epoch and (self.epoch & 1) and e[0]() is p and e[1].device == p.device
                and e[1].dtype == dtype):
            return e[1]
        return None

    def get(self, p, dtype=torch.bfloat16):
        c = self._hit(p, dtype)
        if c is not None:
            return c
        base = p._base             # a reshaping view of a parameter (a conv weight as a matrix): the parameter's copy, viewed alike
        if base is not None and base.numel() == p.numel() and p.is_contiguous() and p.storage_offset() == base.storage_offset():
            c = self._hit(base, dtype)
            if c is not None:
                return c.view(p.shape)
        return p.detach().to(dtype)

    def layout(self, kind, p, dtype):
        """The copy of ``p`` in the layout ``kind`` that this epoch's launch made (_EpochCopies), or None."""
        e = self.layouts.get((kind, id(p), dtype))
        if e is not None and e[2] == self.epoch and (self.epoch & 1) and e[0]() is p:
            return e[1]
        return None

    def open(self):
        self.epoch += 1 if (self.epoch & 1) == 0 else 2          # a nested / aborted forward just opens a new epoch

    def begin(self, params, dtype=torch.bfloat16):
        import weakref
        self.open()
        if not params:
            return
        flat = torch.empty(sum(p.numel() for p in params), dtype=dtype, device=params[0].device)
        views = [v.view(p.shape) for v, p in zip(flat.split([p.numel() for p in params]), params)]
        torch._foreach_copy_(views, [p.detach() for p in params])
        if len(self.entries) > 4096:               # drop entries of collected parameters
            self.entries = {k: v for k, v in self.entries.items() if v[0]() is not None}
        for p, v in zip(params, views):
            self.entries[(id(p), dtype)] = (weakref.ref(p), v, self.epoch)

    def end(self):
        if self.epoch & 1:
            self.epoch += 1


BF16_COPIES = _Bf16Copies()


class _DropPool:
    """The per-sample drop-path scales of ONE forward from ONE random draw.  A ViT-Adapter-B step has 28 drop-path sites; as
    `new_empty(B).bernoulli_(keep).div_(keep)` each is two 4-us kernels in a stream of much larger ones (56 launches per
    step).  Inside a forward epoch the sites are served rows of `floor(keep_i + U[0,1)) / keep_i` - timm's own DropPath
    formula, drawn for all sites at once - in the order the previous forward of the same module asked for them; a site
    that does not match the recorded sequence (another batch size, another model path) ends the pooling for that forward
    and draws on its own.  Off for modules that recompute activations (with_cp): the recomputation replays torch's RNG
    state, which a pooled draw made at the start of the forward is not part of."""

    def __init__(self):
        self.rows = self.seq = self.module = None
        self.pos, self.recording = 0, []

    def begin(self, module, device):
        self.module, self.recording, self.pos, self.rows = module, [], 0, None
        d = module.__dict__
        self.seq = d.get('_vah_drop_trace')
        if 'vah_drop_pool_ok' not in d:
            d['vah_drop_pool_ok'] = not any(getattr(m, 'with_cp', False) for m in module.modules())
        if not (self.seq and d['vah_drop_pool_ok'] and ENABLED.get('drop_pool', True)):
            self.seq = None
            return
        keeps = d.get('_vah_drop_keeps')
        if keeps is None or keeps.device != device or keeps.shape[0] != len(self.seq):
            keeps = d['_vah_drop_keeps'] = torch.tensor([k for k, _ in self.seq], dtype=torch.float32, device=device)[:, None]
        B = self.seq[0][1]
        if any(b != B for _, b in self.seq):
            self.seq = None
            return
        self.rows = torch.rand((len(self.seq), B), device=device).add_(keeps).floor_().div_(keeps)

    def take(self, x, keep):
        B = x.shape[0]
        if self.module is not None:
            self.recording.append((keep, B))
            if self.rows is not None:
                if self.pos < len(self.seq) and self.seq[self.pos] == (keep, B) and self.rows.device == x.device:
                    self.pos += 1
                    return self.rows[self.pos - 1]
                self.rows = None            # not the recorded sequence: every site of this forward draws on its own
        return x.new_empty((B,)).bernoulli_(keep).div_(keep)

    def end(self):
        if self.module is not None:
            d = self.module.__dict__
            if d.get('_vah_drop_trace') != self.recording:
                d['_vah_drop_trace'] = self.recording
                d.pop('_vah_drop_keeps', None)
        self.module = self.rows = self.seq = None


DROP_POOL = _DropPool()


class forward_epoch:
    """``with fused.forward_epoch(model): ...`` around a model's forward: on entry ONE launch (_EpochCopies; with
    ENABLED['epoch_copies'] off, or without a usable job table, one multi-tensor cast of the nn.Linear parameters alone)
    makes the 16-bit copies (the autocast's type) of its fp32 parameters, which then serve every fused operator of
    this forward; on exit (also by an exception) the epoch closes and later uses cast on their own, so
    a parameter written between two forwards - by any means, `.data` included - is always seen."""

    def __init__(self, module):
        self.module = module

    def __enter__(self):
        module = self.module
        t16 = autocast_16('fp16_linear')
        if not (ENABLED['linear'] and t16 is not None):
            return self
        # the list is cached on the module; a parameter that is replaced later is simply not part of the
        # bulk cast and gets its own cast on use (slower, never stale)
        params = module.__dict__.get('_vah_linear_params')
        if params is None:
            params = [p for m in module.modules() if isinstance(m, torch.nn.Linear)
                      for p in (m.weight, m.bias) if p is not None]
            module.__dict__['_vah_linear_params'] = params
        live = [p for p in params if p.dtype == torch.float32 and p.is_cuda]
        if live:
            # one launch for every copy and layout of this forward (_EpochCopies), or the multi-tensor cast of the Linear
            # parameters with every other copy made on use
            if not (ENABLED['epoch_copies'] and EPOCH_COPIES.begin(module, t16, live[0].device)):
                BF16_COPIES.begin(live, t16)
            SIDE.begin_epoch()
            BIAS_PARTIALS.begin_epoch()
            if module.training:
                DROP_POOL.begin(module, live[0].device)
        return self

    def __exit__(self, *exc):
        BF16_COPIES.end()
        DROP_POOL.end()
        return False


_GEMM_WS_BYTES = 32 << 20
WGRAD_F32 = os.environ.get('VAH_LINEAR_WGRAD', 'f32') == 'f32'
GEMM_TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tuning',
                          'gemm_table_mi355x_base_det_1024.txt')
GEMM_TABLE_F16 = GEMM_TABLE[:-len('.txt')] + '_f16.txt'       # the fp16 problems of the same step ('f16 ' lines only)


def _configure_gemm():
    """VAH_GEMM_TUNING = mode[,candidates] (0 first heuristic answer, 1 time the heuristic
    candidates [default], 2 time every algorithm);  VAH_GEMM_TABLE = path of a tuned table to load
    ('' = none; default: the committed tables, bf16 and fp16);  VAH_GEMM_TABLE_DUMP = path to write the table to
    at exit."""
    spec = os.environ.get('VAH_GEMM_TUNING')
    if spec:
        parts = [int(v) for v in spec.split(',')]
        _vah.check(_vah.lib.vah_gemm_set_tuning(parts[0], parts[1] if len(parts) > 1 else 32), 'gemm_set_tuning')
    dump = os.environ.get('VAH_GEMM_TABLE_DUMP')
    if dump:
        import atexit
        atexit.register(lambda: open(dump, 'w').write(_vah.gemm_table_dump()))


_configure_gemm()
_GEMM_TABLE_LOADED = False


def _load_gemm_table():
    """On the first GEMM (needs the GPU: the table is tied to the hipBLASLt build that is loaded)."""
    global _GEMM_TABLE_LOADED
    _GEMM_TABLE_LOADED = True
    path = os.environ.get('VAH_GEMM_TABLE')
    for path in ((GEMM_TABLE, GEMM_TABLE_F16) if path is None else (path,)):
        if path and os.path.exists(path):
            _vah.gemm_table_load(open(path).read())


def gemm_16(a, b, trans_a=False, trans_b=False, out_dtype=None, bias=None, out=None):
    """op(a) @ op(b) for contiguous 2-D matrices of one 16-bit type (bf16 or fp16) on the tuned hipBLASLt dispatcher
    (csrc/gemm.hip); fp32 accumulation; the result in the operands' type (out_dtype None) or fp32.  A 16-bit bias is
    of the operands' type."""
    t16 = a.dtype
    assert t16 in (torch.bfloat16, torch.float16) and b.dtype == t16, (a.dtype, b.dtype)
    if out_dtype is None:
        out_dtype = t16
    assert out_dtype in (t16, torch.float32) and (bias is None or bias.dtype in (t16, torch.float32))
    M, K = (a.shape[1], a.shape[0]) if trans_a else a.shape
    N = b.shape[0] if trans_b else b.shape[1]
    assert (b.shape[1] if trans_b else b.shape[0]) == K and a.is_contiguous() and b.is_contiguous()
    if out is not None:
        assert out.shape == (M, N) and out.is_contiguous()
        d, out_dtype = out, out.dtype
    else:
        d = torch.empty((M, N), dtype=out_dtype, device=a.device)
    if M == 0 or N == 0:
        return d
    if K == 0:
        return d.zero_()
    if bias is not None and bias.dtype == torch.float16 and out_dtype == torch.float32:
        bias = bias.float()       # hipBLASLt misreads an fp16 bias into an fp32 output (the entry point refuses the pairing)
    if not _GEMM_TABLE_LOADED:
        _load_gemm_table()
    ws_bytes = _GEMM_WS_BYTES
    if bias is None and K >= 4096:       # room for the fp32 partial products of a split-K run
        ws_bytes += min(64 * M * N * 4, 160 << 20)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device)
    epilogue = _vah.GEMM_EPI_BIAS if bias is not None else _vah.GEMM_EPI_NONE
    with _vah.on(a.device):
        _vah.call('vah_gemm_bf16', t16, int(trans_a), int(trans_b), M, N, K, a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1], d.data_ptr(), N,
                  int(out_dtype == torch.float32), epilogue, bias.data_ptr() if bias is not None else None,
                  int(bias is not None and bias.dtype == torch.float32), ws.data_ptr(), ws_bytes, _stream(a))
    return d


gemm_bf16 = gemm_16         # the name from before the dispatcher took fp16 operands: for callers outside this module


def _wgrad_bgrad(g2, x2, partials=None, row_map=None):
    """(dW, db) = (g2^T x2 in fp32, column sums of g2) of a Linear backward: column-sum partials, the
    (split-K) GEMM and ONE launch that both reduces the GEMM's slices and sums the partials.  g2, x2: one 16-bit type
    (bf16 or fp16), which picks the entry points.  ``partials``:
    (rows of partial column sums of g2, their number) left by the kernel that wrote g2 (_BiasPartials) - no
    column-sum launch and no second read of g2 then.  ``row_map``: see _wgrad_bgrad_mapped (a third result then)."""
    import ctypes
    R, N = g2.shape
    K = x2.shape[1]
    t16 = g2.dtype
    assert x2.dtype == t16
    if not _GEMM_TABLE_LOADED:
        _load_gemm_table()
    dev = g2.device
    gw = torch.empty((N, K), dtype=torch.float32, device=dev)
    gb = torch.empty(N, dtype=torch.float32, device=dev)
    ws_bytes = _GEMM_WS_BYTES + (min(64 * N * K * 4, 160 << 20) if R >= 4096 else 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with _vah.on(dev):
        st = _stream(g2)
        if partials is not None:
            cws, nparts = partials[0], ctypes.c_int64(partials[1])
        else:
            cws, nparts = _scratch(N, dev), ctypes.c_int64(0)
            _vah.call('vah_colsum_bf16_partials', t16, g2.data_ptr(), R, N, cws.data_ptr(), ctypes.byref(nparts), st)
        if row_map is not None:
            applied = ctypes.c_int(0)
            fn = _vah.lib.vah_gemm_bf16_fin_rowmap if t16 == torch.bfloat16 else _vah.lib.vah_gemm_f16_fin_rowmap
            _vah.check(fn(1, 0, N, K, R, g2.data_ptr(), N, x2.data_ptr(), K, gw.data_ptr(), K, 1, ws.data_ptr(), ws_bytes,
                          cws.data_ptr(), nparts.value, N, gb.data_ptr(), row_map.data_ptr(), ctypes.byref(applied), st), fn.__name__)
            return gw, gb, bool(applied.value)
        _vah.call('vah_gemm_bf16_fin', t16, 1, 0, N, K, R, g2.data_ptr(), N, x2.data_ptr(), K, gw.data_ptr(), K, 1, ws.data_ptr(), ws_bytes,
                  cws.data_ptr(), nparts.value, N, gb.data_ptr(), st)
    return gw, gb


def _wgrad_bgrad_mapped(g2, x2, row_map):
    """_wgrad_bgrad with dW's row r stored to row ``row_map[r]`` and db's sum k to element ``row_map[k]`` (int32, N entries,
    a permutation) by the reduction launch itself -> (dW, db, applied).  applied False: the dispatcher ran the product
    without a reduction launch (split 1) and dW, db are in the product's own row order."""
    assert row_map.dtype == torch.int32 and row_map.numel() == g2.shape[1] and row_map.is_contiguous() and row_map.device == g2.device
    return _wgrad_bgrad(g2, x2, None, row_map)


class _SideStream:
    """Weight-gradient GEMMs on a second HIP stream.  In a Linear backward the input gradient is on the critical path
    (the next layer's backward waits for it), the weight / bias gradients are not: nobody reads them before the
    optimizer.  Their GEMMs reduce over the tokens into a few output tiles (768 x 768: 36 tiles for 256 CUs, split-K
    brings that to ~150 workgroups) and leave most of the chip idle, so they run beside the main stream's kernels.
      fork:  side.wait_stream(current)                       - the operands exist
      join:  current.wait_stream(side), ONCE per backward pass, from an autograd engine callback queued by the first
             fork of the pass (the engine runs callbacks after the last node: before anything can read a .grad)
    A gradient left on the side stream is NOT handed to autograd: the engine may add it to another gradient of the
    same parameter (a second use of the weight by any operator, two forwards before one backward, retain_graph) on the
    main stream the moment the node returns, which would race with the side stream.  The node returns None for it and
    the join, once the main stream is ordered behind the side stream, stores it in (or adds it to) the parameter's
    .grad itself - what AccumulateGrad does, at the end of the pass instead of in the middle.  That is only the same thing
    when nothing observes the accumulation: see may_defer.
    The operands are kept alive until the join (their memory is freed on the main stream's pool only after the main
    stream is ordered behind the side stream), the gradients are allocated while the side stream is current.
    Off when a process group exists (DDP's bucket hooks read a gradient the moment autograd produces it, and its
    .grad tensors are views into the buckets) and under HIP-graph capture (the fork / join edges cost a replayed graph more than the overlap gains).
    Measured on base_det, eager: 27.5 -> 26.7 ms per step."""

    def __init__(self):
        self.streams = {}
        self.pending = {}          # device index -> (main stream, [tensors kept alive], [(parameter, gradient)])

    def begin_epoch(self):
        for idx in list(self.pending):      # a backward pass that died before its callback: join now, never leave a fork open
            self.join(idx)

    def note(self, weight, bias):
        """Forward: weak references to the parameters whose gradients the backward may leave on the side stream.  The
        DECISION is taken at backward time (may_defer)."""
        import weakref
        if not weight.is_leaf or (bias is not None and not bias.is_leaf) or not (BF16_COPIES.epoch & 1):
            return None
        if not weight.requires_grad or (bias is not None and not bias.requires_grad):
            return None
        return tuple(weakref.ref(p) for p in (weight, bias) if p is not None)

    @staticmethod
    def _only_accumulated(p):
        """Will this backward pass do nothing with the parameter's gradient but accumulate it into .grad?  No tensor hooks
        (they see or rewrite the gradient in mid-pass), and AccumulateGrad scheduled by the engine: under
        torch.autograd.grad() gradients are RETURNED, and backward(inputs=...) may leave the parameter out."""
        if p is None or getattr(p, '_backward_hooks', None) or getattr(p, '_post_accumulate_grad_hooks', None):
            return False
        with torch.enable_grad():       # the parameter's AccumulateGrad node (not kept: a node that outlives its pass pins a stream)
            acc = p.view_as(p).grad_fn.next_functions[0][0]
        try:
            return bool(torch._C._will_engine_execute_node(acc))
        except RuntimeError:            # autograd.grad(), or not inside a backward pass at all
            return False

    def may_defer(self, token, dev):
        """Backward: may this node's weight / bias gradients be produced on the side stream and stored by the join?"""
        if token is None or not (ENABLED['wgrad_overlap'] and dev.type == 'cuda'):
            return False
        if torch.cuda.is_current_stream_capturing():
            return False               # measured: ~80 fork / join edges per step cost a replayed HIP graph 0.35 ms more than the overlap gains
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():      # DDP owns the .grad tensors (bucket views) and watches them arrive
            return False
        return all(self._only_accumulated(r()) for r in token)

    def fork(self, dev, keep):
        """-> the side stream, ordered behind everything enqueued on the current stream so far."""
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        side = self.streams.get(idx)
        if side is None:
            side = self.streams[idx] = torch.cuda.Stream(device=dev)
        cur = torch.cuda.current_stream(dev)
        side.wait_stream(cur)
        entry = self.pending.get(idx)
        if entry is None:
            self.pending[idx] = entry = (cur, [], [])
            torch.autograd.Variable._execution_engine.queue_callback(lambda: self.join(idx))
        entry[1].extend(keep)
        return side

    def deliver(self, dev, token, grads):
        """The side stream's gradients of this node, for the join to accumulate (same order as the token)."""
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        self.pending[idx][2].extend((r(), g) for r, g in zip(token, grads))

    def join(self, idx):
        entry = self.pending.pop(idx, None)
        if entry is None:
            return
        main, keep, grads = entry
        main.wait_stream(self.streams[idx])
        with torch.no_grad(), torch.cuda.stream(main):
            for p, g in grads:
                if p is None:           # the parameter died with its module before the pass ended
                    continue
                if g.dtype != p.dtype:
                    g = g.to(p.dtype)
                if p.grad is None:
                    p.grad = g.view_as(p)
                else:
                    p.grad.add_(g.view_as(p))
        keep.clear()


SIDE = _SideStream()


class _BiasPartials:
    """Bias-gradient partials from the kernels that write a Linear's dY.  The bias gradient of a Linear is the column sum
    of dY; where dY comes out of one of our own row-streaming backward kernels (residual + LayerNorm, residual, GELU) that
    kernel sums the columns of what it writes and leaves the partial rows here, and the Linear's backward hands them to the
    finalize job of its weight-gradient GEMM instead of launching a column-sum kernel over dY.
      forward:   fused.linear marks its output (``mark``); residual / residual_ln / gelu see the mark on their branch input
                 (``wanted``) and remember it
      backward:  the producer records (dz, partial rows, count); _LinearBF16.backward takes them (``take``) when its
                 gradient IS that tensor: same storage, offset, element count, row width, contiguous, and the version
                 recorded - a gradient autograd summed, a dropout in between, a hook's copy or an in-place edit all
                 miss, and a miss runs the column-sum kernel as before.  What is looked up is the tensor, not the
                 layer: whichever Linear reads exactly these bytes wants exactly their column sums.
    An entry holds a reference to dz (its address cannot be recycled while the entry lives) and is dropped when taken;
    whatever is left goes at the end of the backward pass (an engine callback, as _SideStream's join) and when the next
    forward epoch begins.  Nothing here waits for the device."""

    ATTR = '_vah_bias_dy'

    def __init__(self):
        self.passes = {}          # device index (None: CPU) -> {(storage pointer, offset): (dz, version, partial rows, count)}

    @staticmethod
    def mark(y, bias):
        if ENABLED['bias_partials'] and bias is not None and bias.requires_grad and torch.is_grad_enabled():
            setattr(y, _BiasPartials.ATTR, True)
        return y

    @staticmethod
    def wanted(z):
        return bool(ENABLED['bias_partials'] and getattr(z, _BiasPartials.ATTR, False) and takes_16(z.dtype, 'fp16_linear')
                    and z.shape[-1] % 8 == 0)

    @staticmethod
    def _key(t):
        return (t.untyped_storage().data_ptr(), t.storage_offset())

    def record(self, dz, bpart, nparts):
        idx = dz.device.index
        entries = self.passes.get(idx)
        if entries is None:
            entries = self.passes[idx] = {}
            try:                    # the engine runs it after the last node of this backward pass
                torch.autograd.Variable._execution_engine.queue_callback(lambda: self.end_pass(idx))
            except RuntimeError:    # not inside a backward pass: the next epoch clears
                pass
        entries[self._key(dz)] = (dz, dz._version, bpart, int(nparts))

    def take(self, g2):
        """-> (partial rows, count) for the contiguous (R, N) gradient ``g2``, or None."""
        entries = self.passes.get(g2.device.index)
        if not entries:
            return None
        key = self._key(g2)
        e = entries.get(key)
        if e is None:
            return None
        dz, version, bpart, nparts = e
        if (g2.dim() != 2 or not g2.is_contiguous() or not dz.is_contiguous() or dz.dtype != g2.dtype
                or dz.shape[-1] != g2.shape[1] or dz.numel() != g2.numel() or dz._version != version
                or g2._version != version or nparts < 1):
            return None
        del entries[key]
        return bpart, nparts

    def end_pass(self, idx):
        self.passes.pop(idx, None)

    def begin_epoch(self):
        self.passes.clear()


BIAS_PARTIALS = _BiasPartials()


def _bias_partials_out(C, device):
    """The partial rows a producer leaves for a Linear: an allocation of its own (they outlive the call, unlike _scratch)
    and the slot for their count."""
    import ctypes
    return torch.empty(_vah.lib.vah_reduce_ws_floats(C), dtype=torch.float32, device=device), ctypes.c_int64(0)


class _LinearBF16(torch.autograd.Function):
    """y = x W^T + b with 16-bit operands (``t16``: bf16 or fp16, the autocast's type) and fp32 accumulation (what
    autocast makes of F.linear).  Backward: dX in t16 (an fp16 dX overflows to inf, as torch's does), dW straight into
    fp32 from the GEMM (no 16-bit rounding, no cast kernel), db by the column-sum kernel.  The backward takes the type
    from the saved operands."""

    @staticmethod
    def forward(ctx, x, weight, bias, t16=torch.bfloat16):
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        if x2.dtype != t16:
            x2 = x2.to(t16)
        x2 = x2.contiguous()
        wb = BF16_COPIES.get(weight, t16)
        y = gemm_16(x2, wb, trans_b=True, bias=bias.detach() if bias is not None else None)
        ctx.save_for_backward(x2, wb)
        ctx.has_bias = bias is not None
        ctx.side = SIDE.note(weight, bias)
        ctx.in_shape = x.shape
        ctx.in_dtype = x.dtype
        return y.view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, g):
        x2, wb = ctx.saved_tensors
        N = wb.shape[0]
        t16 = wb.dtype
        g2 = g.reshape(-1, N)
        if g2.dtype != t16:
            g2 = g2.to(t16)
        g2 = g2.contiguous()
        gx = gw = gb = None
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        fin = ctx.needs_input_grad[1] and want_b and WGRAD_F32 and g2.shape[0] > 0 and ENABLED['wgrad_fin']
        partials = BIAS_PARTIALS.take(g2) if fin else None       # the kernel that wrote g2 summed its columns
        deferred = fin and SIDE.may_defer(ctx.side, g2.device)
        if deferred:                    # weight / bias gradients beside the input gradient, on the side stream
            keep = (g2, x2) if partials is None else (g2, x2, partials[0])
            with torch.cuda.stream(SIDE.fork(g2.device, keep)):
                SIDE.deliver(g2.device, ctx.side, _wgrad_bgrad(g2, x2, partials))
        if ctx.needs_input_grad[0]:
            gx = gemm_16(g2, wb).view(ctx.in_shape)
            if gx.dtype != ctx.in_dtype:
                gx = gx.to(ctx.in_dtype)
        if deferred:
            pass
        elif fin:
            gw, gb = _wgrad_bgrad(g2, x2, partials)
        else:
            if ctx.needs_input_grad[1]:
                if WGRAD_F32:
                    gw = gemm_16(g2, x2, trans_a=True, out_dtype=torch.float32)
                else:
                    gw = gemm_16(g2, x2, trans_a=True).float()
            if want_b:
                gb = torch.empty(N, dtype=torch.float32, device=g2.device)
                ws = _scratch(N, g2.device)
                with _vah.on(g2.device):
                    _vah.call('vah_colsum_bf16', t16, g2.data_ptr(), g2.shape[0], N, gb.data_ptr(), ws.data_ptr(), _stream(g2))
        return gx, gw, gb, None


class _PairCopies:
    """16-bit [Wa; Wb] (rows concatenated) and fp32 [ba; bb] of two Linear layers that read the same
    input: built once per forward epoch and 16-bit type (see _Bf16Copies), on every use outside one."""

    def __init__(self):
        self.entries = {}

    def get(self, a, b, dtype=torch.bfloat16):
        key = (id(a.weight), id(b.weight), dtype)
        epoch = BF16_COPIES.epoch
        e = self.entries.get(key)
        if e is not None and e[0] == epoch and (epoch & 1) and e[1].device == a.weight.device and e[3]() is a.weight:
            return e[1], e[2]
        import weakref
        with torch.no_grad():
            w = torch.cat([a.weight.detach(), b.weight.detach()], 0).to(dtype)
            bias = torch.cat([a.bias.detach(), b.bias.detach()], 0).float()
        if len(self.entries) > 1024:
            self.entries.clear()
        self.entries[key] = (epoch, w, bias, weakref.ref(a.weight))
        return w, bias


PAIR_COPIES = _PairCopies()


class _LinearPairBF16(torch.autograd.Function):
    """(x Wa^T + ba, x Wb^T + bb) as ONE GEMM over the concatenated weights, and one input-gradient
    GEMM, one weight-gradient GEMM and one column sum in the backward.  For MSDeformAttn's
    sampling_offsets / attention_weights (ms_deform_attn.py:108-109): two skinny GEMMs (96 and 48
    outputs per level) over the same 43008 x 768 query matrix plus the add autograd needs to sum the
    two input gradients."""

    @staticmethod
    def forward(ctx, x, wa, ba, wb, bb, pair, f32_out=False):
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        w, bias = pair
        t16 = w.dtype                          # bf16 or fp16: the type of the pair's weight copy
        if x2.dtype != t16:
            x2 = x2.to(t16)
        x2 = x2.contiguous()
        y = gemm_16(x2, w, trans_b=True, bias=bias, out_dtype=torch.float32 if f32_out else t16)
        na = wa.shape[0]
        ctx.save_for_backward(x2, w)
        ctx.na, ctx.in_shape, ctx.in_dtype = na, x.shape, x.dtype
        lead = x.shape[:-1]
        return y[:, :na].contiguous().view(*lead, na), y[:, na:].contiguous().view(*lead, w.shape[0] - na)

    @staticmethod
    def backward(ctx, ga, gb):
        x2, w = ctx.saved_tensors
        na = ctx.na
        nb = w.shape[0] - na
        R = x2.shape[0]
        g = torch.empty((R, na + nb), dtype=w.dtype, device=x2.device)
        g[:, :na] = ga.reshape(R, na) if ga is not None else 0
        g[:, na:] = gb.reshape(R, nb) if gb is not None else 0
        gx = gw = gbias = None
        if ctx.needs_input_grad[0]:
            gx = gemm_16(g, w).view(ctx.in_shape)
            if gx.dtype != ctx.in_dtype:
                gx = gx.to(ctx.in_dtype)
        want_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[3]
        want_b = ctx.needs_input_grad[2] or ctx.needs_input_grad[4]
        if want_w and want_b and R > 0 and ENABLED['wgrad_fin']:
            gw, gbias = _wgrad_bgrad(g, x2)
        else:
            if want_w:
                gw = gemm_16(g, x2, trans_a=True, out_dtype=torch.float32)
            if want_b:
                gbias = torch.empty(na + nb, dtype=torch.float32, device=g.device)
                ws = _scratch(na + nb, g.device)
                with _vah.on(g.device):
                    _vah.call('vah_colsum_bf16', g.dtype, g.data_ptr(), R, na + nb, gbias.data_ptr(), ws.data_ptr(), _stream(g))
        return (gx, gw[:na] if gw is not None else None, gbias[:na] if gbias is not None else None,
                gw[na:] if gw is not None else None, gbias[na:] if gbias is not None else None, None, None)


def linear_pair(lin_a, lin_b, x, f32_out=False):
    """``(lin_a(x), lin_b(x))`` for two nn.Linear layers on the same input.  f32_out: the outputs straight from the fp32
    accumulators (MSDeformAttn's sampling offsets: the reference keeps them in fp32, and d(out)/d(location) jumps at
    integer pixel coordinates, so 8-bit offsets cost the upstream gradients 0.3 - 0.7 of relative L2 on small maps)."""
    wa, wb = lin_a.weight, lin_b.weight
    # fp16 autocast: the form with 16-bit outputs only (fp32 offsets under fp16 are MSDeformAttn's own business)
    t16 = autocast_16('fp16_linear')
    if f32_out and t16 != torch.bfloat16:
        t16 = None
    if (ENABLED['linear'] and ENABLED['linear_pair'] and x.is_cuda and t16 is not None and wa.dtype == torch.float32
            and wb.dtype == torch.float32 and lin_a.bias is not None and lin_b.bias is not None
            and x.dtype in (t16, torch.float32) and (wa.shape[0] + wb.shape[0]) % 8 == 0
            and wa.shape[1] % 8 == 0 and wa.shape[1] == wb.shape[1] and x.numel() > 0
            and type(lin_a) is torch.nn.Linear and type(lin_b) is torch.nn.Linear):
        return _LinearPairBF16.apply(x, wa, lin_a.bias, wb, lin_b.bias, PAIR_COPIES.get(lin_a, lin_b, t16), f32_out)
    if f32_out and x.is_cuda and _bf16_autocast():
        # widths the paired GEMM does not take (a single deformable head: 8 + 4 outputs): two plain fp32 Linears
        with torch.autocast('cuda', enabled=False):
            xf = x.float()
            return torch.nn.functional.linear(xf, wa.float(), lin_a.bias), torch.nn.functional.linear(xf, wb.float(), lin_b.bias)
    return linear(lin_a, x), linear(lin_b, x)


class _PairCoreCopies:
    """bf16 rows of [sampling_offsets; attention_weights] reordered head by head - [offsets of head 0 | logits of head 0 |
    offsets of head 1 | ...] - with the fp32 bias in the same order, and the permutation (see msda_pair_core)."""

    def __init__(self):
        self.entries = {}

    def perm(self, a, b, M):
        """(permutation, its inverse, the permutation as the int32 row map of the weight-gradient reduction): made once
        per module and device, not per call."""
        e = self.entries.get((id(a.weight), id(b.weight)))
        na, nb = a.weight.shape[0], b.weight.shape[0]
        po, pl = na // M, nb // M
        dev = a.weight.device
        if e is not None and e[4]() is a.weight and e[3][0].device == dev and e[3][0].numel() == na + nb:
            return e[3]     # of this very module: id() of a collected module's weights comes back for another module's
        fw = torch.cat([torch.cat((torch.arange(m * po, (m + 1) * po), na + torch.arange(m * pl, (m + 1) * pl))) for m in range(M)])
        inv = torch.empty_like(fw)
        inv[fw] = torch.arange(fw.numel())
        return (fw.to(dev), inv.to(dev), fw.to(torch.int32).to(dev))

    def put(self, a, b, epoch, w, bias, perm):
        """The copies this epoch's launch made (_EpochCopies)."""
        import weakref
        if len(self.entries) > 1024:
            self.entries.clear()
        self.entries[(id(a.weight), id(b.weight))] = (epoch, w, bias, perm, weakref.ref(a.weight))

    def get(self, a, b, M):
        key = (id(a.weight), id(b.weight))
        epoch = BF16_COPIES.epoch
        e = self.entries.get(key)
        if e is not None and e[0] == epoch and (epoch & 1) and e[1].device == a.weight.device and e[4]() is a.weight:
            return e[1], e[2], e[3]
        import weakref
        perm = self.perm(a, b, M)
        with torch.no_grad():
            w = torch.cat([a.weight.detach(), b.weight.detach()], 0).index_select(0, perm[0]).to(torch.bfloat16)
            bias = torch.cat([a.bias.detach(), b.bias.detach()], 0).float().index_select(0, perm[0])
        if len(self.entries) > 1024:
            self.entries.clear()
        self.entries[key] = (epoch, w, bias, perm, weakref.ref(a.weight))
        return w, bias, perm


PAIR_CORE_COPIES = _PairCoreCopies()


class _EpochTable:
    """The job table of one model and 16-bit type (see _EpochCopies): device tensors ``jobs`` / ``chunks``, the sizes of
    the two destination buffers, what every parameter looked like when the table was built (``sig``) and how the
    buffers are handed out (``serve``)."""

    def __init__(self, dtype, device):
        self.dtype, self.device = dtype, device
        self.rows, self.params, self.sig, self.serve = [], [], [], []
        self.n16 = self.n32 = 0
        self.jobs = self.chunks = None
        self.nchunks = 0

    def valid(self):
        for p, (ptr, shape, dtype) in zip(self.params, self.sig):
            if p.data_ptr() != ptr or p.shape != shape or p.dtype != dtype:
                return False
        return True

    def uses(self, p):
        if not any(q is p for q in self.params):
            self.params.append(p)
            self.sig.append((p.data_ptr(), p.shape, p.dtype))

    def alloc(self, n, f32=False):
        """Offset of ``n`` elements in the 16-bit (fp32) destination buffer, starting on a 16-byte (32-byte) boundary."""
        if f32:
            off, self.n32 = self.n32, self.n32 + (n + 7) // 8 * 8
        else:
            off, self.n16 = self.n16, self.n16 + (n + 7) // 8 * 8
        return off

    def job(self, p, src_off, dst, dims, strides, lims=None, f32=False):
        """Gather ``dims`` (destination order, up to 4) from parameter ``p`` at element offset ``src_off`` with element
        ``strides``; ``lims``: the source's extents (an index beyond reads as zero)."""
        dims, strides = (1,) * (4 - len(dims)) + tuple(dims), (0,) * (4 - len(strides)) + tuple(strides)
        lims = dims if lims is None else (1,) * (4 - len(lims)) + tuple(lims)
        n = dims[0] * dims[1] * dims[2] * dims[3]
        assert 0 < n < 2 ** 31 and p.dtype == torch.float32 and p.is_contiguous() and 0 <= src_off < p.numel()
        last = sum((min(d, l) - 1) * s for d, l, s in zip(dims, lims, strides))
        assert min(strides) >= 0 and src_off + last < p.numel(), 'a job reads past its parameter'
        packed = (dims[1] * dims[2] * dims[3], dims[2] * dims[3], dims[3], 1)
        dense = all(d == 1 or s == c for d, s, c in zip(dims, strides, packed)) and all(l >= d for l, d in zip(lims, dims))
        self.uses(p)
        self.rows.append([p.data_ptr() + 4 * src_off, dst, n, dims[1], dims[2], dims[3], *strides, *lims,
                          (1 if dense else 0) | (2 if f32 else 0), p.numel() - src_off])

    def finish(self):
        chunk = int(_vah.lib.vah_epoch_chunk_elems())
        assert _vah.lib.vah_epoch_job_bytes() == 16 * 8
        if not self.rows:
            return self
        jobs = torch.tensor(self.rows, dtype=torch.int64)
        counts = (jobs[:, 2] + chunk - 1) // chunk
        job_of = torch.repeat_interleave(torch.arange(len(self.rows)), counts)
        first = torch.cumsum(counts, 0) - counts
        k = torch.arange(job_of.numel()) - first[job_of]
        self.chunks = torch.stack([job_of, k], 1).to(torch.int32).contiguous().to(self.device)
        self.jobs = jobs.to(self.device)
        self.nchunks = int(job_of.numel())
        return self


class _EpochCopies:
    """ONE launch (csrc/epoch_copies.hip) makes every 16-bit copy of fp32 parameters that a forward epoch serves: the plain
    copies of the nn.Linear parameters and of the 1x1 / patch-embedding convolution weights (_Bf16Copies.get), the
    head-interleaved [offsets of head m | logits of head m] rows and fp32 bias of every MSDeformAttn pair
    (_PairCoreCopies; 2 * M contiguous row-block jobs each, no permutation array), the tap-major (Cout, 9, Cin) and
    (Cin, 9, Cout) layouts of the bias-free 3x3 convolutions (spm_nhwc._Conv3x3; a 3-channel stem weight zero-padded to the
    16-channel image) and the (dy, dx, co)-row matrix of a 2x2 / stride 2 transposed convolution (_UpFromTokens).

    The table is built once per model and 16-bit type, cached on the module, and checked at every epoch against the
    parameters' data_ptr(), shape and dtype (a mismatch rebuilds it: the jobs hold addresses).  The destination is a fresh
    allocation per epoch - the kernel takes its base as an argument, jobs hold offsets - so a copy saved for a backward
    keeps the values of its own forward.  Building a table copies it to the device: inside a graph capture an epoch
    without a valid table takes the per-use path instead (begin returns False).  A parameter the table does not hold is
    cast on use, as outside an epoch.  Modules are recognised by type and geometry alone; a model with other 3x3
    convolutions gets copies nobody reads (they cost bandwidth, never correctness)."""

    ATTR = '_vah_epoch_tables'

    @staticmethod
    def _ok(p, dev):
        return (isinstance(p, torch.Tensor) and p.dtype == torch.float32 and p.device == dev and p.is_contiguous()
                and 0 < p.numel() < 2 ** 31)

    def build(self, module, t16, dev):
        nn = torch.nn
        tab = _EpochTable(t16, dev)
        plain = set()

        def add_plain(p):
            if self._ok(p, dev) and id(p) not in plain:
                plain.add(id(p))
                off = tab.alloc(p.numel())
                tab.job(p, 0, off, (p.numel(),), (1,))
                tab.serve.append(('plain', p, off))

        for m in module.modules():
            if isinstance(m, nn.Linear):
                add_plain(m.weight)
                add_plain(m.bias)
            elif isinstance(m, nn.ConvTranspose2d):
                w = m.weight
                if (m.kernel_size == (2, 2) and m.stride == (2, 2) and m.padding == (0, 0) and m.output_padding == (0, 0)
                        and m.groups == 1 and m.dilation == (1, 1) and self._ok(w, dev)):
                    C, Co = w.shape[0], w.shape[1]
                    off = tab.alloc(w.numel())
                    tab.job(w, 0, off, (2, 2, Co, C), (2, 1, 4, Co * 4))            # rows (dy, dx, co)
                    tab.serve.append(('up', w, off, (4 * Co, C)))
            elif isinstance(m, nn.Conv2d) and m.groups == 1 and m.dilation == (1, 1) and self._ok(m.weight, dev):
                w, k = m.weight, m.kernel_size
                Co, Ci = w.shape[0], w.shape[1]
                if k == (3, 3) and m.padding == (1, 1) and m.bias is None:
                    cin = (Ci + 15) // 16 * 16                       # the stem reads the image as 16 channels, 3..15 zero
                    o9, ot9 = tab.alloc(Co * 9 * cin), tab.alloc(cin * 9 * Co)
                    tab.job(w, 0, o9, (Co, 3, 3, cin), (Ci * 9, 3, 1, 9), (Co, 3, 3, Ci))
                    tab.job(w, 0, ot9, (cin, 3, 3, Co), (9, 3, 1, Ci * 9), (Ci, 3, 3, Co))
                    tab.serve.append(('conv9', w, o9, (Co, 9, cin), ot9, (cin, 9, Co)))
                elif t16 == torch.bfloat16 and m.padding == (0, 0) and k == m.stride:
                    add_plain(w)                                     # patch embedding / 1x1: a matrix as it lies (bf16 paths only)
            a, b = getattr(m, 'sampling_offsets', None), getattr(m, 'attention_weights', None)
            M = getattr(m, 'n_heads', None)
            if (t16 == torch.bfloat16 and type(a) is nn.Linear and type(b) is nn.Linear and isinstance(M, int) and M > 0
                    and all(self._ok(p, dev) for p in (a.weight, a.bias, b.weight, b.bias))
                    and a.weight.shape[1] == b.weight.shape[1] and a.weight.shape[0] % M == 0 and b.weight.shape[0] % M == 0):
                na, nb, K = a.weight.shape[0], b.weight.shape[0], a.weight.shape[1]
                po, pl = na // M, nb // M
                ow, ob = tab.alloc((na + nb) * K), tab.alloc(na + nb, f32=True)
                for h in range(M):
                    r = h * (po + pl)
                    tab.job(a.weight, h * po * K, ow + r * K, (po * K,), (1,))
                    tab.job(b.weight, h * pl * K, ow + (r + po) * K, (pl * K,), (1,))
                    tab.job(a.bias, h * po, ob + r, (po,), (1,), f32=True)
                    tab.job(b.bias, h * pl, ob + r + po, (pl,), (1,), f32=True)
                tab.serve.append(('pair_core', a, b, ow, (na + nb, K), ob, PAIR_CORE_COPIES.perm(a, b, M)))
        return tab.finish()

    def begin(self, module, t16, dev):
        """Open an epoch whose copies come from the table's one launch.  False (nothing opened): no usable table - the
        caller makes the epoch's copies the multi-tensor way."""
        tables = module.__dict__.setdefault(self.ATTR, {})
        tab = tables.get((t16, dev))
        if tab is None or not tab.valid():
            if torch.cuda.is_current_stream_capturing():
                return False                    # building copies the table to the device: not inside a capture
            tab = tables[(t16, dev)] = self.build(module, t16, dev)
        if tab.nchunks == 0:
            return False
        import weakref
        out16 = torch.empty(tab.n16, dtype=t16, device=dev)
        out32 = torch.empty(max(tab.n32, 8), dtype=torch.float32, device=dev)
        with _vah.on(dev):
            _vah.check(_vah.lib.vah_epoch_copies(tab.jobs.data_ptr(), tab.jobs.shape[0], tab.chunks.data_ptr(), tab.nchunks,
                                                 1 if t16 == torch.bfloat16 else 2, out16.data_ptr(), tab.n16, out32.data_ptr(),
                                                 tab.n32, _vah.raw_stream(dev)), 'epoch_copies')
        cp = BF16_COPIES
        cp.open()
        epoch = cp.epoch
        if len(cp.entries) > 4096:               # drop entries of collected parameters
            cp.entries = {k: v for k, v in cp.entries.items() if v[0]() is not None}
        if len(cp.layouts) > 1024:
            cp.layouts = {k: v for k, v in cp.layouts.items() if v[0]() is not None}
        for s in tab.serve:
            kind, p = s[0], s[1]
            if kind == 'plain':
                cp.entries[(id(p), t16)] = (weakref.ref(p), out16[s[2]:s[2] + p.numel()].view(p.shape), epoch)
            elif kind == 'up':
                n = s[3][0] * s[3][1]
                cp.layouts[('up', id(p), t16)] = (weakref.ref(p), out16[s[2]:s[2] + n].view(s[3]), epoch)
            elif kind == 'conv9':
                n = s[3][0] * s[3][1] * s[3][2]
                cp.layouts[('conv9', id(p), t16)] = (weakref.ref(p), (out16[s[2]:s[2] + n].view(s[3]), out16[s[4]:s[4] + n].view(s[5])),
                                                     epoch)
            else:
                a, b, ow, wshape, ob, perm = s[1:]
                PAIR_CORE_COPIES.put(a, b, epoch, out16[ow:ow + wshape[0] * wshape[1]].view(wshape), out32[ob:ob + wshape[0]], perm)
        return True


EPOCH_COPIES = _EpochCopies()


class _MSDAPairCore(torch.autograd.Function):
    """MSDeformAttn's sampling_offsets / attention_weights Linear pair AND the fused deformable-attention core as one
    autograd node (ref ops/modules/ms_deform_attn.py:108-128): ONE GEMM over the two weight matrices with its output
    rows ordered head by head - (n, q, m) row = [L*P*2 offsets | L*P logits], fp32 straight from the accumulators - which
    the MSDA kernels read in place through a row stride.  What this removes per call: the two slice copies of the
    paired GEMM's output and the two that rebuild the gradient matrix, the bf16 rounding of the sampling offsets (the
    reference keeps them in fp32: ms_deform_attn_func.py:21; d(out)/d(location) jumps at integer pixel coordinates, so
    8-bit offsets cost the upstream gradients 0.2-0.35 of relative L2 on small problems), and one cache line per list
    entry in the backward's tile pass (a row's offsets and logits now sit side by side).  The gradients come back in
    bf16, written by the tile pass into the gradient matrix of the pair GEMM's backward in the same row order."""

    @staticmethod
    def forward(ctx, query, value, shapes, lsi, ref, wa, ba, wb, bb, copies, M, L, P):
        from ops.functions import ms_deform_attn_fused as mf
        K = query.shape[-1]
        x2 = query.reshape(-1, K)
        if x2.dtype != torch.bfloat16:
            x2 = x2.to(torch.bfloat16)
        x2 = x2.contiguous()
        w, bias, perm = copies
        y = gemm_16(x2, w, trans_b=True, bias=bias, out_dtype=torch.float32)         # (N * Lq, M * 3 * L * P) fp32
        N, Lq = query.shape[0], query.shape[1]
        PS = 3 * L * P
        yv = y.view(N, Lq, M, PS)
        offsets = yv[..., :2 * L * P].unflatten(-1, (L, P, 2))
        logits = yv[..., 2 * L * P:]
        value = value.contiguous()
        refc = ref.detach().float().contiguous().view(ref.shape[0], Lq, -1, ref.shape[-1])          # points, or boxes (cx, cy, w, h)
        # the window-forward schedule rides on a grid the batch shares; one grid per image has no such schedule
        out = mf.fused_forward(value, shapes, lsi, offsets, logits, PS, PS, refc, carrier=ref if refc.shape[0] == 1 else None,
                               token=BF16_COPIES.epoch)
        ctx.save_for_backward(x2, w, y, value, shapes, lsi, refc, perm[1], perm[2])
        ctx.dims = (N, Lq, M, L, P, wa.shape[0])
        ctx.in_shape, ctx.in_dtype = query.shape, query.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x2, w, y, value, shapes, lsi, refc, inv, row_map = ctx.saved_tensors
        N, Lq, M, L, P, na = ctx.dims
        S, D = value.shape[1], value.shape[3]
        PS = 3 * L * P
        R = x2.shape[0]
        gout = gout.contiguous().to(value.dtype)
        g = torch.empty((R, M * PS), dtype=torch.bfloat16, device=x2.device)
        grad_value = torch.empty_like(value)
        ws_bytes = _vah.lib.vah_msda_tile_ws_bytes(N, S, M * (D // 32), L, Lq, P)      # per 32-channel head slice
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=value.device)
        from ops.functions.ms_deform_attn_fused import box_entry
        name, comps = box_entry('vah_msda_fused_backward_tiled', refc.shape[3])          # boxes: the *_box entry point
        with _vah.on(value.device):
            rc = getattr(_vah.lib, name)(
                value.data_ptr(), 1, shapes.data_ptr(), lsi.data_ptr(), y.data_ptr(), y.data_ptr() + 2 * L * P * 4, 0, PS, PS,
                refc.data_ptr(), refc.shape[2], refc.shape[0], *comps, gout.data_ptr(), N, S, M, D, L, Lq, P, grad_value.data_ptr(), 1,
                g.data_ptr(), g.data_ptr() + 2 * L * P * 2, 1, PS, PS, ws.data_ptr(), ws_bytes, _stream(value))
        _vah.check(rc, name)
        gx = gw = gbias = None
        if ctx.needs_input_grad[0]:
            gx = gemm_16(g, w).view(ctx.in_shape)
            if gx.dtype != ctx.in_dtype:
                gx = gx.to(ctx.in_dtype)
        if any(ctx.needs_input_grad[5:9]):
            # the reduction launch of the weight-gradient GEMM stores rows and bias sums in parameter order; a product the
            # dispatcher runs without a reduction launch (split 1) comes back head-interleaved and is reordered here
            if ENABLED['epoch_copies']:
                gw, gbias, mapped = _wgrad_bgrad_mapped(g, x2, row_map)
            else:
                (gw, gbias), mapped = _wgrad_bgrad(g, x2), False
            if not mapped:
                gw, gbias = gw.index_select(0, inv), gbias.index_select(0, inv)
        return (gx, grad_value if ctx.needs_input_grad[1] else None, None, None, None,
                gw[:na] if gw is not None else None, gbias[:na] if gbias is not None else None,
                gw[na:] if gw is not None else None, gbias[na:] if gbias is not None else None, None, None, None, None)


def msda_pair_core_ok(mod, query, value, reference_points):
    """The one-node form of MSDeformAttn's offsets / weights pair + core: bf16 autocast on the GPU with bf16 values, the
    tile-pass backward and shapes the fused kernels cover (D in {32, 64}, P == 4, L in {1, 3, 4}), reference points shared by
    the batch or one grid per image (not learned ones: ops.functions.ms_deform_attn_fused.ref_points_ok), points or boxes
    (cx, cy, w, h): the tile pass, which every call here needs, is also all that serves boxes."""
    import os
    from ops.functions.ms_deform_attn_fused import ref_points_ok
    a, b = mod.sampling_offsets, mod.attention_weights
    M, L, P = mod.n_heads, mod.n_levels, mod.n_points
    return (ENABLED['linear'] and ENABLED['linear_pair'] and ENABLED['pair_core'] and query.is_cuda and _bf16_autocast()
            and value.dtype == torch.bfloat16 and value.dim() == 4 and value.shape[-1] in (32, 64) and P == 4 and L in (1, 3, 4)
            and (M * 3 * L * P) % 8 == 0            # rows of the pair GEMM / its column sums: 16-byte multiples
            and type(a) is torch.nn.Linear and type(b) is torch.nn.Linear and a.bias is not None and b.bias is not None
            and a.weight.dtype == torch.float32 and b.weight.dtype == torch.float32 and a.weight.shape[1] % 8 == 0
            and ref_points_ok(reference_points, value.shape[0], L)
            and query.numel() > 0 and value.numel() > 0 and query.dtype in (torch.bfloat16, torch.float32)
            and os.environ.get('VAH_MSDA_FUSED', '1') != '0' and os.environ.get('VAH_MSDA_TILED', '1') != '0'
            and _vah.lib.vah_msda_tile_ws_bytes(value.shape[0], value.shape[1], M * (value.shape[-1] // 32), L,
                                                query.shape[1], P) >= 0)


def msda_pair_core(mod, query, value, shapes, lsi, reference_points):
    a, b = mod.sampling_offsets, mod.attention_weights
    return _MSDAPairCore.apply(query, value, shapes, lsi, reference_points, a.weight, a.bias, b.weight, b.bias,
                               PAIR_CORE_COPIES.get(a, b, mod.n_heads), mod.n_heads, mod.n_levels, mod.n_points)


class _Conv1x1BF16(torch.autograd.Function):
    """1x1 convolution without bias on NCHW bf16 as plain GEMMs on the planes: out[b] (Co x HW) =
    W (Co x Ci) x[b] (Ci x HW) - no NCHW <-> NHWC conversions around an implicit-GEMM kernel; the
    weight gradient reduces over HW (65536 at the stride-4 map) with split-K."""

    @staticmethod
    def forward(ctx, x, weight):
        B, Ci, H, W = x.shape
        Co = weight.shape[0]
        x = x.contiguous()
        wb = BF16_COPIES.get(weight).view(Co, Ci)
        out = torch.empty((B, Co, H, W), dtype=torch.bfloat16, device=x.device)
        for b in range(B):
            gemm_16(wb, x[b].view(Ci, H * W), out=out[b].view(Co, H * W))
        ctx.save_for_backward(x, wb)
        return out

    @staticmethod
    def backward(ctx, g):
        x, wb = ctx.saved_tensors
        B, Ci, H, W = x.shape
        Co = wb.shape[0]
        g = g.contiguous().to(torch.bfloat16)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            for b in range(B):
                gemm_16(wb, g[b].view(Co, H * W), trans_a=True, out=dx[b].view(Ci, H * W))
        if ctx.needs_input_grad[1]:
            for b in range(B):
                part = gemm_16(g[b].view(Co, H * W), x[b].view(Ci, H * W), trans_b=True, out_dtype=torch.float32)
                dw = part if dw is None else dw.add_(part)
            dw = dw.view(Co, Ci, 1, 1)
        return dx, dw


class _UpFromTokens(torch.autograd.Function):
    """ConvTranspose2d(C, Co, kernel 2, stride 2) WITHOUT bias applied to a map given as its token rows:
    rows (B, h*w, C) -> NCHW planes (B, Co, 2h, 2w) in ``t16`` (bf16 | fp16).  The transposed convolution with stride = kernel is a plain
    GEMM per image, U_b (4*Co, h*w) = Wcat (4*Co, C) rows_b^T with Wcat rows (dy, dx, co), followed by the 2 x 2 sub-pixel
    interleave (csrc/tail_ops.hip::pixel_shuffle2); the backward is the inverse interleave and two GEMMs.  MIOpen's
    NCHW transposed convolution took 494 + 846 us for this layer at base_det (2 x 768 x 128 x 128).
    bf16: the products are gemm_16.  fp16: they are torch's fp16 library GEMMs on the token rows (this operator's fp16
    form was not moved to the dispatcher with the Linear layers); dW is what autocast gives conv_transpose2d - fp16 products per image, summed over the images in fp32."""

    @staticmethod
    def forward(ctx, rows, weight, h, w, addend, t16):
        B, T, C = rows.shape
        Co = weight.shape[1]
        xb = rows.detach().to(t16).contiguous()
        wc = BF16_COPIES.layout('up', weight, t16)              # rows (dy, dx, co): made by the epoch's launch, or here
        if t16 == torch.bfloat16:
            if wc is None:
                wc = BF16_COPIES.get(weight).permute(2, 3, 1, 0).reshape(4 * Co, C).contiguous()
            U = torch.empty((B, 4 * Co, T), dtype=torch.bfloat16, device=rows.device)
            for b in range(B):
                gemm_16(wc, xb[b], trans_b=True, out=U[b])
        else:
            if wc is None:
                wc = weight.detach().to(t16).permute(2, 3, 1, 0).reshape(4 * Co, C).contiguous()
            U = torch.bmm(wc.unsqueeze(0).expand(B, 4 * Co, C), xb.transpose(1, 2))
        out = torch.empty((B, Co, 2 * h, 2 * w), dtype=t16, device=rows.device)
        add = addend.contiguous() if addend is not None else None
        with _vah.on(rows.device):
            _vah.call('vah_pixel_shuffle2_bf16', t16, U.data_ptr(), B, Co, h, w, out.data_ptr(), 0, add.data_ptr() if add is not None else None,
                      _stream(rows))
        ctx.save_for_backward(xb, wc)
        ctx.meta = (h, w, Co, rows.dtype, t16)
        return out

    @staticmethod
    def backward(ctx, g):
        xb, wc = ctx.saved_tensors
        h, w, Co, in_dtype, t16 = ctx.meta
        B, T, C = xb.shape
        g = g.contiguous().to(t16)
        dU = torch.empty((B, 4 * Co, T), dtype=t16, device=g.device)
        with _vah.on(g.device):
            _vah.call('vah_pixel_shuffle2_bf16', t16, g.data_ptr(), B, Co, h, w, dU.data_ptr(), 1, None, _stream(g))
        dx = dw = None
        if ctx.needs_input_grad[0]:
            if t16 == torch.bfloat16:
                dx = torch.empty((B, T, C), dtype=torch.bfloat16, device=g.device)
                for b in range(B):
                    gemm_16(dU[b], wc, trans_a=True, out=dx[b])
            else:
                dx = torch.matmul(dU.transpose(1, 2), wc)
            if dx.dtype != in_dtype:
                dx = dx.to(in_dtype)
        if ctx.needs_input_grad[1]:
            if t16 == torch.bfloat16:
                for b in range(B):
                    part = gemm_16(dU[b], xb[b], out_dtype=torch.float32)
                    dw = part if dw is None else dw.add_(part)
            else:
                dw = torch.bmm(dU, xb).float().sum(0)
            dw = dw.view(2, 2, Co, C).permute(3, 2, 0, 1).contiguous()
        return dx, dw, None, None, (g if ctx.needs_input_grad[4] else None), None      # d(out)/d(addend) = identity


def up_from_tokens(up, rows, h, w, addend=None):
    """``F.conv_transpose2d(rows.transpose(1, 2).view(B, C, h, w), up.weight, None, stride=2)`` for the backbone's
    2 x 2 / stride 2 ``up`` (vit_adapter.py:46), from the token rows of the map and without the bias (the caller folds
    it into the BatchNorm tail); ``addend`` (planes-shaped, in the autocast's 16-bit type, e.g. c1) is summed in by the
    interleave pass - ``up(c2) + c1`` rounded once, as autocast rounds the sum of two half tensors - so the tail reads one
    operand instead of two.  bf16 or (ENABLED['fp16_tail']) fp16 autocast.  None when the GEMM form does not apply."""
    wt = up.weight
    t16 = autocast_16('fp16_tail')
    if (ENABLED['up_gemm'] and ENABLED['linear'] and rows.is_cuda and t16 is not None and isinstance(up, torch.nn.ConvTranspose2d)
            and up.kernel_size == (2, 2) and up.stride == (2, 2) and up.padding == (0, 0) and up.output_padding == (0, 0)
            and up.groups == 1 and up.dilation == (1, 1) and wt.dtype == torch.float32 and rows.dim() == 3
            and rows.shape[1] == h * w and rows.shape[2] == wt.shape[0] and w % 8 == 0 and wt.shape[0] % 8 == 0
            and wt.shape[1] % 8 == 0 and rows.dtype in (torch.float32, t16) and rows.numel() > 0
            and (addend is None or (addend.dtype == t16 and tuple(addend.shape) == (rows.shape[0], wt.shape[1], 2 * h, 2 * w)))):
        return _UpFromTokens.apply(rows, wt, h, w, addend, t16)
    return None


def patch_embed(conv, x):
    """``conv(x).flatten(2).transpose(1, 2)`` for the patch embedding (Conv2d with kernel = stride, base/vit.py:169-190)
    as ONE GEMM on bf16 patch rows - no im2col / NCHW transposes; the rows come out in token order.  Returns
    (tokens (B, N, E) bf16, H/ps, W/ps) or None when the form does not apply (input gradient wanted, other geometry)."""
    w = conv.weight
    ps = conv.kernel_size[0]
    if (ENABLED['patch_gemm'] and ENABLED['linear'] and x.is_cuda and x.dtype == torch.float32 and not x.requires_grad
            and _bf16_autocast() and x.dim() == 4 and isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (ps, ps)
            and conv.stride == (ps, ps) and conv.padding == (0, 0) and conv.groups == 1 and conv.dilation == (1, 1)
            and ps % 8 == 0 and x.shape[2] % ps == 0 and x.shape[3] % ps == 0 and w.dtype == torch.float32
            and w.shape[0] % 8 == 0 and x.numel() > 0):
        B, C, H, W = x.shape
        x = x.contiguous()
        rows = torch.empty((B * (H // ps) * (W // ps), C * ps * ps), dtype=torch.bfloat16, device=x.device)
        with _vah.on(x.device):
            _vah.check(_vah.lib.vah_patchify_bf16(x.data_ptr(), B, C, H, W, ps, rows.data_ptr(), _stream(x)), 'patchify')
        y = _LinearBF16.apply(rows, w.view(w.shape[0], -1), conv.bias)
        return y.view(B, (H // ps) * (W // ps), w.shape[0]), H // ps, W // ps
    return None


def conv1x1(conv, x):
    """``F.conv2d(x, conv.weight, None)`` for a 1x1 nn.Conv2d (the SPM's fc1..fc4 without their bias,
    which the callers fold into the ops that follow)."""
    w = conv.weight
    if (ENABLED['conv1x1'] and ENABLED['linear'] and x.is_cuda and x.dtype == torch.bfloat16 and _bf16_autocast()
            and x.dim() == 4 and w.dtype == torch.float32 and w.shape[2:] == (1, 1) and conv.stride == (1, 1)
            and conv.padding == (0, 0) and conv.groups == 1 and w.shape[0] % 8 == 0 and w.shape[1] % 8 == 0
            and (x.shape[2] * x.shape[3]) % 8 == 0 and x.numel() > 0):
        return _Conv1x1BF16.apply(x, w)
    return F.conv2d(x, w, None)


def linear(lin, x):
    """``lin(x)`` for an nn.Linear (reference: every nn.Linear of base/vit.py, adapter_modules.py
    and ms_deform_attn.py)."""
    w = lin.weight
    t16 = autocast_16('fp16_linear')
    if (ENABLED['linear'] and x.is_cuda and t16 is not None and w.dtype == torch.float32
            and x.dtype in (t16, torch.float32) and w.shape[0] % 8 == 0
            and w.shape[1] % 8 == 0 and x.numel() > 0 and type(lin) is torch.nn.Linear):
        return BIAS_PARTIALS.mark(_LinearBF16.apply(x, w, lin.bias, t16), lin.bias)
    return lin(x)


class _GeluBF16(torch.autograd.Function):
    """Exact GELU on the 16-bit (bf16 or fp16: taken from h) output of a fused Linear: torch's forward kernel; the backward is one kernel that writes
    dh and the partial column sums of dh - the Linear's bias gradient (_BiasPartials)."""

    @staticmethod
    def forward(ctx, h):
        ctx.save_for_backward(h)
        return F.gelu(h)

    @staticmethod
    def backward(ctx, da):
        (h,) = ctx.saved_tensors
        C = h.shape[-1]
        hc = h.contiguous()
        da = da.contiguous().to(h.dtype)
        dh = torch.empty(h.shape, dtype=h.dtype, device=h.device)
        bpart, nparts = _bias_partials_out(C, h.device)
        import ctypes
        with _vah.on(h.device):
            _vah.call('vah_gelu_bwd_bsum_bf16', h.dtype, da.data_ptr(), hc.data_ptr(), h.numel() // C, C, dh.data_ptr(), bpart.data_ptr(),
                      ctypes.byref(nparts), _stream(h))
        BIAS_PARTIALS.record(dh, bpart, nparts.value)
        return dh


def gelu(act, h):
    """``act(h)`` for the activation between two Linears (base/vit.py Mlp): an exact nn.GELU on the marked 16-bit output
    of a fused Linear under bf16 (or, ENABLED['fp16_linear'], fp16) autocast takes the backward kernel that also sums fc1's bias gradient."""
    if (isinstance(act, torch.nn.GELU) and act.approximate == 'none' and h.is_cuda and autocast_16('fp16_linear') is not None
            and BIAS_PARTIALS.wanted(h) and h.numel() > 0 and h.requires_grad and torch.is_grad_enabled()):
        return _GeluBF16.apply(h)
    return act(h)


def _scale_residual_bwd(g, z, gp, s, dims, bias_partials):
    """(dz, dgamma) of y = x + s * gamma * z for the contiguous fp32 gradient g of y; with ``bias_partials`` the kernel
    also leaves the partial column sums of dz for the Linear that made z (_BiasPartials)."""
    import ctypes
    B, rpb, C = dims
    dz = torch.empty_like(z)
    dgamma = torch.empty(C, dtype=torch.float32, device=g.device) if gp is not None else None
    ws = _scratch(C, g.device) if gp is not None else None
    args = (g.data_ptr(), z.data_ptr(), gp.data_ptr() if gp is not None else None,
            s.data_ptr() if s is not None else None, B, rpb, C, dz.data_ptr(),
            dgamma.data_ptr() if dgamma is not None else None, ws.data_ptr() if ws is not None else None)
    with _vah.on(g.device):
        if bias_partials:
            bpart, nparts = _bias_partials_out(C, g.device)
            _vah.call('vah_scale_residual_bwd_bsum', z.dtype, *args, bpart.data_ptr(), ctypes.byref(nparts), _stream(g))
            BIAS_PARTIALS.record(dz, bpart, nparts.value)
        else:
            _vah.call('vah_scale_residual_bwd', z.dtype, *args, _stream(g))
    return dz, dgamma


class _ScaleResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, z, gamma, s, bias_partials=False):
        B, C = x.shape[0], x.shape[-1]
        rpb = x.numel() // (B * C)
        x, z = x.contiguous(), z.contiguous()
        y = torch.empty_like(x)
        gp = gamma.contiguous() if gamma is not None else None
        with _vah.on(x.device):
            _vah.call('vah_scale_residual_fwd', z.dtype, x.data_ptr(), z.data_ptr(), gp.data_ptr() if gp is not None else None,
                      s.data_ptr() if s is not None else None, B, rpb, C, y.data_ptr(), _stream(x))
        ctx.save_for_backward(z, gp, s)
        ctx.dims = (B, rpb, C)
        ctx.bias_partials = bias_partials
        return y

    @staticmethod
    def backward(ctx, g):
        z, gp, s = ctx.saved_tensors
        g = g.contiguous()
        dz, dgamma = _scale_residual_bwd(g, z, gp, s, ctx.dims, ctx.bias_partials)
        return g, dz, dgamma, None, None


def residual(x, z, gamma=None, drop_path=None):
    """``x + drop_path(gamma * z)`` (gamma / drop_path optional), the residual update of the
    reference's Block / Injector / Extractor."""
    prob = float(getattr(drop_path, 'drop_prob', 0.) or 0.)
    training = bool(getattr(drop_path, 'training', False))
    if (ENABLED['residual'] and x.is_cuda and x.dtype == torch.float32 and takes_16(z.dtype, 'fp16_rows')
            and x.shape == z.shape and x.shape[-1] % 4 == 0 and x.numel() > 0
            and (gamma is None or gamma.dtype == torch.float32)):
        s = None
        if prob > 0. and training:
            s = DROP_POOL.take(x, 1.0 - prob)
        return _ScaleResidual.apply(x, z, gamma, s, BIAS_PARTIALS.wanted(z))
    t = gamma * z if gamma is not None else z
    return x + (drop_path(t) if drop_path is not None else t)


class _ResidualLN(torch.autograd.Function):
    """(t, h) = (x + s * gamma * z, LayerNorm(t)) in one pass; the backward sums the gradient of t
    along the residual stream and through the LayerNorm in-kernel and emits dz, dgamma with it."""

    @staticmethod
    def forward(ctx, x, z, gamma, s, weight, bias, eps, bias_partials=False):
        B, C = x.shape[0], x.shape[-1]
        rpb = x.numel() // (B * C)
        x, z = x.contiguous(), z.contiguous()
        t = torch.empty_like(x)
        h = torch.empty(x.shape, dtype=z.dtype, device=x.device)       # the LayerNorm writes z's type (residual_ln checks)
        rows = B * rpb
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        gp = gamma.contiguous() if gamma is not None else None
        w, b = weight.contiguous(), bias.contiguous()
        with _vah.on(x.device):
            _vah.call('vah_residual_layernorm_fwd', z.dtype, x.data_ptr(), z.data_ptr(), gp.data_ptr() if gp is not None else None,
                      s.data_ptr() if s is not None else None, B, rpb, C, w.data_ptr(), b.data_ptr(), float(eps), t.data_ptr(), h.data_ptr(),
                      mean.data_ptr(), rstd.data_ptr(), _stream(x))
        ctx.save_for_backward(t, z, gp, s, w, mean, rstd)
        ctx.dims = (B, rpb, C)
        ctx.bias_partials = bias_partials      # residual_ln asks only without a gamma
        ctx.set_materialize_grads(False)
        return t, h

    @staticmethod
    def backward(ctx, gt, gh):
        t, z, gp, s, w, mean, rstd = ctx.saved_tensors
        B, rpb, C = ctx.dims
        dev = t.device
        if gt is not None:
            gt = gt.contiguous().float()
        if gh is None:                       # the normalised copy was not used: plain residual backward
            if gt is None:
                return (None,) * 8
            dz, dgamma = _scale_residual_bwd(gt, z, gp, s, ctx.dims, ctx.bias_partials)
            return gt, dz, dgamma, None, None, None, None, None
        gh = gh.contiguous().to(z.dtype)
        dt = torch.empty_like(t)
        dz = torch.empty_like(z)
        grads = torch.empty(3, C, dtype=torch.float32, device=dev)
        ws = _scratch(3 * C, dev)
        args = (t.data_ptr(), gh.data_ptr(), w.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                gt.data_ptr() if gt is not None else None, z.data_ptr(),
                gp.data_ptr() if gp is not None else None, s.data_ptr() if s is not None else None, B, rpb, C,
                dt.data_ptr(), dz.data_ptr(), grads[2].data_ptr() if gp is not None else None,
                grads[0].data_ptr(), grads[1].data_ptr(), ws.data_ptr())
        with _vah.on(dev):
            if ctx.bias_partials and gp is None:
                import ctypes
                bpart, nparts = _bias_partials_out(C, dev)
                _vah.call('vah_residual_layernorm_bwd_bsum', z.dtype, *args, bpart.data_ptr(), ctypes.byref(nparts), _stream(t))
                BIAS_PARTIALS.record(dz, bpart, nparts.value)
            else:
                _vah.call('vah_residual_layernorm_bwd', z.dtype, *args, _stream(t))
        return dt, dz, grads[2] if gp is not None else None, None, grads[0], grads[1], None, None


def _drop_path_scale(x, drop_path):
    prob = float(getattr(drop_path, 'drop_prob', 0.) or 0.)
    if prob > 0. and bool(getattr(drop_path, 'training', False)):
        return DROP_POOL.take(x, 1.0 - prob)
    return None


def residual_ln(x, z, gamma, drop_path, norm):
    """``t = x + drop_path(gamma * z); return t, norm(t)`` - a residual update followed by the
    LayerNorm of the next sub-block (base/vit.py:301-306), one pass over the rows each way."""
    # z in the type the LayerNorm will write: a bf16 z under fp16 autocast (or the reverse) takes the torch expression
    if (ENABLED['residual'] and ENABLED['residual_ln'] and _ln_fusable(norm, x) and z.dtype == autocast_16('fp16_rows')
            and x.shape == z.shape
            and x.dim() >= 2 and (gamma is None or gamma.dtype == torch.float32) and x.shape[-1] <= 1024):
        return _ResidualLN.apply(x, z, gamma, _drop_path_scale(x, drop_path), norm.weight, norm.bias, norm.eps,
                                 gamma is None and BIAS_PARTIALS.wanted(z))
    ac = autocast_16('fp16_rows')
    if ENABLED['fp16_rows'] and ac is not None and z.dtype != ac and z.dtype in (torch.bfloat16, torch.float16):
        # a branch output in the other 16-bit type than the one autocast is running: the torch expression, nothing fused
        t = gamma * z if gamma is not None else z
        t = x + (drop_path(t) if drop_path is not None else t)
        return t, norm(t)
    return layer_norm_keep(norm, residual(x, z, gamma, drop_path))


class _DWConvTokens(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, H, W):
        B, N, C = x.shape
        x = x.contiguous()
        w = weight.detach().float().contiguous()
        b = bias.detach().float().contiguous() if bias is not None else None
        y = torch.empty_like(x)
        with _vah.on(x.device):
            _vah.call('vah_dwconv3x3_tokens_bf16', x.dtype, x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None, B, H, W, C, 0,
                      y.data_ptr(), _stream(x))
        ctx.save_for_backward(x, w)
        ctx.dims = (B, H, W, C, bias is not None, weight.dtype)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        B, H, W, C, has_bias, wdtype = ctx.dims
        g = g.contiguous().to(x.dtype)
        dx = torch.empty_like(x)
        dw = torch.empty(C * 9 + C, dtype=torch.float32, device=x.device)
        ws = _scratch(10 * C, x.device)
        with _vah.on(x.device):
            _vah.call('vah_dwconv3x3_tokens_bf16', x.dtype, g.data_ptr(), w.data_ptr(), None, B, H, W, C, 1, dx.data_ptr(), _stream(x))
            _vah.call('vah_dwconv3x3_tokens_wgrad_bf16', x.dtype, x.data_ptr(), g.data_ptr(), B, H, W, C, dw.data_ptr(),
                      dw[C * 9:].data_ptr() if has_bias else None, ws.data_ptr(), _stream(x))
        return (dx, dw[:C * 9].view(C, 1, 3, 3).to(wdtype),
                dw[C * 9:].to(wdtype) if has_bias else None, None, None)


def dwconv_tokens(conv, x, H, W):
    """ConvFFN's DWConv on the concatenated token maps; None when the fused path does not apply."""
    B, N, C = x.shape
    if (ENABLED['dwconv'] and x.is_cuda and takes_16(x.dtype, 'fp16_rows') and C % 4 == 0 and C <= 1024
            and H % 2 == 0 and W % 2 == 0 and N == 21 * (H // 2) * (W // 2) and x.numel() > 0
            and conv.weight.shape == (C, 1, 3, 3)):
        return _DWConvTokens.apply(x, conv.weight, conv.bias, H, W)
    return None


# ---------------------------------------------------------------------------------------
# output tail: BatchNorm(a + b + bilinear_upsample(x))
# ---------------------------------------------------------------------------------------
def _sync_group(norm):
    """Process group whose ranks share the statistics of a SyncBatchNorm in training (None: local)."""
    import torch.distributed as dist
    if not isinstance(norm, torch.nn.SyncBatchNorm) or not dist.is_available() or not dist.is_initialized():
        return None
    group = norm.process_group if norm.process_group is not None else dist.group.WORLD
    if dist.get_world_size(group) > 1:
        return group
    from . import data_parallel
    return group if data_parallel.one_rank_group() else None        # one rank: the collectives run only on request


def bn_finalize(norm, sums, C, count, group, st):
    """Training-mode BatchNorm between its statistics pass and its normalise pass: ``sums`` = [sum (C) | sum of squares
    (C) | slot for the element count] -> (mean, rstd, the count as the 1-element tensor the backward divides by), running
    statistics and num_batches_tracked updated.  Without a process group this is ONE launch (vah_bn_finalize_stats_book:
    the count is stored and the counter advanced by the kernel that makes mean and rstd); with one the count must be in
    ``sums`` before the all-reduce, and fill, all-reduce, finalize and the counter's add are separate steps.  The caller
    has made the tensors' device current."""
    dev = sums.device
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    rstd = torch.empty(C, dtype=torch.float32, device=dev)
    track = norm.running_mean is not None
    rm = norm.running_mean.data_ptr() if track else None
    rv = norm.running_var.data_ptr() if track else None
    nbt = norm.num_batches_tracked if track else None
    if (group is None and ENABLED['epoch_copies']
            and (nbt is None or (nbt.dtype == torch.int64 and nbt.device == dev and nbt.numel() == 1))):
        _vah.check(_vah.lib.vah_bn_finalize_stats_book(
            sums.data_ptr(), C, float(count), float(norm.eps), float(norm.momentum), rm, rv, mean.data_ptr(), rstd.data_ptr(),
            nbt.data_ptr() if nbt is not None else None, st), 'bn_finalize_stats_book')
        return mean, rstd, sums[2 * C:]
    sums[2 * C:].fill_(float(count))
    if group is not None:
        import torch.distributed as dist
        dist.all_reduce(sums, group=group)
    _vah.check(_vah.lib.vah_bn_finalize_stats(sums.data_ptr(), C, float(norm.eps), float(norm.momentum), rm, rv, mean.data_ptr(),
                                              rstd.data_ptr(), st), 'bn_finalize_stats')
    if nbt is not None:
        with torch.no_grad():
            norm.num_batches_tracked += 1
    return mean, rstd, sums[2 * C:]


class _BNTail(torch.autograd.Function):
    """y = [relu] BatchNorm(a + b + upsample(x)): statistics pass, one bookkeeping launch (mean, rstd,
    running statistics), normalise pass; SyncBatchNorm all-reduces the sums in between.  ``t16``: the 16-bit type of
    the call (bf16 | fp16) - it picks the entry points, and an operand is either of that type or fp32."""

    @staticmethod
    def forward(ctx, a, b, x, weight, bias, shift, norm, scale, relu, out_dtype, t16):
        N, C, H, W = a.shape
        sh = shift.detach().float().contiguous() if shift is not None else None
        shp = sh.data_ptr() if sh is not None else None
        a = a.contiguous()
        b = b.contiguous() if b is not None else None
        x = x.contiguous().float() if x is not None else None
        dev, st = a.device, _stream(a)
        ops = (a.data_ptr(), int(a.dtype == t16), b.data_ptr() if b is not None else None,
               int(b is not None and b.dtype == t16), x.data_ptr() if x is not None else None,
               scale, N, C, H, W)
        training = norm.training or norm.running_mean is None
        group = _sync_group(norm) if training else None
        w = weight.detach().float().contiguous() if weight is not None else None
        bb = bias.detach().float().contiguous() if bias is not None else None
        with _vah.on(dev):
            if training:
                sums = torch.empty(2 * C + 1, dtype=torch.float32, device=dev)
                ws = torch.empty(_vah.lib.vah_bn_tail_ws_floats(C), dtype=torch.float32, device=dev)
                _vah.call('vah_bn_tail_stats', t16, *ops, shp, sums.data_ptr(), ws.data_ptr(), st)
                mean, rstd, count = bn_finalize(norm, sums, C, N * H * W, group, st)
            else:
                count = None
                mean = norm.running_mean.float().contiguous()
                rstd = torch.rsqrt(norm.running_var.float() + norm.eps)
            y = torch.empty((N, C, H, W), dtype=out_dtype, device=dev)
            _vah.call('vah_bn_tail_apply', t16, *ops, mean.data_ptr(), rstd.data_ptr(), w.data_ptr() if w is not None else None,
                      bb.data_ptr() if bb is not None else None, int(relu), shp, y.data_ptr(), int(out_dtype == t16), st)
        ctx.save_for_backward(a, b, x, mean, rstd, w, bb, count, sh)
        ctx.meta = (scale, training, group, weight is not None, bias is not None, relu, t16)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, b, x, mean, rstd, w, bb, count, sh = ctx.saved_tensors
        scale, training, group, has_w, has_b, relu, t16 = ctx.meta
        shp = sh.data_ptr() if sh is not None else None
        N, C, H, W = a.shape
        dy = dy.contiguous()
        if dy.dtype not in (torch.float32, t16):
            dy = dy.float()
        dy_bf16 = int(dy.dtype == t16)      # "16-bit (t16) or fp32", as the entry points read the flag
        dev, st = a.device, _stream(a)
        ops = (a.data_ptr(), int(a.dtype == t16), b.data_ptr() if b is not None else None,
               int(b is not None and b.dtype == t16), x.data_ptr() if x is not None else None,
               scale, N, C, H, W)
        wp = w.data_ptr() if w is not None else None
        bp = bb.data_ptr() if bb is not None else None
        with _vah.on(dev):
            sums = torch.empty(2 * C, dtype=torch.float32, device=dev)
            ws = torch.empty(_vah.lib.vah_bn_tail_ws_floats(C), dtype=torch.float32, device=dev)
            _vah.call('vah_bn_tail_bwd_stats', t16, *ops, mean.data_ptr(), rstd.data_ptr(), wp, bp, int(relu), shp, dy.data_ptr(), dy_bf16,
                      sums.data_ptr(), ws.data_ptr(), st)
            local = sums.clone() if (training and group is not None) else sums      # dweight / dbias are per-rank sums
            dweight = local[C:] if has_w else None
            dbias = local[:C] if has_b else None
            if training:
                if group is not None:
                    import torch.distributed as dist
                    dist.all_reduce(sums, group=group)
                means = sums / count
            else:
                means = torch.zeros_like(sums)          # running statistics are constants
            need_a, need_b, need_x = ctx.needs_input_grad[:3]
            da = torch.empty_like(a) if need_a else None
            db = torch.empty_like(b) if (b is not None and need_b) else None
            dx = None
            if x is not None and need_x:
                dx = torch.zeros_like(x) if scale > 1 else torch.empty_like(x)
            if da is not None or db is not None or dx is not None:
                _vah.call('vah_bn_tail_bwd_apply', t16, *ops, mean.data_ptr(), rstd.data_ptr(), wp, bp, int(relu), shp, dy.data_ptr(), dy_bf16,
                          means[:C].data_ptr(), means[C:].data_ptr(), da.data_ptr() if da is not None else None,
                          db.data_ptr() if db is not None else None, dx.data_ptr() if dx is not None else None, st)
        dshift = None
        if sh is not None and ctx.needs_input_grad[5]:
            # d/d(shift) = sum of dt over the channel: BatchNorm in training removes channel constants
            # (exactly 0); with running statistics it is gamma * rstd * sum(dy)
            dshift = torch.zeros_like(sh) if training else (w if w is not None else 1.0) * rstd * local[:C]
        return da, db, dx, dweight, dbias, dshift, None, None, None, None, None


def _bn_fusable(norm, a):
    """bf16 autocast, or fp16 autocast with ENABLED['fp16_tail']; ``a`` in the autocast's 16-bit type or fp32 (a tensor
    of the other 16-bit type takes the reference expression, nothing fused)."""
    t16 = autocast_16('fp16_tail')
    return (isinstance(norm, torch.nn.modules.batchnorm._BatchNorm) and a.is_cuda and t16 is not None
            and a.dim() == 4 and a.dtype in (t16, torch.float32) and a.shape[3] <= 8192
            and a.numel() > 0 and norm.momentum is not None
            and (not norm.training or a.shape[0] * a.shape[2] * a.shape[3] > 1)
            and (norm.training or norm.running_mean is not None)
            and (norm.weight is None or norm.weight.dtype == torch.float32))


def _tail_shape_ok(a, scale, has_x):
    """the shape rule of the four vah_bn_tail_* entry points (batch and LDS-tile limits included): what they refuse
    takes the reference expression"""
    N, C, H, W = a.shape
    return bool(_vah.lib.vah_bn_tail_supported(N, C, H, W, scale, int(has_x)))


def tail_takes_conv_bias(norm, ref):
    """True when bn_tail will run fused for inputs like ``ref``: the caller may then run the
    convolutions that feed it WITHOUT bias and hand the biases to bn_tail as ``shift``."""
    return ENABLED['bn_tail'] and ENABLED['bias_fold'] and _bn_fusable(norm, ref)


def halve(x):
    """``F.interpolate(x, scale_factor=0.5, mode='bilinear', align_corners=False)`` (vit_adapter.py:121).
    With even H, W the taps are (0.5, 0.5) in both directions: the 2x2 mean.  torch's bilinear
    kernel parallelises over output pixels only (706 us for 2x768x32x32 on MI355X); on the bf16 (and,
    ENABLED['fp16_tail'], fp16) GPU path the mean is taken with avg_pool2d, elsewhere the reference call is kept."""
    if (ENABLED['bn_tail'] and x.is_cuda and autocast_16('fp16_tail') is not None and x.dim() == 4 and x.shape[2] % 2 == 0
            and x.shape[3] % 2 == 0):
        return F.avg_pool2d(x.float(), 2)
    return F.interpolate(x, scale_factor=0.5, mode='bilinear', align_corners=False)


def bn_tail(norm, a, b=None, x=None, scale=1, shift=None):
    """``norm(a + b + F.interpolate(x, scale_factor=scale, mode='bilinear', align_corners=False))``
    for a (Sync)BatchNorm2d ``norm`` - the output tail of the backbone (ref vit_adapter.py:106-127);
    ``b`` / ``x`` optional, ``scale == 1`` adds ``x`` as it is.  ``shift`` (C,): per-channel constant
    added to the sum (biases of the convolutions that made ``a`` / ``b``, applied here for free)."""
    t16 = autocast_16('fp16_tail')
    if (ENABLED['bn_tail'] and _bn_fusable(norm, a) and x is not None
            and (b is None or (b.shape == a.shape and b.dtype in (t16, torch.float32)))
            and scale in (1, 2, 4, 8) and a.shape[3] % (4 * scale) == 0 and a.shape[2] % scale == 0
            and tuple(x.shape) == (a.shape[0], a.shape[1], a.shape[2] // scale, a.shape[3] // scale)
            and x.dtype in (t16, torch.float32) and _tail_shape_ok(a, scale, True)):
        return _BNTail.apply(a, b, x, norm.weight, norm.bias, shift, norm, scale, False, torch.float32, t16)
    t = a if b is None else a + b
    if shift is not None:
        t = t + shift.view(1, -1, 1, 1).to(t.dtype)
    if x is not None:
        t = t + (x if scale == 1 else F.interpolate(x, scale_factor=scale, mode='bilinear', align_corners=False))
    return norm(t)


BN_RELU_MIN_NUMEL = int(os.environ.get('VAH_BN_RELU_MIN_NUMEL', 8 << 20))


def bn_relu(norm, a):
    """``relu(norm(a))`` for the conv -> SyncBatchNorm -> ReLU triples of the SpatialPriorModule
    (adapter_modules.py:217-241): statistics pass + normalise-and-clamp pass, output in a's dtype;
    the backward recomputes the ReLU mask from ``a``."""
    # the two-pass form pays from a few million elements on (below that MIOpen's single kernel wins)
    if (ENABLED['bn_relu'] and _bn_fusable(norm, a) and a.shape[3] % 4 == 0 and a.numel() >= BN_RELU_MIN_NUMEL
            and _tail_shape_ok(a, 1, False)):
        return _BNTail.apply(a, None, None, norm.weight, norm.bias, None, norm, 1, True, a.dtype, autocast_16('fp16_tail'))
    return F.relu(norm(a))


# ---------------------------------------------------------------------------------------
# pyramid assembly: token sequences -> NCHW maps
# ---------------------------------------------------------------------------------------
class _TokensToMaps(torch.autograd.Function):
    """(B, T, C) fp32 tokens holding consecutive maps of sizes ``hw`` -> one (B, C, h, w) map each.
    Backward writes every map's gradient straight into its token range of ONE gradient tensor
    (autograd's route: per map a transposed copy, a zero-filled full-size gradient, a slice copy and
    an add)."""

    @staticmethod
    def forward(ctx, tokens, hw, t16):
        B, T, C = tokens.shape
        tokens = tokens.contiguous()
        outs, t0 = [], 0
        with _vah.on(tokens.device):
            for h, w in hw:
                o = torch.empty((B, C, h, w), dtype=torch.float32, device=tokens.device)
                _vah.call('vah_transpose_tokens', t16, tokens.data_ptr(), B, T, t0, h * w, C, o.data_ptr(), 1, 0, None, _stream(tokens))
                outs.append(o)
                t0 += h * w
        ctx.hw, ctx.shape, ctx.t16 = hw, (B, T, C), t16
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        B, T, C = ctx.shape
        dev = next(g.device for g in grads if g is not None)
        gt = torch.empty((B, T, C), dtype=torch.float32, device=dev)
        t0 = 0
        with _vah.on(dev):
            for (h, w), g in zip(ctx.hw, grads):
                if g is None:
                    gt[:, t0:t0 + h * w].zero_()
                else:
                    g = g.contiguous().float()
                    _vah.call('vah_transpose_tokens', ctx.t16, g.data_ptr(), B, T, t0, h * w, C, gt.data_ptr(), 0, 0, None, _stream(g))
                t0 += h * w
        return gt, None, None


def _maps_dtype():
    """The 16-bit type whose instantiation of the token <-> plane transposes serves the call: fp16 under fp16 autocast
    with ENABLED['fp16_tail'] (fp32 planes included, so that the step's profiler rows are all `_f16`), else bf16."""
    return torch.float16 if autocast_16('fp16_tail') == torch.float16 else torch.bfloat16


def tokens_to_maps(tokens, hw):
    """``[tokens[:, a:b].transpose(1, 2).reshape(B, C, h, w).contiguous() for the consecutive ranges]``
    (vit_adapter.py:113-119); ``hw``: list of (h, w) whose areas add up to the token count."""
    hw = tuple((int(h), int(w)) for h, w in hw)
    assert sum(h * w for h, w in hw) == tokens.shape[1]
    if (ENABLED['maps'] and tokens.is_cuda and tokens.dtype == torch.float32 and tokens.dim() == 3
            and tokens.numel() > 0 and tokens.shape[0] <= 65535):
        return list(_TokensToMaps.apply(tokens, hw, _maps_dtype()))
    outs, t0 = [], 0
    B, _, C = tokens.shape
    for h, w in hw:
        outs.append(tokens[:, t0:t0 + h * w].transpose(1, 2).reshape(B, C, h, w).contiguous())
        t0 += h * w
    return outs


class _MapsToTokens(torch.autograd.Function):
    """cat_l(map_l.flatten(2).transpose(1, 2) + vec_l) -> (B, sum T_l, C) fp32 in one pass per map; the
    backward hands each map its gradient already transposed (bf16 like the map) and the vectors the
    column sums of their token ranges."""

    @staticmethod
    def forward(ctx, t16, *args):
        n = len(args) // 2
        maps, vecs = args[:n], args[n:]
        B, C = maps[0].shape[:2]
        hw = [(m.shape[2], m.shape[3]) for m in maps]
        T = sum(h * w for h, w in hw)
        dev = maps[0].device
        out = torch.empty((B, T, C), dtype=torch.float32, device=dev)
        t0 = 0
        with _vah.on(dev):
            for m, v, (h, w) in zip(maps, vecs, hw):
                m = m.contiguous()
                vv = v.detach().float().contiguous() if v is not None else None
                _vah.call('vah_transpose_tokens', t16, m.data_ptr(), B, T, t0, h * w, C, out.data_ptr(), 0, int(m.dtype == t16),
                          vv.data_ptr() if vv is not None else None, _stream(m))
                t0 += h * w
        ctx.meta = (hw, [m.dtype for m in maps], [v is not None for v in vecs], (B, T, C), t16)
        return out

    @staticmethod
    def backward(ctx, g):
        hw, dts, has_vec, (B, T, C), t16 = ctx.meta
        g = g.contiguous().float()
        gmaps, gvecs, t0 = [], [], 0
        with _vah.on(g.device):
            for (h, w), dt, hv in zip(hw, dts, has_vec):
                gm = torch.empty((B, C, h, w), dtype=dt, device=g.device)
                _vah.call('vah_transpose_tokens', t16, g.data_ptr(), B, T, t0, h * w, C, gm.data_ptr(), 1, int(dt == t16), None, _stream(g))
                gmaps.append(gm)
                gv = None
                if hv and C % 4 == 0:
                    gv = torch.empty(C, dtype=torch.float32, device=g.device)
                    ws = _scratch(C, g.device)
                    _vah.check(_vah.lib.vah_colsum_f32(g[:, t0:].data_ptr(), B, T * C, h * w, C, gv.data_ptr(),
                                                       ws.data_ptr(), _stream(g)), 'colsum_f32')
                elif hv:
                    gv = g[:, t0:t0 + h * w].sum((0, 1))
                gvecs.append(gv)
                t0 += h * w
        return (None, *gmaps, *gvecs)


def maps_to_tokens(maps, vecs):
    """``torch.cat([m.flatten(2).transpose(1, 2) + v for m, v in zip(maps, vecs)], dim=1)`` in fp32
    (the SPM's c2..c4 maps with their conv bias + level embedding, vit_adapter.py:94-97)."""
    t16 = _maps_dtype()       # fp16 maps under fp16 autocast (ENABLED['fp16_tail']); maps of the other 16-bit type: reference
    if (ENABLED['maps'] and maps[0].is_cuda and all(m.dim() == 4 and m.dtype in (t16, torch.float32)
                                                    and m.shape[:2] == maps[0].shape[:2] for m in maps)
            and maps[0].numel() > 0 and maps[0].shape[0] <= 65535):
        return _MapsToTokens.apply(t16, *maps, *vecs)
    return torch.cat([m.flatten(2).transpose(1, 2).float() + (v if v is not None else 0.) for m, v in zip(maps, vecs)], dim=1)


class _MaxPool3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        N, C, H, W = x.shape
        x = x.contiguous()
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((N, C, Ho, Wo), dtype=x.dtype, device=x.device)
        idx = torch.empty((N, C, Ho, Wo), dtype=torch.uint8, device=x.device)
        with _vah.on(x.device):
            _vah.call('vah_maxpool3s2_fwd_bf16', x.dtype, x.data_ptr(), N * C, H, W, y.data_ptr(), idx.data_ptr(), _stream(x))
        ctx.save_for_backward(idx)
        ctx.shape, ctx.t16 = (N, C, H, W), x.dtype
        return y

    @staticmethod
    def backward(ctx, gy):
        (idx,) = ctx.saved_tensors
        N, C, H, W = ctx.shape
        gy = gy.contiguous().to(ctx.t16)
        gx = torch.empty((N, C, H, W), dtype=ctx.t16, device=gy.device)
        with _vah.on(gy.device):
            _vah.call('vah_maxpool3s2_bwd_bf16', ctx.t16, gy.data_ptr(), idx.data_ptr(), N * C, H, W, gx.data_ptr(), _stream(gy))
        return gx


def max_pool(pool, x):
    """``pool(x)`` for the SPM stem's nn.MaxPool2d(kernel_size=3, stride=2, padding=1) on bf16 or (ENABLED['fp16_tail'])
    fp16 NCHW input."""
    def _is(v, k):
        return v == k or v == (k, k)
    if (ENABLED['maxpool'] and x.is_cuda and takes_16(x.dtype, 'fp16_tail')
            and x.dim() == 4 and x.numel() > 0
            and isinstance(pool, torch.nn.MaxPool2d) and _is(pool.kernel_size, 3) and _is(pool.stride, 2)
            and _is(pool.padding, 1) and _is(pool.dilation, 1) and not pool.ceil_mode and not pool.return_indices):
        return _MaxPool3s2.apply(x)
    return pool(x)



_GN_CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _gn_rows_ok(t):
    """Is ``t`` (N, T, C) a channels-last rows tensor the GroupNorm kernels address directly: contiguous channels,
    16-byte aligned, strides in multiples of 8 elements?  A contiguous tensor is, and so is a level's row range of an
    (Lq, N, C) buffer seen as (N, T, C)."""
    N, T, C = t.shape
    return (t.stride(2) == 1 and t.data_ptr() % 16 == 0 and (N == 1 or t.stride(0) % 8 == 0)
            and (T == 1 or (t.stride(1) % 8 == 0 and t.stride(1) >= C)))


def _gn_arg(t):
    """(pointer, dtype code, row stride, image stride) of a rows tensor"""
    N, T, C = t.shape
    return t.data_ptr(), _GN_CODES[t.dtype], (t.stride(1) if T > 1 else C), (t.stride(0) if N > 1 else 0)


class _GroupNorm(torch.autograd.Function):
    """GroupNorm (+ ReLU, + addend) over channels-last rows (N, T, C) on csrc/group_norm.hip: fp32 statistics per (image,
    group), one rounding at the store.  ``out``: a rows view to write into (modified in place: it is the first argument,
    as autograd's bookkeeping of an in-place change to a view asks) or None.  The backward recomputes the ReLU mask from
    x; it returns fp32 dgamma / dbeta and dx in x's dtype; the gradient of the addend is dy itself."""

    @staticmethod
    def forward(ctx, out, x, weight, bias, G, eps, relu, add, ydt):
        N, T, C = x.shape
        dev, st, lib = x.device, _stream(x), _vah.lib
        w = weight.detach().float().contiguous() if weight is not None else None
        b = bias.detach().float().contiguous() if bias is not None else None
        mean = torch.empty(N * G, dtype=torch.float32, device=dev)
        rstd = torch.empty(N * G, dtype=torch.float32, device=dev)
        nws = lib.vah_group_norm_ws_floats(N, T, C, G)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        y = out if out is not None else torch.empty((N, T, C), dtype=ydt, device=dev)
        with _vah.on(dev):
            _vah.check(lib.vah_group_norm_stats(*_gn_arg(x), N, T, C, G, eps, mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), nws, st),
                       'vah_group_norm_stats')
            _vah.check(lib.vah_group_norm_apply(*_gn_arg(x), N, T, C, G, mean.data_ptr(), rstd.data_ptr(),
                                                w.data_ptr() if w is not None else None, b.data_ptr() if b is not None else None,
                                                int(relu), add.data_ptr() if add is not None else None, *_gn_arg(y), st),
                       'vah_group_norm_apply')
        ctx.save_for_backward(x, mean, rstd, w, b)
        ctx.meta = (G, relu, weight is not None, bias is not None, out is not None, add is not None)
        if out is not None:
            ctx.mark_dirty(out)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, w, b = ctx.saved_tensors
        G, relu, has_w, has_b, has_out, has_add = ctx.meta
        N, T, C = x.shape
        dev, st, lib = x.device, _stream(x), _vah.lib
        if dy.dtype not in _GN_CODES or (dy.dtype != torch.float32 and x.dtype != torch.float32 and dy.dtype != x.dtype):
            dy = dy.to(x.dtype)
        if not _gn_rows_ok(dy):
            dy = dy.contiguous()
        wp = w.data_ptr() if w is not None else None
        bp = b.data_ptr() if b is not None else None
        gsums = torch.empty(2 * N * G, dtype=torch.float32, device=dev)
        dgamma = torch.empty(C, dtype=torch.float32, device=dev) if has_w else None
        dbeta = torch.empty(C, dtype=torch.float32, device=dev) if has_b else None
        nws = lib.vah_group_norm_ws_floats(N, T, C, G)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        dx = None
        with _vah.on(dev):
            _vah.check(lib.vah_group_norm_bwd_stats(*_gn_arg(x), *_gn_arg(dy), N, T, C, G, mean.data_ptr(), rstd.data_ptr(), wp, bp,
                                                    int(relu), gsums.data_ptr(), dgamma.data_ptr() if has_w else None,
                                                    dbeta.data_ptr() if has_b else None, ws.data_ptr(), nws, st),
                       'vah_group_norm_bwd_stats')
            if ctx.needs_input_grad[1]:
                dx = torch.empty((N, T, C), dtype=x.dtype, device=dev)
                _vah.check(lib.vah_group_norm_bwd_apply(*_gn_arg(x), *_gn_arg(dy), N, T, C, G, mean.data_ptr(), rstd.data_ptr(), wp, bp,
                                                        int(relu), gsums.data_ptr(), *_gn_arg(dx), st), 'vah_group_norm_bwd_apply')
        # `out` was overwritten: its old contents have gradient zero.  Autograd wants a tensor here, not None, to keep the
        # chain through the buffer the view belongs to: one zero, expanded - nothing of dy's size is allocated or filled
        return (dy.new_zeros(()).expand_as(dy) if has_out else None, dx, dgamma, dbeta, None, None, None,
                dy if has_add and ctx.needs_input_grad[7] else None, None)


def group_norm(norm, x, relu=False, add=None, out=None, out_dtype=None):
    """``[relu](norm(x)) [+ add]`` for an nn.GroupNorm on channels-last rows: x (N, T, C) with contiguous channels - an
    NHWC map with its pixels flattened, or a level's rows of an (Lq, N, C) buffer seen as (N, T, C).  ``add``: (N, T, C)
    in the result's dtype.  ``out``: a rows view the result is written into and that is returned; else the result is a
    new (N, T, C) tensor of ``out_dtype`` (default: x's dtype).  The reference's ConvModule (conv -> GN -> ReLU) in the
    pixel decoder, msdeformattn_pixel_decoder.py:84-124.
    On the GPU, for the shapes vah_group_norm_supported serves and with ENABLED['group_norm'], this is csrc/group_norm.hip
    (fp32, bf16, and fp16 under ENABLED['fp16_rows']); otherwise F.group_norm on the (N, C, T) view."""
    N, T, C = x.shape
    G = norm.num_groups
    ydt = out.dtype if out is not None else (out_dtype or x.dtype)
    ok16 = [d == torch.float32 or takes_16(d, 'fp16_rows') for d in (x.dtype, ydt)]
    if (ENABLED['group_norm'] and x.is_cuda and x.numel() > 0 and all(ok16)
            and not (x.dtype != ydt and torch.float32 not in (x.dtype, ydt))
            and _vah.lib.vah_group_norm_supported(C, G) and (out is None or (out.shape == x.shape and _gn_rows_ok(out)))
            and (add is None or add.shape == x.shape)):
        if not _gn_rows_ok(x):
            x = x.contiguous()
        if add is not None:
            add = add.to(ydt).contiguous()
        return _GroupNorm.apply(out, x, norm.weight, norm.bias, G, float(norm.eps), bool(relu), add, ydt)
    y = F.group_norm(x.transpose(1, 2), G, norm.weight, norm.bias, norm.eps).transpose(1, 2)
    if relu:
        y = torch.relu(y)
    if add is not None:
        y = y + add
    if out is not None:
        out.copy_(y)
        return out
    return y.to(out_dtype or x.dtype)           # under autocast F.group_norm answers in fp32


class _ResizeBilinearRows(torch.autograd.Function):
    """Bilinear resize of channels-last rows (N, Hi * Wi, C) -> (N, Ho * Wo, C) on csrc/resize_rows.hip: fp32 arithmetic,
    one rounding at the store.  The backward is the exact transpose in gather form - a fixed order of additions, no
    atomics - and returns dx in x's dtype."""

    @staticmethod
    def forward(ctx, x, hw_in, hw_out, align_corners, ydt):
        N, _, C = x.shape
        (Hi, Wi), (Ho, Wo) = hw_in, hw_out
        dev, st, lib = x.device, _stream(x), _vah.lib
        nws = lib.vah_resize_rows_ws_bytes(Hi, Wi, Ho, Wo)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        y = torch.empty((N, Ho * Wo, C), dtype=ydt, device=dev)
        with _vah.on(dev):
            _vah.check(lib.vah_resize_rows_forward(*_gn_arg(x), N, C, Hi, Wi, Ho, Wo, int(align_corners), *_gn_arg(y),
                                                   ws.data_ptr(), nws, st), 'vah_resize_rows_forward')
        ctx.meta = (hw_in, hw_out, align_corners, x.dtype, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        (Hi, Wi), (Ho, Wo), align_corners, xdt, C = ctx.meta
        N = dy.shape[0]
        dev, st, lib = dy.device, _stream(dy), _vah.lib
        if dy.dtype not in _GN_CODES or (dy.dtype != torch.float32 and xdt != torch.float32 and dy.dtype != xdt):
            dy = dy.to(xdt)
        if not _gn_rows_ok(dy):
            dy = dy.contiguous()
        nws = lib.vah_resize_rows_ws_bytes(Hi, Wi, Ho, Wo)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        dx = torch.empty((N, Hi * Wi, C), dtype=xdt, device=dev)
        with _vah.on(dev):
            _vah.check(lib.vah_resize_rows_backward(*_gn_arg(dy), N, C, Hi, Wi, Ho, Wo, int(align_corners), *_gn_arg(dx),
                                                    ws.data_ptr(), nws, st), 'vah_resize_rows_backward')
        return dx, None, None, None, None


def resize_bilinear_rows(x, hw_in, hw_out, align_corners=False, out_dtype=None):
    """``F.interpolate(x as (N, C, Hi, Wi), size=hw_out, mode='bilinear', align_corners=align_corners)`` on channels-last
    rows: x (N, Hi * Wi, C) with contiguous channels - an NHWC map with its pixels flattened, or a level's rows of an
    (Lq, N, C) buffer seen as (N, T, C), read in place.  Returns a new contiguous (N, Ho * Wo, C) tensor of ``out_dtype``
    (default: x's dtype).  The reference's upsample of the FPN tail, msdeformattn_pixel_decoder.py:258-262.
    On the GPU, for C a multiple of 8 and with ENABLED['bilinear_rows'], this is csrc/resize_rows.hip (fp32, bf16, and fp16
    under ENABLED['fp16_rows']; not a change from one 16-bit type to the other), whose backward is deterministic;
    otherwise F.interpolate on the NCHW-shaped view, then ``.to(out_dtype)``."""
    N, T, C = x.shape
    (Hi, Wi), (Ho, Wo) = hw_in, hw_out
    assert T == Hi * Wi, (tuple(x.shape), hw_in)
    ydt = out_dtype or x.dtype
    ok16 = [d == torch.float32 or takes_16(d, 'fp16_rows') for d in (x.dtype, ydt)]
    if (ENABLED['bilinear_rows'] and x.is_cuda and x.numel() > 0 and Ho * Wo > 0 and C % 8 == 0 and all(ok16)
            and not (x.dtype != ydt and torch.float32 not in (x.dtype, ydt))):
        if not _gn_rows_ok(x):
            x = x.contiguous()
        return _ResizeBilinearRows.apply(x, (int(Hi), int(Wi)), (int(Ho), int(Wo)), bool(align_corners), ydt)
    y = F.interpolate(x.permute(0, 2, 1).reshape(N, C, Hi, Wi), size=(Ho, Wo), mode='bilinear', align_corners=align_corners)
    return y.permute(0, 2, 3, 1).reshape(N, Ho * Wo, C).to(ydt).contiguous()


def mca_pack_mask(mask_logits):
    """(N, Q, Lk) mask logits (fp32, bf16 or fp16, contiguous keys) -> (N, Q, ceil(Lk / 32)) keep-bits as int32 words on
    csrc/masked_attn.hip: key j is kept iff not (x < 0), a row that keeps nothing keeps everything
    (include/vitadapter_hip_masked_attn.h).  No gradient, nothing read back to the host."""
    x = mask_logits.detach()
    if x.dtype not in _GN_CODES:
        x = x.float()
    if x.stride(2) != 1:
        x = x.contiguous()
    N, Q, Lk = x.shape
    bits = torch.empty((N, Q, (Lk + 31) // 32), dtype=torch.int32, device=x.device)
    with _vah.on(x.device):
        _vah.check(_vah.lib.vah_mca_pack_mask(x.data_ptr(), _GN_CODES[x.dtype], x.stride(1), x.stride(0), N, Q, Lk, bits.data_ptr(),
                                              _stream(x)), 'vah_mca_pack_mask')
    return bits


def _mca_rows_ok(t):
    """(L, N, E) with contiguous channels, 16-byte aligned, strides in multiples of 8 elements"""
    return t.stride(2) == 1 and t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0


def _mca_arg(t):
    """(pointer, dtype code, token stride, image stride) of an (L, N, E) tensor"""
    return t.data_ptr(), _GN_CODES[t.dtype], t.stride(0), t.stride(1)


class _MaskedCrossAttention(torch.autograd.Function):
    """softmax(scale q k^T + (-inf where excluded)) v on csrc/masked_attn.hip: q (Lq, N, H * 32), k and v (Lk, N, H * 32) in
    one 16-bit type (strided forms are read in place), ``bits`` from mca_pack_mask.  Deterministic in both directions; no
    gradient for the mask."""

    @staticmethod
    def forward(ctx, q, k, v, bits, H, scale):
        q, k, v = (t if _mca_rows_ok(t) else t.contiguous() for t in (q, k, v))
        Lq, N, E = q.shape
        Lk = k.shape[0]
        dev, st, lib = q.device, _stream(q), _vah.lib
        nws = lib.vah_mca_ws_bytes(N, H, Lq, Lk)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        out = torch.empty((Lq, N, E), dtype=q.dtype, device=dev)
        lse = torch.empty((N, H, Lq), dtype=torch.float32, device=dev)
        with _vah.on(dev):
            _vah.check(lib.vah_mca_forward(*_mca_arg(q), *_mca_arg(k), *_mca_arg(v), bits.data_ptr(), N, H, Lq, Lk, E // H, scale,
                                           *_mca_arg(out), lse.data_ptr(), ws.data_ptr(), nws, st), 'vah_mca_forward')
        ctx.save_for_backward(q, k, v, bits, out, lse)
        ctx.meta = (H, scale)
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, k, v, bits, out, lse = ctx.saved_tensors
        H, scale = ctx.meta
        Lq, N, E = q.shape
        Lk = k.shape[0]
        dev, st, lib = q.device, _stream(q), _vah.lib
        if d_out.dtype != q.dtype:
            d_out = d_out.to(q.dtype)
        if not _mca_rows_ok(d_out):
            d_out = d_out.contiguous()
        nws = lib.vah_mca_ws_bytes(N, H, Lq, Lk)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        dq = torch.empty((Lq, N, E), dtype=q.dtype, device=dev)
        dkv = torch.empty((2, Lk, N, E), dtype=q.dtype, device=dev)
        with _vah.on(dev):
            _vah.check(lib.vah_mca_backward(*_mca_arg(q), *_mca_arg(k), *_mca_arg(v), bits.data_ptr(), *_mca_arg(out), *_mca_arg(d_out),
                                            lse.data_ptr(), N, H, Lq, Lk, E // H, scale, *_mca_arg(dq), *_mca_arg(dkv[0]),
                                            *_mca_arg(dkv[1]), ws.data_ptr(), nws, st), 'vah_mca_backward')
        return dq, dkv[0], dkv[1], None, None, None


def masked_cross_attention(q, k, v, mask_logits, num_heads):
    """Cross-attention of Mask2Former's query decoder (the reference's mask2former_head.py:404-525 around
    nn.MultiheadAttention): q (Lq, N, E), k and v (Lk, N, E) - the projected rows, possibly column slices of a packed
    projection - and mask_logits (N, Lq, Lk), the interpolated mask prediction of the previous layer.  Key j is excluded for
    query i where mask_logits[n, i, j] < 0 (sigmoid < 0.5 in exact arithmetic); a row that excludes every key excludes
    none.  The mask is shared by the heads and gets no gradient.  Returns (Lq, N, E).
    On the GPU under bf16 or fp16 autocast, with ENABLED['masked_attn'], heads of 32 channels and Lq <= 128, this is
    csrc/masked_attn.hip; otherwise the same expression in torch, which does not synchronise with the host either."""
    Lq, N, E = q.shape
    Lk = k.shape[0]
    D = E // num_heads
    scale = 1.0 / math.sqrt(D)
    t16 = torch.get_autocast_dtype('cuda') if torch.is_autocast_enabled() else None
    if (ENABLED['masked_attn'] and q.is_cuda and t16 in (torch.bfloat16, torch.float16) and D == 32 and E == 32 * num_heads
            and 1 <= Lq <= 128 and Lk >= 1 and N >= 1):
        return _MaskedCrossAttention.apply(q.to(t16), k.to(t16), v.to(t16), mca_pack_mask(mask_logits), num_heads, scale)
    x = mask_logits.detach()
    keep = ~(x < 0)
    keep = keep | ~keep.any(-1, keepdim=True)
    qh, kh, vh = (t.reshape(t.shape[0], N * num_heads, D).transpose(0, 1) for t in (q, k, v))
    s = torch.bmm(qh, kh.transpose(1, 2)) * scale
    s = s.view(N, num_heads, Lq, Lk).masked_fill(~keep[:, None], float('-inf'))
    p = torch.softmax(s, -1).view(N * num_heads, Lq, Lk)
    return torch.bmm(p.to(vh.dtype), vh).transpose(0, 1).reshape(Lq, N, E)


_PTS_CODES = {torch.float32: 0, torch.uint8: 3, torch.bool: 3}


def _pts_maps(maps):
    """(M, h, w) maps as the point kernels read them: fp32 or uint8 (bool is read as its bytes), contiguous columns"""
    if maps.dtype not in _PTS_CODES:
        maps = maps.float()
    if maps.dtype == torch.bool:
        maps = maps.view(torch.uint8)
    if maps.stride(2) != 1 or maps.stride(0) < 0 or maps.stride(1) < maps.shape[2]:
        maps = maps.contiguous()
    return maps


def _pts_idx(idx, device):
    if idx is None:
        return None
    return torch.as_tensor(idx, device=device).to(torch.int32).contiguous()


def _pts_on(t):
    return ENABLED['point_loss'] and t.is_cuda


def _grid_sample_points(maps, points):
    """mmcv ``point_sample(maps[:, None], points, align_corners=False)[:, 0]``: maps (R, h, w), points (R, P, 2) -> (R, P)"""
    if maps.shape[0] == 0:
        return maps.new_zeros((0, points.shape[1])) + 0 * maps.sum()
    return F.grid_sample(maps[:, None], 2.0 * points[:, None] - 1.0, mode='bilinear', padding_mode='zeros', align_corners=False)[:, 0, 0]


def point_sample(maps, points, map_idx=None, set_idx=None):
    """Row r of the result samples ``maps[map_idx[r]]`` at the points ``points[set_idx[r]]``: maps (M, h, w) fp32, uint8 or
    bool (ground-truth masks as stored), points (S, P, 2) fp32 in mmcv's convention ((x, y), the unit square is the map), an
    index of None is the identity.  -> (R, P) fp32, no gradient.  mmcv's ``point_sample(input, points, align_corners=False)``
    of the reference's mask2former_head.py:237-243, :338-342 and point_sample.py:63.  On the GPU with ENABLED['point_loss']
    this is vah_pts_sample (csrc/point_loss.hip); otherwise F.grid_sample."""
    maps, points = maps.detach(), points.detach().float()
    dev = maps.device
    if _pts_on(maps) and maps.dim() == 3 and maps.numel() > 0 and points.shape[1] > 0:
        maps, points = _pts_maps(maps), points.contiguous()
        mi, si = _pts_idx(map_idx, dev), _pts_idx(set_idx, dev)
        M, h, w = maps.shape
        S, P, _ = points.shape
        R = mi.numel() if mi is not None else (si.numel() if si is not None else M)
        out = torch.empty((R, P), dtype=torch.float32, device=dev)
        with _vah.on(dev):
            _vah.check(_vah.lib.vah_pts_sample(maps.data_ptr(), _PTS_CODES[maps.dtype], maps.stride(0), maps.stride(1), M, h, w,
                                               points.data_ptr(), S, P, mi.data_ptr() if mi is not None else None,
                                               si.data_ptr() if si is not None else None, R, out.data_ptr(), _stream(maps)),
                       'vah_pts_sample')
        return out
    m = maps if map_idx is None else maps[torch.as_tensor(map_idx, device=dev).long()]
    p = points if set_idx is None else points[torch.as_tensor(set_idx, device=dev).long()]
    return _grid_sample_points(m.float(), p)


def match_costs(xs, ts, cls_scores, labels, gt_counts, weights, eps=1.0, gt_offsets=None):
    """The cost matrices of the reference's MaskHungarianAssigner (models/utils/assigner.py:126-145 with ClassificationCost,
    CrossEntropyLossCost(use_sigmoid=True) and DiceCost(pred_act=True) of models/losses/match_costs.py) for one decoder output:
    xs (N * Q, P) sampled mask logits, ts (G_total, P) sampled ground truth of all images (image n owns ``gt_counts[n]`` rows,
    in order), cls_scores (N, Q, classes + 1), labels (G_total,), weights = (w_cls, w_mask, w_dice), eps the dice cost's.
    -> (N, Q, max(gt_counts)) fp32, columns past an image's own count +inf.  No gradient, nothing read back to the host.
    ``gt_offsets``: the int32 (N + 1,) running sum of gt_counts on the device, if the caller keeps one.
    On the GPU with ENABLED['point_loss'] this is vah_pts_match_cost; otherwise the reference's formulas."""
    xs, ts, cls_scores = xs.detach().float(), ts.detach().float(), cls_scores.detach().float()
    N, Q, C1 = cls_scores.shape
    P = xs.shape[1]
    gt_counts = [int(c) for c in gt_counts]
    Gmax, G_total = max(gt_counts) if gt_counts else 0, sum(gt_counts)
    dev = xs.device
    w_cls, w_mask, w_dice = (float(v) for v in weights)
    cost = torch.full((N, Q, Gmax), float('inf'), dtype=torch.float32, device=dev) if not _pts_on(xs) else None
    if N * Q * Gmax == 0:
        return torch.empty((N, Q, Gmax), dtype=torch.float32, device=dev)
    if _pts_on(xs):
        if gt_offsets is None:
            gt_offsets = torch.tensor([sum(gt_counts[:i]) for i in range(N + 1)], dtype=torch.int32, device=dev)
        xs, ts, cls_scores, labels = xs.contiguous(), ts.contiguous(), cls_scores.contiguous(), labels.long().contiguous()
        cost = torch.empty((N, Q, Gmax), dtype=torch.float32, device=dev)
        with _vah.on(dev):
            _vah.check(_vah.lib.vah_pts_match_cost(xs.data_ptr(), ts.data_ptr(), gt_offsets.data_ptr(), cls_scores.data_ptr(),
                                                   labels.data_ptr(), N, Q, C1, G_total, Gmax, P, w_cls, w_mask, w_dice, float(eps),
                                                   cost.data_ptr(), _stream(xs)), 'vah_pts_match_cost')
        return cost
    lo = 0
    for n, G in enumerate(gt_counts):
        if G == 0:
            continue
        x, t, lab = xs[n * Q:(n + 1) * Q], ts[lo:lo + G], labels[lo:lo + G].long()
        lo += G
        c_cls = -cls_scores[n].softmax(-1)[:, lab] * w_cls
        pos = F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction='none')
        neg = F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction='none')
        c_mask = (torch.einsum('nc,mc->nm', pos, t) + torch.einsum('nc,mc->nm', neg, 1 - t)) / P * w_mask
        s = x.sigmoid()
        c_dice = (1 - (2 * torch.einsum('nc,mc->nm', s, t) + eps) / (s.sum(-1)[:, None] + t.sum(-1)[None, :] + eps)) * w_dice
        cost[n, :, :G] = c_cls + c_mask + c_dice
    return cost


class _PointMaskLosses(torch.autograd.Function):
    """point_mask_losses on vah_pml_forward / vah_pml_backward: mask_pred (N, Q, h, w) fp32 on the GPU, rows / tgt_rows int32
    (K,), targets as _pts_maps gives them, points (K, P, 2) fp32 contiguous.  Gradient into mask_pred only."""

    @staticmethod
    def forward(ctx, mask_pred, rows, targets, tgt_rows, points, eps):
        dev = mask_pred.device
        pred = mask_pred.detach().flatten(0, 1)
        if pred.stride(2) != 1 or pred.stride(0) < 0 or pred.stride(1) < pred.shape[2]:
            pred = pred.contiguous()
        Mp, h, w = pred.shape
        Mt, H, W = targets.shape
        K, P, _ = points.shape
        rows, tgt_rows = rows.contiguous(), tgt_rows.contiguous()
        nbytes = _vah.lib.vah_pml_ws_bytes(K, P, h, w)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        bce, dice = torch.empty((K,), dtype=torch.float32, device=dev), torch.empty((K,), dtype=torch.float32, device=dev)
        xs, ts = torch.empty((K, P), dtype=torch.float32, device=dev), torch.empty((K, P), dtype=torch.float32, device=dev)
        sums = torch.empty((K, 4), dtype=torch.float32, device=dev)
        with _vah.on(dev):
            _vah.check(_vah.lib.vah_pml_forward(pred.data_ptr(), pred.stride(0), pred.stride(1), Mp, h, w, targets.data_ptr(),
                                                _PTS_CODES[targets.dtype], targets.stride(0), targets.stride(1), Mt, H, W,
                                                points.data_ptr(), P, rows.data_ptr(), tgt_rows.data_ptr(), K, eps, bce.data_ptr(),
                                                dice.data_ptr(), xs.data_ptr(), ts.data_ptr(), sums.data_ptr(), ws.data_ptr(), nbytes,
                                                _stream(pred)), 'vah_pml_forward')
        ctx.save_for_backward(points, xs, ts, sums, rows)
        ctx.shape, ctx.eps, ctx.nbytes = tuple(mask_pred.shape), eps, nbytes
        return bce, dice

    @staticmethod
    def backward(ctx, g_bce, g_dice):
        points, xs, ts, sums, rows = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        dev = points.device
        N, Q, h, w = ctx.shape
        K, P, _ = points.shape
        g_bce = (torch.zeros_like(xs[:, 0]) if g_bce is None else g_bce.float()).contiguous()
        g_dice = (torch.zeros_like(xs[:, 0]) if g_dice is None else g_dice.float()).contiguous()
        ws = torch.empty((ctx.nbytes,), dtype=torch.uint8, device=dev)
        dmaps = torch.empty((K, h, w), dtype=torch.float32, device=dev)
        with _vah.on(dev):
            _vah.check(_vah.lib.vah_pml_backward(points.data_ptr(), xs.data_ptr(), ts.data_ptr(), sums.data_ptr(), g_bce.data_ptr(),
                                                 g_dice.data_ptr(), K, P, h, w, ctx.eps, dmaps.data_ptr(), ws.data_ptr(), ctx.nbytes,
                                                 _stream(points)), 'vah_pml_backward')
        grad = torch.zeros((N * Q, h, w), dtype=torch.float32, device=dev)
        grad.index_put_((rows.long(),), dmaps, accumulate=True)
        return grad.view(N, Q, h, w), None, None, None, None, None


def point_mask_losses(mask_pred, rows, targets, tgt_rows, points, eps=1.0):
    """The mask losses of K matched queries before their reduction (the reference's mask2former_head.py:338-356 with
    CrossEntropyLoss(use_sigmoid=True) and DiceLoss(naive_dice=True)): row k samples ``mask_pred.flatten(0, 1)[rows[k]]``
    ((N, Q, h, w) logits, differentiable) and ``targets[tgt_rows[k]]`` ((Mt, H, W) masks, fp32 / uint8 / bool at their own
    resolution) at ``points[k]`` ((K, P, 2), as in point_sample) and returns
        bce_sum (K,) = sum_p binary_cross_entropy_with_logits(x, t),   dice (K,) = 1 - (2 sum s t + eps) / (sum s + sum t + eps)
    with s = sigmoid(x).  Targets and points get no gradient.
    On the GPU with ENABLED['point_mask_loss'] and ENABLED['point_loss'], for fp32 logits, this is vah_pml_forward /
    vah_pml_backward (csrc/point_mask_loss.hip): mask_pred is read in place through ``rows``, the masks at their own dtype, and
    the gradient into mask_pred is an ordered gather, so the same inputs give the same bits (``rows`` may repeat: the rows of
    the dense (K, h, w) adjoint are added per map by a deterministic index_put_).  Otherwise the targets are sampled by
    point_sample and the predictions, the two losses and their backward are torch's: F.grid_sample, whose backward into
    mask_pred accumulates with float atomics."""
    dev = mask_pred.device
    rows_l, tgt_l = torch.as_tensor(rows, device=dev).long(), torch.as_tensor(tgt_rows, device=dev).long()
    points = points.detach().float()
    if rows_l.numel() == 0:
        z = mask_pred.flatten(0, 1)[:0].sum((1, 2)).float()
        return z, z
    if (ENABLED['point_mask_loss'] and _pts_on(mask_pred) and mask_pred.dtype == torch.float32 and mask_pred.dim() == 4
            and targets.is_cuda and targets.dim() == 3 and targets.numel() > 0 and points.dim() == 3 and points.shape[1] > 0
            and targets.dtype in (torch.float32, torch.uint8, torch.bool)
            and _vah.lib.vah_pml_ws_bytes(rows_l.numel(), points.shape[1], mask_pred.shape[2], mask_pred.shape[3]) > 0):
        return _PointMaskLosses.apply(mask_pred, rows_l.to(torch.int32), _pts_maps(targets.detach()), tgt_l.to(torch.int32),
                                      points.contiguous(), float(eps))
    x = _grid_sample_points(mask_pred.flatten(0, 1)[rows_l].float(), points)
    t = point_sample(targets, points, map_idx=tgt_l)
    bce = F.binary_cross_entropy_with_logits(x, t, reduction='none').sum(1)
    s = x.sigmoid()
    dice = 1 - (2 * (s * t).sum(1) + eps) / (s.sum(1) + t.sum(1) + eps)
    return bce, dice


# ----------------------------------------------------------------------------------------------------------------------
# the assignment step of Mask2Former's matching (include/vitadapter_hip_assign.h, csrc/assign.hip)
# ----------------------------------------------------------------------------------------------------------------------
ASSIGN_MAX_DIM, ASSIGN_MAX_CELLS, ASSIGN_MAX_IMAGES = 256, 32768, 4096
ASSIGN_ERRORS = {1: 'matrix contains invalid numeric entries', 2: 'cost matrix is infeasible'}       # scipy's two messages


def _hungarian_host(stacked, counts):
    """the path before the kernel: one copy to the host, scipy per problem, -> the (L, 2, K) int64 table on the host"""
    L, N, Q, _ = stacked.shape
    host = stacked.detach().cpu().numpy()                         # the synchronisation of this path
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        raise ImportError('Please run "pip install scipy" to install scipy first.') from None
    firsts = [sum(counts[:n]) for n in range(N)]
    none = torch.zeros(0, dtype=torch.long)
    table = []
    for i in range(L):
        rows, tgts = [none], [none]
        for n in range(N):
            if counts[n]:
                r, c = linear_sum_assignment(host[i, n, :, :counts[n]])
                order = r.argsort(kind='stable')                    # MaskPseudoSampler: positives in query order
                rows.append(torch.from_numpy(r[order]).long() + n * Q)
                tgts.append(torch.from_numpy(c[order]).long() + firsts[n])
        table.append(torch.stack([torch.cat(rows), torch.cat(tgts)]))
    return torch.stack(table) if table else torch.zeros((0, 2, 0), dtype=torch.long)


def hungarian_match(costs, gt_counts, gt_offsets=None):
    """The assignment of the reference's MaskHungarianAssigner (models/utils/assigner.py:147-160, scipy's
    linear_sum_assignment per cost matrix) and the order of its MaskPseudoSampler for every (decoder output, image) of a step:
    ``costs`` the list of per-output (N, Q, Gmax) matrices of ``match_costs`` or their stack (L, N, Q, Gmax), ``gt_counts`` the N
    counts (columns past an image's count are not read), ``gt_offsets`` the int32 (N + 1,) running sum on the device if the
    caller keeps one.  -> (table, status): table (L, 2, K) int64 on the costs' device with K = sum_n min(Q, G_n), per output
    the matched (query row n * Q + q, global target index) pairs, images in order, queries ascending within an image.
    On the GPU with ENABLED['hungarian'], for fp32 costs with Q <= 256, Gmax <= 256 and Q * Gmax <= 32768, this is one launch of
    vah_assign_solve and nothing reaches the host: status is the (L, N) int32 tensor of the header (0 solved, 1 invalid
    entries, 2 infeasible; the pairs of such a problem are the identity pairing).  Otherwise - switch off, CPU, larger
    problems - the costs go to the host in one copy, scipy solves each problem (and raises for the two cases), the table goes
    back in one copy, and status is None."""
    stacked = costs if isinstance(costs, torch.Tensor) else torch.stack(list(costs))
    if stacked.dim() != 4:
        raise ValueError('hungarian_match: costs of shape (L, N, Q, Gmax) or a list of (N, Q, Gmax), got %s' % (tuple(stacked.shape),))
    L, N, Q, Gmax = stacked.shape
    counts = [int(c) for c in gt_counts]
    if len(counts) != N or any(c < 0 or c > Gmax for c in counts):
        raise ValueError('hungarian_match: %d counts in [0, %d] expected, got %r' % (N, Gmax, counts))
    dev = stacked.device
    if (ENABLED['hungarian'] and stacked.is_cuda and stacked.dtype == torch.float32 and 1 <= Q <= ASSIGN_MAX_DIM and Gmax <= ASSIGN_MAX_DIM
            and Q * Gmax <= ASSIGN_MAX_CELLS and N <= ASSIGN_MAX_IMAGES):
        K = sum(min(Q, c) for c in counts)
        stacked = stacked.detach().contiguous()
        if L * N * Gmax == 0 or K == 0:                             # nothing to solve, and no table to point the kernel at
            return torch.zeros((L, 2, 0), dtype=torch.int64, device=dev), torch.zeros((L, N), dtype=torch.int32, device=dev)
        if gt_offsets is None:
            gt_offsets = torch.tensor([sum(counts[:i]) for i in range(N + 1)], dtype=torch.int32, device=dev)
        table = torch.empty((L, 2, K), dtype=torch.int64, device=dev)
        status = torch.empty((L, N), dtype=torch.int32, device=dev)
        with _vah.on(dev):
            _vah.check(_vah.lib.vah_assign_solve(stacked.data_ptr(), gt_offsets.data_ptr(), L, N, Q, Gmax, table.data_ptr(),
                                                 status.data_ptr(), _stream(stacked)), 'vah_assign_solve')
        return table, status
    return _hungarian_host(stacked, counts).to(dev), None


_SEG_FLIPS = {None: 0, False: 0, 'horizontal': 1, 'vertical': 2}


def _seg_on(t):
    return ENABLED['seg_logits'] and t.is_cuda and t.dtype == torch.float32


def _seg_planes(t):
    """(N, C, H, W) fp32 as the segmentor kernels read it: column stride 1, planes that do not overlap"""
    N, C, H, W = t.shape
    si, sp, sr, sc = t.stride()
    plane = (H - 1) * sr + W
    if sc != 1 or sr < W or sp < plane or si < (C - 1) * sp + plane:
        t = t.contiguous()
    return t


def seg_resize_add(src, dst, y0, x0, size, align_corners=False, accumulate=True):
    """``dst[:, :, y0:y0 + Hc, x0:x0 + Wc] (= | +=) resize(src, size=(Hc, Wc), mode='bilinear', align_corners=...)`` in place,
    -> dst: the ``resize`` of the reference's encode_decode (encoder_decoder_mask2former.py:75-79) and the
    ``preds += F.pad(crop_seg_logit, ...)`` of its slide_inference (:181-183) without the upsampled or the padded tensor.
    src (N, C, hs, ws), dst (N, C, Hd, Wd).  On the GPU in fp32 with ENABLED['seg_logits'] this is vah_seg_resize_add;
    otherwise the reference's expression."""
    Hc, Wc = int(size[0]), int(size[1])
    y0, x0 = int(y0), int(x0)
    N, C, Hd, Wd = dst.shape
    if y0 < 0 or x0 < 0 or y0 + Hc > Hd or x0 + Wc > Wd or src.shape[:2] != dst.shape[:2]:
        raise ValueError('seg_resize_add: a %d x %d window at (%d, %d) of %s from %s' % (Hc, Wc, y0, x0, tuple(dst.shape),
                                                                                        tuple(src.shape)))
    if _seg_on(dst) and _seg_on(src) and dst.stride(3) == 1 and dst.stride(2) >= Wd:
        src = _seg_planes(src.detach())
        with _vah.on(dst.device):
            _vah.check(_vah.lib.vah_seg_resize_add(src.data_ptr(), src.stride(0), src.stride(1), src.stride(2), N, C, src.shape[2],
                                                   src.shape[3], Hc, Wc, 1 if align_corners else 0, dst.data_ptr(), dst.stride(0),
                                                   dst.stride(1), dst.stride(2), Hd, Wd, y0, x0, 1 if accumulate else 0,
                                                   _stream(dst)), 'vah_seg_resize_add')
        return dst
    up = F.interpolate(src, size=(Hc, Wc), mode='bilinear', align_corners=align_corners).to(dst.dtype)
    if accumulate:
        dst += F.pad(up, (x0, Wd - x0 - Wc, y0, Hd - y0 - Hc))
    else:
        dst[:, :, y0:y0 + Hc, x0:x0 + Wc] = up
    return dst


def seg_finish(acc, counts=None, region=None, size=None, align_corners=False, flip=None, out=None, accumulate=False, prob=True,
               labels=False):
    """The rest of one view of the reference's slide_inference / whole_inference / inference / simple_test
    (encoder_decoder_mask2former[_aug].py:191-258): ``acc / count_mat`` with count_mat = counts[0][:, None] * counts[1][None, :]
    (int32 vectors; None: no division), the crop to ``region`` = (Hs, Ws) (the Aug class's un-padding; None: all of acc),
    ``resize(..., size=size)`` (None: no resize), softmax over the classes, the flip ('horizontal', 'vertical' or None).
    -> (probabilities or None, labels or None): with ``prob`` the (N, C, Ho, Wo) softmax output - stored into / with
    ``accumulate`` added to ``out`` if that is given - and with ``labels`` its argmax(1), (N, Ho, Wo) int64.  Nothing that is
    not returned is formed.  On the GPU in fp32 with ENABLED['seg_logits'] this is vah_seg_finish, one launch; otherwise the
    reference's expression."""
    N, C, H, W = acc.shape
    Hs, Ws = (H, W) if region is None else (int(region[0]), int(region[1]))
    Ho, Wo = (Hs, Ws) if size is None else (int(size[0]), int(size[1]))
    if flip not in _SEG_FLIPS:
        raise ValueError("seg_finish: flip is None, 'horizontal' or 'vertical', not %r" % (flip,))
    if Hs > H or Ws > W or (out is not None and tuple(out.shape) != (N, C, Ho, Wo)):
        raise ValueError('seg_finish: region %s of %s, out %s' % ((Hs, Ws), tuple(acc.shape), None if out is None else tuple(out.shape)))
    if _seg_on(acc) and (out is None or (_seg_on(out) and out.is_contiguous())) and N * C * Ho * Wo > 0:
        acc = _seg_planes(acc.detach())
        dev = acc.device
        cy, cx = (None, None) if counts is None else (c.to(device=dev, dtype=torch.int32).contiguous() for c in counts)
        p = None
        if prob:
            p = out if out is not None else torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=dev)
        lab = torch.empty((N, Ho, Wo), dtype=torch.int64, device=dev) if labels else None
        if p is None and lab is None:
            return None, None
        with _vah.on(dev):
            _vah.check(_vah.lib.vah_seg_finish(acc.data_ptr(), acc.stride(0), acc.stride(1), acc.stride(2), N, C, Hs, Ws,
                                               None if cy is None else cy.data_ptr(), None if cx is None else cx.data_ptr(),
                                               0 if size is None else 1, Ho, Wo, 1 if align_corners else 0, _SEG_FLIPS[flip],
                                               None if p is None else p.data_ptr(), C * Ho * Wo, Ho * Wo, Wo,
                                               1 if (accumulate and out is not None) else 0,
                                               None if lab is None else lab.data_ptr(), Ho * Wo, Wo, _stream(acc)), 'vah_seg_finish')
        return p, lab
    v = acc
    if counts is not None:
        count_mat = (counts[0].to(acc.device)[:, None] * counts[1].to(acc.device)[None, :]).to(acc.dtype)
        v = v / count_mat
    v = v[:, :, :Hs, :Ws]
    if size is not None:
        v = F.interpolate(v, size=(Ho, Wo), mode='bilinear', align_corners=align_corners)
    p = F.softmax(v, dim=1)
    if flip == 'horizontal':
        p = p.flip(dims=(3,))
    elif flip == 'vertical':
        p = p.flip(dims=(2,))
    lab = p.argmax(dim=1) if labels else None
    if not prob:
        return None, lab
    if out is not None:
        if accumulate:
            out += p
        else:
            out.copy_(p)
        p = out
    return p, lab


def seg_argmax(total, divisor=1):
    """``(total / divisor).argmax(dim=1)``: the last lines of the reference's aug_test (encoder_decoder_mask2former.py:280-281),
    (N, C, H, W) -> (N, H, W) int64, without the quotient.  On the GPU in fp32 with ENABLED['seg_logits'] this is vah_seg_argmax."""
    N, C, H, W = total.shape
    if _seg_on(total) and total.numel() > 0:
        total = _seg_planes(total.detach())
        lab = torch.empty((N, H, W), dtype=torch.int64, device=total.device)
        with _vah.on(total.device):
            _vah.check(_vah.lib.vah_seg_argmax(total.data_ptr(), total.stride(0), total.stride(1), total.stride(2), N, C, H, W,
                                               float(divisor), lab.data_ptr(), H * W, W, _stream(total)), 'vah_seg_argmax')
        return lab
    return (total / divisor).argmax(dim=1)


_SCE_CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


class _SegCrossEntropy(torch.autograd.Function):
    """seg_cross_entropy on vah_sce_forward / vah_sce_backward: seg_logit (N, C, h, w) fp32 / bf16 / fp16 on the GPU, label
    (N, H, W) int64, class_weight fp32 (C,) or None.  -> (loss_sum (), counts (2,) int64); gradient into seg_logit only."""

    @staticmethod
    def forward(ctx, seg_logit, label, align_corners, ignore_index, class_weight):
        x = _seg_planes(seg_logit.detach())
        dev = x.device
        N, C, h, w = x.shape
        H, W = label.shape[1:]
        nbytes = _vah.lib.vah_sce_ws_bytes(N, C, h, w, H, W)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        lse = torch.empty((N, H, W), dtype=torch.float32, device=dev)
        loss_sum = torch.empty((), dtype=torch.float32, device=dev)
        counts = torch.empty((2,), dtype=torch.int64, device=dev)
        ctx.head = (x.data_ptr(), _SCE_CODES[x.dtype], x.stride(0), x.stride(1), x.stride(2), N, C, h, w, label.data_ptr(),
                    label.stride(0), label.stride(1), H, W, 1 if align_corners else 0, int(ignore_index),
                    None if class_weight is None else class_weight.data_ptr())
        with _vah.on(dev):
            _vah.check(_vah.lib.vah_sce_forward(*ctx.head, lse.data_ptr(), loss_sum.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                                nbytes, _stream(x)), 'vah_sce_forward')
        ctx.save_for_backward(x, label, lse, class_weight)          # ctx.head's pointers are theirs
        ctx.nbytes = nbytes
        ctx.mark_non_differentiable(counts)
        return loss_sum, counts

    @staticmethod
    def backward(ctx, g_loss, _g_counts):
        x, label, lse, class_weight = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        dev = x.device
        scale = g_loss.detach().to(torch.float32).reshape(()).contiguous()      # stays on the device
        ws = torch.empty((ctx.nbytes,), dtype=torch.uint8, device=dev)
        dx = torch.empty(x.shape, dtype=x.dtype, device=dev)
        with _vah.on(dev):
            _vah.check(_vah.lib.vah_sce_backward(*ctx.head, lse.data_ptr(), scale.data_ptr(), dx.data_ptr(), dx.stride(0),
                                                 dx.stride(1), dx.stride(2), ws.data_ptr(), ctx.nbytes, _stream(x)),
                       'vah_sce_backward')
        return dx, None, None, None, None


def seg_cross_entropy(seg_logit, seg_label, align_corners=False, ignore_index=255, class_weight=None):
    """What mmseg's ``BaseDecodeHead.losses`` computes from a head's logits before its reductions: with
    ``v = resize(seg_logit, size=seg_label.shape[-2:], mode='bilinear', align_corners=...)`` in fp32 (``@force_fp32``),
        loss_sum  = F.cross_entropy(v, seg_label, weight=class_weight, reduction='none', ignore_index=ignore_index).sum()
        n_valid   = the pixels whose label is not ``ignore_index``
        n_correct = the pixels among them whose label is ``v.argmax(1)``
    (the reference's segmentation/mmseg_custom/models/losses/cross_entropy_loss.py:11-62 and mmseg's ``accuracy``), as device
    tensors: an fp32 scalar and two int64 scalars.  seg_logit (N, C, h, w), differentiable; seg_label (N, H, W) or (N, 1, H, W)
    integer; class_weight a (C,) tensor or None.
    On the GPU with ENABLED['seg_ce_loss'], for fp32 / bf16 / fp16 logits, this is vah_sce_forward / vah_sce_backward
    (csrc/seg_ce_loss.hip): ``v`` is never formed, one fp32 log-sum-exp per pixel is kept for the backward, and the gradient
    is an ordered gather in the logits' dtype, so the same inputs give the same bits.  There a label outside [0, C) that is
    not ``ignore_index`` counts as ignored (torch: a device assert).  Otherwise - switch off, CPU, fp64 - the expression
    above is evaluated as written.  Runs with autocast disabled."""
    if seg_label.dim() == 4:
        seg_label = seg_label.squeeze(1)
    if seg_logit.dim() != 4 or seg_label.dim() != 3 or seg_label.shape[0] != seg_logit.shape[0]:
        raise ValueError('seg_cross_entropy: logits %s, labels %s' % (tuple(seg_logit.shape), tuple(seg_label.shape)))
    with torch.autocast(seg_logit.device.type, enabled=False):
        if (ENABLED['seg_ce_loss'] and seg_logit.is_cuda and seg_logit.dtype in _SCE_CODES and seg_label.is_cuda
                and seg_logit.numel() > 0 and seg_label.numel() > 0
                and _vah.lib.vah_sce_ws_bytes(*seg_logit.shape, *seg_label.shape[1:]) > 0):
            label = seg_label.detach().long()
            if label.stride(2) != 1 or label.stride(1) < label.shape[2] or label.stride(0) < (label.shape[1] - 1) * label.stride(1) + label.shape[2]:
                label = label.contiguous()
            cw = None
            if class_weight is not None:
                cw = torch.as_tensor(class_weight, device=seg_logit.device).detach().float().contiguous()
            loss_sum, counts = _SegCrossEntropy.apply(seg_logit, label, bool(align_corners), int(ignore_index), cw)
            return loss_sum, counts[0], counts[1]
        v = seg_logit if seg_logit.dtype == torch.float64 else seg_logit.float()
        v = F.interpolate(v, size=seg_label.shape[1:], mode='bilinear', align_corners=align_corners)
        label = seg_label.long()
        cw = None if class_weight is None else torch.as_tensor(class_weight, device=v.device).to(v.dtype)
        loss_sum = F.cross_entropy(v, label, weight=cw, reduction='none', ignore_index=ignore_index).sum()
        valid = label != ignore_index
        return loss_sum, valid.sum(), ((v.argmax(dim=1) == label) & valid).sum()


_SEG_EVAL_CODES = {torch.int64: 0, torch.uint8: 1}
_SEG_EVAL_MAPS = {}


def _seg_eval_map(x):
    """(N, H, W) label map as the counting kernel reads it: column stride 1, rows and images that do not overlap"""
    N, H, W = x.shape
    si, sr, sc = x.stride()
    if sc != 1 or sr < W or si < (H - 1) * sr + W:
        x = x.contiguous()
    return x


def _seg_eval_table(label_map, device):
    """label_map {old: new} as the int64 device table of vah_segeval_update (identity outside the keys), built once per
    mapping and device; None for a mapping the table cannot hold (a key outside [0, 256))"""
    items = tuple(sorted((int(k), int(v)) for k, v in label_map.items()))
    if not items or items[0][0] < 0 or items[-1][0] > 255:
        return None
    key = (items, str(device))
    if key not in _SEG_EVAL_MAPS:
        table = list(range(items[-1][0] + 1))
        for old, new in items:
            table[old] = new
        _SEG_EVAL_MAPS[key] = torch.tensor(table, dtype=torch.int64, device=device)
    return _SEG_EVAL_MAPS[key]


def seg_eval_update(pred, label, totals, num_classes, ignore_index=255, reduce_zero_label=False, label_map=None):
    """``totals += (area_intersect, area_pred_label, area_label)`` of mmseg's ``intersect_and_union`` for a batch, in place,
    -> totals.  pred (N, H, W) predicted labels, label (N, H, W) or (N, 1, H, W) ground truth, totals (3, num_classes) int64
    on their device.  Per pixel, in mmseg's order: ``g = label``; ``g = label_map[g]`` for the keys of ``label_map`` (a dict,
    every entry applied to the original value); with ``reduce_zero_label`` ``g = 255 if g in (0, 255) else g - 1``; a pixel
    with ``g == ignore_index`` counts for nothing; otherwise ``area_pred[pred]``, ``area_label[g]`` and - where they agree -
    ``area_intersect[pred]`` grow by one, a value outside [0, num_classes) growing nothing.
    On the GPU with ENABLED['seg_eval'], for int64 predictions and uint8 or int64 ground truth, this is vah_segeval_update
    (csrc/seg_eval.hip): one counting launch and one merge launch, no host synchronisation, integer counts in any order.
    Otherwise - switch off, CPU, other dtypes, more than 4096 classes - the same rule with masks and torch.bincount, integer
    throughout (on a device torch.bincount synchronises)."""
    if label.dim() == 4:
        label = label.squeeze(1)
    C = int(num_classes)
    if pred.dim() != 3 or tuple(label.shape) != tuple(pred.shape) or tuple(totals.shape) != (3, C) or totals.dtype != torch.int64:
        raise ValueError('seg_eval_update: pred %s, label %s, totals %s %s for %d classes'
                         % (tuple(pred.shape), tuple(label.shape), tuple(totals.shape), totals.dtype, C))
    if pred.numel() == 0:
        return totals
    dev = pred.device
    table = None if not label_map else _seg_eval_table(label_map, dev)
    if (ENABLED['seg_eval'] and pred.is_cuda and label.device == dev and totals.device == dev and totals.is_contiguous()
            and pred.dtype == torch.int64 and label.dtype in _SEG_EVAL_CODES and (not label_map or table is not None)
            and _vah.lib.vah_segeval_ws_bytes(*pred.shape, C) > 0):
        p, g = _seg_eval_map(pred.detach()), _seg_eval_map(label.detach())
        N, H, W = p.shape
        nbytes = _vah.lib.vah_segeval_ws_bytes(N, H, W, C)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        with _vah.on(dev):
            _vah.check(_vah.lib.vah_segeval_update(p.data_ptr(), p.stride(0), p.stride(1), g.data_ptr(), _SEG_EVAL_CODES[g.dtype],
                                                   g.stride(0), g.stride(1), N, H, W, C, int(ignore_index),
                                                   1 if reduce_zero_label else 0, None if table is None else table.data_ptr(),
                                                   0 if table is None else table.numel(), totals.data_ptr(), ws.data_ptr(), nbytes,
                                                   _stream(p)), 'vah_segeval_update')
        return totals
    p, g0 = pred.long(), label.to(dev).long()
    g = g0
    if label_map:
        g = g0.clone()
        for old, new in label_map.items():
            g[g0 == old] = new
    if reduce_zero_label:
        g = torch.where((g == 0) | (g == 255), torch.full_like(g, 255), g - 1)
    keep = g != ignore_index
    p_in, g_in = keep & (p >= 0) & (p < C), keep & (g >= 0) & (g < C)
    spill = torch.full_like(p, C)                       # a bin past the classes for what counts for nothing
    rows = [torch.bincount(torch.where(m, v, spill).reshape(-1), minlength=C + 1)[:C]
            for m, v in ((p_in & (p == g), p), (p_in, p), (g_in, g))]
    totals += torch.stack(rows).to(totals.device)
    return totals


# ----------------------------------------------------------------------------------------------------------------------
# Mask2Former's training targets from a label map (include/vitadapter_hip_seg_target.h, csrc/seg_target.hip)
# ----------------------------------------------------------------------------------------------------------------------
class SegTargets:
    """The targets of a batch, as the reference's ToMask step defines them per image (formatting.py:58-77), for all images
    at once: ``masks`` (G_total, H, W) uint8, ``labels`` (G_total,) int64, ``image_of`` (G_total,) int32 - the image of
    each target -, ``counts`` a list of N Python ints and ``offsets`` (N + 1,) int32 on the masks' device, the exclusive
    prefix sums of the counts.  The targets of image n are ``[offsets[n], offsets[n + 1])``, labels ascending."""

    __slots__ = ('masks', 'labels', 'image_of', 'counts', 'offsets')

    def __init__(self, masks, labels, image_of, counts, offsets):
        self.masks, self.labels, self.image_of, self.counts, self.offsets = masks, labels, image_of, counts, offsets

    def finish(self):
        """itself: a finished result stands wherever a pending handle does"""
        return self


_SEG_TARGET_TABLES = {}
_SEG_TARGET_PINNED = {}         # N -> free pinned int32 (N + 2,) buffers; a pending handle holds one from begin to finish


def seg_remap_table(reduce_zero_label=False, label_map=None):
    """The 256-entry uint8 table (a CPU tensor) that ``seg_targets`` applies to the original label value, in the order of
    ``seg_eval_update``: ``label_map`` ({old: new}, every entry on the original value), then ``reduce_zero_label``
    (0 and 255 -> 255, else v - 1).  An entry that does not fit 8 bits is a ValueError."""
    table = list(range(256))
    for old, new in (label_map or {}).items():
        if not 0 <= int(old) < 256:
            raise ValueError('seg_remap_table: label_map key %r is no 8-bit label' % (old,))
        table[int(old)] = int(new)
    if reduce_zero_label:
        table = [255 if v in (0, 255) else v - 1 for v in table]
    for old, new in enumerate(table):
        if not 0 <= new < 256:
            raise ValueError('seg_remap_table: %d -> %d does not fit 8 bits' % (old, new))
    return torch.tensor(table, dtype=torch.uint8)


def _seg_target_table(remap, device):
    """``remap`` as the device table of vah_segtgt_*: a 256-entry uint8 tensor or array (cached per content and device), else None"""
    if not isinstance(remap, torch.Tensor):
        try:
            remap = torch.as_tensor(remap)
        except (TypeError, ValueError, RuntimeError):
            return None
    if remap.dtype != torch.uint8 or tuple(remap.shape) != (256,):
        return None
    if remap.device == device:
        return remap.contiguous()
    key = (bytes(remap.cpu().contiguous().numpy().tobytes()), str(device))
    if key not in _SEG_TARGET_TABLES:
        _SEG_TARGET_TABLES[key] = remap.to(device).contiguous()
    return _SEG_TARGET_TABLES[key]


def _seg_targets_torch(g, ignore_index, remap):
    """the rule with torch.unique and a broadcast comparison per image, on ``g``'s device; labels of any value"""
    N, H, W = g.shape
    dev = g.device
    if remap is not None:
        v = g.long()                                        # a table of any length: values outside it stay what they are
        table = torch.as_tensor(remap).to(dev).long().reshape(-1)
        inside = (v >= 0) & (v < table.numel())
        g = torch.where(inside, table[v.clamp(0, max(table.numel() - 1, 0))], v) if table.numel() else v
    labels, masks, counts = [], [], []
    for n in range(N):
        lab = torch.unique(g[n]).long()                     # int64 before the test: an ignore_index outside the map's dtype
        lab = lab[lab != ignore_index]
        labels.append(lab)
        masks.append((g[n][None] == lab.to(g.dtype)[:, None, None]).to(torch.uint8))
        counts.append(int(lab.numel()))
    offsets = torch.tensor([sum(counts[:n]) for n in range(N + 1)], dtype=torch.int32, device=dev)
    image_of = torch.cat([torch.full((c,), n, dtype=torch.int32, device=dev) for n, c in enumerate(counts)]
                         + [torch.zeros(0, dtype=torch.int32, device=dev)])
    return SegTargets(torch.cat(masks + [torch.zeros((0, H, W), dtype=torch.uint8, device=dev)]),
                      torch.cat(labels + [torch.zeros(0, dtype=torch.int64, device=dev)]), image_of, counts, offsets)


class _PendingSegTargets:
    """What ``seg_targets_begin`` returns: ``finish()`` -> SegTargets.  On the kernel route the scan and the copy of the
    counts to the host are under way; ``finish`` waits for that copy's event only."""

    def __init__(self, g, ignore_index, remap, route=None):
        self.g, self.ignore_index, self.remap, self.route, self.done = g, ignore_index, remap, route, None

    def finish(self):
        if self.done is None:
            self.done = self._finish()
            self.g = self.remap = self.route = None
        return self.done

    def _finish(self):
        if self.route is None:
            return _seg_targets_torch(self.g, self.ignore_index, self.remap)
        g, table, labels, slot, meta, host, event, stream = self.route
        N, H, W = g.shape
        dev = g.device
        event.synchronize()                                 # the copy of meta; not the device, not the stream
        offsets = host[:N + 1].tolist()
        flagged = int(host[N + 1]) != 0
        _SEG_TARGET_PINNED.setdefault(N, []).append(host)
        if flagged:                                         # an int64 value outside [0, 256): the whole call by the rule in torch
            return _seg_targets_torch(g, self.ignore_index, self.remap)
        G = int(offsets[N])
        masks = torch.empty((G, H, W), dtype=torch.uint8, device=dev)
        out_labels = torch.empty((G,), dtype=torch.int64, device=dev)
        image_of = torch.empty((G,), dtype=torch.int32, device=dev)
        with _vah.on(dev):
            now = torch.cuda.current_stream(dev)
            if now != stream:
                now.wait_event(event)
            _vah.check(_vah.lib.vah_segtgt_masks(g.data_ptr(), _SEG_EVAL_CODES[g.dtype], g.stride(0), g.stride(1), N, H, W,
                                                 None if table is None else table.data_ptr(), slot.data_ptr(), labels.data_ptr(),
                                                 meta.data_ptr(), G, masks.data_ptr(), image_of.data_ptr(), out_labels.data_ptr(),
                                                 now.cuda_stream), 'vah_segtgt_masks')
        return SegTargets(masks, out_labels, image_of, [b - a for a, b in zip(offsets, offsets[1:])], meta[:N + 1])


def seg_targets_begin(gt_semantic_seg, ignore_index=255, remap=None):
    """Start building the targets of ``gt_semantic_seg`` ((N, H, W) or (N, 1, H, W) labels); -> a handle whose ``finish()``
    returns the ``SegTargets``.  Per image: the labels are the distinct values of the map - after ``remap``, a 256-entry
    uint8 table (``seg_remap_table``) applied to the original value - ascending, without ``ignore_index``; mask g is 1 where
    the map equals label g.
    On the GPU with ENABLED['seg_targets'], for uint8 or int64 maps with column stride 1, this runs the scan and finish
    launches of csrc/seg_target.hip, starts a non-blocking copy of the N + 2 counts into a pinned buffer and records an event:
    nothing waits here.  ``finish()`` waits for that event, allocates the outputs and runs the mask launch.  An int64 value
    outside [0, 256) comes back as a flag and the call is redone in torch.  Otherwise - switch off, CPU, other dtypes or
    strides, a ``remap`` table of another length or dtype - ``finish()`` evaluates the rule
    with torch.unique and a comparison per image on the input's device, with no limit on the label values."""
    g = gt_semantic_seg
    if g.dim() == 4 and g.shape[1] == 1:
        g = g[:, 0]
    if g.dim() != 3:
        raise ValueError('seg_targets: a label map of shape (N, H, W) or (N, 1, H, W), got %s' % (tuple(gt_semantic_seg.shape),))
    g = g.detach()
    N, H, W = g.shape
    dev = g.device
    table = None if remap is None else (_seg_target_table(remap, dev) if g.is_cuda else None)
    if not (ENABLED['seg_targets'] and g.is_cuda and g.dtype in _SEG_EVAL_CODES and g.numel() > 0 and g.stride(2) == 1
            and g.stride(1) >= W and g.stride(0) >= (H - 1) * g.stride(1) + W and (remap is None or table is not None)
            and _vah.lib.vah_segtgt_ws_bytes(N, H, W) > 0):
        return _PendingSegTargets(g, int(ignore_index), remap)
    nbytes = _vah.lib.vah_segtgt_ws_bytes(N, H, W)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    labels = torch.empty((N, 256), dtype=torch.int64, device=dev)
    slot = torch.empty((N, 256), dtype=torch.int32, device=dev)
    meta = torch.empty((N + 2,), dtype=torch.int32, device=dev)
    free = _SEG_TARGET_PINNED.setdefault(N, [])
    host = free.pop() if free else torch.empty((N + 2,), dtype=torch.int32, pin_memory=True)
    with _vah.on(dev):
        stream = torch.cuda.current_stream(dev)
        _vah.check(_vah.lib.vah_segtgt_scan(g.data_ptr(), _SEG_EVAL_CODES[g.dtype], g.stride(0), g.stride(1), N, H, W, int(ignore_index),
                                            None if table is None else table.data_ptr(), labels.data_ptr(), slot.data_ptr(),
                                            meta.data_ptr(), ws.data_ptr(), nbytes, stream.cuda_stream), 'vah_segtgt_scan')
        host.copy_(meta, non_blocking=True)
        event = torch.cuda.Event()
        event.record(stream)
    return _PendingSegTargets(g, int(ignore_index), remap, (g, table, labels, slot, meta, host, event, stream))


def seg_targets(gt_semantic_seg, ignore_index=255, remap=None):
    """``seg_targets_begin(...).finish()``"""
    return seg_targets_begin(gt_semantic_seg, ignore_index, remap).finish()
