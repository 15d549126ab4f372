"""SpatialPriorModule on NHWC 16-bit activations (bf16 under bf16 autocast, fp16 under fp16 autocast): implicit-GEMM
3x3 convolutions (csrc/conv.hip) with the BatchNorm + ReLU, max-pool and image-layout kernels of csrc/spm_nhwc.hip
between them.

Reference: SpatialPriorModule.forward of
/root/reference/detection/mmdet_custom/models/backbones/adapter_modules.py:217-268.  The arithmetic is the module's
(convolutions with bf16 operands and fp32 accumulation as under autocast, batch statistics in fp32, SyncBatchNorm
all-reduces of the sums); the layout is the kernels': no NCHW <-> NHWC conversion inside the module, and the
stride-8/16/32 maps are already the (B, H*W, C) token rows the 1x1 projections and the adapter consume.
Under fp16 autocast (the reference's AMP mode; VAH_FUSED_DISABLE=fp16_spm restores torch's NCHW module) the same
kernels run instantiated on fp16 (`*_f16` entry points): fp32 sums and statistics, fp32 -> fp16 rounded to nearest
even with overflow to inf and subnormals kept; the weight gradients stay fp32.  The four 1x1 projections then are
torch's fp16 library GEMMs on the NHWC rows (as every other Linear is in that mode).
There is no CPU path behind these functions."""
import torch
import torch.nn.functional as F

import _vah
from . import conv, fused


def _stream(t):
    return _vah.raw_stream(t.device)


def image_to_nhwc16(x, dtype=torch.bfloat16):
    """(N, 3, H, W) fp32 -> (N, H, W, 16) ``dtype`` (bf16 | fp16) with channels 3..15 zero (no gradient: the image is a
    leaf input)."""
    N, C, H, W = x.shape
    assert C == 3 and x.dtype == torch.float32
    x = x.contiguous()
    y = torch.empty((N, H, W, 16), dtype=dtype, device=x.device)
    with _vah.on(x.device):
        _vah.call('vah_image_to_nhwc16_bf16', dtype, x.data_ptr(), N, H, W, y.data_ptr(), _stream(x))
    return y


class _Conv3x3(torch.autograd.Function):
    """nn.Conv2d(k=3, padding=1, bias=False) on NHWC bf16 | fp16; weight (Cout, Cin, 3, 3) fp32.  An input with more channels
    than the weight (the 16-channel image) is matched by zero weight columns."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        cin = x.shape[-1]
        ctx.stride, ctx.wcin = stride, weight.shape[1]
        # both tap-major layouts from the forward epoch's one launch (fused._EpochCopies), the second kept for the backward
        made = fused.BF16_COPIES.layout('conv9', weight, x.dtype)
        ctx.dgrad_ready = made is not None and made[0].shape[2] == cin
        if ctx.dgrad_ready:
            ctx.save_for_backward(x, made[1])
            return conv.conv3x3_forward(x, made[0], stride)
        w = weight.detach()
        if w.shape[1] != cin:
            w = F.pad(w, (0, 0, 0, 0, 0, cin - w.shape[1]))
        wb = w.to(x.dtype)
        ctx.save_for_backward(x, wb)
        return conv.conv3x3_forward(x, conv.forward_weight(wb, x.dtype), stride)

    @staticmethod
    def backward(ctx, gy):
        x, wb = ctx.saved_tensors
        gy = gy.contiguous().to(x.dtype)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            wt9 = wb if ctx.dgrad_ready else conv.dgrad_weight(wb, x.dtype)
            gx = conv.conv3x3_input_grad(gy, wt9, ctx.stride, x.shape[1:3])
        if ctx.needs_input_grad[1]:
            gw = conv.conv3x3_weight_grad(x, gy, ctx.stride).permute(0, 3, 1, 2)[:, :ctx.wcin].contiguous()
        return gx, gw, None


class _BNRelu(torch.autograd.Function):
    """relu(BatchNorm(x)) over the rows of an NHWC tensor; the statistics / SyncBatchNorm protocol of fused._BNTail."""

    @staticmethod
    def forward(ctx, x, weight, bias, norm, relu):
        C = x.shape[-1]
        rows = x.numel() // C
        x = x.contiguous()
        dev, st = x.device, _stream(x)
        training = norm.training or norm.running_mean is None
        group = fused._sync_group(norm) if training else None
        w = weight.detach().float().contiguous() if weight is not None else None
        b = bias.detach().float().contiguous() if bias is not None else None
        with _vah.on(dev):
            if training:
                sums = torch.empty(2 * C + 1, dtype=torch.float32, device=dev)
                ws = torch.empty(_vah.lib.vah_bn_nhwc_ws_floats(C), dtype=torch.float32, device=dev)
                _vah.call('vah_bn_nhwc_stats', x.dtype, x.data_ptr(), rows, C, sums.data_ptr(), ws.data_ptr(), st)
                mean, rstd, count = fused.bn_finalize(norm, sums, C, rows, group, st)
            else:
                count = None
                mean = norm.running_mean.float().contiguous()
                rstd = torch.rsqrt(norm.running_var.float() + norm.eps)
            y = torch.empty_like(x)
            _vah.call('vah_bn_nhwc_apply', x.dtype, x.data_ptr(), rows, C, mean.data_ptr(), rstd.data_ptr(), w.data_ptr() if w is not None else None,
                      b.data_ptr() if b is not None else None, int(relu), y.data_ptr(), st)
        ctx.save_for_backward(x, mean, rstd, w, b, count)
        ctx.meta = (training, group, weight is not None, bias is not None, relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, w, b, count = ctx.saved_tensors
        training, group, has_w, has_b, relu = ctx.meta
        C = x.shape[-1]
        rows = x.numel() // C
        dy = dy.contiguous().to(x.dtype)
        dev, st = x.device, _stream(x)
        wp = w.data_ptr() if w is not None else None
        bp = b.data_ptr() if b is not None else None
        with _vah.on(dev):
            sums = torch.empty(2 * C, dtype=torch.float32, device=dev)
            ws = torch.empty(_vah.lib.vah_bn_nhwc_ws_floats(C), dtype=torch.float32, device=dev)
            _vah.call('vah_bn_nhwc_bwd_stats', x.dtype, x.data_ptr(), dy.data_ptr(), rows, C, mean.data_ptr(), rstd.data_ptr(), wp, bp, int(relu),
                      sums.data_ptr(), ws.data_ptr(), st)
            local = sums.clone() if (training and group is not None) else sums      # dweight / dbias are per-rank sums
            dweight = local[C:] if has_w else None
            dbias = local[:C] if has_b else None
            dx = None
            if ctx.needs_input_grad[0]:
                if training:
                    if group is not None:
                        import torch.distributed as dist
                        dist.all_reduce(sums, group=group)
                    means = sums / count
                else:
                    means = torch.zeros_like(sums)          # running statistics are constants
                dx = torch.empty_like(x)
                _vah.call('vah_bn_nhwc_bwd_apply', x.dtype, x.data_ptr(), dy.data_ptr(), rows, C, mean.data_ptr(), rstd.data_ptr(), wp, bp,
                          int(relu), means[:C].data_ptr(), means[C:].data_ptr(), dx.data_ptr(), st)
        return dx, dweight, dbias, None, None


class _MaxPool(torch.autograd.Function):
    """MaxPool2d(3, stride 2, padding 1) on NHWC bf16 | fp16."""

    @staticmethod
    def forward(ctx, x):
        N, H, W, C = x.shape
        x = x.contiguous()
        y = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=x.dtype, device=x.device)
        idx = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
        with _vah.on(x.device):
            _vah.call('vah_maxpool3s2_nhwc_fwd_bf16', x.dtype, x.data_ptr(), N, H, W, C, y.data_ptr(), idx.data_ptr(), _stream(x))
        ctx.save_for_backward(idx)
        ctx.in_shape, ctx.in_dtype = x.shape, x.dtype
        return y

    @staticmethod
    def backward(ctx, gy):
        idx, = ctx.saved_tensors
        N, H, W, C = ctx.in_shape
        gy = gy.contiguous().to(ctx.in_dtype)
        gx = torch.empty(ctx.in_shape, dtype=ctx.in_dtype, device=gy.device)
        with _vah.on(gy.device):
            _vah.call('vah_maxpool3s2_nhwc_bwd_bf16', ctx.in_dtype, gy.data_ptr(), idx.data_ptr(), N, H, W, C, gx.data_ptr(), _stream(gy))
        return gx


class _Conv1x1ToPlanes(torch.autograd.Function):
    """1x1 convolution without bias from an NHWC bf16 map to NCHW bf16 planes as plain GEMMs:
    out[b] (Co x HW) = W (Co x Ci) x[b]^T, x[b] the (HW x Ci) token rows."""

    @staticmethod
    def forward(ctx, x, weight):
        B, H, W, Ci = x.shape
        Co = weight.shape[0]
        wb = fused.BF16_COPIES.get(weight).view(Co, Ci)
        out = torch.empty((B, Co, H, W), dtype=torch.bfloat16, device=x.device)
        for b in range(B):
            fused.gemm_bf16(wb, x[b].view(H * W, Ci), trans_b=True, out=out[b].view(Co, H * W))
        ctx.save_for_backward(x, wb)
        return out

    @staticmethod
    def backward(ctx, g):
        x, wb = ctx.saved_tensors
        B, H, W, Ci = x.shape
        Co = wb.shape[0]
        g = g.contiguous().to(torch.bfloat16)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            for b in range(B):
                fused.gemm_bf16(g[b].view(Co, H * W), wb, trans_a=True, out=dx[b].view(H * W, Ci))
        if ctx.needs_input_grad[1]:
            for b in range(B):
                part = fused.gemm_bf16(g[b].view(Co, H * W), x[b].view(H * W, Ci), out_dtype=torch.float32)
                dw = part if dw is None else dw.add_(part)
            dw = dw.view(Co, Ci, 1, 1)
        return dx, dw


def autocast_dtype():
    """The 16-bit type the NHWC path runs in under the active autocast: torch.bfloat16, torch.float16, or None (no
    autocast, another autocast type, or fp16 with its switch off: VAH_FUSED_DISABLE=fp16_spm, for A/B runs)."""
    return fused.autocast_16('fp16_spm')


def takes(spm, x, fold):
    """Does the backbone hand the module to forward()?  When the BatchNorm tail takes fc1's bias (``fold``: bf16
    autocast, and fp16 autocast with ENABLED['fp16_tail']); under fp16 autocast also without it, whenever usable() holds
    (the tail is then torch's and forward() adds the bias)."""
    if not (fold or autocast_dtype() == torch.float16):
        return False
    return usable(spm, x) and not (spm.with_cp and x.requires_grad)


def usable(spm, x):
    """The NHWC path serves the module as the reference builds it (3x3 / padding 1 / bias-free convolutions with
    64-multiple widths, (Sync)BatchNorm + ReLU, the 3/2/1 max-pool) on a CUDA fp32 image under bf16 or fp16
    autocast."""
    # the image's own gradient is not produced by this path: an input that requires grad takes the module as written
    if not (fused.ENABLED.get('spm_nhwc', True) and x.is_cuda and x.dtype == torch.float32 and not x.requires_grad and x.dim() == 4 and x.shape[1] == 3
            and autocast_dtype() is not None and x.shape[2] % 32 == 0 and x.shape[3] % 32 == 0 and x.numel() > 0):
        return False
    convs = [spm.stem[0], spm.stem[3], spm.stem[6], spm.conv2[0], spm.conv3[0], spm.conv4[0]]
    for i, c in enumerate(convs):
        if not (isinstance(c, torch.nn.Conv2d) and c.kernel_size == (3, 3) and c.padding == (1, 1) and c.bias is None
                and c.groups == 1 and c.dilation == (1, 1) and c.out_channels % 64 == 0 and c.out_channels <= 256
                and (c.out_channels & (c.out_channels - 1)) == 0 and (i == 0 or c.in_channels % 64 == 0)
                and c.weight.dtype == torch.float32):
            return False
    norms = [spm.stem[1], spm.stem[4], spm.stem[7], spm.conv2[1], spm.conv3[1], spm.conv4[1]]
    return all(isinstance(n, torch.nn.modules.batchnorm._BatchNorm) and n.momentum is not None
               and (n.training or n.running_mean is not None) for n in norms)


def _cbr(conv_mod, norm, x):
    y = _Conv3x3.apply(x, conv_mod.weight, conv_mod.stride[0])
    return _BNRelu.apply(y, norm.weight, norm.bias, norm, True)


def _fc1_planes_f16(fc1, c1, with_bias):
    """fc1 (1x1 convolution) of the NHWC fp16 map c1 as NCHW fp16 planes: out[b] (Co x HW) = W (Co x Ci) x[b]^T, one
    batched library GEMM on the token rows (no layout copy of the activations), plain autograd."""
    B, H, W, Ci = c1.shape
    Co = fc1.weight.shape[0]
    w = fc1.weight.view(1, Co, Ci).expand(B, Co, Ci)
    rows_t = c1.view(B, H * W, Ci).transpose(1, 2)
    if with_bias and fc1.bias is not None:
        out = torch.baddbmm(fc1.bias.view(1, Co, 1), w, rows_t)
    else:
        out = torch.bmm(w, rows_t)
    return out.view(B, Co, H, W)


def forward(spm, x, level_embed, c1_bias=False):
    """-> (c1, c): c1 = fc1's output as NCHW 16-bit planes, WITHOUT its bias unless ``c1_bias`` (the caller folds the
    bias into the BatchNorm tail; only under fp16 with ENABLED['fp16_tail'] off, where the tail is torch's, does it ask
    for the bias),
    c = cat([fc_l(c_l) + level_embed[l-2] for l = 2, 3, 4]) as (B, T, E) fp32 token rows."""
    dtype = autocast_dtype() or torch.bfloat16
    t = image_to_nhwc16(x, dtype)
    t = _cbr(spm.stem[0], spm.stem[1], t)
    t = _cbr(spm.stem[3], spm.stem[4], t)
    t = _cbr(spm.stem[6], spm.stem[7], t)
    c1 = _MaxPool.apply(t)
    c2 = _cbr(spm.conv2[0], spm.conv2[1], c1)
    c3 = _cbr(spm.conv3[0], spm.conv3[1], c2)
    c4 = _cbr(spm.conv4[0], spm.conv4[1], c3)
    B = x.shape[0]
    toks = []
    if dtype == torch.float16:
        # the 1x1 projections are GEMMs: torch's fp16 library calls on the NHWC rows, as every Linear in this mode
        for l, (fc, c) in enumerate(((spm.fc2, c2), (spm.fc3, c3), (spm.fc4, c4))):
            w = fc.weight.view(fc.weight.shape[0], fc.weight.shape[1])
            toks.append(F.linear(c.view(B, -1, c.shape[-1]), w, fc.bias + level_embed[l]))
        return _fc1_planes_f16(spm.fc1, c1, c1_bias), torch.cat(toks, dim=1).float()
    assert not c1_bias, 'bf16: fc1.bias travels to the BatchNorm tail'
    for l, (fc, c) in enumerate(((spm.fc2, c2), (spm.fc3, c3), (spm.fc4, c4))):
        w = fc.weight.view(fc.weight.shape[0], fc.weight.shape[1])
        toks.append(fused._LinearBF16.apply(c.view(B, -1, c.shape[-1]), w, fc.bias + level_embed[l]))
    return _Conv1x1ToPlanes.apply(c1, spm.fc1.weight), torch.cat(toks, dim=1).float()
