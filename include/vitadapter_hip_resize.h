/*
 * vitadapter_hip_resize.h -- C ABI of libvitadapter_hip.so, fourth part: bilinear resize on channels-last rows
 * (csrc/resize_rows.hip).  Conventions, error codes and the ABI version are those of vitadapter_hip.h (adding symbols
 * does not move the version); layout, dtype codes, alignment and stride rules are those of vitadapter_hip_group_norm.h.
 *
 * Replaces the F.interpolate(..., mode='bilinear', align_corners=False) of the FPN tail in Mask2Former's pixel decoder
 * (segmentation/mmseg_custom/models/plugins/msdeformattn_pixel_decoder.py:258-262: cur_feat + F.interpolate(outs[-1],
 * size=cur_feat.shape[-2:], mode='bilinear', align_corners=False)) and its adjoint upsample_bilinear2d_backward, which torch runs as fp32 NCHW operators -
 * the adjoint with float atomics.
 *
 *   semantics  torch's upsample_bilinear2d for size= (no scale factor), per axis with `in` input and `out` output positions:
 *                align_corners == 0:  scale = (float)in / out,  src = max(scale * (dst + 0.5f) - 0.5f, 0)
 *                align_corners != 0:  scale = out > 1 ? (float)(in - 1) / (out - 1) : 0,  src = scale * dst
 *                i0 = min((int)src, in - 1),  i1 = i0 + (i0 < in - 1),  l1 = min(max(src - i0, 0), 1),  l0 = 1 - l1
 *              every operation of src rounded to fp32 on its own (no fused multiply-add), and
 *                y = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11)
 *              with all four products always taken: a zero weight times inf is NaN, as in torch.
 *   layout     rows: element [n][t][c] sits at n * img_stride + t * row_stride + c, t = y * W + x (strides in ELEMENTS).
 *              The input of the forward (and dx of the backward) may be a level's rows of an (Lq, N, C) buffer.
 *   dtypes     0 fp32, 1 bf16, 2 fp16 per operand; bf16 and fp16 never meet in one call (VAH_E_UNSUPPORTED).  All arithmetic
 *              is fp32; each output element is rounded once, at its store (fp16 overflows to inf).
 *   shapes     C a multiple of 8 (else VAH_E_UNSUPPORTED): a thread owns one 16-byte piece - 8 channels - of a pixel.
 *              Any Hi, Wi, Ho, Wo >= 1: upsampling, downsampling, identity.  A negative size, an empty source for a
 *              non-empty result, N > 65535 or an image of 2^31 or more pieces is VAH_E_SHAPE.
 *   alignment  every tensor pointer 16-byte aligned, every stride a multiple of 8 elements (VAH_E_ALIGN);
 *              row_stride >= C (VAH_E_SHAPE).
 *   workspace  vah_resize_rows_ws_bytes(Hi, Wi, Ho, Wo) bytes, 16-byte aligned: per output row and column (i0, i1, l1, l0),
 *              per input row and column the range [lo, hi) of output rows / columns that tap it.  A smaller ws_bytes is
 *              VAH_E_SHAPE ("workspace too small").  The backward fills it with one small launch of its own; the forward
 *              computes its taps in registers (by the same function) and only checks the argument.
 *   order      argument checks come before any device work; N * Ho * Wo == 0 (forward) or N * Hi * Wi == 0 (backward)
 *              returns VAH_OK and reads no pointer.
 *
 * vah_resize_rows_forward   y[n][oy * Wo + ox][c] from the four taps of x.
 * vah_resize_rows_backward  the exact transpose, as a gather: a thread owns 8 channels of an INPUT pixel and adds, output rows
 *                           ascending and columns ascending within a row, w * dy of every output pixel that taps it, where
 *                           w = wy * wx and wy = (i0 == iy ? l0 : 0) + (i1 == iy ? l1 : 0) from the forward's own taps (a
 *                           border-clamped output, i0 == i1, gives l0 + l1); fp32 accumulators, one store, zeros where
 *                           nothing taps.  No atomics, counters or flags, nothing read back to the host: the call captures
 *                           into a graph, and the same inputs give the same bits.
 *   profile    rows resize_rows_fwd, resize_rows_bwd, with `_f16` appended where a 16-bit operand is fp16.
 */
#ifndef VITADAPTER_HIP_RESIZE_H
#define VITADAPTER_HIP_RESIZE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t vah_resize_rows_ws_bytes(int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo);
int vah_resize_rows_forward(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride,
                            int64_t N, int64_t C, int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo, int align_corners,
                            void *y, int y_dtype, int64_t y_row_stride, int64_t y_img_stride,
                            void *ws, int64_t ws_bytes, void *stream);
int vah_resize_rows_backward(const void *dy, int dy_dtype, int64_t dy_row_stride, int64_t dy_img_stride,
                             int64_t N, int64_t C, int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo, int align_corners,
                             void *dx, int dx_dtype, int64_t dx_row_stride, int64_t dx_img_stride,
                             void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_RESIZE_H */
