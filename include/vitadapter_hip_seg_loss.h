/*
 * vitadapter_hip_seg_loss.h -- C ABI of libvitadapter_hip.so, ninth part: the training loss of the UperNet heads
 * (csrc/seg_ce_loss.hip).  Conventions, error codes and the ABI version are those of vitadapter_hip.h (adding symbols does
 * not move the version): argument checks come before any device work, strides are in ELEMENTS, an empty problem returns
 * VAH_OK and reads no pointer.
 *
 * Replaces mmseg's BaseDecodeHead.losses as the reference's UperNet configs run it: resize(seg_logit, size=seg_label.shape[2:],
 * mode='bilinear'), the reference's CrossEntropyLoss (segmentation/mmseg_custom/models/losses/cross_entropy_loss.py:11-62:
 * F.cross_entropy(reduction='none', ignore_index=...) and a sum) and the top-1 count of `accuracy`, forward and backward,
 * without a tensor of N * C * H * W elements: the training counterpart of the seventh part's finish call, on the same tap
 * function (csrc/resize_tap.h).
 *
 *   logits     (N, C, h, w) NCHW, element [n][c][y][x] at n * img_stride + c * plane_stride + y * row_stride + x (column
 *              stride 1), dtype code 0 fp32, 1 bf16, 2 fp16 (VAH_E_UNSUPPORTED otherwise).  Every value is converted to
 *              fp32 first (mmseg's @force_fp32) and all arithmetic is fp32.  row_stride >= w,
 *              plane_stride >= (h - 1) * row_stride + w, img_stride >= (C - 1) * plane_stride + that: planes never overlap
 *              (VAH_E_SHAPE).  dlogits: the same shape and dtype with strides of its own.
 *   labels     int64 (N, H, W), [n][y][x] at n * img_stride + y * row_stride + x, under the same stride rules.  A pixel is
 *              VALID if label != ignore_index and 0 <= label < C.  A label outside [0, C) that is not ignore_index is
 *              treated as IGNORED: torch raises a device assert there, here nothing is read out of bounds and the pixel
 *              counts for nothing.
 *   resize     v[c] = the bilinear blend of the four taps of class c at the output pixel, by exactly the tap rule of
 *              vitadapter_hip_resize.h and the blend of vitadapter_hip_seg.h's header text: every product and sum rounded on
 *              its own, all four products always taken (a zero weight times inf is NaN, as in torch).
 *   class_weight  fp32 [C], or NULL: all ones.
 *   order      no float atomics, counters or flags, nothing read back to the host: the same inputs give the same bits, and
 *              both calls capture into a graph.
 *   limits     sizes >= 0 and < 2^31, N <= 65535, planes of fewer than 2^31 pixels (VAH_E_SHAPE); an empty source for a
 *              non-empty result is VAH_E_SHAPE.  fp32 pointers 4-byte, 16-bit logits 2-byte, labels and counts 8-byte,
 *              the workspace 16-byte aligned (VAH_E_ALIGN).  Empty: N * C * H * W == 0.
 *
 * vah_sce_ws_bytes  bytes of workspace for either call (0 for an empty or impossible problem): the forward's per-workgroup
 *                   partials (12 bytes per 256 output pixels) and the backward's tap tables (H + W) and gather ranges
 *                   (h + w).  O(N * H * W + h + w + H + W), never O(N * C * H * W).
 * vah_sce_forward   per output pixel, over the C classes in one walk:
 *                     lse     = log sum_c exp(v[c]), running-maximum form, accurate expf / logf; NaN when a v[c] is NaN or
 *                               +inf or all are -inf, as torch's log_softmax gives
 *                     argmax  = the first index of the largest v[c], a NaN counting as largest
 *                   Outputs: lse fp32 (N, H, W) contiguous, written for EVERY pixel; loss_sum fp32 scalar = sum over the
 *                   valid pixels of class_weight[label] * (lse - v[label]) (an ignored pixel adds 0 whatever its logits
 *                   hold; a valid pixel with a NaN lse makes the sum NaN); counts int64[2] = {valid pixels, valid pixels
 *                   whose argmax is the label}.  A workgroup of 256 pixels writes one partial of each; a second launch of
 *                   one workgroup adds them in a fixed order (the counts as integers).  Profile row sce_forward.
 * vah_sce_backward  dlogits[n][c][iy][ix] = sum over the output pixels (oy, ox) whose taps name (iy, ix), rows ascending and
 *                   columns ascending within a row, of
 *                     wy * wx * scale * class_weight[label] * (exp(v[c] - lse) - [c == label])
 *                   with wy, wx the weights of the forward's own taps (a clamped tap, named twice, gives l0 + l1), `scale`
 *                   a DEVICE fp32 scalar (grad_output * loss_weight / avg_factor, formed by the caller) and lse the
 *                   forward's output.  fp32 accumulators, one store per element in the logits' dtype, zeros where no
 *                   valid pixel taps.  An ignored pixel with a finite lse adds exactly nothing; an ignored pixel whose lse
 *                   is not finite adds NaN to every class of the pixels it taps (torch: 0 * NaN for the offending class
 *                   at least).  Two launches: tables, gather.  Profile row sce_backward.
 */
#ifndef VITADAPTER_HIP_SEG_LOSS_H
#define VITADAPTER_HIP_SEG_LOSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t vah_sce_ws_bytes(int64_t N, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W);
int vah_sce_forward(const void *logits, int logits_dtype, int64_t logits_img_stride, int64_t logits_plane_stride,
                    int64_t logits_row_stride, int64_t N, int64_t C, int64_t h, int64_t w, const void *labels,
                    int64_t labels_img_stride, int64_t labels_row_stride, int64_t H, int64_t W, int align_corners,
                    int64_t ignore_index, const void *class_weight, void *lse, void *loss_sum, void *counts, void *ws,
                    int64_t ws_bytes, void *stream);
int vah_sce_backward(const void *logits, int logits_dtype, int64_t logits_img_stride, int64_t logits_plane_stride,
                     int64_t logits_row_stride, int64_t N, int64_t C, int64_t h, int64_t w, const void *labels,
                     int64_t labels_img_stride, int64_t labels_row_stride, int64_t H, int64_t W, int align_corners,
                     int64_t ignore_index, const void *class_weight, const void *lse, const void *scale, void *dlogits,
                     int64_t dlogits_img_stride, int64_t dlogits_plane_stride, int64_t dlogits_row_stride, void *ws,
                     int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_SEG_LOSS_H */
