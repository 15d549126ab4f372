/*
 * vitadapter_hip_point_mask_loss.h -- C ABI of libvitadapter_hip.so, eighth part: the sampled mask losses of the matched
 * queries of Mask2Former's training head and their backward into mask_pred (csrc/point_mask_loss.hip).  Conventions, error
 * codes, the dtype codes of a map (0 fp32, 3 uint8), the sampling convention and the ABI version are those of
 * vitadapter_hip_points.h (adding symbols does not move the version): argument checks come before any device work, strides
 * are in ELEMENTS, a zero-size call (K == 0) returns VAH_OK and reads no pointer, P <= 0 is VAH_E_SHAPE.
 *
 * Replaces, in the reference's Mask2FormerHead.loss (segmentation/mmseg_custom/models/decode_heads/mask2former_head.py:338-356),
 * the point_sample of the matched mask_pred rows and of their targets, CrossEntropyLoss(use_sigmoid=True) and
 * DiceLoss(naive_dice=True) before their reduction, and the backward of all three into mask_pred, for one decoder output.
 *
 * All math is fp32 with the accurate expf / log1pf.  No floating-point atomics, no counters or flags between workgroups beyond
 * kernel boundaries, nothing read back to the host: the same inputs give the same bits, in every output, and a row's bits do
 * not depend on which other rows the call has or on the row's position k.  (The backward counts points per cell with integer
 * atomics; an integer count does not depend on the order of its increments, and the lists they place are sorted before use.)
 *
 * A sample is that of vah_pts_sample, from the same device function: x = fma(px, w, -0.5), floor, taps x0 and x0 + 1 with
 * weights 1 - fx and fx, the same in y, value = ((wy0 wx0 v00 + wy0 wx1 v01) + wy1 wx0 v10) + wy1 wx1 v11.  A tap outside the
 * map is not part of the sum and forms no address; an in-range tap is always multiplied, so a non-finite value propagates as in
 * torch (0 * inf = NaN).
 *
 * vah_pml_ws_bytes   bytes of workspace either call needs for (K, P, h, w) (the larger of the two); 0 for an empty or bad shape.
 *                    16-byte aligned, contents undefined between calls.
 * vah_pml_forward    Row k samples map rows[k] of pred ((Mp, h, w) fp32: element [m][y][x] at m * pred_map_stride +
 *                    y * pred_row_stride + x; read in place, no gathered copy) and map tgt_rows[k] of tgt ((Mt, H, W), fp32 or
 *                    uint8, at its own resolution) at points[k] ((K, P, 2) fp32 contiguous, (x, y), x first).  rows and tgt_rows
 *                    are int32[K] on the device, NULL = identity (needs K <= Mp / K <= Mt: VAH_E_SHAPE otherwise); an index read
 *                    on the device that is out of range makes every output of its row NaN, no address is formed from it.
 *                    With x_p, t_p the two samples, s = sigmoid(x) taken from the same exp(-|x|) as softplus(x) = max(x, 0) +
 *                    log1p(exp(-|x|)):
 *                        bce[k]  = sum_p softplus(x_p) - x_p t_p
 *                        A = sum_p s_p t_p, B = sum_p s_p, T = sum_p t_p, D = (B + T) + eps
 *                        dice[k] = 1 - (2 A + eps) / D
 *                    Outputs, fp32 contiguous, every element written: bce (K,), dice (K,), xs (K, P), ts (K, P) and
 *                    sums (K, 4) = (A, B, T, bce), the last three kept for the backward.
 *                    Two launches.  pml_forward: a workgroup of 256 threads owns 1024 consecutive points of a row, chunk c =
 *                    points [1024 c, 1024 c + 1024); it writes xs and ts and four partial sums into the workspace.
 *                    pml_merge: one thread per row adds the row's chunks.
 *                    Order of every sum over p: lane l of the workgroup adds p = 1024 c + l, + 256, + 512, + 768 in ascending
 *                    order (a serial run of 4; a point p >= P is not added), the 64 lanes of a wave are added in a butterfly
 *                    of 6 levels (distances 1, 2, within 8, within 16, 16, 32), the four waves in ascending order, then the
 *                    ceil(P / 1024) chunks in ascending order starting from the first chunk's sum.
 * vah_pml_backward   dmaps (K, h, w) fp32 contiguous, every element written: the gradient of sum_k g_bce[k] bce[k] +
 *                    g_dice[k] dice[k] with respect to the K sampled maps (row k of dmaps belongs to pred map rows[k]; the
 *                    caller adds rows that name the same map).  From xs, ts, sums of the forward and points:
 *                        gx[k][p] = g_bce[k] (s_p - t_p) + g_dice[k] s_p (1 - s_p) ((2 A + eps) / D^2 - 2 t_p / D)
 *                        dmaps[k][y][x] = sum over the points p with a tap on (y, x) of weight(p, tap) gx[k][p]
 *                    with the tap weights of the forward.  A point's tap outside the map is dropped, as in the forward.
 *                    Gather form: the points of a row are binned by cell, cell(p) = (y0 + 1) * (w + 1) + (x0 + 1) over the
 *                    (h + 1) * (w + 1) cells with an in-range tap (integer counts, an exclusive scan, a fill, each list sorted by
 *                    point index), then one thread per pixel walks the lists of its four cells.
 *                    Order of the sum of a pixel (y, x): it starts from +0.0; the cells (y0, x0) = (y - 1, x - 1), (y - 1, x),
 *                    (y, x - 1), (y, x) in this order (ascending cell number; the pixel is their tap 11, 10, 01, 00); within
 *                    a cell in ascending order of the point index p; each term is (wy wx) gx, added serially.  A pixel no
 *                    point touches is exactly +0.0.  A non-finite gx reaches every in-range tap of its point (0 * NaN = NaN).
 *                    Five launches after one memset of the counts: pml_bwd_gx (gx and the counts), pml_bwd_scan (a workgroup
 *                    per row), pml_bwd_fill, pml_bwd_sort (a thread per cell, insertion sort: lists are one or two points long
 *                    in training, and a row whose P points share one cell is still right, only slow), pml_bwd_gather.
 * shapes      1 <= h, w, H, W; row strides >= the width, map strides >= 0, (h + 1) * (w + 1) < 2^31 and h * row stride < 2^31
 *             for both maps; 1 <= P (P <= 0 is VAH_E_SHAPE), K * max(P, (h + 1) * (w + 1)) < 2^31.  Zero size: K == 0.
 *             Nothing in the design bounds h * w or P by an on-chip memory: there is no VAH_E_UNSUPPORTED shape, only the dtype
 *             codes.  A workspace smaller than vah_pml_ws_bytes is VAH_E_SHAPE.
 * alignment   points 8-byte aligned; the workspace 16-byte; fp32 and int32 arrays 4-byte; a uint8 map none.  VAH_E_ALIGN otherwise.
 */
#ifndef VITADAPTER_HIP_POINT_MASK_LOSS_H
#define VITADAPTER_HIP_POINT_MASK_LOSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t vah_pml_ws_bytes(int64_t K, int64_t P, int64_t h, int64_t w);
int vah_pml_forward(const void *pred, int64_t pred_map_stride, int64_t pred_row_stride, int64_t Mp, int64_t h, int64_t w,
                    const void *tgt, int tgt_dtype, int64_t tgt_map_stride, int64_t tgt_row_stride, int64_t Mt, int64_t H, int64_t W,
                    const void *points, int64_t P, const void *rows, const void *tgt_rows, int64_t K, float dice_eps, void *bce,
                    void *dice, void *xs, void *ts, void *sums, void *ws, int64_t ws_bytes, void *stream);
int vah_pml_backward(const void *points, const void *xs, const void *ts, const void *sums, const void *g_bce, const void *g_dice,
                     int64_t K, int64_t P, int64_t h, int64_t w, float dice_eps, void *dmaps, void *ws, int64_t ws_bytes,
                     void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_POINT_MASK_LOSS_H */
