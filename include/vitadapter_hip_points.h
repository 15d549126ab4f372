/*
 * vitadapter_hip_points.h -- C ABI of libvitadapter_hip.so, sixth part: point sampling and the matching cost of Mask2Former's
 * training head (csrc/point_loss.hip).  Conventions, error codes and the ABI version are those of
 * vitadapter_hip.h (adding symbols does not move the version): argument checks come before any device work, strides are in
 * ELEMENTS, a zero-size call returns VAH_OK and reads no pointer.
 *
 * Replaces, in the reference's Mask2FormerHead.loss (segmentation/mmseg_custom/models/decode_heads/mask2former_head.py:154-402),
 * mmcv's point_sample where it needs no gradient (matching, ground truth, the oversample step) and the three match costs of
 * MaskHungarianAssigner (models/losses/match_costs.py).  The sampled BCE and dice of the matched masks and their backward into
 * mask_pred are not part of this header: they are vitadapter_hip_point_mask_loss.h's, from the same sampling function.
 *
 * All math is fp32 with the accurate expf / log1pf.  No atomics, no counters or flags between workgroups, nothing read back
 * to the host: launches are ordered by kernel boundaries on the stream only, and the same inputs give the same bits.
 *
 * dtype codes of a map: 0 fp32, 3 uint8 (this header only: ground-truth masks as stored, 0 / 1 or bool; the byte's value is
 * the map's value).  Any other code is VAH_E_UNSUPPORTED.
 * index arrays (map_idx, set_idx) are int32 on the device; NULL means identity (row r names map r / set r), which needs
 * R <= M (R <= S): VAH_E_SHAPE otherwise, the one index error the host can see.  An index read on the device that is out of
 * range makes its row NaN: no address is formed from it.
 *
 * Sampling convention: mmcv point_sample(input, points, align_corners=False) = F.grid_sample(input, 2 * points - 1, 'bilinear',
 * 'zeros', align_corners=False).  A point is (px, py), x first, finite fp32, possibly outside [0, 1]:
 *     x = fma(px, w, -0.5), x0 = floor(x), fx = x - x0: taps x0 and x0 + 1 with weights 1 - fx and fx; the same in y.
 *     value = ((wy0 wx0 v00 + wy0 wx1 v01) + wy1 wx0 v10) + wy1 wx1 v11
 * A tap outside [0, w) x [0, h) is not part of the sum (its address is never formed: the load goes to a clamped, in-range
 * element whose value is discarded).  An in-range tap is always multiplied, so a non-finite map value reaches the output as
 * in torch (0 * inf = NaN).
 *
 * vah_pts_sample      out[r][p] = sample of map map_idx[r] at point p of set set_idx[r].  maps (M, h, w): element [m][y][x]
 *                     at m * map_stride + y * row_stride + x; points (S, P, 2) fp32 contiguous; out (R, P) fp32 contiguous,
 *                     every element written.  One thread per four points of a row, all sixteen taps loaded before the first is
 *                     used.  Profile row pts_sample.
 * vah_pts_match_cost  cost[n][q][g], (N, Q, Gmax) fp32 contiguous, of MaskHungarianAssigner for one decoder output:
 *                         w_cls * (-softmax(cls[n][q])[labels[g]])
 *                       + w_mask * (sum_p softplus(-x) t + softplus(x) (1 - t)) / P
 *                       + w_dice * (1 - (2 sum_p sigmoid(x) t + eps) / (sum_p sigmoid(x) + sum_p t + eps))
 *                     with x = xs[n * Q + q][p] (sampled predictions, (N * Q, P)), t = ts[gt_offsets[n] + g][p] (sampled ground
 *                     truth, (G_total, P); a bilinear sample of a 0 / 1 mask, so in [0, 1] and not binary), cls (N, Q, C1) fp32
 *                     with C1 = classes + 1, labels[G_total] int64, gt_offsets[N + 1] int32 (ascending, last = G_total).
 *                     softplus(x) = max(x, 0) + log1p(exp(-|x|)); sigmoid(x) from the same exp(-|x|).
 *                     Columns g >= G_n = gt_offsets[n + 1] - gt_offsets[n] are written as +inf; offsets or labels that are
 *                     out of range give +inf columns / NaN entries.  A workgroup of 256 threads owns (n, q, eight columns).
 *                     Order of every sum over p: lane l of the workgroup adds p = l, l + 256, ... in ascending order (a serial
 *                     run of ceil(P / 256)), the 64 lanes of a wave are added in a butterfly of 6 levels (distances 1, 2,
 *                     within 8, within 16, 16, 32), the four waves in ascending order.  Profile row pts_match_cost.
 * shapes      1 <= h, w and row_stride >= w, map_stride >= 0, (h + 1) * (w + 1) < 2^31, h * row_stride < 2^31; P >= 1
 *             (P <= 0 is VAH_E_SHAPE), P <= 2^31 - 1024 (sample) / P < 2^31 (cost).  Zero size: R == 0 (sample), N * Q * Gmax == 0 (cost).
 * alignment   points 8-byte aligned (a point is loaded as one 8-byte pair; a row of P points starts at 8 P bytes, so a wider
 *             load has no alignment to rely on when P is odd); fp32 and int32 arrays 4-byte, int64 arrays (labels) 8-byte aligned;
 *             uint8 maps none.  VAH_E_ALIGN otherwise.
 */
#ifndef VITADAPTER_HIP_POINTS_H
#define VITADAPTER_HIP_POINTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int vah_pts_sample(const void *maps, int map_dtype, int64_t map_stride, int64_t row_stride, int64_t M, int64_t h, int64_t w,
                   const void *points, int64_t S, int64_t P, const void *map_idx, const void *set_idx, int64_t R, void *out,
                   void *stream);
int vah_pts_match_cost(const void *xs, const void *ts, const void *gt_offsets, const void *cls, const void *labels, int64_t N,
                       int64_t Q, int64_t C1, int64_t G_total, int64_t Gmax, int64_t P, float w_cls, float w_mask, float w_dice,
                       float dice_eps, void *cost, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_POINTS_H */
