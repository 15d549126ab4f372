/*
 * vitadapter_hip_group_norm.h -- C ABI of libvitadapter_hip.so, third part: GroupNorm on channels-last rows
 * (csrc/group_norm.hip).  Conventions, error codes and the ABI version are those of vitadapter_hip.h (adding symbols
 * does not move the version).
 *
 * Replaces nn.GroupNorm(G, C) forward and backward in the ConvModules of Mask2Former's pixel decoder
 * (segmentation/mmseg_custom/models/plugins/msdeformattn_pixel_decoder.py:84-124: 1x1 conv -> GN, 3x3 conv -> GN ->
 * ReLU), which torch runs as an fp32 NCHW operator under autocast.
 *
 *   layout     channels-last rows: element x[n][t][c] sits at n * img_stride + t * row_stride + c (strides in ELEMENTS,
 *              the c run contiguous).  A contiguous (N, T, C) tensor - an NHWC map with T = H * W - has row_stride = C,
 *              img_stride = T * C; a level's slice of an (Lq, N, C) query buffer has row_stride = N * C, img_stride = C.
 *   dtypes     every tensor operand carries a code: 0 fp32, 1 bf16, 2 fp16.  bf16 and fp16 never meet in one call
 *              (VAH_E_UNSUPPORTED).  All arithmetic, the statistics, sums and the workspace are fp32; each output element is
 *              rounded once, at its store (to nearest even; fp16 overflows to inf and keeps subnormals).
 *   shapes     C a power of two in [64, 512], C / G in {1, 2, 4, 8}: eight consecutive channels of a pixel - one 16-byte
 *              load of 16-bit data, two of fp32 - hold whole groups.  vah_group_norm_supported(C, G) answers on the host;
 *              anything else is VAH_E_UNSUPPORTED.
 *   alignment  every tensor pointer 16-byte aligned, every stride a multiple of 8 elements (VAH_E_ALIGN);
 *              row_stride >= C (VAH_E_SHAPE).
 *   workspace  vah_group_norm_ws_floats(N, T, C, G) floats for vah_group_norm_stats and vah_group_norm_bwd_stats; a
 *              smaller ws_floats is VAH_E_SHAPE ("workspace too small").
 *   order      argument checks come before any device work; N * T == 0 returns VAH_OK and reads no pointer.
 *   sums       a workgroup adds a chunk of an image's rows into one partial row of the workspace; a second launch adds
 *              the partial rows in a fixed order.  No atomics, no waiting between workgroups, nothing read back to the
 *              host: the calls capture into a graph, and the same inputs give the same bits.
 *
 * vah_group_norm_stats      mean[N * G], rstd[N * G] (fp32): mean = sum / cnt, var = max(sumsq / cnt - mean^2, 0)
 *                           (biased; a NaN stays a NaN), rstd = 1 / sqrt(var + eps), cnt = T * C / G - the arithmetic of
 *                           vah_bn_nhwc_stats + vah_bn_finalize_stats.
 * vah_group_norm_apply      y = [relu](x * sc + sh) [+ add],  sc = rstd * w[c], sh = b[c] - mean * sc (one fma);
 *                           w, b fp32 or NULL (1, 0); add: contiguous (N, T, C) in y's dtype, or NULL.
 * vah_group_norm_bwd_stats  g' = dy where x * sc + sh > 0 (all of dy without relu; the mask is recomputed, y is not
 *                           saved), xhat = (x - mean) * rstd:
 *                             gsums[n * G + g]         = sum over the group's channels and rows of g' w
 *                             gsums[N * G + n * G + g] = sum of g' w xhat
 *                             dgamma[c] = sum over images and rows of g' xhat,  dbeta[c] = sum of g'   (NULL: not written)
 * vah_group_norm_bwd_apply  dx = rstd * (g' w - m1 - xhat * m2),  m1 = gsums[n * G + g] / cnt, m2 = gsums[N * G + ...] / cnt.
 *                           The gradient of `add` is dy itself.
 *   profile    rows gn_stats, gn_apply, gn_bwd_stats, gn_bwd_apply, with `_f16` appended where a 16-bit operand is fp16.
 */
#ifndef VITADAPTER_HIP_GROUP_NORM_H
#define VITADAPTER_HIP_GROUP_NORM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int vah_group_norm_supported(int64_t C, int64_t G);
int64_t vah_group_norm_ws_floats(int64_t N, int64_t T, int64_t C, int64_t G);
int vah_group_norm_stats(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride,
                         int64_t N, int64_t T, int64_t C, int64_t G, float eps,
                         float *mean, float *rstd, float *ws, int64_t ws_floats, void *stream);
int vah_group_norm_apply(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride,
                         int64_t N, int64_t T, int64_t C, int64_t G,
                         const float *mean, const float *rstd, const float *w, const float *b, int relu,
                         const void *add, void *y, int y_dtype, int64_t y_row_stride, int64_t y_img_stride,
                         void *stream);
int vah_group_norm_bwd_stats(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride,
                             const void *dy, int dy_dtype, int64_t dy_row_stride, int64_t dy_img_stride,
                             int64_t N, int64_t T, int64_t C, int64_t G,
                             const float *mean, const float *rstd, const float *w, const float *b, int relu,
                             float *gsums, float *dgamma, float *dbeta, float *ws, int64_t ws_floats,
                             void *stream);
int vah_group_norm_bwd_apply(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride,
                             const void *dy, int dy_dtype, int64_t dy_row_stride, int64_t dy_img_stride,
                             int64_t N, int64_t T, int64_t C, int64_t G,
                             const float *mean, const float *rstd, const float *w, const float *b, int relu,
                             const float *gsums, void *dx, int dx_dtype, int64_t dx_row_stride,
                             int64_t dx_img_stride, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_GROUP_NORM_H */
