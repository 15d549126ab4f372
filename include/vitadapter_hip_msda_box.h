/*
 * vitadapter_hip_msda_box.h -- C ABI of libvitadapter_hip.so, second part: the fused MSDeformAttn core with
 * reference BOXES.  Conventions, error codes and the ABI version are those of vitadapter_hip.h (adding symbols does
 * not move the version); the tensors and dtype codes are those of vah_msda_fused_forward_nref /
 * vah_msda_fused_backward_tiled_nref there.
 *
 * Replaces, inside the reference's MSDeformAttn.forward, the second branch of
 * detection/ops/modules/ms_deform_attn.py:117-122
 *     if reference_points.shape[-1] == 2:
 *         sampling_locations = reference_points[:, :, None, :, None, :]
 *                              + sampling_offsets / offset_normalizer[None, None, None, :, None, :]
 *     elif reference_points.shape[-1] == 4:
 *         sampling_locations = reference_points[:, :, None, :, None, :2]
 *                              + sampling_offsets / self.n_points * reference_points[:, :, None, :, None, 2:] * 0.5
 * together with the softmax in front and MSDeformAttnFunction behind (:108-128), as the point form of the fused core
 * does.  It is the form every iterative-refinement decoder of the reference tree calls the op in
 * (segmentation/mmseg_custom/models/utils/transformer.py:595-615, wsdm2023/mmdet_custom/models/utils/transformer.py:
 * 93-118): the boxes (cx, cy, w, h) arrive detached and get no gradient here.
 *
 * The two entry points are vah_msda_fused_forward_nref and vah_msda_fused_backward_tiled_nref with one more argument,
 * ref_comps, directly after ref_batch:
 *   ref        (ref_batch, Lq, ref_levels, ref_comps) fp32; image n reads
 *              ref[((n * rq + q) * ref_levels + (ref_levels > 1 ? l : 0)) * ref_comps],  rq as for the *_nref functions
 *   ref_comps  2: points.  The *_nref call: same kernels, same bits.
 *              4: boxes.   loc = (cx, cy) + off * (0.5 / P) * (w, h), one fp32 fma per coordinate, in the forward, the
 *                 binning pass and the tile pass alike; d_offsets = d(out)/d(loc) * (w, h) * 0.5 / P, formed in fp32 from
 *                 the pixel-space gradient g the kernels accumulate as g * (W, H) * (w, h) * 0.5 / P BEFORE the one
 *                 rounding to a 16-bit gradient type (at D == 64: each half-head's fp32 partial record is scaled, the
 *                 finishing pass adds the two and rounds once).  d_logits and grad_value are those of the point form
 *                 at the same locations.  A NaN or +-inf box component makes every location it enters non-finite:
 *                 the rows it feeds are NaN, as for a non-finite offset.
 *              anything else: VAH_E_SHAPE, decided on the host before any HIP call.
 *   alignment  that of the *_nref functions; with ref_comps == 4 ref must be 16-byte aligned (VAH_E_ALIGN).
 *   errors     those of the *_nref functions: VAH_E_NULL, VAH_E_SHAPE (dims, ref_levels, ref_batch, ref_comps, a
 *              workspace that is too small), VAH_E_UNSUPPORTED (D not 32 / 64, (L, P) outside {1, 3, 4} x {4}, dtype
 *              codes, fp16 mixed with another type), VAH_E_ALIGN.  N * Lq * M == 0 returns VAH_OK and reads no pointer.
 *   workspace  vah_msda_tile_ws_bytes(N, S, M * (D / 32), L, Lq, P), as for the point form.
 *   profile    rows msda_fused_fwd[_f16] / msda_fused_bwd[_f16], as for the point form.
 *
 * Boxes exist where the tile pass serves (P == 4, L in {1, 3, 4}, D in {32, 64}, every dtype form of the tiled
 * backward, row-strided offsets / logits / gradients).  There is no box form of vah_msda_fused_forward_win (its
 * schedule comes from one shared point grid) nor of the atomic vah_msda_fused_backward[_nref].
 */
#ifndef VITADAPTER_HIP_MSDA_BOX_H
#define VITADAPTER_HIP_MSDA_BOX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int vah_msda_fused_forward_box(const void *value, int value_dtype, const int64_t *shapes, const int64_t *lsi,
                               const void *offsets, const void *logits, int param_dtype,
                               int64_t offsets_stride, int64_t logits_stride,
                               const float *ref, int64_t ref_levels, int64_t ref_batch, int64_t ref_comps,
                               int64_t N, int64_t S, int64_t M, int64_t D, int64_t L, int64_t Lq, int64_t P,
                               void *out, void *stream);
int vah_msda_fused_backward_tiled_box(const void *value, int value_dtype, const int64_t *shapes,
                                      const int64_t *lsi, const void *offsets, const void *logits,
                                      int param_dtype, int64_t offsets_stride, int64_t logits_stride,
                                      const float *ref, int64_t ref_levels, int64_t ref_batch, int64_t ref_comps,
                                      const void *grad_out, int64_t N, int64_t S, int64_t M, int64_t D,
                                      int64_t L, int64_t Lq, int64_t P, void *grad_value,
                                      int grad_value_dtype, void *d_offsets, void *d_logits,
                                      int grad_param_dtype, int64_t d_offsets_stride, int64_t d_logits_stride,
                                      void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_MSDA_BOX_H */
