// Cross-file hooks of the MSDA kernels (not part of the C ABI).
#pragma once
#include "../../include/vitadapter_hip_msda_box.h"
#include "common.h"

namespace vah {

// d(loc), d(attn) of the plain fp32 backward WITHOUT the grad_value scatter (msda.hip: msda_bwd_lanec<32, PU, false>;
// spec cuh:301-403 minus its col2im atomics).  D must be 32.
int msda_grad_taps_f32(const float *value, const int64_t *shapes, const int64_t *lsi, const float *loc, const float *attn,
                       const float *grad_out, int64_t N, int64_t S, int64_t M, int64_t D, int64_t L, int64_t Lq, int64_t P,
                       float *grad_loc, float *grad_attn, hipStream_t st);

// Rows of the fused core's reference points between consecutive images: Lq for a per-image grid (ref_batch == N > 1),
// 0 for one the batch shares.
int64_t msda_ref_rows_per_image(int64_t ref_batch, int64_t N, int64_t Lq);

// d(offsets), d(logits) of the fused core, nothing scattered (msda_fused.hip: msda_fused_bwd_vec4 / msda_fused_bwd).
// rq: msda_ref_rows_per_image.  ref_comps: 2 (points) or 4 (boxes).  D: 32, or 64 with fp32 values.
int msda_fused_grad_taps(const void *value, int value_dtype, const int64_t *shapes, const int64_t *lsi, const void *offsets,
                         const void *logits, int param_dtype, const float *ref, int64_t ref_levels, int64_t rq,
                         int64_t ref_comps, const void *grad_out, int64_t N, int64_t S, int64_t M, int64_t D, int64_t L,
                         int64_t Lq, int64_t P, void *d_offsets, void *d_logits, hipStream_t st);

// Components of a reference of the fused core: 2 or 4; VAH_OK, or VAH_E_SHAPE with the message set.
int msda_check_ref_comps(const char *fn, int64_t ref_comps);

// Dtype codes of the fused core: 0 = fp32, 1 = bf16, 2 = fp16.  fp32 and bf16 mix freely between values and
// parameters; fp16 comes in one form (values, offsets, logits - and every gradient - fp16) and only where f16_ok:
// the forward entry points and the tiled backward.  VAH_OK, or VAH_E_UNSUPPORTED with the message set.
int msda_check_dtypes(const char *fn, int value_dtype, int param_dtype, bool f16_ok);
inline int64_t msda_dtype_bytes(int code) { return code == 0 ? 4 : 2; }

}  // namespace vah
