// The bilinear tap rule of include/vitadapter_hip_resize.h, shared by the kernels that resize: csrc/resize_rows.hip
// (channels-last rows), csrc/seg_logits.hip (NCHW logit planes) and csrc/seg_ce_loss.hip (the loss on resized logits).
// One function, so that every resize in the library gets the same indices and fractions as torch's
// upsample_bilinear2d for size= (no scale factor).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vah {
namespace {

struct Tap {
    int i0, i1;
    float l1, l0;
};

struct Axis {
    int in, out;
    float scale;
    int align;
};

// a product that stays a value of its own: HIP's __fmul_rn / __fadd_rn are plain * and + inside the header and
// `#pragma clang fp contract(off)` is not honoured under -ffp-contract=fast - either way the ISA showed v_fma_f32 for
// scale * (dst + 0.5) - 0.5.  An empty asm that "rewrites" the register keeps the multiply apart from what consumes it.
__device__ __forceinline__ float mul_rn(float a, float b) {
    float p = a * b;
    asm("" : "+v"(p));
    return p;
}

// torch's area_pixel_compute_source_index + guard_index_and_lambda; every operation of src rounded on its own, so that a
// restatement in fp32 gets the same indices and fractions whatever the contraction mode
__device__ __forceinline__ Tap tap_of(const Axis a, int dst) {
    const float d = (float)dst;
    const float src = a.align ? mul_rn(a.scale, d) : fmaxf(mul_rn(a.scale, d + 0.5f) - 0.5f, 0.f);
    Tap t;
    t.i0 = min((int)src, a.in - 1);
    t.i1 = t.i0 + (t.i0 < a.in - 1 ? 1 : 0);
    t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
    t.l0 = 1.f - t.l1;
    return t;
}

// the value of the four taps with every product and sum rounded on its own (so two evaluations give the same bits wherever
// the compiler inlines them) and all four products taken: 0 * inf = NaN as in torch
__device__ __forceinline__ float blend_rn(const Tap ty, const Tap tx, float v00, float v01, float v10, float v11) {
    float r0 = mul_rn(tx.l0, v00) + mul_rn(tx.l1, v01);
    float r1 = mul_rn(tx.l0, v10) + mul_rn(tx.l1, v11);
    asm("" : "+v"(r0));
    asm("" : "+v"(r1));
    return mul_rn(ty.l0, r0) + mul_rn(ty.l1, r1);
}

// the weight with which the output position of tap t reads input position i (0 if it does not)
__device__ __forceinline__ float weight_of(const Tap t, int i) { return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f); }

// first output position in [0, out] whose i1 (UPPER = false) reaches i / whose i0 (UPPER = true) exceeds i: the tap
// indices are monotone, so [bisect<false>, bisect<true>) are the output positions whose taps name input position i
template <bool UPPER>
__device__ __forceinline__ int bisect(const Axis a, int i) {
    int lo = 0, hi = a.out;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const Tap t = tap_of(a, mid);
        if (UPPER ? t.i0 > i : t.i1 >= i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

inline Axis axis_of(int64_t in, int64_t out, int align) {
    Axis a;
    a.in = (int)in, a.out = (int)out, a.align = align ? 1 : 0;
    a.scale = align ? (out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f) : (float)in / (float)out;
    return a;
}

}  // namespace
}  // namespace vah
