// What the point kernels share (point_loss.hip, point_mask_loss.hip): the one statement of the sampling convention of
// include/vitadapter_hip_points.h (tap indices and fractions, clamped loads, the pinned sum of the four taps), the
// transcendental terms of a logit, the ordered workgroup sum and the host-side operand checks.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"

namespace vah {
namespace {

struct Taps {
    int x0, y0;       // clamped to [-2, w] / [-2, h]: anything further out has no tap in range either
    float fx, fy;
};

__device__ __forceinline__ Taps taps_of(float2 p, int h, int w) {
    const float x = __fmaf_rn(p.x, (float)w, -0.5f), y = __fmaf_rn(p.y, (float)h, -0.5f);
    const float xf = floorf(x), yf = floorf(y);
    Taps t;
    t.fx = x - xf;
    t.fy = y - yf;
    t.x0 = (int)fminf(fmaxf(xf, -2.f), (float)w);
    t.y0 = (int)fminf(fmaxf(yf, -2.f), (float)h);
    return t;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct Quad {
    float v[4];       // v00, v01, v10, v11 (y major)
};

// the four loads of a point, unconditional: clamped addresses
template <typename T>
__device__ __forceinline__ Quad load_quad(const T *__restrict__ map, int rs, int h, int w, const Taps t) {
    const int xa = clampi(t.x0, 0, w - 1), xb = clampi(t.x0 + 1, 0, w - 1);
    const int ya = clampi(t.y0, 0, h - 1) * rs, yb = clampi(t.y0 + 1, 0, h - 1) * rs;
    Quad q;
    q.v[0] = (float)map[ya + xa];
    q.v[1] = (float)map[ya + xb];
    q.v[2] = (float)map[yb + xa];
    q.v[3] = (float)map[yb + xb];
    return q;
}

// an in-range tap is always multiplied (0 * inf = NaN as in torch), a tap out of range is not part of the sum
__device__ __forceinline__ float combine(const Quad q, const Taps t, int h, int w) {
    const bool xa = t.x0 >= 0 && t.x0 < w, xb = t.x0 + 1 >= 0 && t.x0 + 1 < w;
    const bool ya = t.y0 >= 0 && t.y0 < h, yb = t.y0 + 1 >= 0 && t.y0 + 1 < h;
    const float wx0 = 1.f - t.fx, wx1 = t.fx, wy0 = 1.f - t.fy, wy1 = t.fy;
    const float c00 = ya && xa ? (wy0 * wx0) * q.v[0] : 0.f;
    const float c01 = ya && xb ? (wy0 * wx1) * q.v[1] : 0.f;
    const float c10 = yb && xa ? (wy1 * wx0) * q.v[2] : 0.f;
    const float c11 = yb && xb ? (wy1 * wx1) * q.v[3] : 0.f;
    return ((c00 + c01) + c10) + c11;
}

__device__ __forceinline__ float quiet_nan() { return __builtin_nanf(""); }

// ---------------------------------------------------------------------------------------
// transcendental terms of a logit, from one exp and one log1p
// ---------------------------------------------------------------------------------------
struct Terms {
    float s, sp_pos, sp_neg;      // sigmoid(x), softplus(x), softplus(-x)
};

__device__ __forceinline__ Terms terms_of(float x) {
    const float e = expf(-fabsf(x)), l = log1pf(e), d = 1.f / (1.f + e);
    Terms t;
    t.s = x >= 0.f ? d : e * d;
    t.sp_pos = fmaxf(x, 0.f) + l;
    t.sp_neg = fmaxf(-x, 0.f) + l;
    return t;
}

// sum over the workgroup's WAVES waves, in ascending order, valid in every thread; `slot` is LDS of WAVES floats
template <int WAVES>
__device__ __forceinline__ float block_sum(float v, float *slot) {
    v = wave_sum(v);
    __syncthreads();                      // the previous use of slot
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = slot[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) r += slot[i];
    return r;
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
constexpr int64_t kLim = (int64_t)1 << 31;

int map_check(const char *fn, const char *name, const void *ptr, int dtype, int64_t ms, int64_t rs, int64_t M, int64_t h, int64_t w) {
    if (M < 0 || h < 1 || w < 1 || M >= kLim || (h + 1) * (w + 1) >= kLim)
        return fail(VAH_E_SHAPE, "%s: bad dims (%s: %lld maps of %lld x %lld)", fn, name, (long long)M, (long long)h, (long long)w);
    if (dtype != 0 && dtype != 3) return fail(VAH_E_UNSUPPORTED, "%s: dtype codes of a map are 0 (fp32) and 3 (uint8) (%s)", fn, name);
    if (rs < w || ms < 0 || h * rs >= kLim) return fail(VAH_E_SHAPE, "%s: %s strides (row stride >= w, h * row stride < 2^31)", fn, name);
    if (!ptr) return fail(VAH_E_NULL, "%s: null pointer (%s)", fn, name);
    if (dtype == 0 && (uintptr_t)ptr % 4) return fail(VAH_E_ALIGN, "%s: %s misaligned (4-byte pointer)", fn, name);
    return 0;
}

struct Arr {
    const char *name;
    const void *ptr;
    int align;
    bool optional;
};

template <int NA>
int arr_check(const char *fn, const Arr (&arrs)[NA]) {
    for (const Arr &a : arrs)
        if (!a.ptr && !a.optional) return fail(VAH_E_NULL, "%s: null pointer (%s)", fn, a.name);
    for (const Arr &a : arrs)
        if ((uintptr_t)a.ptr % a.align) return fail(VAH_E_ALIGN, "%s: %s misaligned (%d-byte pointer)", fn, a.name, a.align);
    return 0;
}

}  // namespace
}  // namespace vah
