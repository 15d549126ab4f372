// Point sampling and the matching cost of Mask2Former's training head (include/vitadapter_hip_points.h): mmcv's point_sample
// and the costs of MaskHungarianAssigner (the reference's segmentation/mmseg_custom/models/decode_heads/mask2former_head.py:199-267).
//
// These are gather and latency kernels: a point costs four taps of a map that sits in L2, nothing here is near a bandwidth or
// a matrix limit.  What the kernels are built around:
//   * a tap outside the map is handled by clamping its ADDRESS and discarding its VALUE, so that the four loads of a
//     point are unconditional and issue back to back; several points per thread are loaded before the first is used;
//   * the tap indices and fractions come from one function, taps_of() of point_sample.h (shared with point_mask_loss.hip),
//     whose arithmetic is pinned (an explicit fma);
//   * every sum over points is: a serial run per lane in ascending p, wave_sum()'s butterfly, the waves in ascending order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/vitadapter_hip_points.h"
#include "point_sample.h"

namespace vah {
namespace {

// ---------------------------------------------------------------------------------------
// vah_pts_sample: block b -> row b / chunks, points [(b % chunks) * 1024, +1024): 4 per thread, 256 apart
// ---------------------------------------------------------------------------------------
constexpr int kSampleU = 4;

template <typename T>
__global__ __launch_bounds__(256) void pts_sample_kernel(const T *__restrict__ maps, int64_t ms, int rs, int M, int h, int w,
                                                         const float2 *__restrict__ points, int S, int P,
                                                         const int *__restrict__ map_idx, const int *__restrict__ set_idx,
                                                         unsigned chunks, float *__restrict__ out) {
    const unsigned r = blockIdx.x / chunks, chunk = blockIdx.x - r * chunks;
    const int m = map_idx ? map_idx[r] : (int)r, s = set_idx ? set_idx[r] : (int)r;
    const int p0 = (int)chunk * 256 * kSampleU + (int)threadIdx.x;
    float *o = out + (int64_t)r * P;
    if (m < 0 || m >= M || s < 0 || s >= S) {       // block-uniform
#pragma unroll
        for (int u = 0; u < kSampleU; ++u)
            if (p0 + u * 256 < P) o[p0 + u * 256] = quiet_nan();
        return;
    }
    const T *map = maps + (int64_t)m * ms;
    const float2 *pts = points + (int64_t)s * P;
    Taps t[kSampleU];
    Quad q[kSampleU];
#pragma unroll
    for (int u = 0; u < kSampleU; ++u) t[u] = taps_of(pts[min(p0 + u * 256, P - 1)], h, w);
#pragma unroll
    for (int u = 0; u < kSampleU; ++u) q[u] = load_quad(map, rs, h, w, t[u]);
#pragma unroll
    for (int u = 0; u < kSampleU; ++u)
        if (p0 + u * 256 < P) o[p0 + u * 256] = combine(q[u], t[u], h, w);
}

// ---------------------------------------------------------------------------------------
// vah_pts_match_cost: block -> (n * Q + q, tile of kCostG columns)
// ---------------------------------------------------------------------------------------
constexpr int kCostG = 8;

__global__ __launch_bounds__(256) void pts_match_cost_kernel(const float *__restrict__ xs, const float *__restrict__ ts,
                                                             const int *__restrict__ gt_offsets, const float *__restrict__ cls,
                                                             const int64_t *__restrict__ labels, int Q, int C1, int G_total,
                                                             int Gmax, int P, unsigned tiles, float w_cls, float w_mask,
                                                             float w_dice, float eps, float *__restrict__ cost) {
    __shared__ float slot[4];
    const unsigned nq = blockIdx.x / tiles, tile = blockIdx.x - nq * tiles;
    const int n = (int)(nq / (unsigned)Q), g0 = (int)tile * kCostG;
    const int lo = gt_offsets[n], hi = gt_offsets[n + 1];
    int G = hi - lo;
    if (lo < 0 || hi > G_total || G < 0 || G > Gmax) G = 0;          // block-uniform: bad offsets -> all +inf
    float *row = cost + (int64_t)nq * Gmax;
    const int cols = min(kCostG, G - g0);                          // live columns of this tile (may be <= 0)
    if (cols > 0) {
        const float *x = xs + (int64_t)nq * P;
        const float *t0 = ts + (int64_t)(lo + g0) * P;
        float a[kCostG], mk[kCostG], c[kCostG], b = 0.f;
#pragma unroll
        for (int j = 0; j < kCostG; ++j) a[j] = mk[j] = c[j] = 0.f;
        for (int p = (int)threadIdx.x; p < P; p += 256) {
            float tv[kCostG];
#pragma unroll
            for (int j = 0; j < kCostG; ++j) tv[j] = t0[(int64_t)min(j, cols - 1) * P + p];     // unconditional, clamped row
            const Terms e = terms_of(x[p]);
            b += e.s;
#pragma unroll
            for (int j = 0; j < kCostG; ++j) {
                a[j] += e.s * tv[j];
                mk[j] += e.sp_neg * tv[j] + e.sp_pos * (1.f - tv[j]);
                c[j] += tv[j];
            }
        }
        b = block_sum<4>(b, slot);
        float res = 0.f;
#pragma unroll
        for (int j = 0; j < kCostG; ++j) {
            const float aj = block_sum<4>(a[j], slot), mj = block_sum<4>(mk[j], slot), cj = block_sum<4>(c[j], slot);
            if ((int)threadIdx.x == j) res = w_mask * (mj / (float)P) + w_dice * (1.f - (2.f * aj + eps) / (b + cj + eps));
        }
        if ((int)threadIdx.x < cols) {
            const int64_t label = labels[lo + g0 + (int)threadIdx.x];
            float prob = quiet_nan();
            if (label >= 0 && label < C1) {
                const float *z = cls + (int64_t)nq * C1;
                float mx = z[0];
                for (int i = 1; i < C1; ++i) mx = fmaxf(mx, z[i]);
                float sum = 0.f;
                for (int i = 0; i < C1; ++i) sum += expf(z[i] - mx);
                prob = expf(z[label] - mx) / sum;
            }
            row[g0 + (int)threadIdx.x] = w_cls * (-prob) + res;
        }
    }
    const int first = g0 + max(cols, 0);
    if ((int)threadIdx.x < kCostG && first + (int)threadIdx.x < min(g0 + kCostG, Gmax)) row[first + (int)threadIdx.x] = INFINITY;
}

}  // namespace
}  // namespace vah

extern "C" {

int vah_pts_sample(const void *maps, int map_dtype, int64_t map_stride, int64_t row_stride, int64_t M, int64_t h, int64_t w,
                   const void *points, int64_t S, int64_t P, const void *map_idx, const void *set_idx, int64_t R, void *out,
                   void *stream) {
    using namespace vah;
    const char *fn = "vah_pts_sample";
    clear_error();
    if (R < 0 || S < 0 || P > kLim - 256 * kSampleU || R >= kLim || S >= kLim)       // p0 + 3 * 256 is int arithmetic
        return fail(VAH_E_SHAPE, "%s: bad dims (R %lld, S %lld, P %lld)", fn, (long long)R, (long long)S, (long long)P);
    if (P <= 0) return fail(VAH_E_SHAPE, "%s: P must be positive (P %lld)", fn, (long long)P);
    if (map_dtype != 0 && map_dtype != 3) return fail(VAH_E_UNSUPPORTED, "%s: dtype codes of a map are 0 (fp32) and 3 (uint8) (maps)", fn);
    if (R == 0) return VAH_OK;
    if (int rc = map_check(fn, "maps", maps, map_dtype, map_stride, row_stride, M, h, w)) return rc;
    if ((!map_idx && R > M) || (!set_idx && R > S))
        return fail(VAH_E_SHAPE, "%s: index out of range (identity rows: R %lld, M %lld, S %lld)", fn, (long long)R, (long long)M, (long long)S);
    const Arr arrs[] = {{"points", points, 8, false}, {"map_idx", map_idx, 4, true}, {"set_idx", set_idx, 4, true}, {"out", out, 4, false}};
    if (int rc = arr_check(fn, arrs)) return rc;
    const int64_t chunks = (P + 256 * kSampleU - 1) / (256 * kSampleU);
    if (R * chunks >= kLim) return fail(VAH_E_SHAPE, "%s: bad dims (R * ceil(P / 1024) must stay below 2^31)", fn);
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope("pts_sample", R * P * (8 + 4 + 4 * (map_dtype ? 1 : 4)), st);
    const dim3 grid((unsigned)(R * chunks)), block(256);
    if (map_dtype == 0)
        hipLaunchKernelGGL(pts_sample_kernel<float>, grid, block, 0, st, (const float *)maps, map_stride, (int)row_stride, (int)M, (int)h,
                           (int)w, (const float2 *)points, (int)S, (int)P, (const int *)map_idx, (const int *)set_idx, (unsigned)chunks,
                           (float *)out);
    else
        hipLaunchKernelGGL(pts_sample_kernel<uint8_t>, grid, block, 0, st, (const uint8_t *)maps, map_stride, (int)row_stride, (int)M,
                           (int)h, (int)w, (const float2 *)points, (int)S, (int)P, (const int *)map_idx, (const int *)set_idx,
                           (unsigned)chunks, (float *)out);
    return check_launch(fn);
}

int vah_pts_match_cost(const void *xs, const void *ts, const void *gt_offsets, const void *cls, const void *labels, int64_t N,
                       int64_t Q, int64_t C1, int64_t G_total, int64_t Gmax, int64_t P, float w_cls, float w_mask, float w_dice,
                       float dice_eps, void *cost, void *stream) {
    using namespace vah;
    const char *fn = "vah_pts_match_cost";
    clear_error();
    if (N < 0 || Q < 0 || C1 < 0 || G_total < 0 || Gmax < 0 || N >= kLim || Q >= kLim || C1 >= kLim || G_total >= kLim || Gmax >= kLim ||
        P >= kLim || Gmax > G_total)
        return fail(VAH_E_SHAPE, "%s: bad dims (N %lld, Q %lld, C1 %lld, G_total %lld, Gmax %lld, P %lld)", fn, (long long)N, (long long)Q,
                    (long long)C1, (long long)G_total, (long long)Gmax, (long long)P);
    if (P <= 0) return fail(VAH_E_SHAPE, "%s: P must be positive (P %lld)", fn, (long long)P);
    if (N * Q * Gmax == 0) return VAH_OK;
    if (C1 < 1) return fail(VAH_E_SHAPE, "%s: bad dims (no classes)", fn);
    const Arr arrs[] = {{"xs", xs, 4, false}, {"ts", ts, 4, false}, {"gt_offsets", gt_offsets, 4, false}, {"cls", cls, 4, false},
                        {"labels", labels, 8, false}, {"cost", cost, 4, false}};
    if (int rc = arr_check(fn, arrs)) return rc;
    const int64_t tiles = (Gmax + kCostG - 1) / kCostG;
    if (N * Q * tiles >= kLim) return fail(VAH_E_SHAPE, "%s: bad dims (N * Q * ceil(Gmax / 8) must stay below 2^31)", fn);
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope("pts_match_cost", 4 * (N * Q * P + G_total * P + N * Q * (C1 + Gmax)), st);
    hipLaunchKernelGGL(pts_match_cost_kernel, dim3((unsigned)(N * Q * tiles)), dim3(256), 0, st, (const float *)xs, (const float *)ts,
                       (const int *)gt_offsets, (const float *)cls, (const int64_t *)labels, (int)Q, (int)C1, (int)G_total, (int)Gmax,
                       (int)P, (unsigned)tiles, w_cls, w_mask, w_dice, dice_eps, (float *)cost);
    return check_launch(fn);
}

}  // extern "C"
