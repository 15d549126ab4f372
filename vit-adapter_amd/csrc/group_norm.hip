// GroupNorm on channels-last rows (include/vitadapter_hip_group_norm.h): the five GroupNorms of Mask2Former's pixel
// decoder (/root/reference/segmentation/mmseg_custom/models/plugins/msdeformattn_pixel_decoder.py:84-124), C = 256 in
// 32 groups, which torch runs as an fp32 NCHW operator under autocast.
//
// Element x[n][t][c] sits at n * img_stride + t * row_stride + c, so the same kernels serve an NHWC map and a level's
// rows of the encoder's (Lq, N, C) query buffer.  Every kernel moves pieces of 8 channels of one pixel (16 bytes of
// 16-bit data, two float4 of fp32); C / G <= 8 divides 8, so a piece holds whole groups and a thread, which keeps the
// same 8 channels for all its rows, loads its per-channel constants once.  A workgroup is 256 threads = C / 8 pieces x
// 256 / (C / 8) row lanes.
//   * statistics (forward and backward): grid (parts, N); a workgroup walks a contiguous chunk of an image's rows, four
//     rows in flight per thread, adds its row lanes in LDS in order and writes one partial row of 2C floats; the second
//     launch adds the partial rows in a fixed order (four chains per lane, 8 lanes), then the channels of a group in
//     order.  No atomics, no waiting between workgroups.
//   * apply / backward apply: grid (blocks, N), rows strided over the blocks, four rows in flight per thread.
// The element types are template parameters (float, __bf16, _Float16): they appear in loads, stores and converts only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vitadapter_hip_group_norm.h"
#include "common.h"
#include "elem16.h"

namespace vah {
namespace {

constexpr int kGnMaxParts = 512;        // partial rows per call (two workgroups per CU)
constexpr int kGnMinParts = 16;         // per image, however many images
constexpr int kGnPartRows = 64;         // at least this many rows per partial
constexpr int kGnApplyRows = 4;         // rows per thread and step
constexpr int kGnApplyBlocks = 2048;    // per call

struct GnParams {
    const float *mean, *rstd, *w, *b;
    int G, shift;                       // shift = log2(C / G)
};

// the constants of this thread's 8 channels in image n: pre-activation = fma(x, sc, sh), xhat = (x - mu) * rs
__device__ __forceinline__ void load_consts(const GnParams &p, int n, int c0, float (&sc)[8], float (&sh)[8], float (&mu)[8],
                                            float (&rs)[8], float (&w)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int g = n * p.G + ((c0 + j) >> p.shift);
        mu[j] = p.mean[g], rs[j] = p.rstd[g];
        w[j] = p.w ? p.w[c0 + j] : 1.f;
        sc[j] = rs[j] * w[j];
        sh[j] = (p.b ? p.b[c0 + j] : 0.f) - mu[j] * sc[j];
    }
}

// MODE 0: part = [sum x | sum x^2];  MODE 1: part = [sum g' | sum g' xhat] per channel, over rows [r0, r1) of image n
template <typename TX, typename TD, int MODE>
__global__ __launch_bounds__(256) void gn_stats_kernel(const TX *__restrict__ x, int64_t xrs, int64_t xis,
                                                       const TD *__restrict__ dy, int64_t drs, int64_t dis, int64_t T, int C,
                                                       GnParams p, int relu, float *__restrict__ part) {
    __shared__ float s_red[256][17];
    const int C8 = C >> 3, cp = threadIdx.x % C8, rl = threadIdx.x / C8, RL = 256 / C8;
    const int c0 = cp * 8, n = blockIdx.y;
    float sc[8], sh[8], mu[8], rs[8], w[8];
    if (MODE == 1) load_consts(p, n, c0, sc, sh, mu, rs, w);
    float a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = b[j] = 0.f;
    const int64_t per = (T + gridDim.x - 1) / gridDim.x, r0 = per * blockIdx.x, r1 = r0 + per < T ? r0 + per : T;
    const TX *xp = x + n * xis + c0;
    const TD *dp = dy + n * dis + c0;
    auto add = [&](const float (&xv)[8], const float (&gv)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (MODE == 0) {
                a[j] += xv[j];
                b[j] += xv[j] * xv[j];
            } else {
                const float g = (!relu || fmaf(xv[j], sc[j], sh[j]) > 0.f) ? gv[j] : 0.f;
                a[j] += g;
                b[j] += g * ((xv[j] - mu[j]) * rs[j]);
            }
        }
    };
    int64_t r = r0 + rl;
    for (; r + 3 * RL < r1; r += 4 * RL) {              // four rows in flight
        float xv[4][8], gv[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            load8_f32(xp + (r + u * RL) * xrs, xv[u]);
            if (MODE == 1) load8_f32(dp + (r + u * RL) * drs, gv[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) add(xv[u], MODE == 1 ? gv[u] : xv[u]);
    }
    for (; r < r1; r += RL) {
        float xv[8], gv[8];
        load8_f32(xp + r * xrs, xv);
        if (MODE == 1) load8_f32(dp + r * drs, gv);
        add(xv, MODE == 1 ? gv : xv);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s_red[threadIdx.x][j] = a[j], s_red[threadIdx.x][8 + j] = b[j];
    __syncthreads();
    // thread t < 2C adds channel (t % C) of half (t / C) over the row lanes, in order
    float *out = part + ((int64_t)n * gridDim.x + blockIdx.x) * 2 * C;
    for (int t = threadIdx.x; t < 2 * C; t += 256) {
        const int half = t / C, c = t - half * C;
        float s = 0.f;
        for (int l = 0; l < RL; ++l) s += s_red[l * C8 + (c >> 3)][half * 8 + (c & 7)];
        out[t] = s;
    }
}

// columns c and C + c of image n's partial rows, for the 32 channels of this workgroup: lane pl adds rows pl, pl + 8, ...
// in four chains, then s_c[half][col] = the 8 lanes in order
__device__ __forceinline__ void gn_sum_parts(const float *__restrict__ base, int parts, int C, float (&s_p)[2][8][33],
                                             float (&s_c)[2][32], float &total) {
    const int col = threadIdx.x & 31, pl = threadIdx.x >> 5, c = blockIdx.x * 32 + col;
    float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
    int i = pl;
    for (; i + 24 < parts; i += 32) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s[u] += base[(int64_t)(i + 8 * u) * 2 * C + c];
            q[u] += base[(int64_t)(i + 8 * u) * 2 * C + C + c];
        }
    }
    for (; i < parts; i += 8) {
        s[0] += base[(int64_t)i * 2 * C + c];
        q[0] += base[(int64_t)i * 2 * C + C + c];
    }
    s_p[0][pl][col] = (s[0] + s[1]) + (s[2] + s[3]);
    s_p[1][pl][col] = (q[0] + q[1]) + (q[2] + q[3]);
    __syncthreads();
    if (pl < 2) {
        float t = 0.f;
#pragma unroll
        for (int l = 0; l < 8; ++l) t += s_p[pl][l][col];
        s_c[pl][col] = t;
        total = t;
    }
    __syncthreads();
}

// grid (C / 32, N): mean, rstd of the 32 / cpg groups of this workgroup's channels
__global__ __launch_bounds__(256) void gn_finalize_kernel(const float *__restrict__ part, int parts, int64_t T, int C, int cpg,
                                                          float eps, float *__restrict__ mean, float *__restrict__ rstd) {
    __shared__ float s_p[2][8][33], s_c[2][32];
    const int n = blockIdx.y, gpb = 32 / cpg, G = C / cpg;
    float unused;
    gn_sum_parts(part + (int64_t)n * parts * 2 * C, parts, C, s_p, s_c, unused);
    if ((int)threadIdx.x < gpb) {
        float a = 0.f, b = 0.f;
        for (int k = 0; k < cpg; ++k) a += s_c[0][threadIdx.x * cpg + k], b += s_c[1][threadIdx.x * cpg + k];
        const float cnt = (float)(T * cpg), mu = a / cnt;
        // IEEE maximum: an inf or NaN in the group gives a NaN variance and then a NaN group, as torch's
        const float var = __builtin_elementwise_maximum(b / cnt - mu * mu, 0.f);
        const int g = n * G + blockIdx.x * gpb + threadIdx.x;
        mean[g] = mu;
        rstd[g] = rsqrtf(var + eps);
    }
}

// grid (C / 32): the images in order; gsums = [sum g' w | sum g' w xhat] per (n, g), dbeta / dgamma per channel
__global__ __launch_bounds__(256) void gn_bwd_finalize_kernel(const float *__restrict__ part, int parts, int N, int C, int cpg,
                                                              const float *__restrict__ w, float *__restrict__ gsums,
                                                              float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ float s_p[2][8][33], s_c[2][32];
    const int col = threadIdx.x & 31, pl = threadIdx.x >> 5, gpb = 32 / cpg, G = C / cpg;
    float acc = 0.f;
    for (int n = 0; n < N; ++n) {
        float t = 0.f;
        gn_sum_parts(part + (int64_t)n * parts * 2 * C, parts, C, s_p, s_c, t);
        acc += t;
        if ((int)threadIdx.x < 2 * gpb) {
            const int half = threadIdx.x / gpb, gl = threadIdx.x - half * gpb;
            float a = 0.f;
            for (int k = 0; k < cpg; ++k) {
                const int cl = gl * cpg + k;
                a += s_c[half][cl] * (w ? w[blockIdx.x * 32 + cl] : 1.f);
            }
            gsums[(int64_t)half * N * G + (int64_t)n * G + blockIdx.x * gpb + gl] = a;
        }
    }
    if (pl == 0 && dbeta) dbeta[blockIdx.x * 32 + col] = acc;
    if (pl == 1 && dgamma) dgamma[blockIdx.x * 32 + col] = acc;
}

template <typename TX, typename TY>
__global__ __launch_bounds__(256) void gn_apply_kernel(const TX *__restrict__ x, int64_t xrs, int64_t xis, int64_t T, int C,
                                                       GnParams p, int relu, const TY *__restrict__ add, TY *__restrict__ y,
                                                       int64_t yrs, int64_t yis) {
    const int C8 = C >> 3, cp = threadIdx.x % C8, rl = threadIdx.x / C8, RL = 256 / C8;
    const int c0 = cp * 8, n = blockIdx.y;
    float sc[8], sh[8], mu[8], rs[8], w[8];
    load_consts(p, n, c0, sc, sh, mu, rs, w);
    const TX *xp = x + n * xis + c0;
    TY *yp = y + n * yis + c0;
    const TY *ap = add ? add + (int64_t)n * T * C + c0 : nullptr;
    const int64_t step = (int64_t)gridDim.x * RL;
    auto finish = [&](int64_t t, float (&v)[8], const float (&av)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float u = fmaf(v[j], sc[j], sh[j]);
            // IEEE maximum, not fmaxf (which returns the other operand for a NaN): relu(NaN) = NaN
            v[j] = relu ? __builtin_elementwise_maximum(u, 0.f) : u;
            if (ap) v[j] += av[j];
        }
        store8_f32(yp + t * yrs, v);
    };
    int64_t t = (int64_t)blockIdx.x * RL + rl;
    for (; t + (kGnApplyRows - 1) * step < T; t += kGnApplyRows * step) {
        float v[kGnApplyRows][8], av[kGnApplyRows][8];
#pragma unroll
        for (int u = 0; u < kGnApplyRows; ++u) {
            load8_f32(xp + (t + u * step) * xrs, v[u]);
            if (ap) load8_f32(ap + (t + u * step) * C, av[u]);
        }
#pragma unroll
        for (int u = 0; u < kGnApplyRows; ++u) finish(t + u * step, v[u], ap ? av[u] : v[u]);
    }
    for (; t < T; t += step) {
        float v[8], av[8];
        load8_f32(xp + t * xrs, v);
        if (ap) load8_f32(ap + t * C, av);
        finish(t, v, ap ? av : v);
    }
}

// dx = rstd (g' w - m1 - xhat m2)
template <typename TX, typename TD, typename TG>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const TX *__restrict__ x, int64_t xrs, int64_t xis,
                                                           const TD *__restrict__ dy, int64_t drs, int64_t dis, int64_t T, int C,
                                                           int N, GnParams p, int relu, const float *__restrict__ gsums,
                                                           TG *__restrict__ dx, int64_t grs, int64_t gis) {
    const int C8 = C >> 3, cp = threadIdx.x % C8, rl = threadIdx.x / C8, RL = 256 / C8;
    const int c0 = cp * 8, n = blockIdx.y;
    float sc[8], sh[8], mu[8], rs[8], w[8], m1[8], m2[8];
    load_consts(p, n, c0, sc, sh, mu, rs, w);
    const float inv = 1.f / (float)(T << p.shift);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int g = n * p.G + ((c0 + j) >> p.shift);
        m1[j] = gsums[g] * inv, m2[j] = gsums[(int64_t)N * p.G + g] * inv;
    }
    const TX *xp = x + n * xis + c0;
    const TD *dp = dy + n * dis + c0;
    TG *gp = dx + n * gis + c0;
    const int64_t step = (int64_t)gridDim.x * RL;
    auto finish = [&](int64_t t, float (&v)[8], const float (&gv)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float g = (!relu || fmaf(v[j], sc[j], sh[j]) > 0.f) ? gv[j] : 0.f;
            v[j] = rs[j] * (g * w[j] - m1[j] - (v[j] - mu[j]) * rs[j] * m2[j]);
        }
        store8_f32(gp + t * grs, v);
    };
    int64_t t = (int64_t)blockIdx.x * RL + rl;
    for (; t + (kGnApplyRows - 1) * step < T; t += kGnApplyRows * step) {
        float v[kGnApplyRows][8], gv[kGnApplyRows][8];
#pragma unroll
        for (int u = 0; u < kGnApplyRows; ++u) {
            load8_f32(xp + (t + u * step) * xrs, v[u]);
            load8_f32(dp + (t + u * step) * drs, gv[u]);
        }
#pragma unroll
        for (int u = 0; u < kGnApplyRows; ++u) finish(t + u * step, v[u], gv[u]);
    }
    for (; t < T; t += step) {
        float v[8], gv[8];
        load8_f32(xp + t * xrs, v);
        load8_f32(dp + t * drs, gv);
        finish(t, v, gv);
    }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
bool gn_supported(int64_t C, int64_t G) {
    if (C < 64 || C > 512 || (C & (C - 1)) || G < 1 || C % G) return false;
    const int64_t cpg = C / G;
    return cpg == 1 || cpg == 2 || cpg == 4 || cpg == 8;
}

int gn_shift(int64_t C, int64_t G) {
    int s = 0;
    while (((int64_t)G << s) < C) ++s;
    return s;
}

// partial rows per image
int gn_parts(int64_t N, int64_t T) {
    int64_t cap = kGnMaxParts / (N < 1 ? 1 : N);
    cap = cap < kGnMinParts ? kGnMinParts : cap;
    const int64_t p = (T + kGnPartRows - 1) / kGnPartRows;
    return (int)(p < 1 ? 1 : (p > cap ? cap : p));
}

unsigned gn_apply_blocks(int64_t N, int64_t T, int64_t C) {
    const int64_t RL = 256 / (C / 8);
    int64_t cap = kGnApplyBlocks / (N < 1 ? 1 : N);
    cap = cap < 1 ? 1 : cap;
    const int64_t want = (T + RL * kGnApplyRows - 1) / (RL * kGnApplyRows);
    return (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
}

int gn_check_dims(const char *fn, int64_t N, int64_t T, int64_t C, int64_t G) {
    if (N < 0 || T < 0 || C < 1 || G < 1 || N > 65535 || T > (int64_t)1 << 31)
        return fail(VAH_E_SHAPE, "%s: bad dims (N %lld, T %lld, C %lld, G %lld)", fn, (long long)N, (long long)T, (long long)C,
                    (long long)G);
    if (!gn_supported(C, G))
        return fail(VAH_E_UNSUPPORTED, "%s: C must be a power of two in [64, 512] and C / G one of 1, 2, 4, 8 (C %lld, G %lld)", fn,
                    (long long)C, (long long)G);
    return 0;
}

int gn_check_dtypes(const char *fn, int a, int b, int c) {
    bool bf = false, fp = false;
    for (int d : {a, b, c}) {
        if (d < 0 || d > 2) return fail(VAH_E_UNSUPPORTED, "%s: dtype codes are 0 (fp32), 1 (bf16), 2 (fp16)", fn);
        bf |= d == 1, fp |= d == 2;
    }
    if (bf && fp) return fail(VAH_E_UNSUPPORTED, "%s: fp16 mixed with bf16", fn);
    return 0;
}

int gn_check_tensor(const char *fn, const char *name, const void *ptr, int64_t rs, int64_t is, int64_t C) {
    if (!ptr) return fail(VAH_E_NULL, "%s: null pointer (%s)", fn, name);
    if ((uintptr_t)ptr % 16 || rs % 8 || is % 8) return fail(VAH_E_ALIGN, "%s: %s misaligned (16-byte pointer, strides in multiples of 8)", fn, name);
    if (rs < C || is < 0) return fail(VAH_E_SHAPE, "%s: %s strides (row stride >= C)", fn, name);
    return 0;
}

int gn_check_ws(const char *fn, const float *ws, int64_t ws_floats, int64_t N, int64_t T, int64_t C) {
    if (!ws) return fail(VAH_E_NULL, "%s: null pointer (ws)", fn);
    if (ws_floats < (int64_t)N * gn_parts(N, T) * 2 * C) return fail(VAH_E_SHAPE, "%s: workspace too small", fn);
    return 0;
}

const char *gn_name(bool f16, const char *a, const char *b) { return f16 ? b : a; }

}  // namespace
}  // namespace vah

extern "C" {

int vah_group_norm_supported(int64_t C, int64_t G) { return vah::gn_supported(C, G) ? 1 : 0; }

int64_t vah_group_norm_ws_floats(int64_t N, int64_t T, int64_t C, int64_t G) {
    if (N < 1 || T < 1 || !vah::gn_supported(C, G)) return 0;
    return N * vah::gn_parts(N, T) * 2 * C;
}

int vah_group_norm_stats(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride, int64_t N, int64_t T, int64_t C,
                         int64_t G, float eps, float *mean, float *rstd, float *ws, int64_t ws_floats, void *stream) {
    using namespace vah;
    const char *fn = "vah_group_norm_stats";
    clear_error();
    if (int rc = gn_check_dims(fn, N, T, C, G)) return rc;
    if (int rc = gn_check_dtypes(fn, x_dtype, 0, 0)) return rc;
    if (N * T == 0) return VAH_OK;
    if (int rc = gn_check_tensor(fn, "x", x, x_row_stride, x_img_stride, C)) return rc;
    if (!mean || !rstd) return fail(VAH_E_NULL, "%s: null pointer (mean / rstd)", fn);
    if (int rc = gn_check_ws(fn, ws, ws_floats, N, T, C)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int parts = gn_parts(N, T), cpg = (int)(C / G);
    LaunchScope scope(gn_name(x_dtype == 2, "gn_stats", "gn_stats_f16"), N * T * C * esize(x_dtype), st, N * T * C * 4);
    int rc = with_type(x_dtype, [&](auto tx) {
        typedef typename decltype(tx)::type TX;
        hipLaunchKernelGGL((gn_stats_kernel<TX, TX, 0>), dim3(parts, (unsigned)N), dim3(256), 0, st, (const TX *)x, x_row_stride,
                           x_img_stride, (const TX *)nullptr, (int64_t)0, (int64_t)0, T, (int)C, GnParams{}, 0, ws);
        return check_launch(fn);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3((unsigned)(C / 32), (unsigned)N), dim3(256), 0, st, (const float *)ws, parts, T, (int)C,
                       cpg, eps, mean, rstd);
    return check_launch(fn);
}

int vah_group_norm_apply(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride, int64_t N, int64_t T, int64_t C,
                         int64_t G, const float *mean, const float *rstd, const float *w, const float *b, int relu, const void *add,
                         void *y, int y_dtype, int64_t y_row_stride, int64_t y_img_stride, void *stream) {
    using namespace vah;
    const char *fn = "vah_group_norm_apply";
    clear_error();
    if (int rc = gn_check_dims(fn, N, T, C, G)) return rc;
    if (int rc = gn_check_dtypes(fn, x_dtype, y_dtype, 0)) return rc;
    if (N * T == 0) return VAH_OK;
    if (int rc = gn_check_tensor(fn, "x", x, x_row_stride, x_img_stride, C)) return rc;
    if (int rc = gn_check_tensor(fn, "y", y, y_row_stride, y_img_stride, C)) return rc;
    if (!mean || !rstd) return fail(VAH_E_NULL, "%s: null pointer (mean / rstd)", fn);
    if (add && (uintptr_t)add % 16) return fail(VAH_E_ALIGN, "%s: add misaligned (16-byte pointer)", fn);
    hipStream_t st = (hipStream_t)stream;
    const GnParams p{mean, rstd, w, b, (int)G, gn_shift(C, G)};
    LaunchScope scope(gn_name(x_dtype == 2 || y_dtype == 2, "gn_apply", "gn_apply_f16"),
                      N * T * C * (esize(x_dtype) + esize(y_dtype) * (add ? 2 : 1)), st, N * T * C * (add ? 12 : 8));
    return with_type(x_dtype, [&](auto tx) {
        return with_type(y_dtype, [&](auto ty) {
            typedef typename decltype(tx)::type TX;
            typedef typename decltype(ty)::type TY;
            if constexpr (!mixed16<TX, TY>())
                hipLaunchKernelGGL((gn_apply_kernel<TX, TY>), dim3(gn_apply_blocks(N, T, C), (unsigned)N), dim3(256), 0, st, (const TX *)x,
                                   x_row_stride, x_img_stride, T, (int)C, p, relu, (const TY *)add, (TY *)y, y_row_stride, y_img_stride);
            return check_launch(fn);
        });
    });
}

int vah_group_norm_bwd_stats(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride, const void *dy, int dy_dtype,
                             int64_t dy_row_stride, int64_t dy_img_stride, int64_t N, int64_t T, int64_t C, int64_t G,
                             const float *mean, const float *rstd, const float *w, const float *b, int relu, float *gsums,
                             float *dgamma, float *dbeta, float *ws, int64_t ws_floats, void *stream) {
    using namespace vah;
    const char *fn = "vah_group_norm_bwd_stats";
    clear_error();
    if (int rc = gn_check_dims(fn, N, T, C, G)) return rc;
    if (int rc = gn_check_dtypes(fn, x_dtype, dy_dtype, 0)) return rc;
    if (N * T == 0) return VAH_OK;
    if (int rc = gn_check_tensor(fn, "x", x, x_row_stride, x_img_stride, C)) return rc;
    if (int rc = gn_check_tensor(fn, "dy", dy, dy_row_stride, dy_img_stride, C)) return rc;
    if (!mean || !rstd || !gsums) return fail(VAH_E_NULL, "%s: null pointer (mean / rstd / gsums)", fn);
    if (int rc = gn_check_ws(fn, ws, ws_floats, N, T, C)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int parts = gn_parts(N, T), cpg = (int)(C / G);
    const GnParams p{mean, rstd, w, b, (int)G, gn_shift(C, G)};
    LaunchScope scope(gn_name(x_dtype == 2 || dy_dtype == 2, "gn_bwd_stats", "gn_bwd_stats_f16"),
                      N * T * C * (esize(x_dtype) + esize(dy_dtype)), st, N * T * C * 8);
    int rc = with_type(x_dtype, [&](auto tx) {
        return with_type(dy_dtype, [&](auto td) {
            typedef typename decltype(tx)::type TX;
            typedef typename decltype(td)::type TD;
            if constexpr (!mixed16<TX, TD>())
                hipLaunchKernelGGL((gn_stats_kernel<TX, TD, 1>), dim3(parts, (unsigned)N), dim3(256), 0, st, (const TX *)x, x_row_stride,
                                   x_img_stride, (const TD *)dy, dy_row_stride, dy_img_stride, T, (int)C, p, relu, ws);
            return check_launch(fn);
        });
    });
    if (rc) return rc;
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3((unsigned)(C / 32)), dim3(256), 0, st, (const float *)ws, parts, (int)N, (int)C, cpg, w,
                       gsums, dgamma, dbeta);
    return check_launch(fn);
}

int vah_group_norm_bwd_apply(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride, const void *dy, int dy_dtype,
                             int64_t dy_row_stride, int64_t dy_img_stride, int64_t N, int64_t T, int64_t C, int64_t G,
                             const float *mean, const float *rstd, const float *w, const float *b, int relu, const float *gsums,
                             void *dx, int dx_dtype, int64_t dx_row_stride, int64_t dx_img_stride, void *stream) {
    using namespace vah;
    const char *fn = "vah_group_norm_bwd_apply";
    clear_error();
    if (int rc = gn_check_dims(fn, N, T, C, G)) return rc;
    if (int rc = gn_check_dtypes(fn, x_dtype, dy_dtype, dx_dtype)) return rc;
    if (N * T == 0) return VAH_OK;
    if (int rc = gn_check_tensor(fn, "x", x, x_row_stride, x_img_stride, C)) return rc;
    if (int rc = gn_check_tensor(fn, "dy", dy, dy_row_stride, dy_img_stride, C)) return rc;
    if (int rc = gn_check_tensor(fn, "dx", dx, dx_row_stride, dx_img_stride, C)) return rc;
    if (!mean || !rstd || !gsums) return fail(VAH_E_NULL, "%s: null pointer (mean / rstd / gsums)", fn);
    hipStream_t st = (hipStream_t)stream;
    const GnParams p{mean, rstd, w, b, (int)G, gn_shift(C, G)};
    LaunchScope scope(gn_name(x_dtype == 2 || dy_dtype == 2 || dx_dtype == 2, "gn_bwd_apply", "gn_bwd_apply_f16"),
                      N * T * C * (esize(x_dtype) + esize(dy_dtype) + esize(dx_dtype)), st, N * T * C * 12);
    return with_type(x_dtype, [&](auto tx) {
        return with_type(dy_dtype, [&](auto td) {
            return with_type(dx_dtype, [&](auto tg) {
                typedef typename decltype(tx)::type TX;
                typedef typename decltype(td)::type TD;
                typedef typename decltype(tg)::type TG;
                if constexpr (!mixed16<TX, TD>() && !mixed16<TX, TG>() && !mixed16<TD, TG>())
                    hipLaunchKernelGGL((gn_bwd_apply_kernel<TX, TD, TG>), dim3(gn_apply_blocks(N, T, C), (unsigned)N), dim3(256), 0, st,
                                       (const TX *)x, x_row_stride, x_img_stride, (const TD *)dy, dy_row_stride, dy_img_stride, T, (int)C,
                                       (int)N, p, relu, gsums, (TG *)dx, dx_row_stride, dx_img_stride);
                return check_launch(fn);
            });
        });
    });
}

}  // extern "C"
