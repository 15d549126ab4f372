// Fused memory-bound operators of the ViT-Adapter blocks for gfx950 (all HBM-bound: one pass over
// the activations each, 16-byte accesses, fp32 math).
//
//   layernorm_f32_bf16     y = LN(x) over the last dim, fp32 in -> bf16 out (the next op is always a
//                          bf16 GEMM under autocast: the separate fp32->bf16 cast pass disappears);
//                          backward produces dx (fp32), dweight, dbias in one pass
//   scale_residual         y = x + s[b] * gamma[c] * z     x,y fp32 residual stream, z bf16 branch
//                          output, gamma = layer-scale (optional), s[b] = DropPath mask / keep
//                          (optional): replaces mul, div, mul, add kernels of
//                          x + drop_path(gamma * f(x))  (ref: detection/mmdet_custom/models/backbones/
//                          base/vit.py:301-306); backward gives dz (bf16) and dgamma
//   dwconv3x3_tokens       the ConvFFN depthwise 3x3 (+bias) applied directly on the (B, 21n, C)
//                          token tensor whose three level maps are concatenated along the token axis
//                          (ref: segmentation/mmseg_custom/models/backbones/adapter_modules.py:72-87):
//                          no slice / transpose / contiguous / cat copies, no MIOpen naive bf16
//                          depthwise kernels (3.3 ms per step measured)
//
// The kernels that touch a 16-bit operand are templates on its element type T: __bf16 (bf16 autocast) or
// _Float16 (fp16 autocast, the *_f16 entry points).  All arithmetic, statistics, partial rows and parameter
// gradients are fp32 for both; T appears in loads, stores and converts only.  float -> _Float16 is the plain
// cast (v_cvt_f16_f32 / v_cvt_pk_f16_f32: round to nearest even, overflow to +-inf, subnormals kept - what
// torch's .to(float16) does): loss-scaled gradients live in fp16's subnormal range and an overflow has to
// reach GradScaler as inf, so no cvt_pkrtz, no saturation, no flushed denormals.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "elem16.h"

namespace vah {
namespace {

// fp32 -> T where a kernel both stores the rounded value and sums it (the bias partials), or has to agree bit for bit
// with another kernel's store: every dz / dh store of the residual, residual + LayerNorm and GELU backward kernels.  For _Float16 the fp32 value is made opaque first: with -ffp-contract=fast the compiler
// otherwise folds the multiply that produced it into v_fma_mixlo_f16 (one rounding, from the exact product) for one use
// and keeps v_mul_f32 + v_cvt_pk_f16_f32 (fp32 product, then fp16: two roundings) for another, and the two differ by an
// fp16 ulp about once in 10^4 elements - the sum then is not the sum of what was stored.  What is kept is the second
// form: the fp32 value rounded once to fp16, which is also what torch's kernels do.  (bf16 has no such instruction.)
template <typename T>
__device__ __forceinline__ T round16(float v) {
    if constexpr (std::is_same<T, _Float16>::value) asm("" : "+v"(v));
    return (T)v;
}

constexpr int kMaxVecAll = 8;    // float4 groups per lane: C <= 64 * 4 * 8 = 2048 (template NV <= 8)

// ---------------------------------------------------------------------------------------
// LayerNorm forward: one wave per row
// ---------------------------------------------------------------------------------------
// With a residual update fused in front (z != NULL):  t = x + sc[b] * gamma * z  is written to `sum`
// (fp32) and normalised in the same pass - the pattern  x = x + drop_path(gamma * f(..)); h = norm(x)
// of consecutive sub-blocks (base/vit.py:301-306), which otherwise re-reads x from HBM.
template <typename T>
struct ResidualIn {
    const T *z;               // NULL: plain LayerNorm of x
    const float *gamma, *sc;  // optional
    int64_t rows_per_batch;
    float *sum;               // t out (forward) / unused (backward)
};

template <typename T, int kMaxVec, bool kRes>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float *__restrict__ x,
                                                     const float *__restrict__ w,
                                                     const float *__restrict__ b, int64_t rows, int C,
                                                     float eps, ResidualIn<T> res, T *__restrict__ y,
                                                     float *__restrict__ mean, float *__restrict__ rstd) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nvec = C >> 2;
    const float *xr = x + row * C;
    float4 v[kMaxVec];
    float s = 0.f;
    // every load of the row is requested before the first is used: with the residual operands read
    // under `if (res.z)` inside the slot loop each slot waited for its own x / z / gamma round trip
    vec4<T> zv[kMaxVec];
    float4 gm[kMaxVec], wv4[kMaxVec], bv4[kMaxVec];
    float sb = 1.f;
    if constexpr (kRes) sb = res.sc ? res.sc[row / res.rows_per_batch] : 1.f;
#pragma unroll
    for (int j = 0; j < kMaxVec; ++j) {
        const int i = min(lane + 64 * j, nvec - 1);          // clamped: dead slots re-read the last vector
        v[j] = *reinterpret_cast<const float4 *>(xr + 4 * i);
        if constexpr (kRes) {
            zv[j] = *reinterpret_cast<const vec4<T> *>(res.z + row * C + 4 * i);
            gm[j] = make_float4(1.f, 1.f, 1.f, 1.f);
            if (res.gamma) gm[j] = *reinterpret_cast<const float4 *>(res.gamma + 4 * i);
        }
        wv4[j] = *reinterpret_cast<const float4 *>(w + 4 * i);      // affine parameters too: their latency hides
        bv4[j] = *reinterpret_cast<const float4 *>(b + 4 * i);      // behind the two reductions
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < kMaxVec; ++j) {
        const int i = lane + 64 * j;
        if (i < nvec) {
            if constexpr (kRes) {
                v[j].x += sb * gm[j].x * (float)zv[j][0];
                v[j].y += sb * gm[j].y * (float)zv[j][1];
                v[j].z += sb * gm[j].z * (float)zv[j][2];
                v[j].w += sb * gm[j].w * (float)zv[j][3];
                *reinterpret_cast<float4 *>(res.sum + row * C + 4 * i) = v[j];
            }
        } else {
            v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        s += v[j].x + v[j].y + v[j].z + v[j].w;
    }
    const float mu = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxVec; ++j) {
        const int i = lane + 64 * j;
        if (i < nvec) {
            const float a = v[j].x - mu, b2 = v[j].y - mu, c = v[j].z - mu, d = v[j].w - mu;
            q += a * a + b2 * b2 + c * c + d * d;
        }
    }
    const float rs = rsqrtf(wave_sum(q) / (float)C + eps);
    T *yr = y + row * C;
#pragma unroll
    for (int j = 0; j < kMaxVec; ++j) {
        const int i = lane + 64 * j;
        if (i < nvec) {
            const float4 ww = wv4[j], bb = bv4[j];
            vec4<T> o;
            o[0] = (T)((v[j].x - mu) * rs * ww.x + bb.x);
            o[1] = (T)((v[j].y - mu) * rs * ww.y + bb.y);
            o[2] = (T)((v[j].z - mu) * rs * ww.z + bb.z);
            o[3] = (T)((v[j].w - mu) * rs * ww.w + bb.w);
            *reinterpret_cast<vec4<T> *>(yr + 4 * i) = o;
        }
    }
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs;
    }
}

// Column sums that every workgroup contributes to (dweight, dbias, dgamma, conv weight grads) are
// NOT accumulated with atomics: thousands of workgroups adding into the same few 128-byte lines run
// an order of magnitude below the atomic rate (measured: the atomic version made the whole training
// step 15 % slower).  Each workgroup writes one row of partials; finalize_partials sums the rows.
constexpr int kMaxParts = 512;
#ifndef VAH_LN_FLY
#define VAH_LN_FLY 1           // rows in flight per wave in ln_bwd_kernel
#endif

// out[k] = sum_p part[p][k].  Workgroup = 32 columns x 8 partial-row lanes, 8 independent loads in
// flight per thread (a one-thread-per-column loop over the rows is a 500-deep dependent-latency
// chain: measured 235 us per call, 18 ms per training step).
__global__ __launch_bounds__(256) void finalize_partials(const float *__restrict__ part, int nparts,
                                                         int K, float *__restrict__ out0, int K0,
                                                         float *__restrict__ out1, int K1,
                                                         float *__restrict__ out2) {
    __shared__ float s_acc[8][32];
    const int col = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int k = blockIdx.x * 32 + col;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k < K) {
        int p = pl;
        for (; p + 56 < nparts; p += 64) {
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += part[(int64_t)(p + 8 * u) * K + k];
        }
        for (; p < nparts; p += 8) acc[0] += part[(int64_t)p * K + k];
    }
    s_acc[pl][col] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    __syncthreads();
    if (pl == 0 && k < K) {
        float t = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) t += s_acc[u][col];
        if (k < K0) out0[k] = t;
        else if (k - K0 < K1) {
            if (out1) out1[k - K0] = t;
        } else if (out2) out2[k - K0 - K1] = t;
    }
}

// LayerNorm backward: a wave walks rows (grid stride); the waves of a workgroup are summed through
// LDS into one partial row [dw | db] or, with a fused residual update in front, [dw | db | dgamma].
//
// Register budget decides this kernel: with the per-column accumulators and the affine weights in
// registers it needed 256 VGPRs at C = 768 (2 waves per SIMD = ONE 8-wave workgroup per CU, so a
// 512-workgroup grid ran as two back-to-back rounds, each a full load -> reduce -> store latency
// chain).  The accumulators now live in the wave's own LDS row (plain read-add-write, no atomics:
// nobody else touches it; ~100 LDS clocks per row) and the weights are read from LDS where used.
//
// kBsum (with kRes and no gamma only): dz is the gradient a Linear reads next, and its bias gradient is the column
// sum of dz.  Without a gamma the third LDS column would hold a dgamma nobody reads; it sums the rounded dz
// instead and goes out as one row of `bpart` (stride C), the rows [dw | db] of `part` then have stride 2C.  z is
// not read at all in this form.
template <typename T, int kMaxVec, int kWaves, bool kRes, int kFly, bool kBsum = false>
__global__ __launch_bounds__(64 * kWaves) void ln_bwd_kernel(const float *__restrict__ x,
                                                     const T *__restrict__ g,
                                                     const float *__restrict__ w,
                                                     const float *__restrict__ mean,
                                                     const float *__restrict__ rstd,
                                                     const float *__restrict__ gres, int64_t rows, int C,
                                                     ResidualIn<T> res, T *__restrict__ dz,
                                                     float *__restrict__ dx, float *__restrict__ part,
                                                     float *__restrict__ bpart = nullptr) {
    static_assert(kRes || !kBsum, "the bias partials ride on the residual form");
    constexpr int ncol = kRes ? 3 : 2;       // kRes: res.z != nullptr (compile time: its registers)
    extern __shared__ __attribute__((aligned(16))) float s_red[];      // [kWaves][ncol * C] | w[C] | gamma[C]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nvec = C >> 2;
    float *acc = s_red + wv * ncol * C;                 // this wave's [dw | db | dgamma] sums
    float *s_w = s_red + kWaves * ncol * C;
    float *s_gm = s_w + C;
    for (int k = lane; k < ncol * nvec; k += 64)
        reinterpret_cast<float4 *>(acc)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = threadIdx.x; k < nvec; k += 64 * kWaves) {
        reinterpret_cast<float4 *>(s_w)[k] = *reinterpret_cast<const float4 *>(w + 4 * k);
        if constexpr (kRes)
            reinterpret_cast<float4 *>(s_gm)[k] =
                res.gamma ? *reinterpret_cast<const float4 *>(res.gamma + 4 * k) : make_float4(1.f, 1.f, 1.f, 1.f);
    }
    __syncthreads();
    const float invC = 1.f / (float)C;
    // kFly rows per wave in flight: one row's loads -> two wave reductions -> stores is a serial chain
    const int64_t stride = (int64_t)gridDim.x * kWaves;
    for (int64_t row = (int64_t)blockIdx.x * kWaves + wv; row < rows; row += kFly * stride) {
        int64_t rws[kFly];
        float4 xv[kFly][kMaxVec], rv[kFly][kMaxVec];
        vec4<T> gv[kFly][kMaxVec], zv[kFly][kMaxVec];
        float mu[kFly], rs[kFly], sb[kFly];
#pragma unroll
        for (int u = 0; u < kFly; ++u) {
            rws[u] = row + u * stride;
            if (rws[u] >= rows) rws[u] = row;            // harmless duplicate loads, results unused
            mu[u] = mean[rws[u]];
            rs[u] = rstd[rws[u]];
            sb[u] = (kRes && res.sc) ? res.sc[rws[u] / res.rows_per_batch] : 1.f;
#pragma unroll
            for (int j = 0; j < kMaxVec; ++j) {
                const int i = lane + 64 * j;
                if (i < nvec) {
                    xv[u][j] = *reinterpret_cast<const float4 *>(x + rws[u] * C + 4 * i);
                    gv[u][j] = *reinterpret_cast<const vec4<T> *>(g + rws[u] * C + 4 * i);
                    rv[u][j] = gres ? *reinterpret_cast<const float4 *>(gres + rws[u] * C + 4 * i)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
                    if constexpr (kRes && !kBsum) zv[u][j] = *reinterpret_cast<const vec4<T> *>(res.z + rws[u] * C + 4 * i);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kFly; ++u) {
            if (row + u * stride >= rows) break;
            float4 xh[kMaxVec], gw[kMaxVec];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int j = 0; j < kMaxVec; ++j) {
                const int i = lane + 64 * j;
                xh[j] = gw[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < nvec) {
                    const float4 xr = xv[u][j];
                    const float4 wj = *reinterpret_cast<const float4 *>(s_w + 4 * i);
                    const float g0 = (float)gv[u][j][0], g1 = (float)gv[u][j][1], g2 = (float)gv[u][j][2],
                                g3 = (float)gv[u][j][3];
                    xh[j] = make_float4((xr.x - mu[u]) * rs[u], (xr.y - mu[u]) * rs[u], (xr.z - mu[u]) * rs[u],
                                        (xr.w - mu[u]) * rs[u]);
                    gw[j] = make_float4(g0 * wj.x, g1 * wj.y, g2 * wj.z, g3 * wj.w);
                    s1 += gw[j].x + gw[j].y + gw[j].z + gw[j].w;
                    s2 += gw[j].x * xh[j].x + gw[j].y * xh[j].y + gw[j].z * xh[j].z + gw[j].w * xh[j].w;
                    float4 *pw = reinterpret_cast<float4 *>(acc + 4 * i), *pb = reinterpret_cast<float4 *>(acc + C + 4 * i);
                    float4 aw = *pw, ab = *pb;
                    aw.x += g0 * xh[j].x;
                    aw.y += g1 * xh[j].y;
                    aw.z += g2 * xh[j].z;
                    aw.w += g3 * xh[j].w;
                    ab.x += g0;
                    ab.y += g1;
                    ab.z += g2;
                    ab.w += g3;
                    *pw = aw;
                    *pb = ab;
                }
            }
            const float m1 = wave_sum(s1) * invC, m2 = wave_sum(s2) * invC;
            float *dr = dx + rws[u] * C;
#pragma unroll
            for (int j = 0; j < kMaxVec; ++j) {
                const int i = lane + 64 * j;
                if (i < nvec) {
                    const float4 r = rv[u][j];           // gradient of the residual branch of x (or 0)
                    const float k = rs[u];
                    const float4 d =
                        make_float4(r.x + k * (gw[j].x - m1 - xh[j].x * m2), r.y + k * (gw[j].y - m1 - xh[j].y * m2),
                                    r.z + k * (gw[j].z - m1 - xh[j].z * m2), r.w + k * (gw[j].w - m1 - xh[j].w * m2));
                    *reinterpret_cast<float4 *>(dr + 4 * i) = d;
                    if constexpr (kRes) {                 // t = x + sc * gamma * z in front: dz, dgamma from dt = d
                        const float4 gm = *reinterpret_cast<const float4 *>(s_gm + 4 * i);
                        vec4<T> o;
                        o[0] = round16<T>(sb[u] * gm.x * d.x);
                        o[1] = round16<T>(sb[u] * gm.y * d.y);
                        o[2] = round16<T>(sb[u] * gm.z * d.z);
                        o[3] = round16<T>(sb[u] * gm.w * d.w);
                        *reinterpret_cast<vec4<T> *>(dz + rws[u] * C + 4 * i) = o;
                        float4 *pg = reinterpret_cast<float4 *>(acc + 2 * C + 4 * i);
                        float4 ag = *pg;
                        if constexpr (kBsum) {            // the bias gradient's term: dz as the Linear will read it
                            ag.x += (float)o[0];
                            ag.y += (float)o[1];
                            ag.z += (float)o[2];
                            ag.w += (float)o[3];
                        } else {
                            ag.x += sb[u] * d.x * (float)zv[u][j][0];
                            ag.y += sb[u] * d.y * (float)zv[u][j][1];
                            ag.z += sb[u] * d.z * (float)zv[u][j][2];
                            ag.w += sb[u] * d.w * (float)zv[u][j][3];
                        }
                        *pg = ag;
                    }
                }
            }
        }
    }
    __syncthreads();
    const int K = ncol * C;
    float *pr = part + (int64_t)blockIdx.x * (kBsum ? 2 * C : K);
    for (int k = threadIdx.x; k < K; k += 64 * kWaves) {
        float t = 0.f;
#pragma unroll
        for (int u = 0; u < kWaves; ++u) t += s_red[u * K + k];
        if (kBsum && k >= 2 * C) bpart[(int64_t)blockIdx.x * C + (k - 2 * C)] = t;
        else pr[k] = t;
    }
}

// ---------------------------------------------------------------------------------------
// Two LayerNorms of the SAME rows with different affine parameters (equal eps): the adapter
// normalises c with injector.feat_norm and, unchanged, again with extractor.query_norm
// (adapter_modules.py:112-117, 141-146), and x with extractor.feat_norm and the next injector's
// query_norm.  Statistics and xhat are shared: one read of x for both outputs, and one backward pass
//   dx = gres + rstd * (gw - mean(gw) - xhat * mean(gw * xhat)),   gw = ga * wa + gb * wb
// instead of two chained passes over 132 MB rows.
// ---------------------------------------------------------------------------------------
template <typename T, int kMaxVec>
__global__ __launch_bounds__(256) void ln_dual_fwd_kernel(const float *__restrict__ x, const float *__restrict__ wa,
                                                          const float *__restrict__ ba, const float *__restrict__ wb,
                                                          const float *__restrict__ bb, int64_t rows, int C, float eps,
                                                          T *__restrict__ ya, T *__restrict__ yb,
                                                          float *__restrict__ mean, float *__restrict__ rstd) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nvec = C >> 2;
    const float *xr = x + row * C;
    float4 v[kMaxVec];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxVec; ++j) {
        const int i = lane + 64 * j;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < nvec) v[j] = *reinterpret_cast<const float4 *>(xr + 4 * i);
        s += v[j].x + v[j].y + v[j].z + v[j].w;
    }
    const float mu = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxVec; ++j) {
        const int i = lane + 64 * j;
        if (i < nvec) {
            const float a = v[j].x - mu, b2 = v[j].y - mu, c = v[j].z - mu, d = v[j].w - mu;
            q += a * a + b2 * b2 + c * c + d * d;
        }
    }
    const float rs = rsqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int j = 0; j < kMaxVec; ++j) {
        const int i = lane + 64 * j;
        if (i < nvec) {
            const float4 xh = make_float4((v[j].x - mu) * rs, (v[j].y - mu) * rs, (v[j].z - mu) * rs, (v[j].w - mu) * rs);
            const float4 w1 = *reinterpret_cast<const float4 *>(wa + 4 * i), b1 = *reinterpret_cast<const float4 *>(ba + 4 * i);
            const float4 w2 = *reinterpret_cast<const float4 *>(wb + 4 * i), b2 = *reinterpret_cast<const float4 *>(bb + 4 * i);
            vec4<T> o1, o2;
            o1[0] = (T)(xh.x * w1.x + b1.x);
            o1[1] = (T)(xh.y * w1.y + b1.y);
            o1[2] = (T)(xh.z * w1.z + b1.z);
            o1[3] = (T)(xh.w * w1.w + b1.w);
            o2[0] = (T)(xh.x * w2.x + b2.x);
            o2[1] = (T)(xh.y * w2.y + b2.y);
            o2[2] = (T)(xh.z * w2.z + b2.z);
            o2[3] = (T)(xh.w * w2.w + b2.w);
            *reinterpret_cast<vec4<T> *>(ya + row * C + 4 * i) = o1;
            *reinterpret_cast<vec4<T> *>(yb + row * C + 4 * i) = o2;
        }
    }
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs;
    }
}

// partial row: [dwa | dba | dwb | dbb]
template <typename T, int kMaxVec>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kMaxVec <= 3 ? 3 : 1))) void ln_dual_bwd_kernel(const float *__restrict__ x, const T *__restrict__ ga,
                                                          const T *__restrict__ gb, const float *__restrict__ wa,
                                                          const float *__restrict__ wb, const float *__restrict__ mean,
                                                          const float *__restrict__ rstd, const float *__restrict__ gres,
                                                          int64_t rows, int C, float *__restrict__ dx,
                                                          float *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float s_red[];      // [4][4C]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nvec = C >> 2;
    float4 w1[kMaxVec], w2[kMaxVec], aw1[kMaxVec], ab1[kMaxVec], aw2[kMaxVec], ab2[kMaxVec];
#pragma unroll
    for (int j = 0; j < kMaxVec; ++j) {
        const int i = lane + 64 * j;
        w1[j] = w2[j] = aw1[j] = ab1[j] = aw2[j] = ab2[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < nvec) {
            w1[j] = *reinterpret_cast<const float4 *>(wa + 4 * i);
            w2[j] = *reinterpret_cast<const float4 *>(wb + 4 * i);
        }
    }
    const float invC = 1.f / (float)C;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < rows; row += (int64_t)gridDim.x * 4) {
        const float mu = mean[row], rs = rstd[row];
        float4 xh[kMaxVec], gw[kMaxVec], rv[kMaxVec];
        float s1 = 0.f, s2 = 0.f;
        // every load of the row is requested before the first is used (optional operands: a valid
        // stand-in address + select): with the loads under `ga ? .. : ..` inside the slot loop each vector
        // slot paid its own memory round trip, three per row
        float4 xl[kMaxVec];
        vec4<T> g1l[kMaxVec], g2l[kMaxVec];
        {
            const T *gap = ga ? ga : reinterpret_cast<const T *>(x);
            const T *gbp = gb ? gb : reinterpret_cast<const T *>(x);
            const float *grp = gres ? gres : x;
#pragma unroll
            for (int j = 0; j < kMaxVec; ++j) {
                const int i = min(lane + 64 * j, nvec - 1);
                xl[j] = *reinterpret_cast<const float4 *>(x + row * C + 4 * i);
                g1l[j] = *reinterpret_cast<const vec4<T> *>(gap + row * C + 4 * i);
                g2l[j] = *reinterpret_cast<const vec4<T> *>(gbp + row * C + 4 * i);
                rv[j] = *reinterpret_cast<const float4 *>(grp + row * C + 4 * i);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < kMaxVec; ++j) {
            const int i = lane + 64 * j;
            xh[j] = gw[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!gres || i >= nvec) rv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < nvec) {
                const float4 xv = xl[j];
                vec4<T> g1 = g1l[j], g2 = g2l[j];
                if (!ga) g1 = vec4<T>{};
                if (!gb) g2 = vec4<T>{};
                xh[j] = make_float4((xv.x - mu) * rs, (xv.y - mu) * rs, (xv.z - mu) * rs, (xv.w - mu) * rs);
                const float a0 = (float)g1[0], a1 = (float)g1[1], a2 = (float)g1[2], a3 = (float)g1[3];
                const float b0 = (float)g2[0], b1 = (float)g2[1], b2 = (float)g2[2], b3 = (float)g2[3];
                gw[j] = make_float4(a0 * w1[j].x + b0 * w2[j].x, a1 * w1[j].y + b1 * w2[j].y, a2 * w1[j].z + b2 * w2[j].z,
                                    a3 * w1[j].w + b3 * w2[j].w);
                s1 += gw[j].x + gw[j].y + gw[j].z + gw[j].w;
                s2 += gw[j].x * xh[j].x + gw[j].y * xh[j].y + gw[j].z * xh[j].z + gw[j].w * xh[j].w;
                aw1[j].x += a0 * xh[j].x, aw1[j].y += a1 * xh[j].y, aw1[j].z += a2 * xh[j].z, aw1[j].w += a3 * xh[j].w;
                ab1[j].x += a0, ab1[j].y += a1, ab1[j].z += a2, ab1[j].w += a3;
                aw2[j].x += b0 * xh[j].x, aw2[j].y += b1 * xh[j].y, aw2[j].z += b2 * xh[j].z, aw2[j].w += b3 * xh[j].w;
                ab2[j].x += b0, ab2[j].y += b1, ab2[j].z += b2, ab2[j].w += b3;
            }
        }
        const float m1 = wave_sum(s1) * invC, m2 = wave_sum(s2) * invC;
#pragma unroll
        for (int j = 0; j < kMaxVec; ++j) {
            const int i = lane + 64 * j;
            if (i < nvec)
                *reinterpret_cast<float4 *>(dx + row * C + 4 * i) =
                    make_float4(rv[j].x + rs * (gw[j].x - m1 - xh[j].x * m2), rv[j].y + rs * (gw[j].y - m1 - xh[j].y * m2),
                                rv[j].z + rs * (gw[j].z - m1 - xh[j].z * m2), rv[j].w + rs * (gw[j].w - m1 - xh[j].w * m2));
        }
    }
    const int K = 4 * C;
#pragma unroll
    for (int j = 0; j < kMaxVec; ++j) {
        const int i = lane + 64 * j;
        if (i < nvec) {
            *reinterpret_cast<float4 *>(s_red + wv * K + 4 * i) = aw1[j];
            *reinterpret_cast<float4 *>(s_red + wv * K + C + 4 * i) = ab1[j];
            *reinterpret_cast<float4 *>(s_red + wv * K + 2 * C + 4 * i) = aw2[j];
            *reinterpret_cast<float4 *>(s_red + wv * K + 3 * C + 4 * i) = ab2[j];
        }
    }
    __syncthreads();
    float *pr = part + (int64_t)blockIdx.x * K;
    for (int k = threadIdx.x; k < K; k += 256) pr[k] = (s_red[k] + s_red[K + k]) + (s_red[2 * K + k] + s_red[3 * K + k]);
}

// ---------------------------------------------------------------------------------------
// Column sums of a 16-bit (T: bf16 or fp16) [rows, C] matrix (bias gradient of a Linear).  Workgroup = 32 column lanes
// (8 elements = 16 bytes each: 256 columns) x 8 row lanes over a strip of rows; one partial row each.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void colsum_bf16_kernel(const T *__restrict__ g, int64_t rows,
                                                          int C, int rows_per_block,
                                                          float *__restrict__ part) {
    __shared__ float s_acc[8][256 + 8];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 256 + cl * 8;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = min(rows, r0 + rows_per_block);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c0 < C) {
        int64_t r = r0 + rl;
        for (; r + 24 < r1; r += 32) {           // 4 independent 16-byte loads in flight
            vec8<T> v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const vec8<T> *>(g + (r + 8 * u) * C + c0);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += (float)v[u][e];
        }
        for (; r < r1; r += 8) {
            const vec8<T> v = *reinterpret_cast<const vec8<T> *>(g + r * C + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s_acc[rl][cl * 8 + e] = acc[e];
    __syncthreads();
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        float t = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) t += s_acc[u][threadIdx.x];
        part[(int64_t)blockIdx.y * C + c] = t;
    }
}

// fp32 variant over `batch` row blocks of a strided tensor (token range [t0, t0 + rows) of every batch
// element of a (B, T, C) gradient): 32 column lanes x 4 floats, 8 row lanes; blockIdx.z = batch element.
__global__ __launch_bounds__(256) void colsum_f32_kernel(const float *__restrict__ g, int64_t rows, int C,
                                                         int64_t batch_stride, int rows_per_block,
                                                         float *__restrict__ part) {
    __shared__ float s_acc[8][128 + 4];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 128 + cl * 4;
    const float *gb = g + (int64_t)blockIdx.z * batch_stride;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = min(rows, r0 + rows_per_block);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 < C) {
        int64_t r = r0 + rl;
        for (; r + 24 < r1; r += 32) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4 *>(gb + (r + 8 * u) * C + c0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc.x += v[u].x;
                acc.y += v[u].y;
                acc.z += v[u].z;
                acc.w += v[u].w;
            }
        }
        for (; r < r1; r += 8) {
            const float4 v = *reinterpret_cast<const float4 *>(gb + r * C + c0);
            acc.x += v.x;
            acc.y += v.y;
            acc.z += v.z;
            acc.w += v.w;
        }
    }
    s_acc[rl][cl * 4 + 0] = acc.x;
    s_acc[rl][cl * 4 + 1] = acc.y;
    s_acc[rl][cl * 4 + 2] = acc.z;
    s_acc[rl][cl * 4 + 3] = acc.w;
    __syncthreads();
    const int c = blockIdx.x * 128 + threadIdx.x;
    if (threadIdx.x < 128 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) t += s_acc[u][threadIdx.x];
        part[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * C + c] = t;
    }
}

// ---------------------------------------------------------------------------------------
// y = x + s[b] * gamma[c] * z
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void scale_residual_fwd_kernel(
    const float *__restrict__ x, const T *__restrict__ z, const float *__restrict__ gamma,
    const float *__restrict__ s, int64_t rows_per_batch, int C, int64_t total_vec, float *__restrict__ y) {
    const int nvec = C >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_vec; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / nvec;
        const int cv = (int)(i - row * nvec);
        const float sb = s ? s[row / rows_per_batch] : 1.f;
        const float4 xv = *reinterpret_cast<const float4 *>(x + 4 * i);
        const vec4<T> zv = *reinterpret_cast<const vec4<T> *>(z + 4 * i);
        float4 gm = make_float4(1.f, 1.f, 1.f, 1.f);
        if (gamma) gm = *reinterpret_cast<const float4 *>(gamma + 4 * cv);
        *reinterpret_cast<float4 *>(y + 4 * i) =
            make_float4(xv.x + sb * gm.x * (float)zv[0], xv.y + sb * gm.y * (float)zv[1],
                        xv.z + sb * gm.z * (float)zv[2], xv.w + sb * gm.w * (float)zv[3]);
    }
}

// dz = s[b] * gamma * g (bf16);  dgamma[c] += sum s[b] * g * z.  A wave owns 64 float4 column groups
// (1 KB of a row), the 4 waves of a workgroup take every 4th row of the strip with 4 rows in flight
// each (a thread-per-column-group walk with one row in flight ran at 1.5 TB/s); dgamma partials stay
// in registers and are summed over the 4 waves through LDS.
// kBsum: a second register accumulator sums the rounded dz (the bias gradient of the Linear that made z), reduced
// like the first into row blockIdx.x of `bpart`; kDg = false (no gamma: no dgamma) leaves z unread.
template <typename T, bool kBsum = false, bool kDg = true>
__global__ __launch_bounds__(256) void scale_residual_bwd_kernel(
    const float *__restrict__ g, const T *__restrict__ z, const float *__restrict__ gamma,
    const float *__restrict__ s, int64_t rows, int64_t rows_per_batch, int C, int rows_per_block,
    T *__restrict__ dz, float *__restrict__ part, float *__restrict__ bpart = nullptr) {
    __shared__ float4 s_acc[4][64];
    __shared__ float4 s_bacc[kBsum ? 4 : 1][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nvec = C >> 2;
    const int64_t row0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t row1 = min(rows, row0 + (int64_t)rows_per_block);
    for (int cv0 = 0; cv0 < nvec; cv0 += 64) {
        const int cv = cv0 + lane;
        const bool on = cv < nvec;
        float4 gm = make_float4(1.f, 1.f, 1.f, 1.f);
        if (gamma && on) gm = *reinterpret_cast<const float4 *>(gamma + 4 * cv);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), bacc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t r = row0 + wv; r < row1; r += 16) {
            float4 gv[4];
            vec4<T> zv[4];
            float sb[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t rr = r + 4 * u;
                ok[u] = on && rr < row1;
                if (ok[u]) {
                    const int64_t off = rr * C + 4 * cv;
                    gv[u] = *reinterpret_cast<const float4 *>(g + off);
                    if constexpr (kDg) zv[u] = *reinterpret_cast<const vec4<T> *>(z + off);
                    sb[u] = s ? s[rr / rows_per_batch] : 1.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!ok[u]) continue;
                const int64_t off = (r + 4 * u) * C + 4 * cv;
                vec4<T> o;
                o[0] = round16<T>(sb[u] * gm.x * gv[u].x);
                o[1] = round16<T>(sb[u] * gm.y * gv[u].y);
                o[2] = round16<T>(sb[u] * gm.z * gv[u].z);
                o[3] = round16<T>(sb[u] * gm.w * gv[u].w);
                *reinterpret_cast<vec4<T> *>(dz + off) = o;
                if constexpr (kDg) {
                    acc.x += sb[u] * gv[u].x * (float)zv[u][0];
                    acc.y += sb[u] * gv[u].y * (float)zv[u][1];
                    acc.z += sb[u] * gv[u].z * (float)zv[u][2];
                    acc.w += sb[u] * gv[u].w * (float)zv[u][3];
                }
                if constexpr (kBsum) {
                    bacc.x += (float)o[0];
                    bacc.y += (float)o[1];
                    bacc.z += (float)o[2];
                    bacc.w += (float)o[3];
                }
            }
        }
        if constexpr (kBsum) {
            if constexpr (kDg) s_acc[wv][lane] = acc;
            s_bacc[wv][lane] = bacc;
            __syncthreads();
            if (wv == 0 && on && kDg && part) {
                const float4 a = s_acc[0][lane], b = s_acc[1][lane], c = s_acc[2][lane], d = s_acc[3][lane];
                *reinterpret_cast<float4 *>(part + (int64_t)blockIdx.x * C + 4 * cv) =
                    make_float4((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y), (a.z + b.z) + (c.z + d.z),
                                (a.w + b.w) + (c.w + d.w));
            }
            if (wv == 1 && on) {
                const float4 a = s_bacc[0][lane], b = s_bacc[1][lane], c = s_bacc[2][lane], d = s_bacc[3][lane];
                *reinterpret_cast<float4 *>(bpart + (int64_t)blockIdx.x * C + 4 * cv) =
                    make_float4((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y), (a.z + b.z) + (c.z + d.z),
                                (a.w + b.w) + (c.w + d.w));
            }
            __syncthreads();
        } else if (part) {
            s_acc[wv][lane] = acc;
            __syncthreads();
            if (wv == 0 && on) {
                const float4 a = s_acc[0][lane], b = s_acc[1][lane], c = s_acc[2][lane], d = s_acc[3][lane];
                *reinterpret_cast<float4 *>(part + (int64_t)blockIdx.x * C + 4 * cv) =
                    make_float4((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y), (a.z + b.z) + (c.z + d.z),
                                (a.w + b.w) + (c.w + d.w));
            }
            __syncthreads();
        }
    }
}

// dz = s[b] * g without a layer scale: no column reduction to carry, a flat streaming pass
// (blockIdx.y = batch element, so no per-element division for s[b]).
template <typename T>
__global__ __launch_bounds__(256) void scale_only_bwd_kernel(const float *__restrict__ g, const float *__restrict__ s,
                                                             int64_t vec_per_batch, T *__restrict__ dz) {
    const float sb = s ? s[blockIdx.y] : 1.f;
    const int64_t base = (int64_t)blockIdx.y * vec_per_batch;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < vec_per_batch; i += (int64_t)gridDim.x * 256) {
        const float4 v = *reinterpret_cast<const float4 *>(g + 4 * (base + i));
        vec4<T> o;
        o[0] = round16<T>(sb * v.x);
        o[1] = round16<T>(sb * v.y);
        o[2] = round16<T>(sb * v.z);
        o[3] = round16<T>(sb * v.w);
        *reinterpret_cast<vec4<T> *>(dz + 4 * (base + i)) = o;
    }
}

// ---------------------------------------------------------------------------------------
// depthwise 3x3 on the concatenated token maps
// ---------------------------------------------------------------------------------------
struct Maps {          // token ranges [t0, t1) of the 3 maps and their (h, w)
    int t[4];
    int h[3], w[3];
};

__device__ __forceinline__ int map_of(const Maps &mp, int tok) { return tok >= mp.t[2] ? 2 : (tok >= mp.t[1] ? 1 : 0); }

// Work item of the depthwise kernels: one pixel column of a strip of R rows of one map of one image, for one group of
// 4 channels.  Items are numbered image by image, map by map, strip by strip, left to right, so the token slots of a
// workgroup are neighbouring columns and share their left / right neighbour rows in L1.  An item never leaves its map.
__host__ __device__ inline int dw_items_per_image(const Maps &mp, int R) {
    int n = 0;
    for (int m = 0; m < 3; ++m) n += (mp.h[m] + R - 1) / R * mp.w[m];
    return n;
}

struct DwItem {
    int64_t tok0;      // first token of the item's map in its image, counted over the whole (B, N) tensor
    int H, W, y0, px;  // the map's size, the strip's first row, the column
};

template <int R>
__device__ __forceinline__ DwItem dw_item(const Maps &mp, int N, int items_per_img, int item) {
    const int b = item / items_per_img;
    int r = item - b * items_per_img, m = 0;
    for (; m < 2; ++m) {
        const int n = (mp.h[m] + R - 1) / R * mp.w[m];
        if (r < n) break;
        r -= n;
    }
    DwItem it;
    it.H = mp.h[m], it.W = mp.w[m];
    const int strip = r / it.W;
    it.px = r - strip * it.W;
    it.y0 = strip * R;
    it.tok0 = (int64_t)b * N + mp.t[m];
    return it;
}

// The R + 2 rows x 3 columns of neighbours an item needs, every one requested before the first is used.  Coordinates
// are clamped into the map (the taps outside get a zero weight), so no load sits under a condition: loads under
// `if (inside)` each got their own s_waitcnt vmcnt(0).
template <typename T, int R>
__device__ __forceinline__ void dw_load_window(const T *__restrict__ x, const DwItem &it, int C, int cv, vec4<T> (&v)[R + 2][3]) {
    const T *base = x + it.tok0 * C + 4 * cv;
#pragma unroll
    for (int j = 0; j < R + 2; ++j) {
        const int yc = min(max(it.y0 + j - 1, 0), it.H - 1);
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int xc = min(max(it.px + dx - 1, 0), it.W - 1);
            v[j][dx] = *reinterpret_cast<const vec4<T> *>(base + (int64_t)(yc * it.W + xc) * C);
        }
    }
}

constexpr int kDwRows = 8;       // rows per item, forward and input gradient: 30 loads for 8 outputs (a thread per
                                 // output took 9 each, and paid the 36 tap loads of its prologue for 2 outputs)
constexpr int kDwRowsWgrad = 4;  // weight gradient: 18 + 4 loads for 4 tokens; shorter strips spread the items evenly
                                 // over the at most kMaxParts workgroups

// mode 0: out = conv(x) + bias      (weights as given)
// mode 1: out = conv with the flipped kernel (input gradient), no bias
// Thread = (item, channel group of 4): the 36 filter taps of its channels stay in registers while it walks down its
// column; each output is the same sum in the same order as one thread per output gave (bias, taps 0..8, one cast).
template <typename T, int MODE>
__global__ __launch_bounds__(256) void dwconv_kernel(const T *__restrict__ x,
                                                     const float *__restrict__ w,
                                                     const float *__restrict__ bias, Maps mp, int N,
                                                     int C, int items_per_img, int total_items, T *__restrict__ y) {
    constexpr int R = kDwRows;
    const int nvec = C >> 2;
    const int slots = 256 / nvec;
    const int slot = threadIdx.x / nvec, cv = threadIdx.x - slot * nvec;
    const int item = (int)blockIdx.x * slots + slot;
    if (slot >= slots || item >= total_items) return;
    const DwItem it = dw_item<R>(mp, N, items_per_img, item);
    // the 36 taps of 4 channels are 144 contiguous bytes
    float wr[36];
    const float *wp = w + 36 * cv;
    if (((uintptr_t)w & 15) == 0) {
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const float4 t = *reinterpret_cast<const float4 *>(wp + 4 * q);
            wr[4 * q] = t.x, wr[4 * q + 1] = t.y, wr[4 * q + 2] = t.z, wr[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 36; ++k) wr[k] = wp[k];
    }
    // flipped taps and the column's left / right border folded into the weights once
    const bool in_l = it.px > 0, in_r = it.px + 1 < it.W;
    float wt[4][9];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float v = wr[c * 9 + (MODE == 0 ? t : 8 - t)];
            wt[c][t] = t % 3 == 0 ? (in_l ? v : 0.f) : (t % 3 == 2 ? (in_r ? v : 0.f) : v);
        }
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MODE == 0 && bias) b4 = *reinterpret_cast<const float4 *>(bias + 4 * cv);
    vec4<T> v[R + 2][3];
    dw_load_window<T, R>(x, it, C, cv, v);
    __builtin_amdgcn_sched_barrier(0);                  // keep the loads above their uses (the scheduler sank them)
    T *yp = y + (it.tok0 + (int64_t)it.y0 * it.W + it.px) * C + 4 * cv;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int py = it.y0 + r;
        float4 acc = b4;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            // row above: outside only for the first row of the map; row below: outside for the last
            const bool in = tap < 3 ? (r > 0 || it.y0 > 0) : (tap < 6 ? true : py + 1 < it.H);
            const vec4<T> &n = v[r + tap / 3][tap % 3];
            acc.x += (in ? wt[0][tap] : 0.f) * (float)n[0];
            acc.y += (in ? wt[1][tap] : 0.f) * (float)n[1];
            acc.z += (in ? wt[2][tap] : 0.f) * (float)n[2];
            acc.w += (in ? wt[3][tap] : 0.f) * (float)n[3];
        }
        vec4<T> o;
        o[0] = (T)acc.x;
        o[1] = (T)acc.y;
        o[2] = (T)acc.z;
        o[3] = (T)acc.w;
        // a strip may end below the map; its first row never does (said so that the row above it is not loaded under
        // this condition, after the wait for all the other rows)
        if (r == 0 || py < it.H) *reinterpret_cast<vec4<T> *>(yp + (int64_t)r * it.W * C) = o;
    }
}

// dw[c][tap] = sum_tok g[tok,c] * x[neighbour(tok,tap), c];  db[c] = sum g.  Thread = (token slot, channel group):
// walks items with a grid stride, 40 partial sums in registers; the slots of a workgroup are summed through LDS into
// one partial row [dw (C*9) | db (C)].  Items, slots and the order of every sum are fixed by the shape: two calls
// agree bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const T *__restrict__ x,
                                                           const T *__restrict__ g, Maps mp, int N,
                                                           int C, int items_per_img, int total_items,
                                                           float *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float s_red[];      // [slots][C*10]
    constexpr int R = kDwRowsWgrad;
    const int nvec = C >> 2;
    const int slots = 256 / nvec;                    // token slots per block (>= 1 when C <= 1024)
    const int slot = threadIdx.x / nvec, cv = threadIdx.x - slot * nvec;
    const bool live = slot < slots;
    float aw[4][9], ab[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < 9; ++t) aw[c][t] = 0.f;
    if (live)
        for (int item = (int)blockIdx.x * slots + slot; item < total_items; item += (int)gridDim.x * slots) {
            const DwItem it = dw_item<R>(mp, N, items_per_img, item);
            const bool in_l = it.px > 0, in_r = it.px + 1 < it.W;
            vec4<T> v[R + 2][3], gv[R];
            dw_load_window<T, R>(x, it, C, cv, v);
            const T *gp = g + (it.tok0 + it.px) * C + 4 * cv;
#pragma unroll
            for (int r = 0; r < R; ++r)                       // rows past the map's last: its last row again, weight zero
                gv[r] = *reinterpret_cast<const vec4<T> *>(gp + (int64_t)min(it.y0 + r, it.H - 1) * it.W * C);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int py = it.y0 + r;
                const bool row = py < it.H;
                float gf[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    gf[c] = row ? (float)gv[r][c] : 0.f;
                    ab[c] += gf[c];
                }
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const bool in = (tap < 3 ? (r > 0 || it.y0 > 0) : (tap < 6 ? true : py + 1 < it.H)) &&
                                    (tap % 3 == 0 ? in_l : (tap % 3 == 2 ? in_r : true));
#pragma unroll
                    for (int c = 0; c < 4; ++c) aw[c][tap] += (in ? gf[c] : 0.f) * (float)v[r + tap / 3][tap % 3][c];
                }
            }
        }
    const int K = C * 10;
    if (live) {
        float *r = s_red + slot * K;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int t = 0; t < 9; ++t) r[(4 * cv + c) * 9 + t] = aw[c][t];
            r[C * 9 + 4 * cv + c] = ab[c];
        }
    }
    __syncthreads();
    float *pr = part + (int64_t)blockIdx.x * K;
    for (int k = threadIdx.x; k < K; k += 256) {
        float acc = 0.f;
        for (int sl = 0; sl < slots; ++sl) acc += s_red[sl * K + k];
        pr[k] = acc;
    }
}

inline unsigned grid_for(int64_t work_items, int per_block) {
    int64_t g = (work_items + per_block - 1) / per_block;
    const int64_t cap = (int64_t)kCUs * 16;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// ---------------------------------------------------------------------------------------
// Launch helpers: one copy of the argument checks, launch geometry and workspace layout for both element
// types.  `fn` is the entry point's own name (messages), T its 16-bit type.
// ---------------------------------------------------------------------------------------
template <typename T>
int ln_fwd_launch(const char *fn, const float *x, const float *w, const float *b, int64_t rows, int64_t C, float eps,
                  ResidualIn<T> res, void *y, float *mean, float *rstd, void *stream) {
    clear_error();
    if (rows < 0 || C < 4 || C % 4 || C > 64 * 4 * kMaxVecAll) return fail(VAH_E_SHAPE, "%s: C=%lld unsupported", fn, (long long)C);
    if (rows == 0) return VAH_OK;
    if (!x || !w || !b || !y || !mean || !rstd) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)b) % 16 || (uintptr_t)y % 8) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope(res.z ? tname<T>("residual_layernorm_fwd", "residual_layernorm_fwd_f16")
                            : tname<T>("layernorm_fwd", "layernorm_fwd_f16"),
                      rows * C * (res.z ? 12 : 6), st);
#define VAH_LN_FWD(NV)                                                                          \
    do {                                                                                        \
        if (res.z)                                                                              \
            hipLaunchKernelGGL((ln_fwd_kernel<T, NV, true>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, w, b, \
                               rows, (int)C, eps, res, (T *)y, mean, rstd);                     \
        else                                                                                    \
            hipLaunchKernelGGL((ln_fwd_kernel<T, NV, false>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, w, b, \
                               rows, (int)C, eps, res, (T *)y, mean, rstd);                     \
    } while (0)
    if (C <= 256) VAH_LN_FWD(1);
    else if (C <= 512) VAH_LN_FWD(2);
    else if (C <= 768) VAH_LN_FWD(3);
    else if (C <= 1024) VAH_LN_FWD(4);
    else VAH_LN_FWD(8);
#undef VAH_LN_FWD
    return check_launch(fn);
}

// t = x + sc[b] * gamma * z (written to t, fp32), h = LayerNorm(t) (T): the scale-residual forward and the
// LayerNorm forward in one pass over the rows.  gamma, sc optional.
template <typename T>
int residual_ln_fwd(const char *fn, const float *x, const void *z, const float *gamma, const float *sc, int64_t batch,
                    int64_t rows_per_batch, int64_t C, const float *w, const float *b, float eps, float *t, void *h,
                    float *mean, float *rstd, void *stream) {
    clear_error();
    if (batch < 0 || rows_per_batch < 0) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    if (batch * rows_per_batch > 0 && (!z || !t)) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)gamma | (uintptr_t)t) % 16 || (uintptr_t)z % 8) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    return ln_fwd_launch<T>(fn, x, w, b, batch * rows_per_batch, C, eps,
                            ResidualIn<T>{(const T *)z, gamma, sc, std::max<int64_t>(rows_per_batch, 1), t}, h, mean, rstd,
                            stream);
}

template <typename T, bool kBsumT = false>
int ln_bwd_launch(const char *fn, const float *x, const void *g, const float *w, const float *mean, const float *rstd,
                  const float *gres, int64_t rows, int64_t C, ResidualIn<T> res, void *dz, float *dx, float *dw, float *db,
                  float *dgamma, float *ws, void *stream, float *bpart = nullptr, int64_t *nparts = nullptr) {
    clear_error();
    if (rows < 0 || C < 4 || C % 4 || C > 64 * 4 * kMaxVecAll) return fail(VAH_E_SHAPE, "%s: C=%lld unsupported", fn, (long long)C);
    if (!dw || !db || !ws) return fail(VAH_E_NULL, "%s: null pointer", fn);
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {
        (void)hipMemsetAsync(dw, 0, C * 4, st);
        (void)hipMemsetAsync(db, 0, C * 4, st);
        if (dgamma) (void)hipMemsetAsync(dgamma, 0, C * 4, st);
        if (nparts) *nparts = 0;
        return VAH_OK;
    }
    if (!x || !g || !w || !mean || !rstd || !dx) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)dx | (uintptr_t)gres) % 16 || (uintptr_t)g % 8) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    const int ncol = res.z ? 3 : 2;
    const bool bsum = bpart != nullptr;          // residual form without gamma (checked by the entry point)
    // 8 waves per workgroup when their LDS reduction buffer leaves room for two workgroups per CU:
    // the partial-row cap bounds the grid at 512 workgroups, and with 4 waves each that is 2 waves per
    // SIMD - too few to cover the latency of this kernel's load -> reduce -> store chain
    const size_t wbytes = (size_t)(res.z ? 2 : 1) * C * sizeof(float);      // affine weights kept in LDS
    const int waves = (size_t)8 * ncol * C * sizeof(float) + wbytes <= 80 * 1024 ? 8 : 4;
    int64_t nblocks = (rows + waves - 1) / waves;
    nblocks = std::min<int64_t>(nblocks, kMaxParts);          // the scratch holds kMaxParts * ncol * C floats
    const size_t smem = (size_t)waves * ncol * C * sizeof(float) + wbytes;
    LaunchScope scope(res.z ? tname<T>("residual_layernorm_bwd", "residual_layernorm_bwd_f16")
                            : tname<T>("layernorm_bwd", "layernorm_bwd_f16"),
                      rows * C * (res.z ? 18 : 10), st);
    if (smem > 150 * 1024) return fail(VAH_E_SHAPE, "%s: C too large for the fused form", fn);
    constexpr int kLnFly = VAH_LN_FLY;
#define VAH_LN_BWD(NV, WV, RS, BS)                                                                 \
    do {                                                                                         \
        if (smem > 64 * 1024)                                                                    \
            (void)hipFuncSetAttribute((const void *)ln_bwd_kernel<T, NV, WV, RS, kLnFly, BS>,            \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);    \
        hipLaunchKernelGGL((ln_bwd_kernel<T, NV, WV, RS, kLnFly, BS>), dim3((unsigned)nblocks), dim3(64 * WV), smem, st, x, \
                           (const T *)g, w, mean, rstd, gres, rows, (int)C, res, (T *)dz, dx, ws, bpart); \
    } while (0)
#define VAH_LN_BWD_W(NV)        \
    do {                        \
        if constexpr (kBsumT) {                               \
            if (bsum && waves == 8) { VAH_LN_BWD(NV, 8, true, true); break; }  \
            if (bsum) { VAH_LN_BWD(NV, 4, true, true); break; }                \
        }                                                     \
        if (waves == 8 && res.z) VAH_LN_BWD(NV, 8, true, false); \
        else if (waves == 8) VAH_LN_BWD(NV, 8, false, false); \
        else if (res.z) VAH_LN_BWD(NV, 4, true, false); \
        else VAH_LN_BWD(NV, 4, false, false); \
    } while (0)
    if (C <= 256) VAH_LN_BWD_W(1);
    else if (C <= 512) VAH_LN_BWD_W(2);
    else if (C <= 768) VAH_LN_BWD_W(3);
    else if (C <= 1024) VAH_LN_BWD_W(4);
    else VAH_LN_BWD_W(8);
#undef VAH_LN_BWD_W
#undef VAH_LN_BWD
    // partial row = [dw | db | dgamma], or [dw | db] beside the bias partials
    const int fcol = bsum ? 2 : ncol;
    hipLaunchKernelGGL(finalize_partials, dim3((unsigned)((fcol * C + 31) / 32)), dim3(256), 0, st, ws,
                       (int)nblocks, (int)(fcol * C), dw, (int)C, db, (int)C, dgamma);
    if (nparts) *nparts = nblocks;
    return check_launch(fn);
}

// Backward of residual_ln_fwd: dt = gt + LayerNorm'(gh) (the gradient of x as well), dz = sc * gamma * dt (T),
// dgamma = sum sc * dt * z, dw, db.  gt (gradient of t along the residual stream) and gamma / sc / dgamma
// optional.  ws: vah_reduce_ws_floats(3*C).
// kBsum: also the partial rows of the column sums of dz (the bias gradient of the Linear that made z) - *nparts rows
// of C floats in bpart (vah_reduce_ws_floats(C)); without a gamma only.
template <typename T, bool kBsum = false>
int residual_ln_bwd(const char *fn, const float *t, const void *gh, const float *w, const float *mean, const float *rstd,
                    const float *gt, const void *z, const float *gamma, const float *sc, int64_t batch,
                    int64_t rows_per_batch, int64_t C, float *dt, void *dz, float *dgamma, float *dw, float *db, float *ws,
                    void *stream, float *bpart = nullptr, int64_t *nparts = nullptr) {
    clear_error();
    if (batch < 0 || rows_per_batch < 0) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    if (batch * rows_per_batch > 0 && (!z || !dz)) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if ((gamma != nullptr) != (dgamma != nullptr)) return fail(VAH_E_NULL, "%s: gamma and dgamma go together", fn);
    if ((uintptr_t)gamma % 16 || ((uintptr_t)z | (uintptr_t)dz) % 8) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    if constexpr (kBsum) {
        if (gamma) return fail(VAH_E_SHAPE, "%s: bias partials are not carried beside a layer scale (gamma)", fn);
        if (!bpart || !nparts) return fail(VAH_E_NULL, "%s: null pointer", fn);
        if ((uintptr_t)bpart % 16) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    }
    return ln_bwd_launch<T, kBsum>(fn, t, gh, w, mean, rstd, gt, batch * rows_per_batch, C,
                                   ResidualIn<T>{(const T *)z, gamma, sc, std::max<int64_t>(rows_per_batch, 1), nullptr}, dz,
                                   dt, dw, db, dgamma, ws, stream, bpart, nparts);
}

// Two LayerNorms of the same fp32 rows (shared statistics, equal eps): ya, yb of type T.
template <typename T>
int ln_dual_fwd(const char *fn, const float *x, const float *wa, const float *ba, const float *wb, const float *bb,
                int64_t rows, int64_t C, float eps, void *ya, void *yb, float *mean, float *rstd, void *stream) {
    clear_error();
    if (rows < 0 || C < 4 || C % 4 || C > 64 * 4 * 4) return fail(VAH_E_SHAPE, "%s: C=%lld unsupported", fn, (long long)C);
    if (rows == 0) return VAH_OK;
    if (!x || !wa || !ba || !wb || !bb || !ya || !yb || !mean || !rstd) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)x | (uintptr_t)wa | (uintptr_t)ba | (uintptr_t)wb | (uintptr_t)bb) % 16 || ((uintptr_t)ya | (uintptr_t)yb) % 8)
        return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope(tname<T>("layernorm_dual_fwd", "layernorm_dual_fwd_f16"), rows * C * 8, st);
#define VAH_LND_FWD(NV)                                                                                            \
    hipLaunchKernelGGL((ln_dual_fwd_kernel<T, NV>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, wa, ba, wb, bb, rows, \
                       (int)C, eps, (T *)ya, (T *)yb, mean, rstd)
    if (C <= 256) VAH_LND_FWD(1);
    else if (C <= 512) VAH_LND_FWD(2);
    else if (C <= 768) VAH_LND_FWD(3);
    else VAH_LND_FWD(4);
#undef VAH_LND_FWD
    return check_launch(fn);
}

// Backward of both: dx = gres + LN_a'(ga) + LN_b'(gb) in one pass (ga / gb / gres optional);
// dparams (4, C) = [dwa | dba | dwb | dbb].  ws: vah_reduce_ws_floats(2 * C).
template <typename T>
int ln_dual_bwd(const char *fn, const float *x, const void *ga, const void *gb, const float *wa, const float *wb,
                const float *mean, const float *rstd, const float *gres, int64_t rows, int64_t C, float *dx, float *dparams,
                float *ws, void *stream) {
    clear_error();
    if (rows < 0 || C < 4 || C % 4 || C > 64 * 4 * 4) return fail(VAH_E_SHAPE, "%s: C=%lld unsupported", fn, (long long)C);
    if (!dparams || !ws) return fail(VAH_E_NULL, "%s: null pointer", fn);
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {
        (void)hipMemsetAsync(dparams, 0, 4 * C * 4, st);
        return VAH_OK;
    }
    if (!x || !wa || !wb || !mean || !rstd || !dx) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)x | (uintptr_t)wa | (uintptr_t)wb | (uintptr_t)dx | (uintptr_t)gres) % 16 || ((uintptr_t)ga | (uintptr_t)gb) % 8)
        return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    const int64_t nblocks = std::min<int64_t>((rows + 3) / 4, kMaxParts / 2);       // the scratch holds kMaxParts * 2C floats
    const size_t smem = (size_t)4 * 4 * C * sizeof(float);
    if (smem > 64 * 1024) return fail(VAH_E_SHAPE, "%s: C too large", fn);
    LaunchScope scope(tname<T>("layernorm_dual_bwd", "layernorm_dual_bwd_f16"), rows * C * 16, st);
#define VAH_LND_BWD(NV)                                                                                              \
    hipLaunchKernelGGL((ln_dual_bwd_kernel<T, NV>), dim3((unsigned)nblocks), dim3(256), smem, st, x, (const T *)ga,   \
                       (const T *)gb, wa, wb, mean, rstd, gres, rows, (int)C, dx, ws)
    if (C <= 256) VAH_LND_BWD(1);
    else if (C <= 512) VAH_LND_BWD(2);
    else if (C <= 768) VAH_LND_BWD(3);
    else VAH_LND_BWD(4);
#undef VAH_LND_BWD
    // partial row = [dwa | dba | dwb | dbb] = the layout of dparams
    hipLaunchKernelGGL(finalize_partials, dim3((unsigned)((4 * C + 31) / 32)), dim3(256), 0, st, ws, (int)nblocks, (int)(4 * C),
                       dparams, (int)(4 * C), (float *)nullptr, 1 << 30, (float *)nullptr);
    return check_launch(fn);
}

template <typename T>
int scale_residual_fwd(const char *fn, const float *x, const void *z, const float *gamma, const float *s, int64_t batch,
                       int64_t rows_per_batch, int64_t C, float *y, void *stream) {
    clear_error();
    if (batch < 0 || rows_per_batch < 0 || C < 4 || C % 4) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    const int64_t total_vec = batch * rows_per_batch * (C / 4);
    if (total_vec == 0) return VAH_OK;
    if (!x || !z || !y) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma) % 16 || (uintptr_t)z % 8) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope(tname<T>("scale_residual_fwd", "scale_residual_fwd_f16"), total_vec * 40, st);
    hipLaunchKernelGGL(scale_residual_fwd_kernel<T>, dim3(grid_for(total_vec, 256 * 4)), dim3(256), 0, st, x,
                       (const T *)z, gamma, s, rows_per_batch, (int)C, total_vec, y);
    return check_launch(fn);
}

// dgamma (may be NULL when gamma is NULL) is overwritten; ws: vah_reduce_ws_floats(C) floats.
template <typename T>
int scale_residual_bwd(const char *fn, const float *g, const void *z, const float *gamma, const float *s, int64_t batch,
                       int64_t rows_per_batch, int64_t C, void *dz, float *dgamma, float *ws, void *stream) {
    clear_error();
    if (batch < 0 || rows_per_batch < 0 || C < 4 || C % 4) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    const int64_t rows = batch * rows_per_batch;
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {
        if (dgamma) (void)hipMemsetAsync(dgamma, 0, C * 4, st);
        return VAH_OK;
    }
    if (!g || !z || !dz || (dgamma && !ws)) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)g | (uintptr_t)gamma) % 16 || ((uintptr_t)z | (uintptr_t)dz) % 8) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    LaunchScope scope(tname<T>("scale_residual_bwd", "scale_residual_bwd_f16"), rows * C * 8, st);
    if (!gamma && batch <= 65535) {
        const int64_t vpb = rows_per_batch * C / 4;
        const unsigned gx = (unsigned)std::min<int64_t>((vpb + 1023) / 1024, 8192);
        hipLaunchKernelGGL(scale_only_bwd_kernel<T>, dim3(gx, (unsigned)batch), dim3(256), 0, st, g, s, vpb, (T *)dz);
        return check_launch(fn);
    }
    const int rpb = (int)((rows + kMaxParts - 1) / kMaxParts);
    const int64_t nblocks = (rows + rpb - 1) / rpb;
    hipLaunchKernelGGL(scale_residual_bwd_kernel<T>, dim3((unsigned)nblocks), dim3(256), 0, st, g,
                       (const T *)z, gamma, s, rows, rows_per_batch, (int)C, rpb, (T *)dz,
                       dgamma ? ws : nullptr);
    if (dgamma)
        hipLaunchKernelGGL(finalize_partials, dim3((unsigned)((C + 31) / 32)), dim3(256), 0, st, ws,
                           (int)nblocks, (int)C, dgamma, (int)C, (float *)nullptr, 1 << 30, (float *)nullptr);
    return check_launch(fn);
}

// dz = s[b] * g (no layer scale) with the column sums of the rounded dz: the flat scale_only pass has no column
// structure to carry a sum, and the row-strip kernel above (a wave per 1 KB of a row, column groups one after the
// other) streams at half its rate when there is no dgamma to reduce (measured 77 vs 35 us at 43008 x 768).  The
// tiling of colsum_bf16_kernel instead: 32 column lanes x 8 columns x 8 row lanes over a strip of rows, 4 rows
// (8 x 16 bytes of g per thread) requested before the first is used, one partial row per workgroup.
// rows_per_block % 32 == 0, so only the last strip has dead slots (clamped loads, results unused).
template <typename T>
__global__ __launch_bounds__(256) void scale_bsum_bwd_kernel(const float *__restrict__ g, const float *__restrict__ s,
                                                             unsigned rows, unsigned rows_per_batch, int C,
                                                             int rows_per_block, T *__restrict__ dz,
                                                             float *__restrict__ bpart) {
    __shared__ float s_acc[8][256 + 8];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 256 + cl * 8;
    const unsigned r0 = blockIdx.y * (unsigned)rows_per_block;
    const unsigned r1 = min(rows, r0 + (unsigned)rows_per_block);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c0 < C) {
        for (unsigned r = r0 + rl; r < r1; r += 32) {
            float4 lo[4], hi[4];
            float sb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned rr = min(r + 8 * u, r1 - 1);
                const float *gp = g + (int64_t)rr * C + c0;
                lo[u] = *reinterpret_cast<const float4 *>(gp);
                hi[u] = *reinterpret_cast<const float4 *>(gp + 4);
                sb[u] = s ? s[rr / rows_per_batch] : 1.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (r + 8 * u >= r1) break;
                vec8<T> o;
                o[0] = round16<T>(sb[u] * lo[u].x);
                o[1] = round16<T>(sb[u] * lo[u].y);
                o[2] = round16<T>(sb[u] * lo[u].z);
                o[3] = round16<T>(sb[u] * lo[u].w);
                o[4] = round16<T>(sb[u] * hi[u].x);
                o[5] = round16<T>(sb[u] * hi[u].y);
                o[6] = round16<T>(sb[u] * hi[u].z);
                o[7] = round16<T>(sb[u] * hi[u].w);
                *reinterpret_cast<vec8<T> *>(dz + (int64_t)(r + 8 * u) * C + c0) = o;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += (float)o[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s_acc[rl][cl * 8 + e] = acc[e];
    __syncthreads();
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        float t = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) t += s_acc[u][threadIdx.x];
        bpart[(int64_t)blockIdx.y * C + c] = t;
    }
}

// strips of a multiple of 32 rows (the 8 row lanes x 4 rows in flight of the column-tiled kernels), at most kMaxParts
inline void strips_of_32(int64_t rows, int64_t *rpb, int64_t *parts) {
    *rpb = std::max<int64_t>(32, ((rows + kMaxParts - 1) / kMaxParts + 31) / 32 * 32);
    *parts = (rows + *rpb - 1) / *rpb;
}

// scale_residual_bwd plus the partial rows of the column sums of dz (*nparts = the launch's workgroups along the
// rows): with a gamma the row-strip kernel with a second accumulator, without one the column-tiled kernel above
// (the strip kernel where that one does not apply: C % 8 != 0 or 2^31 rows).  bpart: vah_reduce_ws_floats(C).
template <typename T>
int scale_residual_bwd_bsum(const char *fn, const float *g, const void *z, const float *gamma, const float *s,
                                   int64_t batch, int64_t rows_per_batch, int64_t C, void *dz, float *dgamma, float *ws,
                                   float *bpart, int64_t *nparts, void *stream) {
    clear_error();
    if (batch < 0 || rows_per_batch < 0 || C < 4 || C % 4) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    if (!bpart || !nparts) return fail(VAH_E_NULL, "%s: null pointer", fn);
    const int64_t rows = batch * rows_per_batch;
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {
        if (dgamma) (void)hipMemsetAsync(dgamma, 0, C * 4, st);
        *nparts = 0;
        return VAH_OK;
    }
    if (!g || !z || !dz || (dgamma && !ws)) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)g | (uintptr_t)gamma | (uintptr_t)bpart) % 16 || ((uintptr_t)z | (uintptr_t)dz) % 8)
        return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    LaunchScope scope(tname<T>("scale_residual_bwd", "scale_residual_bwd_f16"), rows * C * 8, st);
    const bool dg = gamma && dgamma;
    if (!gamma && C % 8 == 0 && rows < ((int64_t)1 << 31)) {
        int64_t srows, parts;
        strips_of_32(rows, &srows, &parts);
        hipLaunchKernelGGL(scale_bsum_bwd_kernel<T>, dim3((unsigned)((C + 255) / 256), (unsigned)parts), dim3(256), 0, st, g, s,
                           (unsigned)rows, (unsigned)std::max<int64_t>(rows_per_batch, 1), (int)C, (int)srows, (T *)dz, bpart);
        *nparts = parts;
        return check_launch(fn);
    }
    const int rpb = (int)((rows + kMaxParts - 1) / kMaxParts);
    const int64_t nblocks = (rows + rpb - 1) / rpb;
    if (dg)
        hipLaunchKernelGGL((scale_residual_bwd_kernel<T, true, true>), dim3((unsigned)nblocks), dim3(256), 0, st, g,
                           (const T *)z, gamma, s, rows, rows_per_batch, (int)C, rpb, (T *)dz, ws, bpart);
    else
        hipLaunchKernelGGL((scale_residual_bwd_kernel<T, true, false>), dim3((unsigned)nblocks), dim3(256), 0, st, g,
                           (const T *)z, gamma, s, rows, rows_per_batch, (int)C, rpb, (T *)dz, (float *)nullptr, bpart);
    if (dg)
        hipLaunchKernelGGL(finalize_partials, dim3((unsigned)((C + 31) / 32)), dim3(256), 0, st, ws,
                           (int)nblocks, (int)C, dgamma, (int)C, (float *)nullptr, 1 << 30, (float *)nullptr);
    *nparts = nblocks;
    return check_launch(fn);
}

// ---------------------------------------------------------------------------------------
// GELU backward (exact, erf) of a 16-bit (T: bf16 or fp16) [rows, C] matrix with the column sums of its result: the gradient of
// trunk mlp.fc1's output.  dh = T(da * (Phi(h) + h * phi(h))), fp32 math from the 16-bit operands in the
// operation order of torch's GeluBackward kernel (so the two agree to the bit wherever erff / expf do).
// The tiling of colsum_bf16_kernel: 32 column lanes x 8 bf16 x 8 row lanes over a strip of rows; the loads of
// 4 rows are requested before the math of the first.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void gelu_bwd_bsum_kernel(const T *__restrict__ da, const T *__restrict__ h,
                                                            int64_t rows, int C, int rows_per_block,
                                                            T *__restrict__ dh, float *__restrict__ part) {
    __shared__ float s_acc[8][256 + 8];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 256 + cl * 8;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = min(rows, r0 + rows_per_block);
    constexpr float kAlpha = (float)0.70710678118654752440;                              // sqrt(1/2)
    constexpr float kBeta = (float)(1.12837916709551257390 * 0.70710678118654752440 * 0.5);   // 1 / sqrt(2 pi)
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c0 < C) {
        for (int64_t r = r0 + rl; r < r1; r += 32) {
            vec8<T> av[4], hv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t rr = min(r + 8 * u, r1 - 1);          // clamped: a dead slot re-reads a live row
                av[u] = *reinterpret_cast<const vec8<T> *>(da + rr * C + c0);
                hv[u] = *reinterpret_cast<const vec8<T> *>(h + rr * C + c0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (r + 8 * u >= r1) break;
                vec8<T> o;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float x = (float)hv[u][e];
                    const float cdf = 0.5f * (1.f + erff(x * kAlpha));
                    const float pdf = expf(-0.5f * x * x) * kBeta;
                    o[e] = round16<T>((float)av[u][e] * (cdf + x * pdf));
                    acc[e] += (float)o[e];
                }
                *reinterpret_cast<vec8<T> *>(dh + (r + 8 * u) * C + c0) = o;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s_acc[rl][cl * 8 + e] = acc[e];
    __syncthreads();
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        float t = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) t += s_acc[u][threadIdx.x];
        part[(int64_t)blockIdx.y * C + c] = t;
    }
}

template <typename T>
int gelu_bwd_bsum(const char *fn, const void *da, const void *h, int64_t rows, int64_t C, void *dh, float *bpart,
                  int64_t *nparts, void *stream) {
    clear_error();
    if (rows < 0 || C < 8 || C % 8 || C > (1 << 20)) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    if (!bpart || !nparts) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (rows == 0) {
        *nparts = 0;
        return VAH_OK;
    }
    if (!da || !h || !dh) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)da | (uintptr_t)h | (uintptr_t)dh) % 16) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    const int ctiles = (int)((C + 255) / 256);
    // colsum_bf16's tiling, not its strip rule: that one sizes strips to 2048 workgroups whatever the row count
    // (8192 x 3072: 49 rows, 6.1 per row lane = a second, ragged batch of loads), which costs a kernel with this
    // much math per element a quarter of its rate; strips of 32 rows are whole batches
    int64_t parts, rpb;
    strips_of_32(rows, &rpb, &parts);
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope(tname<T>("gelu_bwd", "gelu_bwd_f16"), rows * C * 6, st);
    hipLaunchKernelGGL(gelu_bwd_bsum_kernel<T>, dim3((unsigned)ctiles, (unsigned)parts), dim3(256), 0, st, (const T *)da,
                       (const T *)h, rows, (int)C, (int)rpb, (T *)dh, bpart);
    *nparts = parts;
    return check_launch(fn);
}

template <typename T>
int colsum16_partials(const char *fn, const void *g, int64_t rows, int64_t C, float *ws, int64_t *nparts, void *stream) {
    clear_error();
    if (rows < 1 || C < 8 || C % 8 || C > (1 << 20)) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    if (!g || !ws || !nparts) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if ((uintptr_t)g % 16) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    const int ctiles = (int)((C + 255) / 256);
    // enough strips to fill the chip, at least 32 rows each, at most kMaxParts partial rows
    int64_t parts = std::min<int64_t>(kMaxParts, std::max<int64_t>(1, 2048 / ctiles));
    int64_t rpb = std::max<int64_t>(32, (rows + parts - 1) / parts);
    parts = (rows + rpb - 1) / rpb;
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope(tname<T>("colsum_bf16", "colsum_f16"), rows * C * 2, st);
    hipLaunchKernelGGL(colsum_bf16_kernel<T>, dim3((unsigned)ctiles, (unsigned)parts), dim3(256), 0, st, (const T *)g, rows,
                       (int)C, (int)rpb, ws);
    *nparts = parts;
    return check_launch(fn);
}

// fn_partials: the name the partials entry point reports its own refusals under
template <typename T>
int colsum16(const char *fn, const char *fn_partials, const void *g, int64_t rows, int64_t C, float *out, float *ws,
             void *stream) {
    clear_error();
    if (rows < 0 || C < 8 || C % 8 || C > (1 << 20)) return fail(VAH_E_SHAPE, "%s: C=%lld unsupported", fn, (long long)C);
    if (!out || !ws) return fail(VAH_E_NULL, "%s: null pointer", fn);
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {
        (void)hipMemsetAsync(out, 0, C * 4, st);
        return VAH_OK;
    }
    int64_t parts = 0;
    if (int rc = colsum16_partials<T>(fn_partials, g, rows, C, ws, &parts, stream)) return rc;
    hipLaunchKernelGGL(finalize_partials, dim3((unsigned)((C + 31) / 32)), dim3(256), 0, st, ws, (int)parts,
                       (int)C, out, (int)C, (float *)nullptr, 1 << 30, (float *)nullptr);
    return check_launch(fn);
}

// token ranges and sizes of the (2H,2W), (H,W), (H/2,W/2) maps of a (B, 21n, C) token tensor
inline Maps maps_of(int64_t H, int64_t W) {
    const int64_t n = (H / 2) * (W / 2);
    Maps mp;
    mp.t[0] = 0, mp.t[1] = (int)(16 * n), mp.t[2] = (int)(20 * n), mp.t[3] = (int)(21 * n);
    mp.h[0] = (int)(2 * H), mp.w[0] = (int)(2 * W), mp.h[1] = (int)H, mp.w[1] = (int)W;
    mp.h[2] = (int)(H / 2), mp.w[2] = (int)(W / 2);
    return mp;
}

// x, y: T (B, N, C) with N = 16n + 4n + n tokens of maps (2H,2W), (H,W), (H/2,W/2); w fp32 (C,1,3,3).
// mode 0: forward (+bias); mode 1: input gradient (x = grad_out, flipped taps, bias ignored).
template <typename T>
int dwconv_tokens(const char *fn, const void *x, const float *w, const float *bias, int64_t B, int64_t H, int64_t W,
                  int64_t C, int mode, void *y, void *stream) {
    clear_error();
    if (B < 0 || H < 2 || W < 2 || (H % 2) || (W % 2) || C < 4 || C % 4 || C > 1024) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    if (B == 0) return VAH_OK;
    if (!x || !w || !y) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)x | (uintptr_t)y) % 8 || (uintptr_t)bias % 16) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    const Maps mp = maps_of(H, W);
    const int N = mp.t[3];
    const int64_t total_tok = B * N;
    if (total_tok >= ((int64_t)1 << 31)) return fail(VAH_E_SHAPE, "%s: too many tokens", fn);
    const int slots = 256 / (int)(C / 4);
    const int items_per_img = dw_items_per_image(mp, kDwRows);
    const int total_items = (int)(B * items_per_img);                  // at most one item per token
    const dim3 grid((unsigned)((total_items + slots - 1) / slots));
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope(mode == 0 ? tname<T>("dwconv_tokens_fwd", "dwconv_tokens_fwd_f16")
                                : tname<T>("dwconv_tokens_dgrad", "dwconv_tokens_dgrad_f16"),
                      total_tok * C * 4, st);
    if (mode == 0)
        hipLaunchKernelGGL((dwconv_kernel<T, 0>), grid, dim3(256), 0, st,
                           (const T *)x, w, bias, mp, N, (int)C, items_per_img, total_items, (T *)y);
    else
        hipLaunchKernelGGL((dwconv_kernel<T, 1>), grid, dim3(256), 0, st,
                           (const T *)x, w, bias, mp, N, (int)C, items_per_img, total_items, (T *)y);
    return check_launch(fn);
}

// dw (C*9) and db (C, may be NULL) are overwritten; ws: vah_reduce_ws_floats(10*C) floats.
template <typename T>
int dwconv_tokens_wgrad(const char *fn, const void *x, const void *g, int64_t B, int64_t H, int64_t W, int64_t C, float *dw,
                        float *db, float *ws, void *stream) {
    clear_error();
    if (B < 0 || H < 2 || W < 2 || (H % 2) || (W % 2) || C < 4 || C % 4 || C > 1024) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    if (!dw || !ws) return fail(VAH_E_NULL, "%s: null pointer", fn);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        (void)hipMemsetAsync(dw, 0, C * 9 * 4, st);
        if (db) (void)hipMemsetAsync(db, 0, C * 4, st);
        return VAH_OK;
    }
    if (!x || !g) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)x | (uintptr_t)g) % 8) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    const Maps mp = maps_of(H, W);
    const int N = mp.t[3];
    const int64_t total_tok = B * N;
    if (total_tok >= ((int64_t)1 << 31)) return fail(VAH_E_SHAPE, "%s: too many tokens", fn);
    const int slots = 256 / (int)(C / 4);
    const int items_per_img = dw_items_per_image(mp, kDwRowsWgrad);
    const int total_items = (int)(B * items_per_img);                  // at most one item per token
    int64_t nblocks = (total_items + slots - 1) / slots;
    if (nblocks > kMaxParts) nblocks = kMaxParts;
    if (nblocks < 1) nblocks = 1;
    const size_t smem = (size_t)slots * C * 10 * sizeof(float);
    if (smem > 150 * 1024) return fail(VAH_E_SHAPE, "%s: C too small for the LDS reduction layout", fn);
    if (int rc = allow_dynamic_lds((const void *)dwconv_wgrad_kernel<T>, 160 * 1024 - 512, fn)) return rc;
    LaunchScope scope(tname<T>("dwconv_tokens_wgrad", "dwconv_tokens_wgrad_f16"), total_tok * C * 4, st);
    hipLaunchKernelGGL(dwconv_wgrad_kernel<T>, dim3((unsigned)nblocks), dim3(256), smem, st,
                       (const T *)x, (const T *)g, mp, N, (int)C, items_per_img, total_items, ws);
    hipLaunchKernelGGL(finalize_partials, dim3((unsigned)((10 * C + 31) / 32)), dim3(256), 0, st, ws,
                       (int)nblocks, (int)(10 * C), dw, (int)(9 * C), db, 1 << 30, (float *)nullptr);
    return check_launch(fn);
}

}  // namespace
}  // namespace vah

extern "C" {

int64_t vah_reduce_ws_floats(int64_t K) { return (int64_t)vah::kMaxParts * K; }

// Every entry point below exists once per 16-bit element type: the bf16 name and its fp16 twin (`_f16`) are the
// same template above with another T, so their checks, codes and messages cannot drift apart.
#define VAH_ENTRY_PAIR(M, BF16_NAME, F16_NAME) M(BF16_NAME, __bf16) M(F16_NAME, _Float16)

#define VAH_LN_FWD_ENTRY(NAME, T)                                                                                       \
    int NAME(const float *x, const float *w, const float *b, int64_t rows, int64_t C, float eps, void *y, float *mean,  \
             float *rstd, void *stream) {                                                                               \
        return vah::ln_fwd_launch<T>(#NAME, x, w, b, rows, C, eps, vah::ResidualIn<T>{nullptr, nullptr, nullptr, 1, nullptr}, \
                                     y, mean, rstd, stream);                                                            \
    }
VAH_ENTRY_PAIR(VAH_LN_FWD_ENTRY, vah_layernorm_fwd_f32_bf16, vah_layernorm_fwd_f32_f16)

// ws: vah_reduce_ws_floats(2*C) floats of scratch.  dw, db are overwritten.
#define VAH_LN_BWD_ENTRY(NAME, T)                                                                                       \
    int NAME(const float *x, const void *g, const float *w, const float *mean, const float *rstd, const float *gres,    \
             int64_t rows, int64_t C, float *dx, float *dw, float *db, float *ws, void *stream) {                       \
        return vah::ln_bwd_launch<T>(#NAME, x, g, w, mean, rstd, gres, rows, C,                                         \
                                     vah::ResidualIn<T>{nullptr, nullptr, nullptr, 1, nullptr}, nullptr, dx, dw, db,    \
                                     nullptr, ws, stream);                                                              \
    }
VAH_ENTRY_PAIR(VAH_LN_BWD_ENTRY, vah_layernorm_bwd_f32_bf16, vah_layernorm_bwd_f32_f16)

#define VAH_RES_LN_FWD_ENTRY(NAME, T)                                                                                   \
    int NAME(const float *x, const void *z, const float *gamma, const float *sc, int64_t batch, int64_t rows_per_batch, \
             int64_t C, const float *w, const float *b, float eps, float *t, void *h, float *mean, float *rstd,         \
             void *stream) {                                                                                            \
        return vah::residual_ln_fwd<T>(#NAME, x, z, gamma, sc, batch, rows_per_batch, C, w, b, eps, t, h, mean, rstd,   \
                                       stream);                                                                         \
    }
VAH_ENTRY_PAIR(VAH_RES_LN_FWD_ENTRY, vah_residual_layernorm_fwd, vah_residual_layernorm_fwd_f16)

#define VAH_RES_LN_BWD_ENTRY(NAME, T)                                                                                   \
    int NAME(const float *t, const void *gh, const float *w, const float *mean, const float *rstd, const float *gt,     \
             const void *z, const float *gamma, const float *sc, int64_t batch, int64_t rows_per_batch, int64_t C,      \
             float *dt, void *dz, float *dgamma, float *dw, float *db, float *ws, void *stream) {                       \
        return vah::residual_ln_bwd<T>(#NAME, t, gh, w, mean, rstd, gt, z, gamma, sc, batch, rows_per_batch, C, dt, dz, \
                                       dgamma, dw, db, ws, stream);                                                     \
    }
VAH_ENTRY_PAIR(VAH_RES_LN_BWD_ENTRY, vah_residual_layernorm_bwd, vah_residual_layernorm_bwd_f16)

#define VAH_LN_DUAL_FWD_ENTRY(NAME, T)                                                                                  \
    int NAME(const float *x, const float *wa, const float *ba, const float *wb, const float *bb, int64_t rows,          \
             int64_t C, float eps, void *ya, void *yb, float *mean, float *rstd, void *stream) {                        \
        return vah::ln_dual_fwd<T>(#NAME, x, wa, ba, wb, bb, rows, C, eps, ya, yb, mean, rstd, stream);                 \
    }
VAH_ENTRY_PAIR(VAH_LN_DUAL_FWD_ENTRY, vah_layernorm_dual_fwd, vah_layernorm_dual_fwd_f16)

#define VAH_LN_DUAL_BWD_ENTRY(NAME, T)                                                                                  \
    int NAME(const float *x, const void *ga, const void *gb, const float *wa, const float *wb, const float *mean,       \
             const float *rstd, const float *gres, int64_t rows, int64_t C, float *dx, float *dparams, float *ws,       \
             void *stream) {                                                                                            \
        return vah::ln_dual_bwd<T>(#NAME, x, ga, gb, wa, wb, mean, rstd, gres, rows, C, dx, dparams, ws, stream);       \
    }
VAH_ENTRY_PAIR(VAH_LN_DUAL_BWD_ENTRY, vah_layernorm_dual_bwd, vah_layernorm_dual_bwd_f16)

#define VAH_SCALE_RES_FWD_ENTRY(NAME, T)                                                                                \
    int NAME(const float *x, const void *z, const float *gamma, const float *s, int64_t batch, int64_t rows_per_batch,  \
             int64_t C, float *y, void *stream) {                                                                       \
        return vah::scale_residual_fwd<T>(#NAME, x, z, gamma, s, batch, rows_per_batch, C, y, stream);                  \
    }
VAH_ENTRY_PAIR(VAH_SCALE_RES_FWD_ENTRY, vah_scale_residual_fwd, vah_scale_residual_fwd_f16)

#define VAH_SCALE_RES_BWD_ENTRY(NAME, T)                                                                                \
    int NAME(const float *g, const void *z, const float *gamma, const float *s, int64_t batch, int64_t rows_per_batch,  \
             int64_t C, void *dz, float *dgamma, float *ws, void *stream) {                                             \
        return vah::scale_residual_bwd<T>(#NAME, g, z, gamma, s, batch, rows_per_batch, C, dz, dgamma, ws, stream);     \
    }
VAH_ENTRY_PAIR(VAH_SCALE_RES_BWD_ENTRY, vah_scale_residual_bwd, vah_scale_residual_bwd_f16)

#define VAH_DWCONV_ENTRY(NAME, T)                                                                                       \
    int NAME(const void *x, const float *w, const float *bias, int64_t B, int64_t H, int64_t W, int64_t C, int mode,    \
             void *y, void *stream) {                                                                                   \
        return vah::dwconv_tokens<T>(#NAME, x, w, bias, B, H, W, C, mode, y, stream);                                   \
    }
VAH_ENTRY_PAIR(VAH_DWCONV_ENTRY, vah_dwconv3x3_tokens_bf16, vah_dwconv3x3_tokens_f16)

#define VAH_DWCONV_WGRAD_ENTRY(NAME, T)                                                                                 \
    int NAME(const void *x, const void *g, int64_t B, int64_t H, int64_t W, int64_t C, float *dw, float *db, float *ws, \
             void *stream) {                                                                                            \
        return vah::dwconv_tokens_wgrad<T>(#NAME, x, g, B, H, W, C, dw, db, ws, stream);                                \
    }
VAH_ENTRY_PAIR(VAH_DWCONV_WGRAD_ENTRY, vah_dwconv3x3_tokens_wgrad_bf16, vah_dwconv3x3_tokens_wgrad_f16)

// The row-streaming backward kernels that write the dY of a Linear, carrying the partial rows of dY's column sums
// (that Linear's bias gradient) in the same pass: bpart (caller-owned, vah_reduce_ws_floats(C) floats) gets *nparts
// <= 512 rows of C floats, for the finalize job of vah_gemm_bf16_fin / vah_gemm_f16_fin.  Summed is every dY element
// after its rounding to the 16-bit type - the term vah_colsum_bf16_partials / _f16_partials adds.  Every other output is
// that of the entry point without _bsum.
#define VAH_RES_LN_BWD_BSUM_ENTRY(NAME, T)                                                                              \
    int NAME(const float *t, const void *gh, const float *w, const float *mean, const float *rstd, const float *gt,     \
             const void *z, const float *gamma, const float *sc, int64_t batch, int64_t rows_per_batch, int64_t C,      \
             float *dt, void *dz, float *dgamma, float *dw, float *db, float *ws, float *bpart, int64_t *nparts,        \
             void *stream) {                                                                                            \
        return vah::residual_ln_bwd<T, true>(#NAME, t, gh, w, mean, rstd, gt, z, gamma, sc, batch, rows_per_batch, C,   \
                                             dt, dz, dgamma, dw, db, ws, stream, bpart, nparts);                        \
    }
VAH_ENTRY_PAIR(VAH_RES_LN_BWD_BSUM_ENTRY, vah_residual_layernorm_bwd_bsum, vah_residual_layernorm_bwd_f16_bsum)

#define VAH_SCALE_RES_BWD_BSUM_ENTRY(NAME, T)                                                                           \
    int NAME(const float *g, const void *z, const float *gamma, const float *s, int64_t batch, int64_t rows_per_batch,  \
             int64_t C, void *dz, float *dgamma, float *ws, float *bpart, int64_t *nparts, void *stream) {              \
        return vah::scale_residual_bwd_bsum<T>(#NAME, g, z, gamma, s, batch, rows_per_batch, C, dz, dgamma, ws, bpart,  \
                                               nparts, stream);                                                         \
    }
VAH_ENTRY_PAIR(VAH_SCALE_RES_BWD_BSUM_ENTRY, vah_scale_residual_bwd_bsum, vah_scale_residual_bwd_f16_bsum)

#define VAH_GELU_BWD_BSUM_ENTRY(NAME, T)                                                                                \
    int NAME(const void *da, const void *h, int64_t rows, int64_t C, void *dh, float *bpart, int64_t *nparts,           \
             void *stream) {                                                                                            \
        return vah::gelu_bwd_bsum<T>(#NAME, da, h, rows, C, dh, bpart, nparts, stream);                                 \
    }
VAH_ENTRY_PAIR(VAH_GELU_BWD_BSUM_ENTRY, vah_gelu_bwd_bsum_bf16, vah_gelu_bwd_bsum_f16)

// Partial rows of the column sums of a 16-bit [rows, C] matrix, C % 8 == 0: ws (vah_reduce_ws_floats(C)) gets
// *nparts rows of C floats; whoever sums them (vah_colsum_bf16 / _f16 below, or the finalize job of
// vah_gemm_bf16_fin / vah_gemm_f16_fin) has the column sums.  rows >= 1.
#define VAH_COLSUM_PARTIALS_ENTRY(NAME, T)                                                                              \
    int NAME(const void *g, int64_t rows, int64_t C, float *ws, int64_t *nparts, void *stream) {                        \
        return vah::colsum16_partials<T>(#NAME, g, rows, C, ws, nparts, stream);                                        \
    }
VAH_ENTRY_PAIR(VAH_COLSUM_PARTIALS_ENTRY, vah_colsum_bf16_partials, vah_colsum_f16_partials)

// out[c] = sum_r g[r][c] for a 16-bit [rows, C] matrix, C % 8 == 0; ws: vah_reduce_ws_floats(C).
#define VAH_COLSUM_ENTRY(NAME, T)                                                                                       \
    int NAME(const void *g, int64_t rows, int64_t C, float *out, float *ws, void *stream) {                             \
        return vah::colsum16<T>(#NAME, #NAME "_partials", g, rows, C, out, ws, stream);                                 \
    }
VAH_ENTRY_PAIR(VAH_COLSUM_ENTRY, vah_colsum_bf16, vah_colsum_f16)

#undef VAH_ENTRY_PAIR

// out[c] = sum over b < batch, r < rows of g[b * batch_stride + r * C + c]  (fp32, C % 4 == 0): column sums
// of a token range of a (B, T, C) tensor - the gradient of a per-channel vector added to that range.
// ws: vah_reduce_ws_floats(C).
int vah_colsum_f32(const float *g, int64_t batch, int64_t batch_stride, int64_t rows, int64_t C, float *out,
                   float *ws, void *stream) {
    using namespace vah;
    clear_error();
    const char *fn = "vah_colsum_f32";
    if (batch < 0 || rows < 0 || C < 4 || C % 4 || C > (1 << 20) || batch > 65535) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    if (!out || !ws) return fail(VAH_E_NULL, "%s: null pointer", fn);
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0 || batch == 0) {
        (void)hipMemsetAsync(out, 0, C * 4, st);
        return VAH_OK;
    }
    if (!g) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if ((uintptr_t)g % 16 || batch_stride % 4) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    const int ctiles = (int)((C + 127) / 128);
    int64_t parts = std::min<int64_t>(kMaxParts / batch, std::max<int64_t>(1, 2048 / (ctiles * batch)));
    parts = std::max<int64_t>(parts, 1);
    if (parts * batch > kMaxParts) return fail(VAH_E_SHAPE, "%s: batch too large", fn);
    int64_t rpb = std::max<int64_t>(32, (rows + parts - 1) / parts);
    parts = (rows + rpb - 1) / rpb;
    LaunchScope scope("colsum_f32", batch * rows * C * 4, st);
    hipLaunchKernelGGL(colsum_f32_kernel, dim3((unsigned)ctiles, (unsigned)parts, (unsigned)batch), dim3(256), 0, st, g, rows,
                       (int)C, batch_stride, (int)rpb, ws);
    hipLaunchKernelGGL(finalize_partials, dim3((unsigned)((C + 31) / 32)), dim3(256), 0, st, ws, (int)(parts * batch),
                       (int)C, out, (int)C, (float *)nullptr, 1 << 30, (float *)nullptr);
    return check_launch(fn);
}

}  // extern "C"
