// Output tail of the adapter backbone:  f = BatchNorm(a + b + upsample_s(x)).
//
// Reference: vit_adapter.py:106-127 (seg) / :101-120 (det)
//     c1 = up(c2) + c1;  c1 = c1 + F.interpolate(x1, scale_factor=4, mode='bilinear');  f1 = norm1(c1)
//     c2 = c2 + F.interpolate(x2, scale_factor=2, ...);  f2 = norm2(c2);  c3 = c3 + x3;  f3 = norm3(c3)
// At 1024^2 the stride-4 map is 2 x 768 x 256 x 256 = 100 M elements; as separate ops (interpolate,
// two adds, BN statistics, BN normalise) it is written or read ~10 times in fp32 (3.8 GB forward).
// Here the sum is never materialised: the statistics pass and the normalise pass both recompute
// a + b + bilinear(x) from the (bf16) operands, so the forward moves 2 reads of the operands plus
// one fp32 write, and the backward likewise.  HBM-bound; no LDS except the adjoint of the upsample.
//
// Layout: NCHW planes.  a: bf16 or fp32 (N, C, H, W); b: optional, bf16 or fp32, same shape;
// x: optional fp32 (N, C, H / s, W / s), s in {1, 2, 4, 8} (s = 1: plain add).  W % 4 == 0.
// Bilinear taps follow torch's upsample_bilinear2d with align_corners = False and an explicit
// scale factor:  src = (dst + 0.5) / s - 0.5, clamped at 0;  i1 = min(i0 + 1, n - 1).
//
// Every kernel that touches a 16-bit operand is a template on its element type T (__bf16, or _Float16 for the `_f16`
// entry points).  T appears in loads, stores and converts only: 16-bit -> fp32 is exact (fp16 subnormals included) and
// fp32 -> 16-bit is the plain (T)f cast (round to nearest even; fp16 overflows to inf and keeps subnormals, as
// torch.Tensor.to(torch.float16) does).  Arithmetic, statistics, partial rows, dxlo and the workspaces are fp32 for
// both.  The runtime `*_bf16` flags keep their meaning "16-bit (of type T) or fp32".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/vitadapter_hip.h"
#include "../../include/vitadapter_hip_epoch.h"
#include "common.h"
#include "elem16.h"

namespace vah {
namespace {

constexpr int kTilePx = 8192;           // hi-res pixels of one plane per workgroup
constexpr int kTailParts = 512;         // partial rows of the channel sums (finalised below)

struct Operands {
    const void *a, *b;
    const float *x;
    int a_bf16, b_bf16, scale;
    int C, H, W, Hl, Wl;
    int rows_per_block, chunks;         // chunks of rows per plane
    int relu, y_bf16, dy_bf16;          // ReLU fused behind the normalisation; dtypes of y and dy
    const float *shift;                 // optional per-channel constant added to the sum (conv biases)
    unsigned quad_magic;                // floor(2^32 / (W / 4)) + 1: item -> (row, quad) by one v_mul_hi (items < 2^16)
    unsigned oct_magic, lo_magic;       // the same for W / 8 (8-pixel items) and for Wl (the adjoint's passes): fixed forms
};

struct Tap {
    int i0, i1;
    float w1;
};

// scale = 2^k (host-checked): src = (2d + 1 - s) / 2s exactly, so floor and fraction are integer ops;
// same values as the float form  src = (d + 0.5) / s - 0.5, clamped at 0  (both are exact in fp32).
__device__ __forceinline__ Tap tap_of(int d, int n_lo, int s) {
    const int sh1 = 32 - __builtin_clz((unsigned)s);            // log2(2s)
    const int n = max(2 * d + 1 - s, 0);
    Tap t;
    t.i0 = min(n >> sh1, n_lo - 1);
    t.i1 = min(t.i0 + 1, n_lo - 1);
    t.w1 = (float)(n & (2 * s - 1)) * (0.5f / (float)s);
    return t;
}

// Raw 4-element load (4 fp32 or 4 16-bit values, dtype uniform) and its decode, kept apart so that a kernel can
// request all of its operands before it touches the first: with the conversion next to the load
// every operand sat in its own uniform branch with its own s_waitcnt vmcnt(0).
struct Raw4 {
    uint32_t w0, w1, w2, w3;
};

__device__ __forceinline__ Raw4 load_raw(const void *p, int64_t idx, int is_bf16) {
    Raw4 r;
    r.w0 = r.w1 = r.w2 = r.w3 = 0u;
    if (is_bf16) {
        const uint2 v = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint16_t *>(p) + idx);
        r.w0 = v.x;
        r.w1 = v.y;
    } else {
        const uint4 v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const float *>(p) + idx);
        r.w0 = v.x;
        r.w1 = v.y;
        r.w2 = v.z;
        r.w3 = v.w;
    }
    return r;
}

// The four 16-bit values of (w0, w1) as fp32: bf16 is the upper half of an fp32 word; fp16 takes v_cvt_f32_f16
// (exact, subnormals included).
template <typename T>
__device__ __forceinline__ float4 widen4(uint32_t w0, uint32_t w1);
template <>
__device__ __forceinline__ float4 widen4<__bf16>(uint32_t w0, uint32_t w1) {
    return make_float4(__uint_as_float(w0 << 16), __uint_as_float(w0 & 0xffff0000u), __uint_as_float(w1 << 16),
                       __uint_as_float(w1 & 0xffff0000u));
}
template <>
__device__ __forceinline__ float4 widen4<_Float16>(uint32_t w0, uint32_t w1) {
    const f16x2 lo = __builtin_bit_cast(f16x2, w0), hi = __builtin_bit_cast(f16x2, w1);
    return make_float4((float)lo[0], (float)lo[1], (float)hi[0], (float)hi[1]);
}

template <typename T>
__device__ __forceinline__ float4 decode(const Raw4 &r, int is_bf16) {
    const float4 h = widen4<T>(r.w0, r.w1);
    const float4 f = make_float4(__uint_as_float(r.w0), __uint_as_float(r.w1), __uint_as_float(r.w2),
                                 __uint_as_float(r.w3));
    return is_bf16 ? h : f;
}

template <typename T>
__device__ __forceinline__ void store4(void *p, int64_t idx, int is_bf16, float4 v) {
    if (is_bf16) {
        vec4<T> o;
        o[0] = (T)v.x;
        o[1] = (T)v.y;
        o[2] = (T)v.z;
        o[3] = (T)v.w;
        *reinterpret_cast<vec4<T> *>(reinterpret_cast<T *>(p) + idx) = o;
    } else {
        *reinterpret_cast<float4 *>(reinterpret_cast<float *>(p) + idx) = v;
    }
}

// t = a + b + up(x) for 4 consecutive pixels (row y, columns x4 .. x4 + 3) of plane `plane`.
// Every load (a, b, the 8 low-res values, and the caller's dy when `dy` is given) is requested before the
// first is decoded.
template <typename T>
__device__ __forceinline__ float4 sum4(const Operands &o, int64_t plane, int y, int x4, const void *dy = nullptr,
                                       Raw4 *dy_raw = nullptr) {
    const int64_t idx = (plane * o.H + y) * o.W + x4;
    const Raw4 ra = load_raw(o.a, idx, o.a_bf16);
    Raw4 rb;
    rb.w0 = rb.w1 = rb.w2 = rb.w3 = 0u;
    if (o.b) rb = load_raw(o.b, idx, o.b_bf16);
    if (dy) *dy_raw = load_raw(dy, idx, o.dy_bf16);
    float sft = 0.f;
    if (o.shift) sft = o.shift[plane % o.C];
    float4 xs = make_float4(0.f, 0.f, 0.f, 0.f);          // scale 1: the low-res row itself
    float c0[4] = {0.f, 0.f, 0.f, 0.f}, c1[4] = {0.f, 0.f, 0.f, 0.f};
    Tap ty;
    ty.i0 = ty.i1 = 0;
    ty.w1 = 0.f;
    int nx0 = 0, bcol = 0;
    const int sc = o.scale, sh1 = 32 - __builtin_clz((unsigned)sc), mask = 2 * sc - 1;
    if (o.x) {
        const float *xp = o.x + plane * o.Hl * o.Wl;
        if (sc == 1) {
            xs = *reinterpret_cast<const float4 *>(xp + (int64_t)y * o.Wl + x4);
        } else {
            // 4 consecutive pixels starting at a multiple of 4 read at most 4 consecutive low-res columns
            // (b .. b + 3, b = floor of the first pixel's source position): 8 loads instead of 16, the
            // pixel's pair picked with selects.  Index clamping at the borders gives what the clamped
            // source position gives: both taps on the same column, r + w * (r - r) = r.
            ty = tap_of(y, o.Hl, sc);
            const float *r0 = xp + (int64_t)ty.i0 * o.Wl, *r1 = xp + (int64_t)ty.i1 * o.Wl;
            nx0 = 2 * x4 + 1 - sc;
            bcol = nx0 >> sh1;                               // arithmetic shift: floor, >= -1
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cj = min(max(bcol + j, 0), o.Wl - 1);
                c0[j] = r0[cj];
                c1[j] = r1[cj];
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);                       // loads above, arithmetic below
    float4 t = decode<T>(ra, o.a_bf16);
    const float4 vb = decode<T>(rb, o.b_bf16);
    t.x += sft + vb.x;
    t.y += sft + vb.y;
    t.z += sft + vb.z;
    t.w += sft + vb.w;
    if (o.x) {
        if (sc == 1) {
            t.x += xs.x;
            t.y += xs.y;
            t.z += xs.z;
            t.w += xs.w;
        } else {
            float u[4];
            // The four pixels start at a multiple of 4, so for s = 2 and s = 4 which low-res column pair a pixel reads and
            // with which weight is the same for every quad: constants instead of shifts, masks and 16 selects per quad
            // (this pass is VALU-bound: the statistics pass over the stride-4 level took as long as the normalise pass,
            // which also WRITES 403 MB).  Other scales take the general form.
            if (sc == 4) {                  // columns b, b, b + 1, b + 1 of (c[0..2]); weights 5/8, 7/8, 1/8, 3/8
                const float t0 = c0[0] + 0.625f * (c0[1] - c0[0]), b0 = c1[0] + 0.625f * (c1[1] - c1[0]);
                const float t1 = c0[0] + 0.875f * (c0[1] - c0[0]), b1 = c1[0] + 0.875f * (c1[1] - c1[0]);
                const float t2 = c0[1] + 0.125f * (c0[2] - c0[1]), b2 = c1[1] + 0.125f * (c1[2] - c1[1]);
                const float t3 = c0[1] + 0.375f * (c0[2] - c0[1]), b3 = c1[1] + 0.375f * (c1[2] - c1[1]);
                u[0] = t0 + ty.w1 * (b0 - t0);
                u[1] = t1 + ty.w1 * (b1 - t1);
                u[2] = t2 + ty.w1 * (b2 - t2);
                u[3] = t3 + ty.w1 * (b3 - t3);
            } else if (sc == 2) {           // columns b, b + 1, b + 1, b + 2; weights 3/4, 1/4, 3/4, 1/4
                const float t0 = c0[0] + 0.75f * (c0[1] - c0[0]), b0 = c1[0] + 0.75f * (c1[1] - c1[0]);
                const float t1 = c0[1] + 0.25f * (c0[2] - c0[1]), b1 = c1[1] + 0.25f * (c1[2] - c1[1]);
                const float t2 = c0[1] + 0.75f * (c0[2] - c0[1]), b2 = c1[1] + 0.75f * (c1[2] - c1[1]);
                const float t3 = c0[2] + 0.25f * (c0[3] - c0[2]), b3 = c1[2] + 0.25f * (c1[3] - c1[2]);
                u[0] = t0 + ty.w1 * (b0 - t0);
                u[1] = t1 + ty.w1 * (b1 - t1);
                u[2] = t2 + ty.w1 * (b2 - t2);
                u[3] = t3 + ty.w1 * (b3 - t3);
            } else {
                const float inv2s = 0.5f / (float)sc;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int nk = nx0 + 2 * k, ik = (nk >> sh1) - bcol;      // 0, 1 or 2
                    const float w1 = (float)(nk & mask) * inv2s;
                    const float a0 = ik == 0 ? c0[0] : (ik == 1 ? c0[1] : c0[2]);
                    const float a1 = ik == 0 ? c0[1] : (ik == 1 ? c0[2] : c0[3]);
                    const float b0 = ik == 0 ? c1[0] : (ik == 1 ? c1[1] : c1[2]);
                    const float b1 = ik == 0 ? c1[1] : (ik == 1 ? c1[2] : c1[3]);
                    const float top = a0 + w1 * (a1 - a0);
                    const float bot = b0 + w1 * (b1 - b0);
                    u[k] = top + ty.w1 * (bot - top);
                }
            }
            t.x += u[0];
            t.y += u[1];
            t.z += u[2];
            t.w += u[3];
        }
    }
    return t;
}

__device__ __forceinline__ float block_sum(float v, float *s_red) {      // 256 threads
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) s_red[wv] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

__device__ __forceinline__ float nanmax(float a, float b) { return __builtin_elementwise_maximum(a, b); }

// part[(n * chunks + chunk)][2C]: (sum t | sum t^2) of the block's pixels, for its channel only.  The C planes of
// one (n, chunk) between them write every column of its row and tail_finalize reads the N * chunks (<= kTailParts)
// rows that were written and no other, so the partial buffer needs no initialisation.
template <typename T>
__global__ __launch_bounds__(256) void tail_stats_kernel(Operands o, float *__restrict__ part) {
    __shared__ float s_red[4];
    const int64_t plane = blockIdx.x / o.chunks;
    const int chunk = blockIdx.x % o.chunks;
    const int c = (int)(plane % o.C);
    const int64_t n = plane / o.C;
    const int r0 = chunk * o.rows_per_block, r1 = min(o.H, r0 + o.rows_per_block);
    const int wv4 = o.W >> 2;
    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < (r1 - r0) * wv4; i += 256) {
        const int iy = wv4 == 1 ? i : (int)__umulhi((unsigned)i, o.quad_magic), y = r0 + iy, x4 = (i - iy * wv4) * 4;
        const float4 t = sum4<T>(o, plane, y, x4);
        s1 += (t.x + t.y) + (t.z + t.w);
        s2 += (t.x * t.x + t.y * t.y) + (t.z * t.z + t.w * t.w);
    }
    s1 = block_sum(s1, s_red);
    s2 = block_sum(s2, s_red);
    if (threadIdx.x == 0) {
        float *row = part + (n * o.chunks + chunk) * 2 * o.C;
        row[c] = s1;
        row[o.C + c] = s2;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void tail_apply_kernel(Operands o, const float *__restrict__ mean,
                                                         const float *__restrict__ rstd,
                                                         const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, void *__restrict__ y) {
    const int64_t plane = blockIdx.x / o.chunks;
    const int chunk = blockIdx.x % o.chunks;
    const int c = (int)(plane % o.C);
    const int r0 = chunk * o.rows_per_block, r1 = min(o.H, r0 + o.rows_per_block);
    const int wv4 = o.W >> 2;
    const float sc = rstd[c] * (gamma ? gamma[c] : 1.f);
    const float sh = (beta ? beta[c] : 0.f) - mean[c] * sc;
    const float lo = o.relu ? 0.f : -INFINITY;
    for (int i = threadIdx.x; i < (r1 - r0) * wv4; i += 256) {
        const int iy = wv4 == 1 ? i : (int)__umulhi((unsigned)i, o.quad_magic), yy = r0 + iy, x4 = (i - iy * wv4) * 4;
        const float4 t = sum4<T>(o, plane, yy, x4);
        // nanmax: IEEE maximum (one v_maximum3_f32), not fmaxf (which returns the other operand for a NaN): a NaN
        // result (an inf or NaN anywhere in the channel makes the batch variance NaN) stays NaN under the ReLU
        store4<T>(y, (plane * o.H + yy) * o.W + x4, o.y_bf16,
               make_float4(nanmax(t.x * sc + sh, lo), nanmax(t.y * sc + sh, lo), nanmax(t.z * sc + sh, lo),
                           nanmax(t.w * sc + sh, lo)));
    }
}

// Gradient reaching the normalisation output: dy, masked by the fused ReLU (y recomputed, not stored).
template <typename T>
__device__ __forceinline__ float4 grad4(const Operands &o, const Raw4 &dy_raw, const float4 &t, float sc, float sh) {
    float4 g = decode<T>(dy_raw, o.dy_bf16);
    if (o.relu) {
        g.x = t.x * sc + sh > 0.f ? g.x : 0.f;
        g.y = t.y * sc + sh > 0.f ? g.y : 0.f;
        g.z = t.z * sc + sh > 0.f ? g.z : 0.f;
        g.w = t.w * sc + sh > 0.f ? g.w : 0.f;
    }
    return g;
}

// part row: (sum dy | sum dy * xhat) for the block's channel.
template <typename T>
__global__ __launch_bounds__(256) void tail_bwd_stats_kernel(Operands o, const float *__restrict__ mean,
                                                             const float *__restrict__ rstd,
                                                             const float *__restrict__ gamma,
                                                             const float *__restrict__ beta,
                                                             const void *__restrict__ dy,
                                                             float *__restrict__ part) {
    __shared__ float s_red[4];
    const int64_t plane = blockIdx.x / o.chunks;
    const int chunk = blockIdx.x % o.chunks;
    const int c = (int)(plane % o.C);
    const int64_t n = plane / o.C;
    const int r0 = chunk * o.rows_per_block, r1 = min(o.H, r0 + o.rows_per_block);
    const int wv4 = o.W >> 2;
    const float mu = mean[c], rs = rstd[c];
    const float sc = rs * (gamma ? gamma[c] : 1.f), sh = (beta ? beta[c] : 0.f) - mu * sc;
    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < (r1 - r0) * wv4; i += 256) {
        const int iy = wv4 == 1 ? i : (int)__umulhi((unsigned)i, o.quad_magic), yy = r0 + iy, x4 = (i - iy * wv4) * 4;
        Raw4 rdy;
        const float4 t = sum4<T>(o, plane, yy, x4, dy, &rdy);
        const float4 g = grad4<T>(o, rdy, t, sc, sh);
        s1 += (g.x + g.y) + (g.z + g.w);
        s2 += (g.x * (t.x - mu) + g.y * (t.y - mu)) + (g.z * (t.z - mu) + g.w * (t.w - mu));
    }
    s1 = block_sum(s1, s_red);
    s2 = block_sum(s2, s_red) * rs;
    if (threadIdx.x == 0) {
        float *row = part + (n * o.chunks + chunk) * 2 * o.C;
        row[c] = s1;
        row[o.C + c] = s2;
    }
}

// dt = gamma * rstd * (dy - mdy - xhat * mdyx);  da = db = dt (in their own dtypes);
// dx_lo += upsample^T(dt): the tile of dt is staged in LDS and every low-res pixel gathers its
// (2s x 2s) footprint, separably (columns, then rows); rows shared with the neighbouring tile go
// through fp32 atomics on the small low-res map.
template <typename T>
__global__ __launch_bounds__(256) void tail_bwd_apply_kernel(Operands o, const float *__restrict__ mean,
                                                             const float *__restrict__ rstd,
                                                             const float *__restrict__ gamma,
                                                             const float *__restrict__ beta,
                                                             const void *__restrict__ dy,
                                                             const float *__restrict__ mdy,
                                                             const float *__restrict__ mdyx, void *__restrict__ da,
                                                             void *__restrict__ db, float *__restrict__ dxlo) {
    extern __shared__ __attribute__((aligned(16))) float s_tile[];     // [rows][W] dt, then [rows][Wl] column sums
    const int64_t plane = blockIdx.x / o.chunks;
    const int chunk = blockIdx.x % o.chunks;
    const int c = (int)(plane % o.C);
    const int r0 = chunk * o.rows_per_block, r1 = min(o.H, r0 + o.rows_per_block);
    const int rows = r1 - r0;
    const int wv4 = o.W >> 2;
    const float mu = mean[c], rs = rstd[c];
    const float k = rs * (gamma ? gamma[c] : 1.f), m1 = mdy[c], m2 = mdyx[c];
    const float sh = (beta ? beta[c] : 0.f) - mu * k;
    const bool want_lo = dxlo != nullptr && o.x != nullptr;
    for (int i = threadIdx.x; i < rows * wv4; i += 256) {
        const int iy = wv4 == 1 ? i : (int)__umulhi((unsigned)i, o.quad_magic), yy = r0 + iy, x4 = (i - iy * wv4) * 4;
        const int64_t idx = (plane * o.H + yy) * o.W + x4;
        Raw4 rdy;
        const float4 t = sum4<T>(o, plane, yy, x4, dy, &rdy);
        const float4 g = grad4<T>(o, rdy, t, k, sh);
        const float4 d = make_float4(k * (g.x - m1 - (t.x - mu) * rs * m2), k * (g.y - m1 - (t.y - mu) * rs * m2),
                                     k * (g.z - m1 - (t.z - mu) * rs * m2), k * (g.w - m1 - (t.w - mu) * rs * m2));
        if (da) store4<T>(da, idx, o.a_bf16, d);
        if (db) store4<T>(db, idx, o.b_bf16, d);
        if (want_lo) {
            if (o.scale == 1) *reinterpret_cast<float4 *>(dxlo + idx) = d;      // same grid: plain store
            else *reinterpret_cast<float4 *>(s_tile + (yy - r0) * o.W + x4) = d;
        }
    }
    if (!want_lo || o.scale == 1) return;
    __syncthreads();
    const int s = o.scale;
    float *s_col = s_tile + rows * o.W;                                  // [rows][Wl]
    for (int i = threadIdx.x; i < rows * o.Wl; i += 256) {
        const int ry = i / o.Wl, j = i % o.Wl;
        const float *row = s_tile + ry * o.W;
        float acc = 0.f;
        const int xa = max(0, s * (j - 1)), xb = min(o.W - 1, s * (j + 2) - 1);
        for (int x = xa; x <= xb; ++x) {
            const Tap t = tap_of(x, o.Wl, s);
            const float w = (t.i0 == j ? 1.f - t.w1 : 0.f) + (t.i1 == j ? t.w1 : 0.f);
            acc += w * row[x];
        }
        s_col[i] = acc;
    }
    __syncthreads();
    const int i_lo = tap_of(r0, o.Hl, s).i0, i_hi = tap_of(r1 - 1, o.Hl, s).i1;
    float *out = dxlo + plane * o.Hl * o.Wl;
    for (int i = threadIdx.x; i < (i_hi - i_lo + 1) * o.Wl; i += 256) {
        const int li = i_lo + i / o.Wl, j = i % o.Wl;
        const int ya = max(r0, s * (li - 1)), yb = min(r1 - 1, s * (li + 2) - 1);
        float acc = 0.f;
        for (int y = ya; y <= yb; ++y) {
            const Tap t = tap_of(y, o.Hl, s);
            const float w = (t.i0 == li ? 1.f - t.w1 : 0.f) + (t.i1 == li ? t.w1 : 0.f);
            acc += w * s_col[(y - r0) * o.Wl + j];
        }
        // rows whose footprint lies wholly inside this tile are owned by it; the others are shared
        const bool owned = s * (li - 1) >= r0 && s * (li + 2) - 1 <= r1 - 1;
        if (owned || (li == 0 && r0 == 0 && s * (li + 2) - 1 <= r1 - 1) ||
            (li == o.Hl - 1 && r1 == o.H && s * (li - 1) >= r0))
            out[(int64_t)li * o.Wl + j] += acc;                         // no other workgroup touches this row
        else
            atomicAdd(out + (int64_t)li * o.Wl + j, acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Fixed forms.  The kernels above are the general form: every operand dtype, scale, b, shift, ReLU and output dtype is a
// run-time (wave-uniform) choice inside the per-quad body, which is what bounds them (VALU, not HBM).  The backbone
// runs three forms only -
//     norm1: 16-bit a + fp32 x at scale 4 + shift;   norm2: fp32 a + fp32 x at scale 2;   norm3: fp32 a + fp32 x, scale 1
// all without b, without ReLU and with fp32 y / dy - and for those the choices are template parameters <A16, S, SHIFT>.
// In stats, bwd_stats and bwd_apply an item is 8 consecutive pixels (W % 8 == 0): 16-bit operands arrive as one 16-byte
// load, fp32 operands as two, and the 8 pixels share the low-res columns of one row pair (4 columns at scale 4, 6 at
// scale 2); apply keeps quads (see sum4_form).  Arithmetic per element is the general form's, expression for expression:
// given the same mean / rstd / mdy / mdyx, y, da and dxlo carry the same bits; the channel sums associate differently
// (another thread sums the quad).  VAH_TAIL_FORM=general (read per call) routes every call to the kernels above.
// ---------------------------------------------------------------------------------------------------------------
template <bool A16>
__device__ __forceinline__ void load8(const void *p, int64_t idx, uint4 &lo, uint4 &hi) {
    if constexpr (A16) {
        lo = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(p) + idx);
        hi = lo;
    } else {
        lo = *reinterpret_cast<const uint4 *>(reinterpret_cast<const float *>(p) + idx);
        hi = *reinterpret_cast<const uint4 *>(reinterpret_cast<const float *>(p) + idx + 4);
    }
}

template <typename T, bool A16>
__device__ __forceinline__ void decode8(const uint4 &lo, const uint4 &hi, float (&v)[8]) {
    if constexpr (A16) {
        const float4 f0 = widen4<T>(lo.x, lo.y), f1 = widen4<T>(lo.z, lo.w);
        v[0] = f0.x, v[1] = f0.y, v[2] = f0.z, v[3] = f0.w;
        v[4] = f1.x, v[5] = f1.y, v[6] = f1.z, v[7] = f1.w;
    } else {
        v[0] = __uint_as_float(lo.x), v[1] = __uint_as_float(lo.y), v[2] = __uint_as_float(lo.z), v[3] = __uint_as_float(lo.w);
        v[4] = __uint_as_float(hi.x), v[5] = __uint_as_float(hi.y), v[6] = __uint_as_float(hi.z), v[7] = __uint_as_float(hi.w);
    }
}

// one pixel of the upsample: the column lerp on the two low-res rows, then the row lerp (sum4's expressions)
__device__ __forceinline__ float lerp2(float p0, float p1, float q0, float q1, float wx, float wy) {
    const float top = p0 + wx * (p1 - p0), bot = q0 + wx * (q1 - q0);
    return top + wy * (bot - top);
}

// t[0..7] = a + (shift + 0) + up(x) for 8 consecutive pixels (row y, columns x8 .. x8 + 7, x8 % 8 == 0) of `plane`;
// DY: g[0..7] = the fp32 dy of the same pixels.  `add` = shift[c] + 0.f (the general form's `sft + vb`, b absent).
// All loads are requested before the first is decoded.
template <typename T, bool A16, int S, bool DY>
__device__ __forceinline__ void sum8(const Operands &o, int64_t plane, int y, int x8, float add, const float *dy, float (&t)[8],
                                     float (&g)[8]) {
    const int64_t idx = (plane * o.H + y) * o.W + x8;
    uint4 alo, ahi, glo, ghi;
    load8<A16>(o.a, idx, alo, ahi);
    if constexpr (DY) load8<false>(dy, idx, glo, ghi);
    const float *xp = o.x + plane * o.Hl * o.Wl;
    constexpr int NC = S == 4 ? 4 : 6;                       // low-res columns under 8 pixels (scale 2: 6, scale 4: 4)
    float c0[NC], c1[NC];
    float4 xs0, xs1;
    float wy = 0.f;
    if constexpr (S == 1) {
        xs0 = *reinterpret_cast<const float4 *>(xp + (int64_t)y * o.Wl + x8);
        xs1 = *reinterpret_cast<const float4 *>(xp + (int64_t)y * o.Wl + x8 + 4);
    } else {
        const Tap ty = tap_of(y, o.Hl, S);
        wy = ty.w1;
        const float *r0 = xp + (int64_t)ty.i0 * o.Wl, *r1 = xp + (int64_t)ty.i1 * o.Wl;
        // columns bc .. bc + NC - 1, bc = floor of the first pixel's source position (>= -1); the inner ones start at
        // a multiple of NC - 2 floats, the two outer ones are clamped as the general form clamps them
        const int bc = x8 / S - 1;
        const int cl = max(bc, 0), cr = min(bc + NC - 1, o.Wl - 1);
        c0[0] = r0[cl];
        c1[0] = r1[cl];
        c0[NC - 1] = r0[cr];
        c1[NC - 1] = r1[cr];
        if constexpr (S == 4) {
            const float2 m0 = *reinterpret_cast<const float2 *>(r0 + bc + 1), m1 = *reinterpret_cast<const float2 *>(r1 + bc + 1);
            c0[1] = m0.x, c0[2] = m0.y;
            c1[1] = m1.x, c1[2] = m1.y;
        } else {
            const float4 m0 = *reinterpret_cast<const float4 *>(r0 + bc + 1), m1 = *reinterpret_cast<const float4 *>(r1 + bc + 1);
            c0[1] = m0.x, c0[2] = m0.y, c0[3] = m0.z, c0[4] = m0.w;
            c1[1] = m1.x, c1[2] = m1.y, c1[3] = m1.z, c1[4] = m1.w;
        }
    }
    __builtin_amdgcn_sched_barrier(0);                       // loads above, arithmetic below
    decode8<T, A16>(alo, ahi, t);
    if constexpr (DY) decode8<T, false>(glo, ghi, g);
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] += add;
    if constexpr (S == 1) {
        t[0] += xs0.x, t[1] += xs0.y, t[2] += xs0.z, t[3] += xs0.w;
        t[4] += xs1.x, t[5] += xs1.y, t[6] += xs1.z, t[7] += xs1.w;
    } else if constexpr (S == 4) {                           // pixel k: columns (k + 2) / 4 and the next; 5/8, 7/8, 1/8, 3/8
        constexpr float w[4] = {0.625f, 0.875f, 0.125f, 0.375f};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int j = (k + 2) >> 2;
            t[k] += lerp2(c0[j], c0[j + 1], c1[j], c1[j + 1], w[k & 3], wy);
        }
    } else {                                                 // pixel k: columns (k + 1) / 2 and the next; 3/4, 1/4
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int j = (k + 1) >> 1;
            t[k] += lerp2(c0[j], c0[j + 1], c1[j], c1[j + 1], (k & 1) ? 0.25f : 0.75f, wy);
        }
    }
}

// item -> (row, first column) of an 8-pixel item; o.oct_magic as o.quad_magic, for W / 8
__device__ __forceinline__ void item8(const Operands &o, int i, int wv8, int r0, int &y, int &x8) {
    const int iy = wv8 == 1 ? i : (int)__umulhi((unsigned)i, o.oct_magic);
    y = r0 + iy;
    x8 = (i - iy * wv8) * 8;
}

template <typename T, bool A16, int S, bool SHIFT>
__global__ __launch_bounds__(256) void tail_stats_form_kernel(Operands o, float *__restrict__ part) {
    __shared__ float s_red[4];
    const int64_t plane = blockIdx.x / o.chunks;
    const int chunk = blockIdx.x % o.chunks;
    const int c = (int)(plane % o.C);
    const int64_t n = plane / o.C;
    const int r0 = chunk * o.rows_per_block, r1 = min(o.H, r0 + o.rows_per_block);
    const int wv8 = o.W >> 3;
    const float add = (SHIFT ? o.shift[c] : 0.f) + 0.f;
    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < (r1 - r0) * wv8; i += 256) {
        int y, x8;
        item8(o, i, wv8, r0, y, x8);
        float t[8], g[8];
        sum8<T, A16, S, false>(o, plane, y, x8, add, nullptr, t, g);
        s1 += (t[0] + t[1]) + (t[2] + t[3]);
        s2 += (t[0] * t[0] + t[1] * t[1]) + (t[2] * t[2] + t[3] * t[3]);
        s1 += (t[4] + t[5]) + (t[6] + t[7]);
        s2 += (t[4] * t[4] + t[5] * t[5]) + (t[6] * t[6] + t[7] * t[7]);
    }
    s1 = block_sum(s1, s_red);
    s2 = block_sum(s2, s_red);
    if (threadIdx.x == 0) {
        float *row = part + (n * o.chunks + chunk) * 2 * o.C;
        row[c] = s1;
        row[o.C + c] = s2;
    }
}

// The same sum for one quad (row y, columns x4 .. x4 + 3): sum4 with its run-time choices resolved.  The normalise pass
// keeps quad items: it is the one pass that streams a full-size fp32 output, and with 8-pixel items a wave's store
// instruction covers every second 16 bytes of 2 KB (measured at stride 4: 130 us against the general form's 111 us),
// with quads it covers 1 KB of whole lines.
template <typename T, bool A16, int S>
__device__ __forceinline__ float4 sum4_form(const Operands &o, int64_t plane, int y, int x4, float add) {
    const int64_t idx = (plane * o.H + y) * o.W + x4;
    uint2 a2 = make_uint2(0u, 0u);
    uint4 a4 = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (A16) a2 = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint16_t *>(o.a) + idx);
    else a4 = *reinterpret_cast<const uint4 *>(reinterpret_cast<const float *>(o.a) + idx);
    const float *xp = o.x + plane * o.Hl * o.Wl;
    constexpr int NC = S == 4 ? 3 : 4;                       // low-res columns under 4 pixels
    float c0[NC], c1[NC];
    float4 xs = make_float4(0.f, 0.f, 0.f, 0.f);
    float wy = 0.f;
    if constexpr (S == 1) {
        xs = *reinterpret_cast<const float4 *>(xp + (int64_t)y * o.Wl + x4);
    } else {
        const Tap ty = tap_of(y, o.Hl, S);
        wy = ty.w1;
        const float *r0 = xp + (int64_t)ty.i0 * o.Wl, *r1 = xp + (int64_t)ty.i1 * o.Wl;
        const int bc = x4 / S - 1;                           // floor((2 x4 + 1 - S) / 2S), x4 % 4 == 0
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int cj = min(max(bc + j, 0), o.Wl - 1);
            c0[j] = r0[cj];
            c1[j] = r1[cj];
        }
    }
    __builtin_amdgcn_sched_barrier(0);                       // loads above, arithmetic below
    float4 t;
    if constexpr (A16) t = widen4<T>(a2.x, a2.y);
    else t = make_float4(__uint_as_float(a4.x), __uint_as_float(a4.y), __uint_as_float(a4.z), __uint_as_float(a4.w));
    t.x += add;
    t.y += add;
    t.z += add;
    t.w += add;
    if constexpr (S == 1) {
        t.x += xs.x;
        t.y += xs.y;
        t.z += xs.z;
        t.w += xs.w;
    } else if constexpr (S == 4) {                           // columns b, b, b + 1, b + 1; weights 5/8, 7/8, 1/8, 3/8
        t.x += lerp2(c0[0], c0[1], c1[0], c1[1], 0.625f, wy);
        t.y += lerp2(c0[0], c0[1], c1[0], c1[1], 0.875f, wy);
        t.z += lerp2(c0[1], c0[2], c1[1], c1[2], 0.125f, wy);
        t.w += lerp2(c0[1], c0[2], c1[1], c1[2], 0.375f, wy);
    } else {                                                 // columns b, b + 1, b + 1, b + 2; weights 3/4, 1/4, 3/4, 1/4
        t.x += lerp2(c0[0], c0[1], c1[0], c1[1], 0.75f, wy);
        t.y += lerp2(c0[1], c0[2], c1[1], c1[2], 0.25f, wy);
        t.z += lerp2(c0[1], c0[2], c1[1], c1[2], 0.75f, wy);
        t.w += lerp2(c0[2], c0[3], c1[2], c1[3], 0.25f, wy);
    }
    return t;
}

template <typename T, bool A16, int S, bool SHIFT>
__global__ __launch_bounds__(256) void tail_apply_form_kernel(Operands o, const float *__restrict__ mean,
                                                              const float *__restrict__ rstd,
                                                              const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, float *__restrict__ y) {
    const int64_t plane = blockIdx.x / o.chunks;
    const int chunk = blockIdx.x % o.chunks;
    const int c = (int)(plane % o.C);
    const int r0 = chunk * o.rows_per_block, r1 = min(o.H, r0 + o.rows_per_block);
    const int wv4 = o.W >> 2;                                // >= 2: W % 8 == 0
    const float add = (SHIFT ? o.shift[c] : 0.f) + 0.f;
    const float sc = rstd[c] * (gamma ? gamma[c] : 1.f);
    const float sh = (beta ? beta[c] : 0.f) - mean[c] * sc;
    for (int i = threadIdx.x; i < (r1 - r0) * wv4; i += 256) {
        const int iy = (int)__umulhi((unsigned)i, o.quad_magic), yy = r0 + iy, x4 = (i - iy * wv4) * 4;
        const float4 t = sum4_form<T, A16, S>(o, plane, yy, x4, add);
        // no ReLU: the general form's nanmax(v, -inf) is v
        *reinterpret_cast<float4 *>(y + (plane * o.H + yy) * o.W + x4) =
            make_float4(t.x * sc + sh, t.y * sc + sh, t.z * sc + sh, t.w * sc + sh);
    }
}

template <typename T, bool A16, int S, bool SHIFT>
__global__ __launch_bounds__(256) void tail_bwd_stats_form_kernel(Operands o, const float *__restrict__ mean,
                                                                  const float *__restrict__ rstd,
                                                                  const float *__restrict__ dy, float *__restrict__ part) {
    __shared__ float s_red[4];
    const int64_t plane = blockIdx.x / o.chunks;
    const int chunk = blockIdx.x % o.chunks;
    const int c = (int)(plane % o.C);
    const int64_t n = plane / o.C;
    const int r0 = chunk * o.rows_per_block, r1 = min(o.H, r0 + o.rows_per_block);
    const int wv8 = o.W >> 3;
    const float add = (SHIFT ? o.shift[c] : 0.f) + 0.f;
    const float mu = mean[c], rs = rstd[c];
    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < (r1 - r0) * wv8; i += 256) {
        int yy, x8;
        item8(o, i, wv8, r0, yy, x8);
        float t[8], g[8];
        sum8<T, A16, S, true>(o, plane, yy, x8, add, dy, t, g);
        s1 += (g[0] + g[1]) + (g[2] + g[3]);
        s2 += (g[0] * (t[0] - mu) + g[1] * (t[1] - mu)) + (g[2] * (t[2] - mu) + g[3] * (t[3] - mu));
        s1 += (g[4] + g[5]) + (g[6] + g[7]);
        s2 += (g[4] * (t[4] - mu) + g[5] * (t[5] - mu)) + (g[6] * (t[6] - mu) + g[7] * (t[7] - mu));
    }
    s1 = block_sum(s1, s_red);
    s2 = block_sum(s2, s_red) * rs;
    if (threadIdx.x == 0) {
        float *row = part + (n * o.chunks + chunk) * 2 * o.C;
        row[c] = s1;
        row[o.C + c] = s2;
    }
}

// The adjoint of the upsample with the weights of the scale as constants.  Low-res index j collects the 2S high-res
// positions S j - S / 2 + u, u = 0 .. 2S - 1, with weights (2u + 1) / 2S rising, then falling: 1/8 3/8 5/8 7/8 | 7/8 5/8 3/8
// 1/8 at S = 4, 1/4 3/4 | 3/4 1/4 at S = 2; every other position of the general form's loop has weight exactly 0.  At the
// two borders the clamped source positions fold both taps onto the border index: the S / 2 positions next to the border
// weigh (1 - w) + w = 1 and the S / 2 beyond it do not exist.  A term that does not exist (or, in the row pass, lies in
// another tile) leaves the sum as it is.  Terms are added in ascending position, as the general form adds them.
// TILE: positions lo .. hi - 1 only are present (the rows of this tile); otherwise the whole axis 0 .. S n_lo - 1 is.
template <int S, bool TILE>
__device__ __forceinline__ float adjoint_taps(const float *p, int stride, int j, int n_lo, int lo, int hi) {
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < 2 * S; ++u) {
        const float wc = (float)(u < S ? 2 * u + 1 : 4 * S - 2 * u - 1) * (0.5f / (float)S);
        const int pos = S * j - S / 2 + u;
        const bool inner = u >= S / 2 && u < S + S / 2;
        const bool at_border = u < S ? j == 0 : j == n_lo - 1;
        const float w = inner && at_border ? 1.f : wc;
        // fmaf, spelled out: the general form's `acc += w * row[x]` contracts to one fma, and so must every term here
        // (left to the compiler, a term under a select became a multiply and an add: two roundings)
        if (!TILE && inner) {                                           // always there: S j <= pos < S (j + 1)
            acc = __builtin_fmaf(w, p[pos * stride], acc);
        } else {
            const bool there = (inner || !at_border) && (!TILE || (pos >= lo && pos < hi));
            const int at = TILE ? min(max(pos, lo), hi - 1) - lo : (u < S ? max(pos, 0) : min(pos, S * n_lo - 1));
            const float sum = __builtin_fmaf(w, p[at * stride], acc);
            acc = there ? sum : acc;
        }
    }
    return acc;
}

// dt, da and dxlo as tail_bwd_apply_kernel; b absent, da and dxlo present, dy fp32
template <typename T, bool A16, int S, bool SHIFT>
__global__ __launch_bounds__(256) void tail_bwd_apply_form_kernel(Operands o, const float *__restrict__ mean,
                                                                  const float *__restrict__ rstd,
                                                                  const float *__restrict__ gamma,
                                                                  const float *__restrict__ dy,
                                                                  const float *__restrict__ mdy,
                                                                  const float *__restrict__ mdyx, void *__restrict__ da,
                                                                  float *__restrict__ dxlo) {
    extern __shared__ __attribute__((aligned(16))) float s_tile[];     // [rows][W] dt, then [rows][Wl] column sums
    const int64_t plane = blockIdx.x / o.chunks;
    const int chunk = blockIdx.x % o.chunks;
    const int c = (int)(plane % o.C);
    const int r0 = chunk * o.rows_per_block, r1 = min(o.H, r0 + o.rows_per_block);
    const int rows = r1 - r0;
    const int wv8 = o.W >> 3;
    const float add = (SHIFT ? o.shift[c] : 0.f) + 0.f;
    const float mu = mean[c], rs = rstd[c];
    const float k = rs * (gamma ? gamma[c] : 1.f), m1 = mdy[c], m2 = mdyx[c];
    for (int i = threadIdx.x; i < rows * wv8; i += 256) {
        int yy, x8;
        item8(o, i, wv8, r0, yy, x8);
        const int64_t idx = (plane * o.H + yy) * o.W + x8;
        float t[8], g[8], d[8];
        sum8<T, A16, S, true>(o, plane, yy, x8, add, dy, t, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = k * (g[e] - m1 - (t[e] - mu) * rs * m2);
        const float4 d0 = make_float4(d[0], d[1], d[2], d[3]), d1 = make_float4(d[4], d[5], d[6], d[7]);
        if constexpr (A16) {
            vec8<T> v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (T)d[e];
            *reinterpret_cast<vec8<T> *>(reinterpret_cast<T *>(da) + idx) = v;
        } else {
            *reinterpret_cast<float4 *>(reinterpret_cast<float *>(da) + idx) = d0;
            *reinterpret_cast<float4 *>(reinterpret_cast<float *>(da) + idx + 4) = d1;
        }
        float *lo = S == 1 ? dxlo + idx : s_tile + (yy - r0) * o.W + x8;         // scale 1: same grid, plain store
        *reinterpret_cast<float4 *>(lo) = d0;
        *reinterpret_cast<float4 *>(lo + 4) = d1;
    }
    if constexpr (S > 1) {
        __syncthreads();
        float *s_col = s_tile + rows * o.W;                              // [rows][Wl]
        const int Wl = o.Wl;
        for (int i = threadIdx.x; i < rows * Wl; i += 256) {
            const int ry = (int)__umulhi((unsigned)i, o.lo_magic), j = i - ry * Wl;
            s_col[i] = adjoint_taps<S, false>(s_tile + ry * o.W, 1, j, Wl, 0, o.W);
        }
        __syncthreads();
        const int i_lo = tap_of(r0, o.Hl, S).i0, i_hi = tap_of(r1 - 1, o.Hl, S).i1;
        float *out = dxlo + plane * o.Hl * Wl;
        for (int i = threadIdx.x; i < (i_hi - i_lo + 1) * Wl; i += 256) {
            const int ly = (int)__umulhi((unsigned)i, o.lo_magic), li = i_lo + ly, j = i - ly * Wl;
            const float acc = adjoint_taps<S, true>(s_col + j, Wl, li, o.Hl, r0, r1);
            // rows whose footprint lies wholly inside this tile are owned by it; the others are shared
            const bool owned = S * (li - 1) >= r0 && S * (li + 2) - 1 <= r1 - 1;
            if (owned || (li == 0 && r0 == 0 && S * (li + 2) - 1 <= r1 - 1) ||
                (li == o.Hl - 1 && r1 == o.H && S * (li - 1) >= r0))
                out[(int64_t)li * Wl + j] += acc;                       // no other workgroup touches this row
            else
                atomicAdd(out + (int64_t)li * Wl + j, acc);
        }
    }
}

__global__ __launch_bounds__(256) void tail_finalize(const float *__restrict__ part, int nparts, int K,
                                                     float *__restrict__ out) {
    __shared__ float s_acc[8][32];
    const int col = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int k = blockIdx.x * 32 + col;
    float acc = 0.f;
    if (k < K)
        for (int p = pl; p < nparts; p += 8) acc += part[(int64_t)p * K + k];
    s_acc[pl][col] = acc;
    __syncthreads();
    if (pl == 0 && k < K) {
        float t = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) t += s_acc[u][col];
        out[k] = t;
    }
}

// sums = [sum t (C) | sum t^2 (C) | count (1)]  ->  mean, rstd (biased variance, as the normalisation
// uses) and the running statistics (unbiased variance, momentum) in ONE small launch; done with
// separate torch ops this bookkeeping was ~10 kernel launches per BatchNorm call.
__device__ __forceinline__ void bn_finalize_channel(const float *__restrict__ sums, int C, int c, float count, float eps,
                                                    float momentum, float *__restrict__ running_mean,
                                                    float *__restrict__ running_var, float *__restrict__ mean,
                                                    float *__restrict__ rstd) {
    const float mu = sums[c] / count;
    // nanmax: an inf or NaN in the channel gives a NaN variance, and BatchNorm then a NaN channel (as torch's)
    const float var = nanmax(sums[C + c] / count - mu * mu, 0.f);
    mean[c] = mu;
    rstd[c] = rsqrtf(var + eps);
    if (running_mean) {
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * var * (count / fmaxf(count - 1.f, 1.f));
    }
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const float *__restrict__ sums, int C, float eps, float momentum,
                                                          float *__restrict__ running_mean,
                                                          float *__restrict__ running_var, float *__restrict__ mean,
                                                          float *__restrict__ rstd) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    bn_finalize_channel(sums, C, c, sums[2 * C], eps, momentum, running_mean, running_var, mean, rstd);
}

// The same with BatchNorm's bookkeeping: the count comes as an argument (no thread reads sums[2 * C], so the thread
// that stores it there for the backward races with nobody) and num_batches_tracked advances by one.  Saves the fill and
// the int64 add that torch ran as launches of their own (2 x 11 per step).
__global__ __launch_bounds__(256) void bn_finalize_book_kernel(float *__restrict__ sums, int C, float count, float eps,
                                                               float momentum, float *__restrict__ running_mean,
                                                               float *__restrict__ running_var, float *__restrict__ mean,
                                                               float *__restrict__ rstd,
                                                               int64_t *__restrict__ num_batches_tracked) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    bn_finalize_channel(sums, C, c, count, eps, momentum, running_mean, running_var, mean, rstd);
    if (c == 0) {
        sums[2 * C] = count;
        if (num_batches_tracked) *num_batches_tracked += 1;
    }
}

// (B, T_total, C) fp32 token rows [t0, t0 + T)  <->  (B, C, T) planes (fp32 or the 16-bit type E), through a
// 32 x 33 LDS tile (both sides coalesced).  TO_PLANES: planes <- tokens; else tokens <- planes
// (+ an optional per-channel vector: conv bias + level embedding of the SPM maps).
template <typename E, bool TO_PLANES>
__global__ __launch_bounds__(256) void transpose_tokens_kernel(const void *__restrict__ src, void *__restrict__ dst,
                                                               int64_t T_total, int64_t t0, int T, int C,
                                                               int planes_bf16, const float *__restrict__ vec) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int tt = blockIdx.x * 32, cc = blockIdx.y * 32;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;          // 32 x 8
    const int64_t tok_off = ((int64_t)b * T_total + t0) * C;
    const int64_t plane_base = (int64_t)b * C * T;
    if (TO_PLANES) {
        const float *tok = reinterpret_cast<const float *>(src) + tok_off;
        float v4[4];                                                  // 4 clamped loads in flight, selected afterwards
#pragma unroll
        for (int u = 0; u < 4; ++u)                                   // tile[token][channel], channel fastest
            v4[u] = tok[(int64_t)min(tt + ly + 8 * u, T - 1) * C + min(cc + lx, C - 1)];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u) tile[ly + 8 * u][lx] = (tt + ly + 8 * u < T && cc + lx < C) ? v4[u] : 0.f;
        __syncthreads();
#pragma unroll
        for (int r = ly; r < 32; r += 8)                              // write plane rows: token fastest
            if (cc + r < C && tt + lx < T) {
                const int64_t o = plane_base + (int64_t)(cc + r) * T + tt + lx;
                if (planes_bf16) reinterpret_cast<E *>(dst)[o] = (E)tile[lx][r];
                else reinterpret_cast<float *>(dst)[o] = tile[lx][r];
            }
    } else {
        float v4[4];
        int64_t o4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)                                   // tile[channel][token], token fastest
            o4[u] = plane_base + (int64_t)min(cc + ly + 8 * u, C - 1) * T + min(tt + lx, T - 1);
        if (planes_bf16) {                                            // dtype branch around the 4 loads, not inside
#pragma unroll
            for (int u = 0; u < 4; ++u) v4[u] = (float)reinterpret_cast<const E *>(src)[o4[u]];
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) v4[u] = reinterpret_cast<const float *>(src)[o4[u]];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u) tile[ly + 8 * u][lx] = (cc + ly + 8 * u < C && tt + lx < T) ? v4[u] : 0.f;
        __syncthreads();
        float *tok = reinterpret_cast<float *>(dst) + tok_off;
        const float add = (vec && cc + lx < C) ? vec[cc + lx] : 0.f;
#pragma unroll
        for (int r = ly; r < 32; r += 8)
            if (tt + r < T && cc + lx < C) tok[(int64_t)(tt + r) * C + cc + lx] = tile[lx][r] + add;
    }
}

// MaxPool2d(kernel 3, stride 2, padding 1) of the SPM stem (adapter_modules.py:229-230), 16-bit NCHW.
// Forward keeps the window position (0..8) of the FIRST maximum in row-major scan order - the element
// torch's max_pool2d routes the gradient to - in one byte per output; backward is a gather: every
// input pixel lies in at most 4 windows and takes their gradients where it is the recorded maximum
// (torch's backward scatters with atomics: 222 us for the 2 x 64 x 512 x 512 stem map).
template <typename T>
__global__ __launch_bounds__(256) void maxpool3s2_fwd_kernel(const T *__restrict__ x, int H, int W, int Ho, int Wo,
                                                             T *__restrict__ y, unsigned char *__restrict__ idx) {
    // block = 64 output columns x 4 output rows of one plane (blockIdx.z): no index divisions
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= Wo || oy >= Ho) return;
    const int64_t plane = blockIdx.z;
    const T *xp = x + plane * H * W;
    // the 9 window values are requested together (clamped coordinates), validity applied afterwards: loads
    // under `if (inside)` were waited on one by one
    float win[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int iy = min(max(2 * oy - 1 + k / 3, 0), H - 1), ix = min(max(2 * ox - 1 + k % 3, 0), W - 1);
        win[k] = (float)xp[(int64_t)iy * W + ix];
    }
    __builtin_amdgcn_sched_barrier(0);
    float best = -INFINITY;
    int pos = 0;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int iy = 2 * oy - 1 + k / 3, ix = 2 * ox - 1 + k % 3;
        const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
        const float v = win[k];
        if (in && (!any || v > best || v != v)) {
            best = v;
            pos = k;
            any = true;
        }
    }
    const int64_t o = (plane * Ho + oy) * Wo + ox;
    y[o] = (T)best;
    idx[o] = (unsigned char)pos;
}

// thread = 8 consecutive input columns of one input row (one 16-byte store); block = 64 x 4 such threads
template <typename T>
__global__ __launch_bounds__(256) void maxpool3s2_bwd_kernel(const T *__restrict__ gy,
                                                             const unsigned char *__restrict__ idx, int H, int W, int Ho,
                                                             int Wo, T *__restrict__ gx) {
    const int ix0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 8;
    const int iy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ix0 >= W || iy >= H) return;
    const int64_t plane = blockIdx.z;
    const T *gp = gy + plane * Ho * Wo;
    const unsigned char *ip = idx + plane * Ho * Wo;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int oy0 = iy >> 1, oy1 = (iy + 1) >> 1;                  // the one or two window rows that contain iy
    const int oxb = ix0 >> 1;                                       // windows oxb .. oxb + 4 touch these 8 columns
    // all 20 loads (2 window rows x 5 windows x {gradient, recorded position}) are requested first, with
    // clamped coordinates; validity is applied afterwards (loads under `in ? .. : ..` were waited on in pairs)
    float g[2][5];
    int p[2][5];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int oyc = min(a == 0 ? oy0 : oy1, Ho - 1);
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int64_t at = (int64_t)oyc * Wo + min(oxb + u, Wo - 1);
            g[a][u] = (float)gp[at];
            p[a][u] = (int)ip[at];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int oy = a == 0 ? oy0 : oy1;
        if ((a == 1 && oy1 == oy0) || oy >= Ho) continue;
        const int ky3 = (iy - (2 * oy - 1)) * 3;
#pragma unroll
        for (int u = 0; u < 5; ++u)
            if (oxb + u >= Wo) p[a][u] = -1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            // column ix0 + e lies in window (ix0 + e) >> 1 at kx = 1 (even e) or 2 (odd e), and in the next
            // window at kx = 0 (odd e only); ix0 is a multiple of 8
            const int u0 = e >> 1;
            const int kx0 = (e & 1) ? 2 : 1;
            if (p[a][u0] == ky3 + kx0) acc[e] += g[a][u0];
            if (e & 1)
                if (p[a][u0 + 1] == ky3 + 0) acc[e] += g[a][u0 + 1];
        }
    }
    T *o = gx + (plane * H + iy) * (int64_t)W + ix0;
    if (ix0 + 8 <= W && (W & 7) == 0) {
        vec8<T> v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (T)acc[e];
        *reinterpret_cast<vec8<T> *>(o) = v;
    } else {
        for (int e = 0; e < 8 && ix0 + e < W; ++e) o[e] = (T)acc[e];
    }
}

constexpr size_t kTailLdsMax = 150 * 1024;      // dynamic LDS of tail_bwd_apply_kernel (160 KB per CU on gfx950)

// The shape rule and the tiling plan of all four passes (and of vah_bn_tail_supported): a shape is accepted by
// every entry point or by none, whichever pointers a particular call passes.
int plan_tail(const char *fn, Operands &o, int has_x, int scale, int64_t N, int64_t C, int64_t H, int64_t W) {
    if (N < 1 || C < 1 || H < 1 || W < 4 || W % 4 || W > kTilePx) return fail(VAH_E_SHAPE, "%s: bad shape", fn);
    if (scale != 1 && scale != 2 && scale != 4 && scale != 8) return fail(VAH_E_SHAPE, "%s: scale must be 1, 2, 4 or 8", fn);
    if (has_x && (H % scale || W % scale || (W / scale) % 4)) return fail(VAH_E_SHAPE, "%s: H, W not multiples of the scale", fn);
    if (N * C * H * W >= ((int64_t)1 << 40)) return fail(VAH_E_SHAPE, "%s: too large", fn);
    // every (image, chunk) owns one partial row of the workspace, and an image has at least one chunk
    if (N > kTailParts) return fail(VAH_E_SHAPE, "%s: batch %lld above %d", fn, (long long)N, kTailParts);
    o.scale = scale;
    o.C = (int)C;
    o.H = (int)H;
    o.W = (int)W;
    o.Hl = (int)(H / scale);
    o.Wl = (int)(W / scale);
    int rpb = std::max<int>(1, kTilePx / (int)W);
    rpb = std::max(scale * 2, rpb / (scale * 2) * (scale * 2));        // multiple of 2s: tiles end between footprints
    rpb = std::min<int>(rpb, (int)H);
    o.rows_per_block = rpb;
    o.chunks = (int)((H + rpb - 1) / rpb);
    if (N * o.chunks > kTailParts) {                                     // keep the partial rows bounded
        o.chunks = std::max<int>(1, kTailParts / (int)N);
        o.rows_per_block = (int)((H + o.chunks - 1) / o.chunks);
        o.rows_per_block = (o.rows_per_block + 2 * scale - 1) / (2 * scale) * (2 * scale);
        o.chunks = (int)((H + o.rows_per_block - 1) / o.rows_per_block);
    }
    // exact for items < 2^16 (a block has rows_per_block * W / 4 <= 8192 / 4 + 2 * scale * W / 4 of them)
    if ((int64_t)o.rows_per_block * (W / 4) >= 65536) return fail(VAH_E_SHAPE, "%s: row too wide for the tiling", fn);
    // the adjoint of the upsample stages a tile of dt and its column sums in LDS; the forward passes are held to
    // the same limit, so that a forward that ran has a backward that runs
    if (has_x && scale > 1 && (size_t)o.rows_per_block * (o.W + o.Wl) * sizeof(float) > kTailLdsMax)
        return fail(VAH_E_SHAPE, "%s: a tile of %d rows x (%d + %d) floats does not fit %d KB of LDS (batch too large for "
                    "this map, or rows too wide)", fn, o.rows_per_block, o.W, o.Wl, (int)(kTailLdsMax / 1024));
    o.quad_magic = W / 4 > 1 ? (unsigned)(((uint64_t)1 << 32) / (uint64_t)(W / 4)) + 1u : 0u;      // one quad per row: no division
    // fixed forms: fewer items than quads, and rows_per_block * Wl <= rows_per_block * W / 2 < 2^16 as well (the LDS
    // limit above holds rows_per_block * W below 38400 where there is an x at scale > 1)
    o.oct_magic = W / 8 > 1 ? (unsigned)(((uint64_t)1 << 32) / (uint64_t)(W / 8)) + 1u : 0u;
    o.lo_magic = o.Wl > 1 ? (unsigned)(((uint64_t)1 << 32) / (uint64_t)o.Wl) + 1u : 0u;
    return VAH_OK;
}

// Which fixed form a call takes (0: the general form).  VAH_TAIL_FORM=general, read per call, sends every call to the
// general form: the A/B handle of tests/test_tail_forms_gpu.py and of the measurements in DESIGN 4.7.
enum TailForm { kFormGeneral = 0, kFormNorm1, kFormNorm2, kFormNorm3 };

TailForm tail_form(const Operands &o, int relu, int out_16) {
    if (o.b || !o.x || relu || out_16 || o.W % 8 || (uintptr_t)o.a % 16) return kFormGeneral;      // 16-byte loads
    const char *e = getenv("VAH_TAIL_FORM");
    if (e && !strcmp(e, "general")) return kFormGeneral;
    if (o.a_bf16 && o.scale == 4 && o.shift) return kFormNorm1;
    if (!o.a_bf16 && o.scale == 2 && !o.shift) return kFormNorm2;
    if (!o.a_bf16 && o.scale == 1 && !o.shift) return kFormNorm3;
    return kFormGeneral;
}

// KERNEL<T, A16, S, SHIFT> of `form` (not kFormGeneral)
#define VAH_TAIL_FORM_LAUNCH(form, KERNEL, grid, smem, st, ...)                                                   \
    do {                                                                                                          \
        if ((form) == kFormNorm1) hipLaunchKernelGGL((KERNEL<T, true, 4, true>), grid, dim3(256), smem, st, __VA_ARGS__);        \
        else if ((form) == kFormNorm2) hipLaunchKernelGGL((KERNEL<T, false, 2, false>), grid, dim3(256), smem, st, __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<T, false, 1, false>), grid, dim3(256), smem, st, __VA_ARGS__);            \
    } while (0)

int fill_operands(const char *fn, Operands &o, const void *a, int a_bf16, const void *b, int b_bf16, const float *x,
                  int scale, int64_t N, int64_t C, int64_t H, int64_t W) {
    if (int rc = plan_tail(fn, o, x != nullptr, scale, N, C, H, W)) return rc;
    if (!a) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)a | (uintptr_t)b) % 8 || (uintptr_t)x % 16 || (!a_bf16 && (uintptr_t)a % 16) || (b && !b_bf16 && (uintptr_t)b % 16))
        return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    o.relu = o.y_bf16 = o.dy_bf16 = 0;
    o.shift = nullptr;
    o.a = a;
    o.b = b;
    o.x = x;
    o.a_bf16 = a_bf16;
    o.b_bf16 = b_bf16;
    return VAH_OK;
}


// ConvTranspose2d(k = 2, stride 2) as GEMMs on token rows: the product U (B, 4 * C, h * w), rows (dy, dx, co), is the
// transposed convolution's output with its 2 x 2 sub-pixels still apart; this pass interleaves them into NCHW planes
//   out[b][co][2 y + dy][2 x + dx] = U[b][(2 dy + dx) * C + co][y * w + x]            (inverse: the other way round)
// One thread: 8 consecutive x of one source row pair (dx = 0, 1) <-> 16 consecutive output pixels (16-byte accesses).
// `add` (forward only, planes-shaped, of type T, or null): dst = interleave(src) + add, rounded once - the `up(c2) + c1`
// of vit_adapter.py:107 in the precision autocast gives it (two 16-bit tensors summed into one)
template <typename T, bool INVERSE>
__global__ __launch_bounds__(256) void pixel_shuffle2_kernel(const T *__restrict__ src, T *__restrict__ dst,
                                                             const T *__restrict__ add, int B, int C, int h, int w,
                                                             int64_t items) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // (b, co, Y, x8)
    if (i >= items) return;
    const int w8 = w >> 3;
    const int x8 = (int)(i % w8);
    int64_t t = i / w8;
    const int Y = (int)(t % (2 * h));
    t /= 2 * h;
    const int co = (int)(t % C), b = (int)(t / C);
    const int y = Y >> 1, dy = Y & 1;
    const int64_t u0 = (((int64_t)b * 4 + 2 * dy) * C + co) * ((int64_t)h * w) + (int64_t)y * w + 8 * x8;       // dx = 0 row
    const int64_t u1 = u0 + (int64_t)C * h * w;                                                                  // dx = 1 row
    const int64_t o = (((int64_t)b * C + co) * (2 * h) + Y) * (2 * (int64_t)w) + 16 * x8;
    if (!INVERSE) {
        const vec8<T> a = *reinterpret_cast<const vec8<T> *>(src + u0), c = *reinterpret_cast<const vec8<T> *>(src + u1);
        vec8<T> lo, hi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lo[2 * j] = a[j], lo[2 * j + 1] = c[j];
            hi[2 * j] = a[4 + j], hi[2 * j + 1] = c[4 + j];
        }
        if (add) {
            const vec8<T> p = *reinterpret_cast<const vec8<T> *>(add + o), q = *reinterpret_cast<const vec8<T> *>(add + o + 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                lo[j] = (T)((float)lo[j] + (float)p[j]);
                hi[j] = (T)((float)hi[j] + (float)q[j]);
            }
        }
        *reinterpret_cast<vec8<T> *>(dst + o) = lo;
        *reinterpret_cast<vec8<T> *>(dst + o + 8) = hi;
    } else {
        const vec8<T> lo = *reinterpret_cast<const vec8<T> *>(src + o), hi = *reinterpret_cast<const vec8<T> *>(src + o + 8);
        vec8<T> a, c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = lo[2 * j], c[j] = lo[2 * j + 1];
            a[4 + j] = hi[2 * j], c[4 + j] = hi[2 * j + 1];
        }
        *reinterpret_cast<vec8<T> *>(dst + u0) = a;
        *reinterpret_cast<vec8<T> *>(dst + u1) = c;
    }
}

// One entry / launch template per pair of entry points (bf16 | `_f16`): checks, messages (function name apart), launch
// geometry, LDS and workspaces are the same code; T picks the kernel instantiation and the profiler row.
template <typename T>
int tail_stats_launch(const char *fn, const void *a, int a_bf16, const void *b, int b_bf16, const float *x, int scale, int64_t N,
                      int64_t C, int64_t H, int64_t W, const float *shift, float *sums, float *ws, void *stream) {
    clear_error();
    Operands o;
    if (int rc = fill_operands(fn, o, a, a_bf16, b, b_bf16, x, scale, N, C, H, W)) return rc;
    if (!sums || !ws) return fail(VAH_E_NULL, "%s: null pointer", fn);
    o.shift = shift;
    hipStream_t st = (hipStream_t)stream;
    const int nparts = (int)N * o.chunks;
    LaunchScope scope(tname<T>("bn_tail_stats", "bn_tail_stats_f16"),
                      N * C * H * W * ((a_bf16 ? 2 : 4) + (b ? (b_bf16 ? 2 : 4) : 0)), st);
    const dim3 grid((unsigned)(N * C * o.chunks));
    if (const TailForm form = tail_form(o, 0, 0)) VAH_TAIL_FORM_LAUNCH(form, tail_stats_form_kernel, grid, 0, st, o, ws);
    else hipLaunchKernelGGL(tail_stats_kernel<T>, grid, dim3(256), 0, st, o, ws);
    hipLaunchKernelGGL(tail_finalize, dim3((unsigned)((2 * C + 31) / 32)), dim3(256), 0, st, ws, nparts, (int)(2 * C), sums);
    return check_launch(fn);
}

template <typename T>
int tail_apply_launch(const char *fn, const void *a, int a_bf16, const void *b, int b_bf16, const float *x, int scale, int64_t N,
                      int64_t C, int64_t H, int64_t W, const float *mean, const float *rstd, const float *gamma,
                      const float *beta, int relu, const float *shift, void *y, int y_bf16, void *stream) {
    clear_error();
    Operands o;
    if (int rc = fill_operands(fn, o, a, a_bf16, b, b_bf16, x, scale, N, C, H, W)) return rc;
    if (!mean || !rstd || !y) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if ((uintptr_t)y % (y_bf16 ? 8 : 16)) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    o.relu = relu != 0;
    o.y_bf16 = y_bf16 != 0;
    o.shift = shift;
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope(tname<T>("bn_tail_apply", "bn_tail_apply_f16"),
                      N * C * H * W * ((a_bf16 ? 2 : 4) + (b ? (b_bf16 ? 2 : 4) : 0) + 4), st);
    const dim3 grid((unsigned)(N * C * o.chunks));
    if (const TailForm form = tail_form(o, o.relu, o.y_bf16))
        VAH_TAIL_FORM_LAUNCH(form, tail_apply_form_kernel, grid, 0, st, o, mean, rstd, gamma, beta, (float *)y);
    else
        hipLaunchKernelGGL(tail_apply_kernel<T>, grid, dim3(256), 0, st, o, mean, rstd, gamma, beta, y);
    return check_launch(fn);
}

template <typename T>
int tail_bwd_stats_launch(const char *fn, const void *a, int a_bf16, const void *b, int b_bf16, const float *x, int scale,
                          int64_t N, int64_t C, int64_t H, int64_t W, const float *mean, const float *rstd,
                          const float *gamma, const float *beta, int relu, const float *shift, const void *dy, int dy_bf16,
                          float *sums, float *ws, void *stream) {
    clear_error();
    Operands o;
    if (int rc = fill_operands(fn, o, a, a_bf16, b, b_bf16, x, scale, N, C, H, W)) return rc;
    if (!mean || !rstd || !dy || !sums || !ws) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if ((uintptr_t)dy % (dy_bf16 ? 8 : 16)) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    o.relu = relu != 0;
    o.dy_bf16 = dy_bf16 != 0;
    o.shift = shift;
    hipStream_t st = (hipStream_t)stream;
    const int nparts = (int)N * o.chunks;
    LaunchScope scope(tname<T>("bn_tail_bwd_stats", "bn_tail_bwd_stats_f16"),
                      N * C * H * W * ((a_bf16 ? 2 : 4) + (b ? (b_bf16 ? 2 : 4) : 0) + 4), st);
    const dim3 grid((unsigned)(N * C * o.chunks));
    if (const TailForm form = tail_form(o, o.relu, o.dy_bf16))
        VAH_TAIL_FORM_LAUNCH(form, tail_bwd_stats_form_kernel, grid, 0, st, o, mean, rstd, (const float *)dy, ws);
    else
        hipLaunchKernelGGL(tail_bwd_stats_kernel<T>, grid, dim3(256), 0, st, o, mean, rstd, gamma, beta, dy, ws);
    hipLaunchKernelGGL(tail_finalize, dim3((unsigned)((2 * C + 31) / 32)), dim3(256), 0, st, ws, nparts, (int)(2 * C), sums);
    return check_launch(fn);
}

template <typename T>
int tail_bwd_apply_launch(const char *fn, const void *a, int a_bf16, const void *b, int b_bf16, const float *x, int scale,
                          int64_t N, int64_t C, int64_t H, int64_t W, const float *mean, const float *rstd,
                          const float *gamma, const float *beta, int relu, const float *shift, const void *dy, int dy_bf16,
                          const float *mdy, const float *mdyx, void *da, void *db, float *dxlo, void *stream) {
    clear_error();
    Operands o;
    if (int rc = fill_operands(fn, o, a, a_bf16, b, b_bf16, x, scale, N, C, H, W)) return rc;
    if (!mean || !rstd || !dy || !mdy || !mdyx) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if ((uintptr_t)dy % (dy_bf16 ? 8 : 16) || (uintptr_t)dxlo % 16 || ((uintptr_t)da | (uintptr_t)db) % 8)
        return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    o.relu = relu != 0;
    o.dy_bf16 = dy_bf16 != 0;
    o.shift = shift;
    hipStream_t st = (hipStream_t)stream;
    size_t smem = 0;
    if (dxlo && x && scale > 1) smem = (size_t)o.rows_per_block * (o.W + o.Wl) * sizeof(float);
    LaunchScope scope(tname<T>("bn_tail_bwd_apply", "bn_tail_bwd_apply_f16"),
                      N * C * H * W * (2 * ((a_bf16 ? 2 : 4) + (b ? (b_bf16 ? 2 : 4) : 0)) + 4), st);
    const dim3 grid((unsigned)(N * C * o.chunks));
    const TailForm form = da && (uintptr_t)da % 16 == 0 && !db && dxlo ? tail_form(o, o.relu, o.dy_bf16) : kFormGeneral;
    if (smem > 64 * 1024) {
        const void *fnp = (const void *)tail_bwd_apply_kernel<T>;
        if (form == kFormNorm1) fnp = (const void *)tail_bwd_apply_form_kernel<T, true, 4, true>;
        else if (form == kFormNorm2) fnp = (const void *)tail_bwd_apply_form_kernel<T, false, 2, false>;
        (void)hipFuncSetAttribute(fnp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    }
    if (form)
        VAH_TAIL_FORM_LAUNCH(form, tail_bwd_apply_form_kernel, grid, smem, st, o, mean, rstd, gamma, (const float *)dy, mdy, mdyx, da,
                             dxlo);
    else
        hipLaunchKernelGGL(tail_bwd_apply_kernel<T>, grid, dim3(256), smem, st, o, mean, rstd, gamma, beta, dy, mdy, mdyx, da, db, dxlo);
    return check_launch(fn);
}

template <typename T>
int transpose_tokens_launch(const char *fn, const void *src, int64_t B, int64_t T_total, int64_t t0, int64_t Tn, int64_t C,
                            void *dst, int to_planes, int planes_bf16, const float *vec, void *stream) {
    clear_error();
    if (B < 0 || T_total < 0 || t0 < 0 || Tn < 0 || t0 + Tn > T_total || C < 1 || B > 65535 || C > 65535 * 32 || Tn >= ((int64_t)1 << 31))
        return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    if (B == 0 || Tn == 0) return VAH_OK;
    if (!src || !dst) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (to_planes && vec) return fail(VAH_E_UNSUPPORTED, "%s: vec only applies to planes -> tokens", fn);
    const dim3 grid((unsigned)((Tn + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope(tname<T>("transpose_tokens", "transpose_tokens_f16"), B * Tn * C * (4 + (planes_bf16 ? 2 : 4)), st);
    if (to_planes)
        hipLaunchKernelGGL((transpose_tokens_kernel<T, true>), grid, dim3(256), 0, st, src, dst, T_total, t0, (int)Tn, (int)C,
                           planes_bf16, vec);
    else
        hipLaunchKernelGGL((transpose_tokens_kernel<T, false>), grid, dim3(256), 0, st, src, dst, T_total, t0, (int)Tn, (int)C,
                           planes_bf16, vec);
    return check_launch(fn);
}

template <typename T>
int maxpool_fwd_launch(const char *fn, const void *x, int64_t planes, int64_t H, int64_t W, void *y, void *idx, void *stream) {
    clear_error();
    if (planes < 0 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    const int64_t Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, total = planes * Ho * Wo;
    if (total == 0) return VAH_OK;
    if (!x || !y || !idx) return fail(VAH_E_NULL, "%s: null pointer", fn);
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope(tname<T>("maxpool_fwd", "maxpool_fwd_f16"), planes * (H * W * 2 + Ho * Wo * 3), st);
    if (planes > 65535 || (Ho + 3) / 4 > 65535) return fail(VAH_E_SHAPE, "%s: too many planes / rows", fn);
    hipLaunchKernelGGL(maxpool3s2_fwd_kernel<T>, dim3((unsigned)((Wo + 63) / 64), (unsigned)((Ho + 3) / 4), (unsigned)planes),
                       dim3(256), 0, st, (const T *)x, (int)H, (int)W, (int)Ho, (int)Wo, (T *)y, (unsigned char *)idx);
    return check_launch(fn);
}

template <typename T>
int maxpool_bwd_launch(const char *fn, const void *gy, const void *idx, int64_t planes, int64_t H, int64_t W, void *gx,
                       void *stream) {
    clear_error();
    if (planes < 0 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    const int64_t Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, total = planes * H * W;
    if (total == 0) return VAH_OK;
    if (!gy || !idx || !gx) return fail(VAH_E_NULL, "%s: null pointer", fn);
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope(tname<T>("maxpool_bwd", "maxpool_bwd_f16"), planes * (H * W * 2 + Ho * Wo * 3), st);
    if (planes > 65535 || (H + 3) / 4 > 65535) return fail(VAH_E_SHAPE, "%s: too many planes / rows", fn);
    if ((uintptr_t)gx % 16) return fail(VAH_E_ALIGN, "%s: misaligned", fn);
    hipLaunchKernelGGL(maxpool3s2_bwd_kernel<T>, dim3((unsigned)((W + 511) / 512), (unsigned)((H + 3) / 4), (unsigned)planes),
                       dim3(256), 0, st, (const T *)gy, (const unsigned char *)idx, (int)H, (int)W, (int)Ho, (int)Wo, (T *)gx);
    return check_launch(fn);
}

template <typename T>
int pixel_shuffle2_launch(const char *fn, const void *src, int64_t B, int64_t C, int64_t h, int64_t w, void *dst, int inverse,
                          const void *add, void *stream) {
    clear_error();
    if (B < 0 || C < 1 || h < 1 || w < 8 || w % 8) return fail(VAH_E_SHAPE, "%s: w must be a multiple of 8", fn);
    if (B == 0) return VAH_OK;
    if (!src || !dst) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (((uintptr_t)src | (uintptr_t)dst) % 16) return fail(VAH_E_ALIGN, "%s: 16-byte alignment", fn);
    const int64_t items = B * C * 2 * h * (w / 8);
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope(tname<T>("pixel_shuffle2", "pixel_shuffle2_f16"), B * C * 4 * h * w * 4, st);
    if (add && (inverse || (uintptr_t)add % 16)) return fail(VAH_E_SHAPE, "%s: add is a forward-only, 16-byte aligned operand", fn);
    if (inverse)
        hipLaunchKernelGGL((pixel_shuffle2_kernel<T, true>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, (const T *)src,
                           (T *)dst, (const T *)nullptr, (int)B, (int)C, (int)h, (int)w, items);
    else
        hipLaunchKernelGGL((pixel_shuffle2_kernel<T, false>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, (const T *)src,
                           (T *)dst, (const T *)add, (int)B, (int)C, (int)h, (int)w, items);
    return check_launch(fn);
}

}  // namespace
}  // namespace vah

extern "C" {

int64_t vah_bn_tail_ws_floats(int64_t C) { return (int64_t)vah::kTailParts * 2 * C; }

int vah_bn_tail_supported(int64_t N, int64_t C, int64_t H, int64_t W, int scale, int has_x) {
    using namespace vah;
    clear_error();
    Operands o;
    return plan_tail("vah_bn_tail_supported", o, has_x != 0, scale, N, C, H, W) == VAH_OK ? 1 : 0;
}

int vah_bn_tail_stats(const void *a, int a_bf16, const void *b, int b_bf16, const float *x, int scale, int64_t N,
                      int64_t C, int64_t H, int64_t W, const float *shift, float *sums, float *ws, void *stream) {
    return vah::tail_stats_launch<__bf16>("vah_bn_tail_stats", a, a_bf16, b, b_bf16, x, scale, N, C, H, W, shift, sums, ws, stream);
}
int vah_bn_tail_stats_f16(const void *a, int a_f16, const void *b, int b_f16, const float *x, int scale, int64_t N,
                          int64_t C, int64_t H, int64_t W, const float *shift, float *sums, float *ws, void *stream) {
    return vah::tail_stats_launch<_Float16>("vah_bn_tail_stats_f16", a, a_f16, b, b_f16, x, scale, N, C, H, W, shift, sums, ws, stream);
}

int vah_bn_tail_apply(const void *a, int a_bf16, const void *b, int b_bf16, const float *x, int scale, int64_t N,
                      int64_t C, int64_t H, int64_t W, const float *mean, const float *rstd, const float *gamma,
                      const float *beta, int relu, const float *shift, void *y, int y_bf16, void *stream) {
    return vah::tail_apply_launch<__bf16>("vah_bn_tail_apply", a, a_bf16, b, b_bf16, x, scale, N, C, H, W, mean, rstd, gamma, beta,
                                          relu, shift, y, y_bf16, stream);
}
int vah_bn_tail_apply_f16(const void *a, int a_f16, const void *b, int b_f16, const float *x, int scale, int64_t N,
                          int64_t C, int64_t H, int64_t W, const float *mean, const float *rstd, const float *gamma,
                          const float *beta, int relu, const float *shift, void *y, int y_f16, void *stream) {
    return vah::tail_apply_launch<_Float16>("vah_bn_tail_apply_f16", a, a_f16, b, b_f16, x, scale, N, C, H, W, mean, rstd, gamma,
                                            beta, relu, shift, y, y_f16, stream);
}

int vah_bn_tail_bwd_stats(const void *a, int a_bf16, const void *b, int b_bf16, const float *x, int scale, int64_t N,
                          int64_t C, int64_t H, int64_t W, const float *mean, const float *rstd, const float *gamma,
                          const float *beta, int relu, const float *shift, const void *dy, int dy_bf16, float *sums,
                          float *ws, void *stream) {
    return vah::tail_bwd_stats_launch<__bf16>("vah_bn_tail_bwd_stats", a, a_bf16, b, b_bf16, x, scale, N, C, H, W, mean, rstd, gamma,
                                              beta, relu, shift, dy, dy_bf16, sums, ws, stream);
}
int vah_bn_tail_bwd_stats_f16(const void *a, int a_f16, const void *b, int b_f16, const float *x, int scale, int64_t N,
                              int64_t C, int64_t H, int64_t W, const float *mean, const float *rstd, const float *gamma,
                              const float *beta, int relu, const float *shift, const void *dy, int dy_f16, float *sums,
                              float *ws, void *stream) {
    return vah::tail_bwd_stats_launch<_Float16>("vah_bn_tail_bwd_stats_f16", a, a_f16, b, b_f16, x, scale, N, C, H, W, mean, rstd,
                                                gamma, beta, relu, shift, dy, dy_f16, sums, ws, stream);
}

int vah_bn_tail_bwd_apply(const void *a, int a_bf16, const void *b, int b_bf16, const float *x, int scale, int64_t N,
                          int64_t C, int64_t H, int64_t W, const float *mean, const float *rstd, const float *gamma,
                          const float *beta, int relu, const float *shift, const void *dy, int dy_bf16, const float *mdy,
                          const float *mdyx, void *da, void *db, float *dxlo, void *stream) {
    return vah::tail_bwd_apply_launch<__bf16>("vah_bn_tail_bwd_apply", a, a_bf16, b, b_bf16, x, scale, N, C, H, W, mean, rstd, gamma,
                                              beta, relu, shift, dy, dy_bf16, mdy, mdyx, da, db, dxlo, stream);
}
int vah_bn_tail_bwd_apply_f16(const void *a, int a_f16, const void *b, int b_f16, const float *x, int scale, int64_t N,
                              int64_t C, int64_t H, int64_t W, const float *mean, const float *rstd, const float *gamma,
                              const float *beta, int relu, const float *shift, const void *dy, int dy_f16, const float *mdy,
                              const float *mdyx, void *da, void *db, float *dxlo, void *stream) {
    return vah::tail_bwd_apply_launch<_Float16>("vah_bn_tail_bwd_apply_f16", a, a_f16, b, b_f16, x, scale, N, C, H, W, mean, rstd,
                                                gamma, beta, relu, shift, dy, dy_f16, mdy, mdyx, da, db, dxlo, stream);
}

// sums = [sum (C) | sum of squares (C) | element count (1)] (as written by vah_bn_tail_stats plus the
// count, all-reduced over the ranks for SyncBatchNorm) -> mean, rstd; running statistics updated in
// place when given (momentum, unbiased variance), as torch.nn.BatchNorm does in training.
int vah_bn_finalize_stats(const float *sums, int64_t C, float eps, float momentum, float *running_mean,
                          float *running_var, float *mean, float *rstd, void *stream) {
    using namespace vah;
    clear_error();
    const char *fn = "vah_bn_finalize_stats";
    if (C < 1) return fail(VAH_E_SHAPE, "%s: bad C", fn);
    if (!sums || !mean || !rstd || ((running_mean != nullptr) != (running_var != nullptr))) return fail(VAH_E_NULL, "%s: null pointer", fn);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sums, (int)C, eps,
                       momentum, running_mean, running_var, mean, rstd);
    return check_launch(fn);
}

// vah_bn_finalize_stats with the bookkeeping of a BatchNorm that has no process group in the same launch
// (include/vitadapter_hip_epoch.h): count -> sums[2 * C], num_batches_tracked += 1 (null: nothing tracked).
int vah_bn_finalize_stats_book(float *sums, int64_t C, float count, float eps, float momentum, float *running_mean,
                               float *running_var, float *mean, float *rstd, int64_t *num_batches_tracked, void *stream) {
    using namespace vah;
    clear_error();
    const char *fn = "vah_bn_finalize_stats_book";
    if (C < 1 || C > (1 << 24)) return fail(VAH_E_SHAPE, "%s: bad C", fn);
    if (!sums || !mean || !rstd || ((running_mean != nullptr) != (running_var != nullptr))) return fail(VAH_E_NULL, "%s: null pointer", fn);
    hipLaunchKernelGGL(bn_finalize_book_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sums, (int)C,
                       count, eps, momentum, running_mean, running_var, mean, rstd, num_batches_tracked);
    return check_launch(fn);
}

// tokens -> planes (to_planes != 0): dst (B, C, T) <- src (B, T_total, C)[:, t0 : t0 + T, :];
// planes -> tokens: dst (B, T_total, C)[:, t0 : t0 + T, :] <- src (B, C, T) (+ vec[C] if given).
// Tokens are fp32; the planes fp32 or 16-bit (planes_bf16: bf16, or fp16 for the `_f16` entry).
// Replaces  c[:, a:b].transpose(1, 2).view(B, C, H, W).contiguous()  of the pyramid assembly
// (vit_adapter.py:113-119) and  cat([fc_l(c_l).flatten(2).transpose(1, 2) + level_embed[l]])  of
// vit_adapter.py:94-97 / adapter_modules.py:262-268, and their backward passes.
int vah_transpose_tokens(const void *src, int64_t B, int64_t T_total, int64_t t0, int64_t T, int64_t C, void *dst,
                         int to_planes, int planes_bf16, const float *vec, void *stream) {
    return vah::transpose_tokens_launch<__bf16>("vah_transpose_tokens", src, B, T_total, t0, T, C, dst, to_planes, planes_bf16, vec,
                                                stream);
}
int vah_transpose_tokens_f16(const void *src, int64_t B, int64_t T_total, int64_t t0, int64_t T, int64_t C, void *dst,
                             int to_planes, int planes_f16, const float *vec, void *stream) {
    return vah::transpose_tokens_launch<_Float16>("vah_transpose_tokens_f16", src, B, T_total, t0, T, C, dst, to_planes, planes_f16,
                                                  vec, stream);
}

// MaxPool2d(3, stride 2, padding 1) on 16-bit NCHW (planes = N * C): y, idx (1 byte per output: window position
// of the first maximum) <- x;  backward: gx <- gy, idx (gather, no atomics).
int vah_maxpool3s2_fwd_bf16(const void *x, int64_t planes, int64_t H, int64_t W, void *y, void *idx, void *stream) {
    return vah::maxpool_fwd_launch<__bf16>("vah_maxpool3s2_fwd_bf16", x, planes, H, W, y, idx, stream);
}
int vah_maxpool3s2_fwd_f16(const void *x, int64_t planes, int64_t H, int64_t W, void *y, void *idx, void *stream) {
    return vah::maxpool_fwd_launch<_Float16>("vah_maxpool3s2_fwd_f16", x, planes, H, W, y, idx, stream);
}

int vah_maxpool3s2_bwd_bf16(const void *gy, const void *idx, int64_t planes, int64_t H, int64_t W, void *gx, void *stream) {
    return vah::maxpool_bwd_launch<__bf16>("vah_maxpool3s2_bwd_bf16", gy, idx, planes, H, W, gx, stream);
}
int vah_maxpool3s2_bwd_f16(const void *gy, const void *idx, int64_t planes, int64_t H, int64_t W, void *gx, void *stream) {
    return vah::maxpool_bwd_launch<_Float16>("vah_maxpool3s2_bwd_f16", gy, idx, planes, H, W, gx, stream);
}

/* inverse == 0: planes (B, C, 2h, 2w) <- U (B, 4*C, h*w), rows (dy, dx, co) [+ add, planes-shaped, optional];
 * inverse != 0: U <- planes.  bf16 (fp16: the `_f16` entry), w % 8 == 0. */
int vah_pixel_shuffle2_bf16(const void *src, int64_t B, int64_t C, int64_t h, int64_t w, void *dst, int inverse, const void *add,
                            void *stream) {
    return vah::pixel_shuffle2_launch<__bf16>("vah_pixel_shuffle2_bf16", src, B, C, h, w, dst, inverse, add, stream);
}
int vah_pixel_shuffle2_f16(const void *src, int64_t B, int64_t C, int64_t h, int64_t w, void *dst, int inverse, const void *add,
                           void *stream) {
    return vah::pixel_shuffle2_launch<_Float16>("vah_pixel_shuffle2_f16", src, B, C, h, w, dst, inverse, add, stream);
}

}  // extern "C"
