// Masked cross-attention of Mask2Former's query decoder (include/vitadapter_hip_masked_attn.h): Lq <= 128 queries attend to
// the Lk keys of one pyramid level, heads of 32 channels, under one keep-bit per (image, query, key) - the reference's
// segmentation/mmseg_custom/models/decode_heads/mask2former_head.py:404-525, which repeats a bool mask over the heads,
// materialises the scores and repairs all-excluded rows with a torch.where (a host synchronisation).
//
// With N * H = 16 sequences and 100 queries a (head, image) grid cannot fill the chip, so the keys are cut into chunks of
// whole 64-key tiles (mca_rule) and a workgroup owns (chunk, head, image) and ALL queries: 4 waves x 32 query rows.
//   * pack: one workgroup per row of logits; a wave ballots 64 keys into two words; a row that keeps nothing is rewritten
//     as all ones below Lk.  Bits >= Lk are 0, so the attention kernels need no test against Lk.
//   * forward: scores transposed (keys on the MFMA rows, a lane's column is one query) as in attn_flash.hip, so the 32 keys
//     of a block are the 32 bits of one mask word per lane.  Online softmax per chunk; an all-excluded chunk keeps
//     m = -inf, l = 0 (the exponent's offset is then 0, never -inf - -inf).  Partials (o, m, l) in fp32, merged in ascending
//     chunk order by a second launch; one chunk writes out and lse directly.
//   * backward: q and dO of all queries stay in registers, P is recomputed from lse in BOTH orientations: keys on the rows
//     (dS^T is then the B operand of dQ^T += K^T dS^T, accumulated over the chunk) and queries on the rows (P and dS are
//     then the B operands of dV^T = dO^T P and dK^T = Q^T dS).  The second orientation is the first with the MFMA operands
//     swapped - the same registers - and costs 4 MFMAs and 16 exp2 per block against a round trip of dS through LDS.
//     dV^T and dK^T of a tile are summed over the four waves through LDS, wave 0 first, and stored once; the chunk's dQ
//     goes to the workspace and a last launch sums the chunks in ascending order.
// Launches are ordered by the stream alone: no atomics, counters or flags.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vitadapter_hip_masked_attn.h"
#include "attn_common.h"
#include "common.h"

namespace vah {
namespace {

using attn::pack_half;

constexpr int kD = 32;             // head dim
constexpr int kKT = 64;            // keys per tile
constexpr int kPad = 40;           // LDS row stride (elements) of a [rows][32] tile: 80 B, 16-byte aligned rows
constexpr int kMaxQ = 128;         // queries per workgroup
constexpr int kMaxSplits = 16;
constexpr int kRedPad = 65;        // LDS row stride (floats) of a [32 d][64 keys] partial
constexpr float kLog2e = 1.4426950408889634f;

struct Rule {
    int64_t tiles_per_chunk, splits;
};
Rule mca_rule(int64_t Lk) {
    const int64_t tiles = (Lk + kKT - 1) / kKT;
    const int64_t want = tiles < kMaxSplits ? tiles : kMaxSplits;
    Rule r;
    r.tiles_per_chunk = (tiles + want - 1) / want;
    r.splits = (tiles + r.tiles_per_chunk - 1) / r.tiles_per_chunk;
    return r;
}
int64_t mca_ws_floats(int64_t N, int64_t H, int64_t Lq, int64_t Lk) {
    const int64_t R = N * H * Lq, S = mca_rule(Lk).splits;
    return (R + 3) / 4 * 4 + 34 * R * S;
}

// lane base for the transposed reads of a row-major [token][32] tile (elem16.h tr_frag): the 16-lane group g covers rows
// 4 (g >> 1) + 0..3 and columns 16 (g & 1) + 0..15, so the lane ends up with column (lane & 31)
template <typename T>
__device__ __forceinline__ const T *tile_lane_base(const T *tile, int lane) {
    const int grp = lane >> 4, i16 = lane & 15;
    return tile + (4 * (grp >> 1) + (i16 >> 2)) * kPad + 16 * (grp & 1) + 4 * (i16 & 3);
}
// A operand X^T[m = d][k = token] of a row-major LDS tile X[token][d] in the k order of pack_half
template <typename T>
__device__ __forceinline__ vec8<T> load_tr(const T *base, int tok0) {
    const T *p0 = base + tok0 * kPad;
    return tr_frag<T>(p0, p0 + 8 * kPad);
}
// across the two 32-lane halves (attn_flash.hip)
__device__ __forceinline__ float max_halves(float x) {
    float a = x, b = x;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}

// ---------------------------------------------------------------------------------------------------------------------
// pack
// ---------------------------------------------------------------------------------------------------------------------
template <typename TX>
__global__ __launch_bounds__(256) void mca_pack_kernel(const TX *__restrict__ x, int64_t rs, int64_t is, int Q, int Lk, int W,
                                                       uint32_t *__restrict__ bits) {
    __shared__ int s_any[4];
    const int row = blockIdx.x, n = row / Q, qi = row - n * Q;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const TX *xr = x + (int64_t)n * is + (int64_t)qi * rs;
    uint32_t *br = bits + (int64_t)row * W;
    const int nblk = (Lk + 63) / 64;
    bool any = false;
    for (int b = wave; b < nblk; b += 4) {
        const int j = b * 64 + lane;
        bool keep = false;
        if (j < Lk) keep = !((float)xr[j] < 0.f);
        const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
        any |= m != 0ull;
        if (lane == 0) {
            br[2 * b] = (uint32_t)m;
            if (2 * b + 1 < W) br[2 * b + 1] = (uint32_t)(m >> 32);
        }
    }
    if (lane == 0) s_any[wave] = any;
    __syncthreads();
    if (s_any[0] | s_any[1] | s_any[2] | s_any[3]) return;
    // nothing kept: keep everything.  The same lane rewrites the words it wrote above.
    for (int b = wave; b < nblk; b += 4) {
        if (lane == 0) {
            const int left = Lk - b * 64;             // >= 1
            const unsigned long long m = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
            br[2 * b] = (uint32_t)m;
            if (2 * b + 1 < W) br[2 * b + 1] = (uint32_t)(m >> 32);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mca_fwd_kernel(const T *__restrict__ q, int64_t q_ts, int64_t q_is,
                                                      const T *__restrict__ k, int64_t k_ts, int64_t k_is,
                                                      const T *__restrict__ v, int64_t v_ts, int64_t v_is,
                                                      const uint32_t *__restrict__ bits, int Lq, int Lk, int W, int H,
                                                      int tiles_per_chunk, int S, float scale_log2, T *__restrict__ out,
                                                      int64_t o_ts, int64_t o_is, float *__restrict__ lse,
                                                      float *__restrict__ part_o, float *__restrict__ part_m,
                                                      float *__restrict__ part_l) {
    __shared__ __attribute__((aligned(16))) T s_k2[2][kKT * kPad];
    __shared__ __attribute__((aligned(16))) T s_v2[2][kKT * kPad];
    const int c = blockIdx.x, h = blockIdx.y, n = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, hf = lane >> 5;
    const int qrow = wave * 32 + r, qc = min(qrow, Lq - 1);
    const bool active = wave * 32 < Lq;                 // wave-uniform
    const int key_begin = c * tiles_per_chunk * kKT;
    const int key_end = min(Lk, key_begin + tiles_per_chunk * kKT);
    const int ntiles = (key_end - key_begin + kKT - 1) / kKT;

    vec8<T> qf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
        qf[kk] = *reinterpret_cast<const vec8<T> *>(q + (int64_t)qc * q_ts + (int64_t)n * q_is + h * kD + 16 * kk + 8 * hf);
    const uint32_t *brow = bits + ((int64_t)n * Lq + qc) * W;

    // staging: 256 pieces of 16 bytes per tile and matrix, one per thread
    const int sr = threadIdx.x >> 2, sc = (threadIdx.x & 3) * 8;
    const T *kp = k + (int64_t)n * k_is + h * kD + sc, *vp = v + (int64_t)n * v_is + h * kD + sc;
    vec8<T> pk, pv;
    auto fetch = [&](int key0) {
        const int64_t g = min(key0 + sr, Lk - 1);
        pk = *reinterpret_cast<const vec8<T> *>(kp + g * k_ts);
        pv = *reinterpret_cast<const vec8<T> *>(vp + g * v_ts);
    };
    auto commit = [&](int buf) {
        *reinterpret_cast<vec8<T> *>(s_k2[buf] + sr * kPad + sc) = pk;
        *reinterpret_cast<vec8<T> *>(s_v2[buf] + sr * kPad + sc) = pv;
    };
    auto words = [&](int key0, uint32_t (&w)[2]) {      // this lane's query, keys key0 .. key0 + 63, shifted to its half
        const int w0 = key0 >> 5;
        w[0] = brow[w0] >> (4 * hf);
        w[1] = (w0 + 1 < W ? brow[w0 + 1] : 0u) >> (4 * hf);
    };

    f32x16 o = zero16(), lsum = zero16();
    vec8<T> ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (T)1.f;
    float m_run = -INFINITY;
    uint32_t mw[2], mw_next[2] = {0u, 0u};
    fetch(key_begin);
    commit(0);
    if (ntiles > 1) fetch(key_begin + kKT);
    words(key_begin, mw);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                 // tile t visible; every wave is done with tile t - 1
        if (t + 1 < ntiles) {
            commit((t + 1) & 1);
            if (t + 2 < ntiles) fetch(key_begin + (t + 2) * kKT);
            words(key_begin + (t + 1) * kKT, mw_next);
        }
        if (active) {
            const T *s_k = s_k2[t & 1];
            const T *vbase = tile_lane_base(s_v2[t & 1], lane);
            f32x16 s[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                s[kb] = zero16();
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
                    s[kb] = mfma(*reinterpret_cast<const vec8<T> *>(s_k + (kb * 32 + r) * kPad + 16 * kk + 8 * hf), qf[kk], s[kb]);
            }
            // log2-domain scores; excluded keys (and keys >= Lk, whose bits are 0) at -inf
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const bool keep = (mw[kb] >> ((i & 3) + 8 * (i >> 2))) & 1u;
                    s[kb][i] = keep ? s[kb][i] * scale_log2 : -INFINITY;
                    mx = fmaxf(mx, s[kb][i]);
                }
            mx = max_halves(mx);
            const float m_new = fmaxf(m_run, mx);
            if (__builtin_amdgcn_ballot_w64(m_new > m_run)) {                // some row's maximum moved: rescale
                // a row still at -inf keeps alpha = 1 (its o and l are 0); -inf - -inf is never formed
                const float alpha = m_new > m_run ? __builtin_amdgcn_exp2f(m_run - m_new) : 1.f;
                lsum[0] *= alpha;                                             // every row of lsum is the same sum: row 0 is read
#pragma unroll
                for (int i = 0; i < 16; ++i) o[i] *= alpha;
                m_run = m_new;
            }
            const float m_use = m_run == -INFINITY ? 0.f : m_run;             // nothing kept so far: exp2(-inf - 0) = 0
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) s[kb][i] = __builtin_amdgcn_exp2f(s[kb][i] - m_use);
            // O^T += V^T P^T; the row sums of the same T-rounded P ride along as a block whose A operand is all ones
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int sp = 0; sp < 2; ++sp) {
                    const vec8<T> pf = pack_half<T>(s[kb], sp);
                    o = mfma(load_tr(vbase, kb * 32 + 16 * sp), pf, o);
                    lsum = mfma(ones, pf, lsum);
                }
        }
        mw[0] = mw_next[0];
        mw[1] = mw_next[1];
    }

    if (!active || qrow >= Lq) return;
    const float l_tot = lsum[0];
    if (S == 1) {
        const float inv = 1.f / l_tot;
        T *op = out + (int64_t)qrow * o_ts + (int64_t)n * o_is + h * kD;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            vec4<T> w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = (T)(o[4 * g + j] * inv);
            *reinterpret_cast<vec4<T> *>(op + 8 * g + 4 * hf) = w;
        }
        if (hf == 0) lse[((int64_t)n * H + h) * Lq + qrow] = m_run + log2f(l_tot);
    } else {
        const int64_t row = (((int64_t)n * H + h) * S + c) * Lq + qrow;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4 *>(part_o + row * kD + 8 * g + 4 * hf) =
                make_float4(o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]);
        if (hf == 0) {
            part_m[row] = m_run;
            part_l[row] = l_tot;
        }
    }
}

// merge the chunks of a row in ascending order: 8 threads per row, 4 channels each
template <typename T>
__global__ __launch_bounds__(256) void mca_fwd_merge_kernel(const float *__restrict__ part_o, const float *__restrict__ part_m,
                                                            const float *__restrict__ part_l, int64_t rows, int Lq, int H, int S,
                                                            T *__restrict__ out, int64_t o_ts, int64_t o_is,
                                                            float *__restrict__ lse) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = idx >> 3;
    const int g = (int)(idx & 7);
    if (row >= rows) return;
    const int64_t nh = row / Lq;
    const int qi = (int)(row - nh * Lq), n = (int)(nh / H), h = (int)(nh - (int64_t)n * H);
    float M = -INFINITY;
    for (int s = 0; s < S; ++s) M = fmaxf(M, part_m[(nh * S + s) * Lq + qi]);
    float L = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int s = 0; s < S; ++s) {
        const int64_t pr = (nh * S + s) * Lq + qi;
        const float m = part_m[pr];
        if (m == -INFINITY) continue;                   // a chunk without a kept key: o = 0, l = 0
        const float w = __builtin_amdgcn_exp2f(m - M);
        const float4 po = *reinterpret_cast<const float4 *>(part_o + pr * kD + 4 * g);
        L += w * part_l[pr];
        a0 += w * po.x, a1 += w * po.y, a2 += w * po.z, a3 += w * po.w;
    }
    const float inv = 1.f / L;
    vec4<T> w4;
    w4[0] = (T)(a0 * inv), w4[1] = (T)(a1 * inv), w4[2] = (T)(a2 * inv), w4[3] = (T)(a3 * inv);
    *reinterpret_cast<vec4<T> *>(out + (int64_t)qi * o_ts + (int64_t)n * o_is + h * kD + 4 * g) = w4;
    if (g == 0) lse[row] = M + log2f(L);
}

// ---------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------
// delta[n][h][q] = sum_d dO o O: one thread per row
template <typename T>
__global__ __launch_bounds__(256) void mca_delta_kernel(const T *__restrict__ o, int64_t o_ts, int64_t o_is,
                                                        const T *__restrict__ d_o, int64_t g_ts, int64_t g_is, int64_t rows, int Lq,
                                                        int H, float *__restrict__ delta) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const int64_t nh = row / Lq;
    const int qi = (int)(row - nh * Lq), n = (int)(nh / H), h = (int)(nh - (int64_t)n * H);
    const T *po = o + (int64_t)qi * o_ts + (int64_t)n * o_is + h * kD, *pg = d_o + (int64_t)qi * g_ts + (int64_t)n * g_is + h * kD;
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const vec8<T> a = *reinterpret_cast<const vec8<T> *>(po + 8 * c), b = *reinterpret_cast<const vec8<T> *>(pg + 8 * c);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += (float)a[j] * (float)b[j];
    }
    delta[row] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void mca_bwd_kernel(const T *__restrict__ q, int64_t q_ts, int64_t q_is,
                                                      const T *__restrict__ k, int64_t k_ts, int64_t k_is,
                                                      const T *__restrict__ v, int64_t v_ts, int64_t v_is,
                                                      const uint32_t *__restrict__ bits, const T *__restrict__ d_o, int64_t g_ts,
                                                      int64_t g_is, const float *__restrict__ lse, const float *__restrict__ delta,
                                                      int Lq, int Lk, int W, int H, int tiles_per_chunk, int S, float scale,
                                                      float scale_log2, T *__restrict__ dq, int64_t dq_ts, int64_t dq_is,
                                                      T *__restrict__ dk, int64_t dk_ts, int64_t dk_is, T *__restrict__ dv,
                                                      int64_t dv_ts, int64_t dv_is, float *__restrict__ dq_part) {
    __shared__ __attribute__((aligned(16))) T s_q[kMaxQ * kPad];
    __shared__ __attribute__((aligned(16))) T s_do[kMaxQ * kPad];
    __shared__ __attribute__((aligned(16))) T s_k[kKT * kPad];
    __shared__ __attribute__((aligned(16))) T s_v[kKT * kPad];
    __shared__ uint32_t s_mask[kMaxQ * 2];
    __shared__ float s_red[2][4][kD * kRedPad];          // [dV, dK][wave][d][key]
    const int c = blockIdx.x, h = blockIdx.y, n = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, hf = lane >> 5;
    const int qrow = wave * 32 + r;
    const int nwaves = (Lq + 31) / 32;
    const bool active = wave < nwaves;                  // wave-uniform
    const int key_begin = c * tiles_per_chunk * kKT;
    const int key_end = min(Lk, key_begin + tiles_per_chunk * kKT);
    const int ntiles = (key_end - key_begin + kKT - 1) / kKT;
    const int64_t nh = (int64_t)n * H + h;

    // q and dO of all queries -> LDS once (rows >= Lq clamped), then into registers in both operand forms
    for (int p = threadIdx.x; p < kMaxQ * 4; p += 256) {
        const int row = p >> 2, col = (p & 3) * 8;
        const int64_t qi = min(row, Lq - 1);
        *reinterpret_cast<vec8<T> *>(s_q + row * kPad + col) =
            *reinterpret_cast<const vec8<T> *>(q + qi * q_ts + (int64_t)n * q_is + h * kD + col);
        *reinterpret_cast<vec8<T> *>(s_do + row * kPad + col) =
            *reinterpret_cast<const vec8<T> *>(d_o + qi * g_ts + (int64_t)n * g_is + h * kD + col);
    }
    __syncthreads();
    vec8<T> qf[2], dof[2], qT[2], doT[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        qf[kk] = *reinterpret_cast<const vec8<T> *>(s_q + qrow * kPad + 16 * kk + 8 * hf);
        dof[kk] = *reinterpret_cast<const vec8<T> *>(s_do + qrow * kPad + 16 * kk + 8 * hf);
        qT[kk] = load_tr(tile_lane_base(s_q + wave * 32 * kPad, lane), 16 * kk);       // Q^T[d = r][q in k order]
        doT[kk] = load_tr(tile_lane_base(s_do + wave * 32 * kPad, lane), 16 * kk);
    }
    // softmax statistics: of this lane's query (keys on the rows) and of the 16 queries of its registers (queries on the
    // rows); lse = +inf for rows that do not exist: P = 0
    const float lse_q = qrow < Lq ? lse[nh * Lq + qrow] : INFINITY, delta_q = qrow < Lq ? delta[nh * Lq + qrow] : 0.f;
    float lse_r[16], delta_r[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int qi = wave * 32 + crow(i, hf);
        lse_r[i] = qi < Lq ? lse[nh * Lq + qi] : INFINITY;
        delta_r[i] = qi < Lq ? delta[nh * Lq + qi] : 0.f;
    }

    const int sr = threadIdx.x >> 2, sc = (threadIdx.x & 3) * 8;
    const T *kp = k + (int64_t)n * k_is + h * kD + sc, *vp = v + (int64_t)n * v_is + h * kD + sc;
    const int mq = min((int)(threadIdx.x >> 1), Lq - 1), mkb = threadIdx.x & 1;
    const uint32_t *brow = bits + ((int64_t)n * Lq + mq) * W;
    vec8<T> pk, pv;
    uint32_t pm = 0u;
    auto fetch = [&](int key0) {
        const int64_t g = min(key0 + sr, Lk - 1);
        pk = *reinterpret_cast<const vec8<T> *>(kp + g * k_ts);
        pv = *reinterpret_cast<const vec8<T> *>(vp + g * v_ts);
        const int w = (key0 >> 5) + mkb;
        pm = w < W ? brow[w] : 0u;
    };

    f32x16 dqt = zero16();
    fetch(key_begin);
    for (int t = 0; t < ntiles; ++t) {
        const int key0 = key_begin + t * kKT;
        __syncthreads();                 // every wave is done with tile t - 1 and with its partials
        *reinterpret_cast<vec8<T> *>(s_k + sr * kPad + sc) = pk;
        *reinterpret_cast<vec8<T> *>(s_v + sr * kPad + sc) = pv;
        s_mask[threadIdx.x] = pm;        // [query][block]
        if (t + 1 < ntiles) fetch(key0 + kKT);
        __syncthreads();
        if (active) {
            const T *kbase = tile_lane_base(s_k, lane);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                vec8<T> kf[2], vf[2];
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    kf[kk] = *reinterpret_cast<const vec8<T> *>(s_k + (kb * 32 + r) * kPad + 16 * kk + 8 * hf);
                    vf[kk] = *reinterpret_cast<const vec8<T> *>(s_v + (kb * 32 + r) * kPad + 16 * kk + 8 * hf);
                }
                {   // keys on the rows, this lane's query: dQ^T[d][q] += K^T dS^T
                    f32x16 s = zero16(), dp = zero16();
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        s = mfma(kf[kk], qf[kk], s);
                        dp = mfma(vf[kk], dof[kk], dp);
                    }
                    const uint32_t mw = s_mask[qrow * 2 + kb] >> (4 * hf);
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const bool keep = (mw >> ((i & 3) + 8 * (i >> 2))) & 1u;
                        const float p = keep ? __builtin_amdgcn_exp2f(s[i] * scale_log2 - lse_q) : 0.f;
                        s[i] = keep ? p * (dp[i] - delta_q) : 0.f;
                    }
#pragma unroll
                    for (int sp = 0; sp < 2; ++sp) dqt = mfma(load_tr(kbase, kb * 32 + 16 * sp), pack_half<T>(s, sp), dqt);
                }
                {   // queries on the rows, this lane's key: dV^T[d][key] = dO^T P, dK^T[d][key] = Q^T dS
                    f32x16 s = zero16(), dp = zero16();
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        s = mfma(qf[kk], kf[kk], s);
                        dp = mfma(dof[kk], vf[kk], dp);
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const bool keep = (s_mask[(wave * 32 + crow(i, hf)) * 2 + kb] >> r) & 1u;
                        const float p = keep ? __builtin_amdgcn_exp2f(s[i] * scale_log2 - lse_r[i]) : 0.f;
                        s[i] = p;
                        dp[i] = keep ? p * (dp[i] - delta_r[i]) : 0.f;
                    }
                    f32x16 dvt = zero16(), dkt = zero16();
#pragma unroll
                    for (int sp = 0; sp < 2; ++sp) {
                        dvt = mfma(doT[sp], pack_half<T>(s, sp), dvt);
                        dkt = mfma(qT[sp], pack_half<T>(dp, sp), dkt);
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        s_red[0][wave][crow(i, hf) * kRedPad + kb * 32 + r] = dvt[i];
                        s_red[1][wave][crow(i, hf) * kRedPad + kb * 32 + r] = dkt[i] * scale;
                    }
                }
            }
        }
        __syncthreads();
        // sum over the waves, wave 0 first; a thread owns 8 channels of one key for dV and dK
        {
            const int key = threadIdx.x >> 2, d8 = (threadIdx.x & 3) * 8;
            if (key0 + key < key_end) {
#pragma unroll
                for (int mat = 0; mat < 2; ++mat) {
                    vec8<T> w8;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float acc = s_red[mat][0][(d8 + j) * kRedPad + key];
                        for (int w = 1; w < nwaves; ++w) acc += s_red[mat][w][(d8 + j) * kRedPad + key];
                        w8[j] = (T)acc;
                    }
                    T *dst = mat == 0 ? dv + (int64_t)(key0 + key) * dv_ts + (int64_t)n * dv_is
                                      : dk + (int64_t)(key0 + key) * dk_ts + (int64_t)n * dk_is;
                    *reinterpret_cast<vec8<T> *>(dst + h * kD + d8) = w8;
                }
            }
        }
    }

    if (!active || qrow >= Lq) return;
    if (S == 1) {
        T *op = dq + (int64_t)qrow * dq_ts + (int64_t)n * dq_is + h * kD;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            vec4<T> w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = (T)(dqt[4 * g + j] * scale);
            *reinterpret_cast<vec4<T> *>(op + 8 * g + 4 * hf) = w;
        }
    } else {
        const int64_t row = ((nh * S) + c) * Lq + qrow;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4 *>(dq_part + row * kD + 8 * g + 4 * hf) =
                make_float4(dqt[4 * g] * scale, dqt[4 * g + 1] * scale, dqt[4 * g + 2] * scale, dqt[4 * g + 3] * scale);
    }
}

// dq = sum of the chunks' parts in ascending order: 8 threads per row, 4 channels each
template <typename T>
__global__ __launch_bounds__(256) void mca_dq_reduce_kernel(const float *__restrict__ dq_part, int64_t rows, int Lq, int H, int S,
                                                            T *__restrict__ dq, int64_t dq_ts, int64_t dq_is) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = idx >> 3;
    const int g = (int)(idx & 7);
    if (row >= rows) return;
    const int64_t nh = row / Lq;
    const int qi = (int)(row - nh * Lq), n = (int)(nh / H), h = (int)(nh - (int64_t)n * H);
    float4 acc = *reinterpret_cast<const float4 *>(dq_part + ((nh * S) * Lq + qi) * kD + 4 * g);
    for (int s = 1; s < S; ++s) {
        const float4 p = *reinterpret_cast<const float4 *>(dq_part + ((nh * S + s) * Lq + qi) * kD + 4 * g);
        acc.x += p.x, acc.y += p.y, acc.z += p.z, acc.w += p.w;
    }
    vec4<T> w4;
    w4[0] = (T)acc.x, w4[1] = (T)acc.y, w4[2] = (T)acc.z, w4[3] = (T)acc.w;
    *reinterpret_cast<vec4<T> *>(dq + (int64_t)qi * dq_ts + (int64_t)n * dq_is + h * kD + 4 * g) = w4;
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
struct Operand {
    const char *name;
    const void *ptr;
    int dt;
    int64_t ts, is;
};

// the checks both directions share; *empty: nothing to do
int mca_check(const char *fn, const Operand *ops, int nops, const void *bits, const void *lse, int64_t N, int64_t H, int64_t Lq,
              int64_t Lk, int64_t D, const void *ws, int64_t ws_bytes, bool *empty) {
    *empty = false;
    if (N < 0 || H < 1 || Lq < 0 || Lk < 0 || N > 65535 || H > 65535 || Lk >= ((int64_t)1 << 30))
        return fail(VAH_E_SHAPE, "%s: bad dims (N %lld, H %lld, Lq %lld, Lk %lld)", fn, (long long)N, (long long)H, (long long)Lq,
                    (long long)Lk);
    if (D != kD) return fail(VAH_E_UNSUPPORTED, "%s: head_dim must be 32 (head_dim %lld)", fn, (long long)D);
    if (Lq > kMaxQ) return fail(VAH_E_UNSUPPORTED, "%s: at most 128 queries (Lq %lld)", fn, (long long)Lq);
    bool bf = false, fp = false;
    for (int i = 0; i < nops; ++i) {
        if (ops[i].dt == 0) return fail(VAH_E_UNSUPPORTED, "%s: fp32 operands are not served (%s)", fn, ops[i].name);
        if (ops[i].dt < 0 || ops[i].dt > 2) return fail(VAH_E_UNSUPPORTED, "%s: dtype codes are 1 (bf16), 2 (fp16) (%s)", fn, ops[i].name);
        bf |= ops[i].dt == 1, fp |= ops[i].dt == 2;
    }
    if (bf && fp) return fail(VAH_E_UNSUPPORTED, "%s: fp16 mixed with bf16", fn);
    if (N * H * Lq == 0) {
        *empty = true;
        return 0;
    }
    if (Lk == 0) return fail(VAH_E_SHAPE, "%s: bad dims (no keys for %lld queries)", fn, (long long)Lq);
    for (int i = 0; i < nops; ++i) {
        if (!ops[i].ptr) return fail(VAH_E_NULL, "%s: null pointer (%s)", fn, ops[i].name);
        if ((uintptr_t)ops[i].ptr % 16 || ops[i].ts % 8 || ops[i].is % 8)
            return fail(VAH_E_ALIGN, "%s: %s misaligned (16-byte pointer, strides in multiples of 8)", fn, ops[i].name);
        if (ops[i].ts < 0 || ops[i].is < 0) return fail(VAH_E_SHAPE, "%s: %s strides (negative)", fn, ops[i].name);
    }
    if (!bits) return fail(VAH_E_NULL, "%s: null pointer (bits)", fn);
    if (!lse) return fail(VAH_E_NULL, "%s: null pointer (lse)", fn);
    if ((uintptr_t)bits % 4 || (uintptr_t)lse % 4) return fail(VAH_E_ALIGN, "%s: bits / lse misaligned (4-byte pointer)", fn);
    if (!ws) return fail(VAH_E_NULL, "%s: null pointer (ws)", fn);
    if ((uintptr_t)ws % 16) return fail(VAH_E_ALIGN, "%s: ws misaligned (16-byte pointer)", fn);
    if (ws_bytes < (mca_ws_floats(N, H, Lq, Lk) + 3) / 4 * 16) return fail(VAH_E_SHAPE, "%s: workspace too small", fn);
    return 0;
}

template <typename T>
int mca_forward_t(const Operand &q, const Operand &k, const Operand &v, const uint32_t *bits, int64_t N, int64_t H, int64_t Lq,
                  int64_t Lk, float scale, const Operand &out, float *lse, float *ws, hipStream_t st) {
    const Rule rule = mca_rule(Lk);
    const int S = (int)rule.splits, W = (int)((Lk + 31) / 32);
    const int64_t R = N * H * Lq;
    float *part_o = ws, *part_m = ws + R * S * kD, *part_l = part_m + R * S;
    {
        LaunchScope scope(tname<T>("mca_fwd", "mca_fwd_f16"), (2 * N * H * Lk * kD + 2 * S * R * kD) * 2 + S * N * Lq * W * 4, st, 0,
                          4 * N * H * Lq * Lk * kD);
        hipLaunchKernelGGL((mca_fwd_kernel<T>), dim3((unsigned)S, (unsigned)H, (unsigned)N), dim3(256), 0, st, (const T *)q.ptr, q.ts,
                           q.is, (const T *)k.ptr, k.ts, k.is, (const T *)v.ptr, v.ts, v.is, bits, (int)Lq, (int)Lk, W, (int)H,
                           (int)rule.tiles_per_chunk, S, scale * kLog2e, (T *)out.ptr, out.ts, out.is, lse, part_o, part_m, part_l);
        if (int rc = check_launch("vah_mca_forward")) return rc;
    }
    if (S == 1) return 0;
    LaunchScope scope(tname<T>("mca_fwd_merge", "mca_fwd_merge_f16"), R * S * 34 * 4 + R * (kD * 2 + 4), st);
    hipLaunchKernelGGL((mca_fwd_merge_kernel<T>), dim3((unsigned)((R * 8 + 255) / 256)), dim3(256), 0, st, part_o, part_m, part_l, R,
                       (int)Lq, (int)H, S, (T *)out.ptr, out.ts, out.is, lse);
    return check_launch("vah_mca_forward");
}

template <typename T>
int mca_backward_t(const Operand &q, const Operand &k, const Operand &v, const uint32_t *bits, const Operand &o, const Operand &g,
                   const float *lse, int64_t N, int64_t H, int64_t Lq, int64_t Lk, float scale, const Operand &dq, const Operand &dk,
                   const Operand &dv, float *ws, hipStream_t st) {
    const Rule rule = mca_rule(Lk);
    const int S = (int)rule.splits, W = (int)((Lk + 31) / 32);
    const int64_t R = N * H * Lq;
    float *delta = ws, *dq_part = ws + (R + 3) / 4 * 4;
    {
        LaunchScope scope(tname<T>("mca_bwd", "mca_bwd_f16"), (4 * N * H * Lk * kD + 3 * S * R * kD) * 2 + S * N * Lq * W * 4, st, 0,
                          14 * N * H * Lq * Lk * kD);
        hipLaunchKernelGGL((mca_delta_kernel<T>), dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, (const T *)o.ptr, o.ts, o.is,
                           (const T *)g.ptr, g.ts, g.is, R, (int)Lq, (int)H, delta);
        if (int rc = check_launch("vah_mca_backward")) return rc;
        hipLaunchKernelGGL((mca_bwd_kernel<T>), dim3((unsigned)S, (unsigned)H, (unsigned)N), dim3(256), 0, st, (const T *)q.ptr, q.ts,
                           q.is, (const T *)k.ptr, k.ts, k.is, (const T *)v.ptr, v.ts, v.is, bits, (const T *)g.ptr, g.ts, g.is, lse,
                           (const float *)delta, (int)Lq, (int)Lk, W, (int)H, (int)rule.tiles_per_chunk, S, scale, scale * kLog2e,
                           (T *)dq.ptr, dq.ts, dq.is, (T *)dk.ptr, dk.ts, dk.is, (T *)dv.ptr, dv.ts, dv.is, dq_part);
        if (int rc = check_launch("vah_mca_backward")) return rc;
    }
    if (S == 1) return 0;
    LaunchScope scope(tname<T>("mca_dq_reduce", "mca_dq_reduce_f16"), R * S * kD * 4 + R * kD * 2, st);
    hipLaunchKernelGGL((mca_dq_reduce_kernel<T>), dim3((unsigned)((R * 8 + 255) / 256)), dim3(256), 0, st, (const float *)dq_part, R,
                       (int)Lq, (int)H, S, (T *)dq.ptr, dq.ts, dq.is);
    return check_launch("vah_mca_backward");
}

}  // namespace
}  // namespace vah

extern "C" {

int64_t vah_mca_splits(int64_t Lk) {
    if (Lk < 1) return 0;
    return vah::mca_rule(Lk).splits;
}

int64_t vah_mca_ws_bytes(int64_t N, int64_t H, int64_t Lq, int64_t Lk) {
    if (N < 1 || H < 1 || Lq < 1 || Lk < 1) return 0;
    return (vah::mca_ws_floats(N, H, Lq, Lk) + 3) / 4 * 16;
}

int vah_mca_pack_mask(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride, int64_t N, int64_t Q, int64_t Lk,
                      void *bits, void *stream) {
    using namespace vah;
    const char *fn = "vah_mca_pack_mask";
    clear_error();
    const int64_t lim = (int64_t)1 << 31;
    if (N < 0 || Q < 0 || Lk < 0 || Lk >= lim / 2 || N * Q >= lim)
        return fail(VAH_E_SHAPE, "%s: bad dims (N %lld, Q %lld, Lk %lld)", fn, (long long)N, (long long)Q, (long long)Lk);
    if (x_dtype < 0 || x_dtype > 2) return fail(VAH_E_UNSUPPORTED, "%s: dtype codes are 0 (fp32), 1 (bf16), 2 (fp16)", fn);
    if (N * Q * Lk == 0) return VAH_OK;
    if (!x) return fail(VAH_E_NULL, "%s: null pointer (x)", fn);
    if (!bits) return fail(VAH_E_NULL, "%s: null pointer (bits)", fn);
    if ((uintptr_t)x % esize(x_dtype) || (uintptr_t)bits % 4) return fail(VAH_E_ALIGN, "%s: x / bits misaligned (element size, 4 bytes)", fn);
    if (x_row_stride < 0 || x_img_stride < 0) return fail(VAH_E_SHAPE, "%s: x strides (negative)", fn);
    hipStream_t st = (hipStream_t)stream;
    const int W = (int)((Lk + 31) / 32);
    LaunchScope scope(x_dtype == 2 ? "mca_pack_f16" : "mca_pack", N * Q * (Lk * esize(x_dtype) + W * 4), st, N * Q * Lk * 5);
    return with_type(x_dtype, [&](auto tx) {
        typedef typename decltype(tx)::type TX;
        hipLaunchKernelGGL((mca_pack_kernel<TX>), dim3((unsigned)(N * Q)), dim3(256), 0, st, (const TX *)x, x_row_stride, x_img_stride,
                           (int)Q, (int)Lk, W, (uint32_t *)bits);
        return check_launch(fn);
    });
}

int vah_mca_forward(const void *q, int q_dtype, int64_t q_tok_stride, int64_t q_img_stride, const void *k, int k_dtype,
                    int64_t k_tok_stride, int64_t k_img_stride, const void *v, int v_dtype, int64_t v_tok_stride, int64_t v_img_stride,
                    const void *bits, int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t head_dim, float scale, void *out,
                    int out_dtype, int64_t out_tok_stride, int64_t out_img_stride, void *lse, void *ws, int64_t ws_bytes,
                    void *stream) {
    using namespace vah;
    const char *fn = "vah_mca_forward";
    clear_error();
    const Operand ops[4] = {{"q", q, q_dtype, q_tok_stride, q_img_stride},
                            {"k", k, k_dtype, k_tok_stride, k_img_stride},
                            {"v", v, v_dtype, v_tok_stride, v_img_stride},
                            {"out", out, out_dtype, out_tok_stride, out_img_stride}};
    bool empty;
    if (int rc = mca_check(fn, ops, 4, bits, lse, N, H, Lq, Lk, head_dim, ws, ws_bytes, &empty)) return rc;
    if (empty) return VAH_OK;
    hipStream_t st = (hipStream_t)stream;
    if (q_dtype == 1)
        return mca_forward_t<__bf16>(ops[0], ops[1], ops[2], (const uint32_t *)bits, N, H, Lq, Lk, scale, ops[3], (float *)lse,
                                     (float *)ws, st);
    return mca_forward_t<_Float16>(ops[0], ops[1], ops[2], (const uint32_t *)bits, N, H, Lq, Lk, scale, ops[3], (float *)lse,
                                   (float *)ws, st);
}

int vah_mca_backward(const void *q, int q_dtype, int64_t q_tok_stride, int64_t q_img_stride, const void *k, int k_dtype,
                     int64_t k_tok_stride, int64_t k_img_stride, const void *v, int v_dtype, int64_t v_tok_stride, int64_t v_img_stride,
                     const void *bits, const void *out, int out_dtype, int64_t out_tok_stride, int64_t out_img_stride,
                     const void *d_out, int d_out_dtype, int64_t d_out_tok_stride, int64_t d_out_img_stride, const void *lse, int64_t N,
                     int64_t H, int64_t Lq, int64_t Lk, int64_t head_dim, float scale, void *dq, int dq_dtype, int64_t dq_tok_stride,
                     int64_t dq_img_stride, void *dk, int dk_dtype, int64_t dk_tok_stride, int64_t dk_img_stride, void *dv, int dv_dtype,
                     int64_t dv_tok_stride, int64_t dv_img_stride, void *ws, int64_t ws_bytes, void *stream) {
    using namespace vah;
    const char *fn = "vah_mca_backward";
    clear_error();
    const Operand ops[8] = {{"q", q, q_dtype, q_tok_stride, q_img_stride},
                            {"k", k, k_dtype, k_tok_stride, k_img_stride},
                            {"v", v, v_dtype, v_tok_stride, v_img_stride},
                            {"out", out, out_dtype, out_tok_stride, out_img_stride},
                            {"d_out", d_out, d_out_dtype, d_out_tok_stride, d_out_img_stride},
                            {"dq", dq, dq_dtype, dq_tok_stride, dq_img_stride},
                            {"dk", dk, dk_dtype, dk_tok_stride, dk_img_stride},
                            {"dv", dv, dv_dtype, dv_tok_stride, dv_img_stride}};
    bool empty;
    if (int rc = mca_check(fn, ops, 8, bits, lse, N, H, Lq, Lk, head_dim, ws, ws_bytes, &empty)) return rc;
    if (empty) return VAH_OK;
    hipStream_t st = (hipStream_t)stream;
    if (q_dtype == 1)
        return mca_backward_t<__bf16>(ops[0], ops[1], ops[2], (const uint32_t *)bits, ops[3], ops[4], (const float *)lse, N, H, Lq, Lk,
                                      scale, ops[5], ops[6], ops[7], (float *)ws, st);
    return mca_backward_t<_Float16>(ops[0], ops[1], ops[2], (const uint32_t *)bits, ops[3], ops[4], (const float *)lse, N, H, Lq, Lk,
                                    scale, ops[5], ops[6], ops[7], (float *)ws, st);
}

}  // extern "C"
