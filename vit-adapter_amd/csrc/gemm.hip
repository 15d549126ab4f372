// bf16 and fp16 GEMMs of the Linear layers (reference: every nn.Linear of base/vit.py, adapter_modules.py and
// ops/modules/ms_deform_attn.py, i.e. F.linear and its two backward products).
//
// The tiles come from hipBLASLt (plain library GEMMs are the one place a library is the right
// tool); what lives here is the part the framework path does badly on this workload:
//   * algorithm choice.  hipBLASLt's first heuristic answer is up to 5x off for the tall-skinny
//     weight-gradient products (K = 8192..43008 rows, 768x768..3072 outputs).  Every distinct
//     problem is timed once, on first use, over the heuristic candidates (or over every algorithm
//     of the library in exhaustive mode) and the winner is cached; the table can be dumped and
//     loaded as text so a tuned table can be shipped.
//   * the weight gradient is written in fp32 straight from the accumulators (no bf16 rounding of
//     the gradient and no cast kernel per parameter).
//   * split-K.  The adapter's weight gradients reduce over 43008 token rows into outputs of at most
//     768 x 768: 18..72 output tiles for 256 CUs.  hipBLASLt runs them at 0.2 PFLOP/s; the same
//     library run as a strided batch over S slices of the rows (S x more tiles) plus one reduction
//     pass over the S fp32 partial products is 2-3x faster.  S is part of the timed choice.
// The 16-bit operand type (bf16 autocast, or fp16 autocast: the vah_gemm_f16 entry points) is part of a problem's key:
// the same shape in the two types is two entries with their own algorithms.  An fp16 result is the plain cast of the
// fp32 accumulator: nearest even, overflow to +-inf (GradScaler has to see it), subnormals kept.
// Row-major in, row-major out; hipBLASLt is column-major, so D^T = op(B)^T op(A)^T is what is run.
#include <hip/hip_runtime.h>
#include <hipblaslt/hipblaslt-ext.hpp>
#include <hipblaslt/hipblaslt.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/vitadapter_hip.h"
#include "../../include/vitadapter_hip_epoch.h"
#include "common.h"

namespace vah {
namespace {

struct Key {
    int f16;                 // 16-bit type of A, B, a 16-bit D and a 16-bit bias: 0 bf16, 1 fp16
    int ta, tb, d32, epi, bias32;
    int64_t M, N, K, lda, ldb, ldd;
    bool operator<(const Key &o) const {
        return std::tie(f16, ta, tb, d32, epi, bias32, M, N, K, lda, ldb, ldd) <
               std::tie(o.f16, o.ta, o.tb, o.d32, o.epi, o.bias32, o.M, o.N, o.K, o.lda, o.ldb, o.ldd);
    }
    hipDataType t16() const { return f16 ? HIP_R_16F : HIP_R_16BF; }
};

struct Choice {
    hipblasLtMatmulAlgo_t algo;
    size_t workspace = 0;
    int index = -1;          // hipblaslt_ext algorithm index (stable within one library build)
    int split = 1;           // slices of the reduction dimension (1: hipBLASLt writes D itself)
    float us = 0.f;          // measured time of the winner (0: not measured)
    bool resolved = false;   // algo valid (an entry loaded from text is resolved on first use)
};

struct Problem;
struct State {
    std::mutex mu;
    hipblasLtHandle_t handle = nullptr;
    std::map<Key, Choice> table;
    // descriptor sets kept per problem: creating and destroying one matmul descriptor and three layouts on every
    // call was a measurable part of the ~20 us of host time a GEMM launch costs (~300 launches per training step)
    std::map<Key, std::shared_ptr<Problem>> problems;
    int mode = 1;            // 0: first heuristic answer, 1: time the heuristic candidates, 2: time all
    int candidates = 32;
    void *probe = nullptr;   // device scratch of the candidate check (two maxima)
    int rejected = 0;        // candidates dropped by the check since the library was loaded
};

State &state() {
    static State s;
    return s;
}

const char *status_name(hipblasStatus_t s) {
    switch (s) {
    case HIPBLAS_STATUS_SUCCESS: return "success";
    case HIPBLAS_STATUS_NOT_INITIALIZED: return "not initialized";
    case HIPBLAS_STATUS_ALLOC_FAILED: return "alloc failed";
    case HIPBLAS_STATUS_INVALID_VALUE: return "invalid value";
    case HIPBLAS_STATUS_NOT_SUPPORTED: return "not supported";
    case HIPBLAS_STATUS_EXECUTION_FAILED: return "execution failed";
    default: return "error";
    }
}

// RAII over the descriptor set of one problem.
struct Problem {
    hipblasLtMatmulDesc_t desc = nullptr;
    hipblasLtMatrixLayout_t la = nullptr, lb = nullptr, ld = nullptr;
    ~Problem() {
        if (la) hipblasLtMatrixLayoutDestroy(la);
        if (lb) hipblasLtMatrixLayoutDestroy(lb);
        if (ld) hipblasLtMatrixLayoutDestroy(ld);
        if (desc) hipblasLtMatmulDescDestroy(desc);
    }
};

struct Call {
    Key k;
    const void *A, *B, *bias;
    void *D;
    void *ws;
    size_t ws_bytes;
    hipStream_t st;
    // optional finalize job riding on the reduction launch: out[c] = sum_p part[p][c] (the column-sum
    // partials of the bias gradient), so a Linear backward needs one small launch less
    const float *fin_part = nullptr;
    int fin_nparts = 0, fin_C = 0;
    float *fin_out = nullptr;
    const int32_t *row_map = nullptr;      // reduction launch only (split > 1): see reduce_splits_body<, MAPPED>
    const float *ref = nullptr;     // tuning: the reference product (M x N fp32) every candidate is held to
};

// split > 1: a strided batch over `split` equal slices of the K rows; the fp32 partial products
// (split, M, N) land in the workspace and reduce_splits() sums them into D.
hipblasStatus_t make_problem(const Call &c, Problem &p, int split) {
    const Key &k0 = c.k;
    Key k = k0;
    k.K = k0.K / split;
    if (split > 1) {
        k.d32 = 1;
        k.ldd = k0.N;
    }
    hipblasStatus_t s = hipblasLtMatmulDescCreate(&p.desc, HIPBLAS_COMPUTE_32F, HIP_R_32F);
    if (s != HIPBLAS_STATUS_SUCCESS) return s;
    // column-major view: first operand = our B, second = our A
    const hipblasOperation_t op1 = k.tb ? HIPBLAS_OP_T : HIPBLAS_OP_N, op2 = k.ta ? HIPBLAS_OP_T : HIPBLAS_OP_N;
    hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_TRANSA, &op1, sizeof(op1));
    hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_TRANSB, &op2, sizeof(op2));
    // our B row-major: (K x N) [tb = 0] or (N x K) [tb = 1]; as column-major (N x K) resp. (K x N)
    s = hipblasLtMatrixLayoutCreate(&p.la, k.t16(), k.tb ? k.K : k.N, k.tb ? k.N : k.K, k.ldb);
    if (s != HIPBLAS_STATUS_SUCCESS) return s;
    // our A row-major: (M x K) [ta = 0] or (K x M) [ta = 1]; as column-major (K x M) resp. (M x K)
    s = hipblasLtMatrixLayoutCreate(&p.lb, k.t16(), k.ta ? k.M : k.K, k.ta ? k.K : k.M, k.lda);
    if (s != HIPBLAS_STATUS_SUCCESS) return s;
    s = hipblasLtMatrixLayoutCreate(&p.ld, k.d32 ? HIP_R_32F : k.t16(), k.N, k.M, k.ldd);
    if (s != HIPBLAS_STATUS_SUCCESS) return s;
    if (split > 1) {
        const int32_t batch = split;
        // a slice of the K rows: K/split rows further down (operand stored K-major) or K/split columns along
        const int64_t sa = k.ta ? k.K * k.lda : k.K, sb = k.tb ? k.K : k.K * k.ldb, sd = k.M * k.N;
        hipblasLtMatrixLayoutSetAttribute(p.la, HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT, &batch, sizeof(batch));
        hipblasLtMatrixLayoutSetAttribute(p.lb, HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT, &batch, sizeof(batch));
        hipblasLtMatrixLayoutSetAttribute(p.ld, HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT, &batch, sizeof(batch));
        hipblasLtMatrixLayoutSetAttribute(p.la, HIPBLASLT_MATRIX_LAYOUT_STRIDED_BATCH_OFFSET, &sb, sizeof(sb));
        hipblasLtMatrixLayoutSetAttribute(p.lb, HIPBLASLT_MATRIX_LAYOUT_STRIDED_BATCH_OFFSET, &sa, sizeof(sa));
        hipblasLtMatrixLayoutSetAttribute(p.ld, HIPBLASLT_MATRIX_LAYOUT_STRIDED_BATCH_OFFSET, &sd, sizeof(sd));
    }
    uint32_t epi = HIPBLASLT_EPILOGUE_DEFAULT;
    switch (k.epi) {
    case VAH_GEMM_EPI_NONE: break;
    case VAH_GEMM_EPI_BIAS: epi = HIPBLASLT_EPILOGUE_BIAS; break;
    default: return HIPBLAS_STATUS_INVALID_VALUE;
    }
    hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &epi, sizeof(epi));
    if (c.bias) {
        hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &c.bias, sizeof(c.bias));
        const int32_t bt = k.bias32 ? HIP_R_32F : k.t16();
        hipblasLtMatmulDescSetAttribute(p.desc, HIPBLASLT_MATMUL_DESC_BIAS_DATA_TYPE, &bt, sizeof(bt));
    }
    return HIPBLAS_STATUS_SUCCESS;
}

size_t partial_bytes(const Key &k, int split) {
    return split > 1 ? ((size_t)split * k.M * k.N * sizeof(float) + 255) / 256 * 256 : 0;
}

// G slices of one float4 position: all G loads are issued, then added to `acc` in slice order (FIRST: the first of
// them starts the sum), so the result is the one chain p0 + p1 + ... whatever the grouping.
template <int G, bool FIRST>
__device__ __forceinline__ void add_slices(const float *__restrict__ p, int64_t MN, float4 &acc) {
    float4 v[G];
#pragma unroll
    for (int u = 0; u < G; ++u) v[u] = *reinterpret_cast<const float4 *>(p + u * MN);
#pragma unroll
    for (int u = 0; u < G; ++u) {
        if (FIRST && u == 0) {
            acc = v[0];
        } else {
            acc.x += v[u].x;
            acc.y += v[u].y;
            acc.z += v[u].z;
            acc.w += v[u].w;
        }
    }
}

// vec (decided by the host): N, ldd and the output pointer allow one 16-byte (fp32) or 8-byte (16-bit) store per
// position; otherwise four scalar stores.
// MAPPED: row r of the product goes to row row_map[r] of D and the finalize job's sum k to fin_out[row_map[k]] (the
// head-interleaved rows of the MSDeformAttn pair GEMM back in parameter order, without an index_select behind the launch);
// an entry outside the rows of D drops its row.  The loads and the add chain do not know about the map.
template <typename OT, bool MAPPED>
__device__ __forceinline__ void reduce_splits_body(const float *__restrict__ part, int split, int64_t MN, int N,
                                                   int64_t ldd, int vec, OT *__restrict__ out, int reduce_blocks,
                                                   const float *__restrict__ fin_part, int fin_nparts, int fin_C,
                                                   float *__restrict__ fin_out, const int32_t *__restrict__ row_map) {
    if ((int)blockIdx.x >= reduce_blocks) {
        // finalize job: 32 columns x 8 partial-row lanes per workgroup
        __shared__ float s_acc[8][32];
        const int col = threadIdx.x & 31, pl = threadIdx.x >> 5;
        const int k = ((int)blockIdx.x - reduce_blocks) * 32 + col;
        float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // 8 independent loads in flight per thread
        if (k < fin_C) {
            int p = pl;
            for (; p + 56 < fin_nparts; p += 64) {
#pragma unroll
                for (int u = 0; u < 8; ++u) a8[u] += fin_part[(int64_t)(p + 8 * u) * fin_C + k];
            }
            for (; p < fin_nparts; p += 8) a8[0] += fin_part[(int64_t)p * fin_C + k];
        }
        s_acc[pl][col] = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
        __syncthreads();
        if (pl == 0 && k < fin_C) {
            float t = 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) t += s_acc[u][col];
            if constexpr (MAPPED) {
                const unsigned kk = (unsigned)row_map[k];
                if (kk < (unsigned)fin_C) fin_out[kk] = t;
            } else {
                fin_out[k] = t;
            }
        }
        return;
    }
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < MN; i += (int64_t)reduce_blocks * 1024) {
        // the largest power-of-two group first (the table's splits are powers of two: one group of loads up to 8,
        // groups of 8 beyond), then what is left in groups of 8, 4, 2, 1
        const float *p = part + i;
        float4 acc;
        int s;
        if (split >= 8) {
            add_slices<8, true>(p, MN, acc);
            s = 8;
        } else if (split >= 4) {
            add_slices<4, true>(p, MN, acc);
            s = 4;
        } else if (split >= 2) {
            add_slices<2, true>(p, MN, acc);
            s = 2;
        } else {
            add_slices<1, true>(p, MN, acc);
            s = 1;
        }
        for (; s + 8 <= split; s += 8) add_slices<8, false>(p + s * MN, MN, acc);
        if (s + 4 <= split) {
            add_slices<4, false>(p + s * MN, MN, acc);
            s += 4;
        }
        if (s + 2 <= split) {
            add_slices<2, false>(p + s * MN, MN, acc);
            s += 2;
        }
        if (s < split) add_slices<1, false>(p + s * MN, MN, acc);
        int64_t o = i;                                 // ldd == N: D is the same flat array
        if (ldd != N) {
            const int64_t row = i / N;
            o = row * ldd + (i - row * N);
        }
        if constexpr (MAPPED) {
            const int64_t row = i / N;                  // N % 4 == 0 (split_candidates): a position lies in one row
            const unsigned to = (unsigned)row_map[row];
            if ((int64_t)to >= MN / N) continue;
            o = (int64_t)to * ldd + (i - row * N);
        }
        typedef OT ov4 __attribute__((ext_vector_type(4)));
        ov4 r;
        r[0] = (OT)acc.x;
        r[1] = (OT)acc.y;
        r[2] = (OT)acc.z;
        r[3] = (OT)acc.w;
        if (vec) {
            *reinterpret_cast<ov4 *>(out + o) = r;
        } else {
            out[o] = r[0];
            out[o + 1] = r[1];
            out[o + 2] = r[2];
            out[o + 3] = r[3];
        }
    }
}

template <typename OT>
__global__ __launch_bounds__(256) void reduce_splits(const float *__restrict__ part, int split, int64_t MN, int N,
                                                     int64_t ldd, int vec, OT *__restrict__ out, int reduce_blocks,
                                                     const float *__restrict__ fin_part, int fin_nparts, int fin_C,
                                                     float *__restrict__ fin_out) {
    reduce_splits_body<OT, false>(part, split, MN, N, ldd, vec, out, reduce_blocks, fin_part, fin_nparts, fin_C, fin_out, nullptr);
}

template <typename OT>
__global__ __launch_bounds__(256) void reduce_splits_mapped(const float *__restrict__ part, int split, int64_t MN, int N,
                                                            int64_t ldd, int vec, OT *__restrict__ out, int reduce_blocks,
                                                            const float *__restrict__ fin_part, int fin_nparts, int fin_C,
                                                            float *__restrict__ fin_out, const int32_t *__restrict__ row_map) {
    reduce_splits_body<OT, true>(part, split, MN, N, ldd, vec, out, reduce_blocks, fin_part, fin_nparts, fin_C, fin_out, row_map);
}

// ---- numerical check of a tuning candidate: its WHOLE output against a plain fp32-accumulating product of the same
// operands computed here (round 2 found exhaustive-mode algorithms that run without an error status and return wrong
// numbers; round 3 found heuristic answers for 1024 x N x 64 that leave most of the output unwritten once the workspace
// holds another product's data - and whose first 64 columns are right).  So the candidate runs twice on an output
// filled with NaN patterns, first over a workspace filled with 0x01 bytes, then over whatever it left there, and every element
// of both results has to agree with the reference.
template <typename T>
__global__ __launch_bounds__(256) void ref_gemm(int ta, int tb, int M, int N, int K, const T *__restrict__ A, int64_t lda,
                                                const T *__restrict__ B, int64_t ldb, const void *__restrict__ bias,
                                                int bias32, float *__restrict__ ref) {
    __shared__ float sa[16][65], sb[16][65];
    const int tm = blockIdx.y * 64, tn = blockIdx.x * 64;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += 16) {
        for (int i = threadIdx.x; i < 1024; i += 256) {
            // the operand's contiguous dimension runs along the lanes
            const int ma = ta ? (i & 63) : (i >> 4), ka = ta ? (i >> 6) : (i & 15);
            const int m = tm + ma, k = k0 + ka;
            sa[ka][ma] = (m < M && k < K) ? (float)(ta ? A[(int64_t)k * lda + m] : A[(int64_t)m * lda + k]) : 0.f;
            const int nb = tb ? (i >> 4) : (i & 63), kb = tb ? (i & 15) : (i >> 6);
            const int n = tn + nb, k2 = k0 + kb;
            sb[kb][nb] = (n < N && k2 < K) ? (float)(tb ? B[(int64_t)n * ldb + k2] : B[(int64_t)k2 * ldb + n]) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = sa[kk][ty * 4 + i];
                b[i] = sb[kk][tx * 4 + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
        }
        __syncthreads();
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const int m = tm + ty * 4 + i, n = tn + tx * 4 + j;
            if (m >= M || n >= N) continue;
            float v = acc[i][j];
            if (bias) v += bias32 ? ((const float *)bias)[n] : (float)((const T *)bias)[n];
            ref[(int64_t)m * N + n] = v;
        }
}

template <typename OT>
__global__ __launch_bounds__(256) void full_compare(const OT *__restrict__ D, int64_t ldd, int64_t MN, int N,
                                                    const float *__restrict__ ref, unsigned *__restrict__ out2) {
    float md = 0.f, mr = 0.f;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < MN; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / N;
        float v = (float)D[r * ldd + (i - r * N)];
        const float w = ref[i];
        if constexpr (std::is_same<OT, _Float16>::value) {
            // an fp16 result that overflowed is right when the reference rounds to the same inf, and is otherwise held
            // to the reference as the first value past fp16's range; finite results are compared as for bf16
            if (isinf(v)) v = v == (float)(_Float16)w ? w : copysignf(65520.f, v);
        }
        const float d = fabsf(v - w);
        bad = bad || !(d == d);
        md = fmaxf(md, d == d ? d : 0.f);
        mr = fmaxf(mr, fabsf(w));
    }
    // non-negative floats order like their bit patterns
    if (bad || md > 0.f) atomicMax(out2, __float_as_uint(bad ? INFINITY : md));
    if (mr > 0.f) atomicMax(out2 + 1, __float_as_uint(mr));
}

// The reference product of this call as M x N fp32 (device memory the caller frees), nullptr if it cannot be had.
float *make_reference(const Call &c) {
    const Key &k = c.k;
    if (k.M > (64 << 16) || k.N > (int64_t)INT32_MAX || k.K > (int64_t)INT32_MAX) return nullptr;
    float *ref = nullptr;
    if (hipMalloc((void **)&ref, (size_t)k.M * k.N * sizeof(float)) != hipSuccess) return nullptr;
    const dim3 grid((unsigned)((k.N + 63) / 64), (unsigned)((k.M + 63) / 64));
    if (k.f16)
        hipLaunchKernelGGL(ref_gemm<_Float16>, grid, dim3(256), 0, c.st, k.ta, k.tb, (int)k.M, (int)k.N, (int)k.K,
                           (const _Float16 *)c.A, k.lda, (const _Float16 *)c.B, k.ldb, c.bias, k.bias32, ref);
    else
        hipLaunchKernelGGL(ref_gemm<__bf16>, grid, dim3(256), 0, c.st, k.ta, k.tb, (int)k.M, (int)k.N, (int)k.K,
                           (const __bf16 *)c.A, k.lda, (const __bf16 *)c.B, k.ldb, c.bias, k.bias32, ref);
    if (hipGetLastError() != hipSuccess) {
        (void)hipFree(ref);
        return nullptr;
    }
    return ref;
}

hipblasStatus_t run(State &S, const Call &c, Problem &p, const hipblasLtMatmulAlgo_t &algo, size_t ws_need, int split);

// -> true if the algorithm reproduces the reference on NaN-filled output, over a poisoned and over a used workspace
bool validate(State &S, const Call &c, Problem &p, const hipblasLtMatmulAlgo_t &algo, size_t ws_need, int split, const float *ref) {
    if (!ref) return true;                                                                           // cannot check: accept
    if (!S.probe && hipMalloc(&S.probe, 2 * sizeof(unsigned)) != hipSuccess) return true;
    unsigned *out2 = (unsigned *)S.probe;
    const Key &k = c.k;
    const size_t es = k.d32 ? 4 : 2;
    const int64_t MN = k.M * k.N;
    const unsigned blocks = (unsigned)std::min<int64_t>(4096, (MN + 255) / 256);
    // dirty, but not hostile: 0x01 bytes are small positive integers / denormal floats - a kernel that expects zeroed flags
    // or partial sums goes wrong on them (and is refused below) without being handed 0xFFFFFFFF as an index
    if (c.ws_bytes && hipMemsetAsync(c.ws, 0x01, c.ws_bytes, c.st) != hipSuccess) return true;
    for (int pass = 0; pass < 2; ++pass) {
        if (hipMemsetAsync(out2, 0, 8, c.st) != hipSuccess) return true;
        if (hipMemset2DAsync(c.D, (size_t)k.ldd * es, 0xFF, (size_t)k.N * es, (size_t)k.M, c.st) != hipSuccess) return true;
        if (run(S, c, p, algo, ws_need, split) != HIPBLAS_STATUS_SUCCESS) return false;
        if (k.d32)
            hipLaunchKernelGGL(full_compare<float>, dim3(blocks), dim3(256), 0, c.st, (const float *)c.D, k.ldd, MN, (int)k.N, ref, out2);
        else if (k.f16)
            hipLaunchKernelGGL(full_compare<_Float16>, dim3(blocks), dim3(256), 0, c.st, (const _Float16 *)c.D, k.ldd, MN, (int)k.N, ref, out2);
        else
            hipLaunchKernelGGL(full_compare<__bf16>, dim3(blocks), dim3(256), 0, c.st, (const __bf16 *)c.D, k.ldd, MN, (int)k.N, ref, out2);
        float h[2] = {0.f, 0.f};
        if (hipMemcpyAsync(h, out2, 8, hipMemcpyDeviceToHost, c.st) != hipSuccess || hipStreamSynchronize(c.st) != hipSuccess) return true;
        // same operands, fp32 accumulation in a different order, bf16 or fp32 result: 2^-6 of the largest value is far
        // above any legitimate difference and far below a wrong or missing tile
        if (!(h[0] <= 0.015625f * fmaxf(h[1], 1e-20f))) return false;
    }
    return true;
}

hipblasStatus_t run(State &S, const Call &c, Problem &p, const hipblasLtMatmulAlgo_t &algo, size_t ws_need, int split) {
    const size_t pb = partial_bytes(c.k, split);
    if (pb + ws_need > c.ws_bytes) return HIPBLAS_STATUS_ALLOC_FAILED;
    const float alpha = 1.f, beta = 0.f;
    void *d = split > 1 ? c.ws : c.D;
    // operands swapped: see the header comment
    const hipblasStatus_t s = hipblasLtMatmul(S.handle, p.desc, &alpha, c.B, p.la, c.A, p.lb, &beta, d, p.ld, d, p.ld, &algo,
                                              (char *)c.ws + pb, c.ws_bytes - pb, c.st);
    if (s != HIPBLAS_STATUS_SUCCESS) return s;
    const bool fin = c.fin_part != nullptr;
    if (split == 1 && !fin) return s;
    const int64_t MN = c.k.M * c.k.N;
    // one float4 position per thread up to 8192 workgroups (the largest product of the table, 3072 x 768, takes 2304):
    // with a lower cap a part of the threads ran a second position after the others had finished
    const unsigned rblocks = split > 1 ? (unsigned)std::min<int64_t>(8192, (MN / 4 + 255) / 256) : 0u;
    const unsigned fblocks = fin ? (unsigned)((c.fin_C + 31) / 32) : 0u;
    // a position is 4 consecutive elements of one row (N % 4 == 0): it leaves as one store where every row starts aligned
    const int vec = c.k.N % 4 == 0 && c.k.ldd % 4 == 0 && (uintptr_t)c.D % (c.k.d32 ? 16 : 8) == 0;
    if (c.row_map && split > 1) {
        const dim3 grid(rblocks + fblocks);
        if (c.k.d32)
            hipLaunchKernelGGL(reduce_splits_mapped<float>, grid, dim3(256), 0, c.st, (const float *)c.ws, split, MN, (int)c.k.N,
                               c.k.ldd, vec, (float *)c.D, (int)rblocks, c.fin_part, c.fin_nparts, c.fin_C, c.fin_out, c.row_map);
        else if (c.k.f16)
            hipLaunchKernelGGL(reduce_splits_mapped<_Float16>, grid, dim3(256), 0, c.st, (const float *)c.ws, split, MN, (int)c.k.N,
                               c.k.ldd, vec, (_Float16 *)c.D, (int)rblocks, c.fin_part, c.fin_nparts, c.fin_C, c.fin_out, c.row_map);
        else
            hipLaunchKernelGGL(reduce_splits_mapped<__bf16>, grid, dim3(256), 0, c.st, (const float *)c.ws, split, MN, (int)c.k.N,
                               c.k.ldd, vec, (__bf16 *)c.D, (int)rblocks, c.fin_part, c.fin_nparts, c.fin_C, c.fin_out, c.row_map);
        return HIPBLAS_STATUS_SUCCESS;
    }
    if (c.k.d32)
        hipLaunchKernelGGL(reduce_splits<float>, dim3(rblocks + fblocks), dim3(256), 0, c.st, (const float *)c.ws, split, MN,
                           (int)c.k.N, c.k.ldd, vec, (float *)c.D, (int)rblocks, c.fin_part, c.fin_nparts, c.fin_C, c.fin_out);
    else if (c.k.f16)
        hipLaunchKernelGGL(reduce_splits<_Float16>, dim3(rblocks + fblocks), dim3(256), 0, c.st, (const float *)c.ws, split, MN,
                           (int)c.k.N, c.k.ldd, vec, (_Float16 *)c.D, (int)rblocks, c.fin_part, c.fin_nparts, c.fin_C, c.fin_out);
    else
        hipLaunchKernelGGL(reduce_splits<__bf16>, dim3(rblocks + fblocks), dim3(256), 0, c.st, (const float *)c.ws, split, MN,
                           (int)c.k.N, c.k.ldd, vec, (__bf16 *)c.D, (int)rblocks, c.fin_part, c.fin_nparts, c.fin_C, c.fin_out);
    return HIPBLAS_STATUS_SUCCESS;
}

// Time one candidate on the caller's stream (the output is simply overwritten).
float time_algo(State &S, const Call &c, Problem &p, const hipblasLtMatmulAlgo_t &algo, size_t ws_need, int split,
                hipEvent_t e0, hipEvent_t e1, int reps) {
    if (run(S, c, p, algo, ws_need, split) != HIPBLAS_STATUS_SUCCESS) return -1.f;      // warm-up + validity
    if (hipEventRecord(e0, c.st) != hipSuccess) return -1.f;
    for (int i = 0; i < reps; ++i)
        if (run(S, c, p, algo, ws_need, split) != HIPBLAS_STATUS_SUCCESS) return -1.f;
    if (hipEventRecord(e1, c.st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) return -1.f;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1.f;
    return ms * 1000.f / reps;
}

// Best algorithm for one value of `split` (timed unless there is a single candidate and nothing to
// compare it with).
hipblasStatus_t choose_for_split(State &S, const Call &c, Problem &p, int split, bool must_time, Choice &out) {
    const size_t pb = partial_bytes(c.k, split);
    if (pb >= c.ws_bytes) return HIPBLAS_STATUS_ALLOC_FAILED;
    const size_t ws_lib = c.ws_bytes - pb;
    std::vector<hipblasLtMatmulHeuristicResult_t> cand;
    const bool d32 = split > 1 || c.k.d32;
    if (S.mode == 2) {
        std::vector<hipblasLtMatmulHeuristicResult_t> all;
        const Key &k = c.k;
        hipblasStatus_t s = hipblaslt_ext::getAllAlgos(
            S.handle, hipblaslt_ext::GemmType::HIPBLASLT_GEMM, k.tb ? HIPBLAS_OP_T : HIPBLAS_OP_N,
            k.ta ? HIPBLAS_OP_T : HIPBLAS_OP_N, k.t16(), k.t16(), d32 ? HIP_R_32F : k.t16(),
            d32 ? HIP_R_32F : k.t16(), HIPBLAS_COMPUTE_32F, all);
        if (s == HIPBLAS_STATUS_SUCCESS)
            for (auto &r : all) {
                size_t need = 0;
                const float one = 1.f, zero = 0.f;
                if (hipblaslt_ext::matmulIsAlgoSupported(S.handle, p.desc, &one, p.la, p.lb, &zero, p.ld, p.ld, r.algo,
                                                         need) == HIPBLAS_STATUS_SUCCESS &&
                    need <= ws_lib) {
                    r.workspaceSize = need;
                    cand.push_back(r);
                }
            }
    }
    if (cand.empty()) {
        hipblasLtMatmulPreference_t pref = nullptr;
        hipblasStatus_t s = hipblasLtMatmulPreferenceCreate(&pref);
        if (s != HIPBLAS_STATUS_SUCCESS) return s;
        const uint64_t wsmax = ws_lib;
        hipblasLtMatmulPreferenceSetAttribute(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &wsmax, sizeof(wsmax));
        const int want = S.mode == 0 ? 1 : (split > 1 ? std::min(S.candidates, 12) : S.candidates);
        cand.resize(want);
        int got = 0;
        s = hipblasLtMatmulAlgoGetHeuristic(S.handle, p.desc, p.la, p.lb, p.ld, p.ld, pref, want, cand.data(), &got);
        hipblasLtMatmulPreferenceDestroy(pref);
        if (s != HIPBLAS_STATUS_SUCCESS) return s;
        cand.resize(std::max(got, 0));
        if (cand.empty()) return HIPBLAS_STATUS_NOT_SUPPORTED;
    }
    out.split = split;
    if (S.mode == 0 || (cand.size() == 1 && !must_time)) {
        if (!validate(S, c, p, cand[0].algo, cand[0].workspaceSize, split, c.ref)) {
            ++S.rejected;
            return HIPBLAS_STATUS_EXECUTION_FAILED;
        }
        out.algo = cand[0].algo;
        out.workspace = cand[0].workspaceSize;
        out.index = hipblaslt_ext::getIndexFromAlgo(out.algo);
        out.resolved = true;
        return HIPBLAS_STATUS_SUCCESS;
    }
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return HIPBLAS_STATUS_ALLOC_FAILED;
    float best = -1.f;
    size_t best_i = 0;
    // coarse pass over everything, then a longer look at the fastest few THAT COMPUTE THE REFERENCE's NUMBERS (walked in
    // order of speed: an algorithm that skips part of the output is fast)
    std::vector<std::pair<float, size_t>> timed;
    for (size_t i = 0; i < cand.size(); ++i) {
        const float us = time_algo(S, c, p, cand[i].algo, cand[i].workspaceSize, split, e0, e1, 3);
        if (us > 0.f) timed.emplace_back(us, i);
    }
    std::sort(timed.begin(), timed.end());
    int looked = 0;
    for (size_t j = 0; j < timed.size() && looked < 4; ++j) {
        const size_t i = timed[j].second;
        if (!validate(S, c, p, cand[i].algo, cand[i].workspaceSize, split, c.ref)) {
            ++S.rejected;
            continue;
        }
        ++looked;
        const float us = time_algo(S, c, p, cand[i].algo, cand[i].workspaceSize, split, e0, e1, 20);
        if (us > 0.f && (best < 0.f || us < best)) {
            best = us;
            best_i = i;
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (best < 0.f) return HIPBLAS_STATUS_EXECUTION_FAILED;
    out.algo = cand[best_i].algo;
    out.workspace = cand[best_i].workspaceSize;
    out.index = hipblaslt_ext::getIndexFromAlgo(out.algo);
    out.us = best;
    out.resolved = true;
    return HIPBLAS_STATUS_SUCCESS;
}

// Slices worth trying: only reductions that are long and leave most of the chip without an output
// tile; the partial products must fit the workspace next to the library's own scratch.
std::vector<int> split_candidates(const State &S, const Call &c) {
    std::vector<int> v{1};
    const Key &k = c.k;
    if (S.mode == 0 || c.bias || k.K < 4096 || k.N % 4) return v;
    const int64_t tiles = ((k.M + 127) / 128) * ((k.N + 127) / 128);
    if (tiles >= 256) return v;
    for (int s = 2; s <= 64; s *= 2) {
        if (k.K % s || k.K / s < 512 || tiles * s > 4096) break;
        if (partial_bytes(k, s) + (8u << 20) > c.ws_bytes) break;
        v.push_back(s);
    }
    return v;
}

hipblasStatus_t choose(State &S, const Call &call, Choice &out) {
    Call c = call;                       // candidates are timed without the piggy-backed finalize job
    c.fin_part = nullptr;
    const std::vector<int> splits = split_candidates(S, c);
    float *ref = S.mode != 0 ? make_reference(c) : nullptr;
    c.ref = ref;
    hipblasStatus_t last = HIPBLAS_STATUS_NOT_SUPPORTED;
    bool have = false;
    for (int split : splits) {
        Problem p;
        hipblasStatus_t s = make_problem(c, p, split);
        Choice ch;
        if (s == HIPBLAS_STATUS_SUCCESS) s = choose_for_split(S, c, p, split, splits.size() > 1, ch);
        if (s != HIPBLAS_STATUS_SUCCESS) {
            last = s;
            continue;
        }
        if (!have || (ch.us > 0.f && ch.us < out.us)) out = ch;
        have = true;
    }
    if (ref) {
        (void)hipStreamSynchronize(c.st);
        (void)hipFree(ref);
    }
    return have ? HIPBLAS_STATUS_SUCCESS : last;
}

// An entry that came from text: look the algorithm up by index and make sure it fits this problem.
bool resolve(State &S, const Call &c, Problem &p, Choice &ch) {
    std::vector<int> idx{ch.index};
    std::vector<hipblasLtMatmulHeuristicResult_t> res;
    if (ch.index < 0 || hipblaslt_ext::getAlgosFromIndex(S.handle, idx, res) != HIPBLAS_STATUS_SUCCESS || res.empty())
        return false;
    size_t need = 0;
    const float one = 1.f, zero = 0.f;
    if (hipblaslt_ext::matmulIsAlgoSupported(S.handle, p.desc, &one, p.la, p.lb, &zero, p.ld, p.ld, res[0].algo, need) !=
            HIPBLAS_STATUS_SUCCESS || need + partial_bytes(c.k, ch.split) > c.ws_bytes)
        return false;
    // an entry is only as good as the build and the workspace use it was tuned with: hold it to the reference once
    Call cc = c;
    cc.fin_part = nullptr;
    float *ref = make_reference(cc);
    const bool ok = validate(S, cc, p, res[0].algo, need, ch.split, ref);
    if (ref) {
        (void)hipStreamSynchronize(c.st);
        (void)hipFree(ref);
    }
    if (!ok) {
        ++S.rejected;
        return false;
    }
    ch.algo = res[0].algo;
    ch.workspace = need;
    ch.resolved = true;
    return true;
}

}  // namespace
}  // namespace vah

extern "C" {

int vah_gemm_set_tuning(int mode, int candidates) {
    using namespace vah;
    clear_error();
    if (mode < 0 || mode > 2 || candidates < 1 || candidates > 4096) return fail(VAH_E_SHAPE, "vah_gemm_set_tuning: bad arguments");
    State &S = state();
    std::lock_guard<std::mutex> lock(S.mu);
    S.mode = mode;
    S.candidates = candidates;
    return VAH_OK;
}

static int gemm_impl(const char *fn, int f16, int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda,
                     const void *B, int64_t ldb, void *D, int64_t ldd, int d_is_f32, int epilogue, const void *bias,
                     int bias_is_f32, void *workspace, int64_t workspace_bytes, void *stream, const float *fin_part,
                     int64_t fin_nparts, int64_t fin_C, float *fin_out, const int32_t *row_map = nullptr, int *applied = nullptr);

int vah_gemm_bf16(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda,
                  const void *B, int64_t ldb, void *D, int64_t ldd, int d_is_f32, int epilogue, const void *bias,
                  int bias_is_f32, void *workspace, int64_t workspace_bytes, void *stream) {
    return gemm_impl("vah_gemm_bf16", 0, trans_a, trans_b, M, N, K, A, lda, B, ldb, D, ldd, d_is_f32, epilogue, bias, bias_is_f32,
                     workspace, workspace_bytes, stream, nullptr, 0, 0, nullptr);
}

// vah_gemm_bf16 plus a finalize job on its last launch: fin_out[c] = sum_{p < fin_nparts} fin_part[p * fin_C + c]
// (the partial rows vah_colsum_bf16_partials wrote).  One Linear backward = partials, GEMM, reduction +
// finalize: a launch less than column sum and weight gradient on their own.
int vah_gemm_bf16_fin(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda,
                      const void *B, int64_t ldb, void *D, int64_t ldd, int d_is_f32, void *workspace,
                      int64_t workspace_bytes, const float *fin_part, int64_t fin_nparts, int64_t fin_C, float *fin_out,
                      void *stream) {
    using namespace vah;
    if (!fin_part || !fin_out || fin_nparts < 1 || fin_C < 1 || fin_nparts > (1 << 20) || fin_C > (1 << 24)) {
        clear_error();
        return fail(VAH_E_SHAPE, "vah_gemm_bf16_fin: bad finalize job");
    }
    return gemm_impl("vah_gemm_bf16_fin", 0, trans_a, trans_b, M, N, K, A, lda, B, ldb, D, ldd, d_is_f32, VAH_GEMM_EPI_NONE, nullptr,
                     0, workspace, workspace_bytes, stream, fin_part, fin_nparts, fin_C, fin_out);
}

// The fp16 twins: A, B, a 16-bit D and a 16-bit bias are _Float16; everything else as above.
int vah_gemm_f16(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda,
                 const void *B, int64_t ldb, void *D, int64_t ldd, int d_is_f32, int epilogue, const void *bias,
                 int bias_is_f32, void *workspace, int64_t workspace_bytes, void *stream) {
    return gemm_impl("vah_gemm_f16", 1, trans_a, trans_b, M, N, K, A, lda, B, ldb, D, ldd, d_is_f32, epilogue, bias, bias_is_f32,
                     workspace, workspace_bytes, stream, nullptr, 0, 0, nullptr);
}

int vah_gemm_f16_fin(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda,
                     const void *B, int64_t ldb, void *D, int64_t ldd, int d_is_f32, void *workspace,
                     int64_t workspace_bytes, const float *fin_part, int64_t fin_nparts, int64_t fin_C, float *fin_out,
                     void *stream) {
    using namespace vah;
    if (!fin_part || !fin_out || fin_nparts < 1 || fin_C < 1 || fin_nparts > (1 << 20) || fin_C > (1 << 24)) {
        clear_error();
        return fail(VAH_E_SHAPE, "vah_gemm_f16_fin: bad finalize job");
    }
    return gemm_impl("vah_gemm_f16_fin", 1, trans_a, trans_b, M, N, K, A, lda, B, ldb, D, ldd, d_is_f32, VAH_GEMM_EPI_NONE, nullptr,
                     0, workspace, workspace_bytes, stream, fin_part, fin_nparts, fin_C, fin_out);
}

// vah_gemm_bf16_fin / vah_gemm_f16_fin with a row map on the reduction launch (include/vitadapter_hip_epoch.h): D's row r
// lands in row row_map[r], the finalize sum k in fin_out[row_map[k]].  *applied = 0 where the product runs with split 1
// (hipBLASLt writes D itself): D and fin_out are then in the product's own order.
static int gemm_fin_rowmap(const char *fn, int f16, int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const void *A,
                           int64_t lda, const void *B, int64_t ldb, void *D, int64_t ldd, int d_is_f32, void *workspace,
                           int64_t workspace_bytes, const float *fin_part, int64_t fin_nparts, int64_t fin_C, float *fin_out,
                           const int32_t *row_map, int *applied, void *stream) {
    using namespace vah;
    if (applied) *applied = 0;
    if (!fin_part || !fin_out || fin_nparts < 1 || fin_C < 1 || fin_nparts > (1 << 20) || fin_C > (1 << 24)) {
        clear_error();
        return fail(VAH_E_SHAPE, "%s: bad finalize job", fn);
    }
    if (!row_map) {
        clear_error();
        return fail(VAH_E_NULL, "%s: null pointer (row_map)", fn);
    }
    if (fin_C != M || (uintptr_t)row_map % 4) {
        clear_error();
        return fail(VAH_E_SHAPE, "%s: the row map serves D's rows and the finalize sums alike (fin_C == M), 4-byte aligned", fn);
    }
    return gemm_impl(fn, f16, trans_a, trans_b, M, N, K, A, lda, B, ldb, D, ldd, d_is_f32, VAH_GEMM_EPI_NONE, nullptr, 0, workspace,
                     workspace_bytes, stream, fin_part, fin_nparts, fin_C, fin_out, row_map, applied);
}

int vah_gemm_bf16_fin_rowmap(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda,
                             const void *B, int64_t ldb, void *D, int64_t ldd, int d_is_f32, void *workspace,
                             int64_t workspace_bytes, const float *fin_part, int64_t fin_nparts, int64_t fin_C,
                             float *fin_out, const int32_t *row_map, int *applied, void *stream) {
    return gemm_fin_rowmap("vah_gemm_bf16_fin_rowmap", 0, trans_a, trans_b, M, N, K, A, lda, B, ldb, D, ldd, d_is_f32, workspace,
                           workspace_bytes, fin_part, fin_nparts, fin_C, fin_out, row_map, applied, stream);
}

int vah_gemm_f16_fin_rowmap(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda,
                            const void *B, int64_t ldb, void *D, int64_t ldd, int d_is_f32, void *workspace,
                            int64_t workspace_bytes, const float *fin_part, int64_t fin_nparts, int64_t fin_C,
                            float *fin_out, const int32_t *row_map, int *applied, void *stream) {
    return gemm_fin_rowmap("vah_gemm_f16_fin_rowmap", 1, trans_a, trans_b, M, N, K, A, lda, B, ldb, D, ldd, d_is_f32, workspace,
                           workspace_bytes, fin_part, fin_nparts, fin_C, fin_out, row_map, applied, stream);
}

static int gemm_impl(const char *fn, int f16, int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda,
                     const void *B, int64_t ldb, void *D, int64_t ldd, int d_is_f32, int epilogue, const void *bias,
                     int bias_is_f32, void *workspace, int64_t workspace_bytes, void *stream, const float *fin_part,
                     int64_t fin_nparts, int64_t fin_C, float *fin_out, const int32_t *row_map, int *applied) {
    using namespace vah;
    clear_error();
    if (M < 0 || N < 0 || K < 0) return fail(VAH_E_SHAPE, "%s: negative dimension", fn);
    if (M == 0 || N == 0) return VAH_OK;
    if (K == 0) return fail(VAH_E_SHAPE, "%s: K = 0 (zero-fill the output instead)", fn);
    if (!A || !B || !D) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if (lda < (trans_a ? M : K) || ldb < (trans_b ? K : N) || ldd < N) return fail(VAH_E_SHAPE, "%s: leading dimension too small", fn);
    if (epilogue != VAH_GEMM_EPI_NONE && epilogue != VAH_GEMM_EPI_BIAS) return fail(VAH_E_SHAPE, "%s: unknown epilogue", fn);
    if ((epilogue == VAH_GEMM_EPI_BIAS) != (bias != nullptr)) return fail(VAH_E_NULL, "%s: bias does not match the epilogue", fn);
    if (workspace_bytes < 0 || (workspace_bytes > 0 && !workspace)) return fail(VAH_E_NULL, "%s: workspace", fn);
    // hipBLASLt's bias epilogue reads an fp16 bias correctly only into an fp16 D: into an fp32 D the result is garbage,
    // with a success status (fused.gemm_16 widens such a bias to fp32 before the call)
    if (f16 && bias && !bias_is_f32 && d_is_f32)
        return fail(VAH_E_UNSUPPORTED, "%s: an fp16 bias into an fp32 output is not supported (pass the bias in fp32)", fn);

    State &S = state();
    std::lock_guard<std::mutex> lock(S.mu);
    if (!S.handle) {
        const hipblasStatus_t s = hipblasLtCreate(&S.handle);
        if (s != HIPBLAS_STATUS_SUCCESS) return fail(VAH_E_UNSUPPORTED, "%s: hipblasLtCreate: %s", fn, status_name(s));
    }
    Call c{{f16 ? 1 : 0, trans_a ? 1 : 0, trans_b ? 1 : 0, d_is_f32 ? 1 : 0, epilogue, bias_is_f32 ? 1 : 0, M, N, K, lda, ldb, ldd},
           A, B, bias, D, workspace, (size_t)workspace_bytes, (hipStream_t)stream};
    c.fin_part = fin_part;
    c.fin_nparts = (int)fin_nparts;
    c.fin_C = (int)fin_C;
    c.fin_out = fin_out;
    hipblasStatus_t s = HIPBLAS_STATUS_SUCCESS;
    // named by the product's role in a Linear layer: nt = forward (x W^T), nn = input gradient (g W), tn = weight gradient
    // (g^T x); flops for the MFMA roofline rows of bench.py
    const char *role = f16 ? (trans_a ? (fin_part ? "gemm_tn_fin_f16" : "gemm_tn_f16") : (trans_b ? "gemm_nt_f16" : "gemm_nn_f16"))
                           : (trans_a ? (fin_part ? "gemm_tn_fin" : "gemm_tn") : (trans_b ? "gemm_nt" : "gemm_nn"));
    LaunchScope scope(role, (M * K + K * N) * 2 + M * N * (d_is_f32 ? 4 : 2), c.st, 0, 2 * M * N * K);
    auto it = S.table.find(c.k);
    if (it != S.table.end() && !it->second.resolved) {
        Problem p;
        const int split = it->second.split;
        if (split < 1 || K % split || make_problem(c, p, split) != HIPBLAS_STATUS_SUCCESS ||
            partial_bytes(c.k, split) >= c.ws_bytes || !resolve(S, c, p, it->second)) {
            S.table.erase(it);
            S.problems.erase(c.k);
            it = S.table.end();
        }
    }
    if (it == S.table.end()) {
        Choice ch;
        s = choose(S, c, ch);
        if (s != HIPBLAS_STATUS_SUCCESS)
            return fail(VAH_E_UNSUPPORTED, "%s: no algorithm for %lldx%lldx%lld ta=%d tb=%d f32=%d epi=%d: %s", fn,
                        (long long)M, (long long)N, (long long)K, trans_a, trans_b, d_is_f32, epilogue, status_name(s));
        it = S.table.emplace(c.k, ch).first;
    }
    std::shared_ptr<Problem> &pp = S.problems[c.k];
    if (!pp) {
        pp = std::make_shared<Problem>();
        s = make_problem(c, *pp, it->second.split);
        if (s != HIPBLAS_STATUS_SUCCESS) {
            S.problems.erase(c.k);
            return fail(VAH_E_UNSUPPORTED, "%s: descriptor: %s", fn, status_name(s));
        }
    } else if (c.bias) {                    // the cached descriptor carries the previous call's bias pointer
        hipblasLtMatmulDescSetAttribute(pp->desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &c.bias, sizeof(c.bias));
    }
    Problem &p = *pp;
    // the map rides on the reduction launch only; tuning and validation above ran without it
    c.row_map = it->second.split > 1 ? row_map : nullptr;
    if (applied) *applied = c.row_map != nullptr;
    s = run(S, c, p, it->second.algo, it->second.workspace, it->second.split);
    if (s != HIPBLAS_STATUS_SUCCESS) return fail(VAH_E_UNSUPPORTED, "%s: hipblasLtMatmul: %s", fn, status_name(s));
    return check_launch(fn);
}

// Version of the hipBLASLt build behind the dispatcher (algorithm indices of a dumped table are only
// meaningful for the same build); < 0 on error.
int64_t vah_gemm_rejected_candidates(void) {
    vah::State &S = vah::state();
    std::lock_guard<std::mutex> lock(S.mu);
    return S.rejected;
}

int64_t vah_gemm_library_version(void) {
    using namespace vah;
    clear_error();
    State &S = state();
    std::lock_guard<std::mutex> lock(S.mu);
    if (!S.handle && hipblasLtCreate(&S.handle) != HIPBLAS_STATUS_SUCCESS)
        return fail(VAH_E_UNSUPPORTED, "vah_gemm_library_version: hipblasLtCreate failed");
    int v = 0;
    if (hipblasLtGetVersion(S.handle, &v) != HIPBLAS_STATUS_SUCCESS)
        return fail(VAH_E_UNSUPPORTED, "vah_gemm_library_version: hipblasLtGetVersion failed");
    return v;
}

// One line per problem: "ta tb d32 epi bias32 M N K lda ldb ldd index split us"; an fp16 problem is the same line
// behind a leading "f16 " token (so no fp16 line starts like a bf16 one).
int64_t vah_gemm_table_dump(char *buf, int64_t cap) {
    using namespace vah;
    State &S = state();
    std::lock_guard<std::mutex> lock(S.mu);
    std::ostringstream os;
    for (auto &kv : S.table) {
        const Key &k = kv.first;
        if (k.f16) os << "f16 ";
        os << k.ta << ' ' << k.tb << ' ' << k.d32 << ' ' << k.epi << ' ' << k.bias32 << ' ' << k.M << ' ' << k.N << ' '
           << k.K << ' ' << k.lda << ' ' << k.ldb << ' ' << k.ldd << ' ' << kv.second.index << ' ' << kv.second.split << ' '
           << kv.second.us << '\n';
    }
    const std::string t = os.str();
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>(t.size(), (size_t)cap - 1);
        memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return (int64_t)t.size() + 1;
}

int vah_gemm_table_load(const char *text) {
    using namespace vah;
    clear_error();
    if (!text) return fail(VAH_E_NULL, "vah_gemm_table_load: null text");
    State &S = state();
    std::lock_guard<std::mutex> lock(S.mu);
    S.problems.clear();             // their split may change with the loaded choices
    std::istringstream is(text);
    std::string line;
    int n = 0;
    while (std::getline(is, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ls(line);
        Key k;
        Choice ch;
        k.f16 = line.compare(0, 4, "f16 ") == 0;
        if (k.f16) ls.ignore(4);
        if (!(ls >> k.ta >> k.tb >> k.d32 >> k.epi >> k.bias32 >> k.M >> k.N >> k.K >> k.lda >> k.ldb >> k.ldd >> ch.index >> ch.split >> ch.us))
            return fail(VAH_E_SHAPE, "vah_gemm_table_load: malformed line '%s'", line.c_str());
        ch.resolved = false;
        S.table[k] = ch;
        ++n;
    }
    return n;
}

}  // extern "C"
