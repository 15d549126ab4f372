// The assignment step of Mask2Former's matching (include/vitadapter_hip_assign.h): every (decoder output, image) problem of a
// training step solved exactly on the device, one wave per problem, the cost block in LDS.
//   * The method is the shortest-augmenting-path form of Jonker-Volgenant for rectangular problems, as scipy's
//     linear_sum_assignment describes it: the smaller dimension is the row set; row `cur` is added by a Dijkstra search over the
//     reduced costs c[i][j] - u[i] - v[j] from `cur` to the nearest unassigned column, the duals of everything the search
//     scanned move by their distance to that column, and the path is flipped.  All of it in fp64, in scipy's expressions
//     (minVal + c - u - v, left to right; no product, so nothing contracts), over the fp32 costs widened to fp64.
//   * Columns are spread over the lanes (column c is slot c / 64 of lane c % 64), rows are walked one at a time: a step reads
//     one row of the block (consecutive words), updates up to four candidates per lane and reduces the key
//     (value, assigned, column) over the wave by an xor butterfly.  The key is a total order, so every lane ends with the same
//     minimum and control flow stays uniform.
//   * What belongs to a column (shortest path cost, predecessor row, assigned row, dual v, scanned bit) stays in its lane's
//     registers; what belongs to a row (dual u, its column) is in LDS.  A scanned row other than `cur` is the assigned row of
//     exactly one scanned column, so the column's lane updates that row's dual: no two lanes write one word.
//   * Every loop has a bound that holds for any input (a search scans a column per step, a path has at most one row per step),
//     every index that forms an address is tested first, and a problem that cannot be solved writes the identity pairing.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/vitadapter_hip_assign.h"
#include "common.h"

namespace vah {
namespace {

constexpr int kMaxDim = 256;                // rows or columns of a block at most
constexpr int kSlots = kMaxDim / kWave;     // columns of a lane
constexpr int64_t kMaxCells = 32768;        // Q * Gmax at most: 128 KiB of fp32
constexpr int64_t kMaxN = 4096;
constexpr int kRowBytes = kMaxDim * (8 + 4);        // u (fp64) and col4row (int32) in front of the block
constexpr int kAssignedBit = 1 << 16;

struct Key {
    double val;
    int tie;                                // assigned << 16 | column; INT_MAX: no candidate
};

__device__ __forceinline__ bool before(const Key a, const Key b) { return a.val < b.val || (a.val == b.val && a.tie < b.tie); }

__device__ __forceinline__ Key wave_min(Key k) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        Key o;
        o.val = __shfl_xor(k.val, d, kWave);
        o.tie = __shfl_xor(k.tie, d, kWave);
        if (before(o, k)) k = o;
    }
    return k;
}

__device__ __forceinline__ int wave_sum_int(int x) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) x += __shfl_xor(x, d, kWave);
    return x;
}

// a[slot] of lane `src` for a slot that is the same in every lane (no indexed register array)
__device__ __forceinline__ int pick(const int (&a)[kSlots], int slot, int src) {
    const int mine = slot == 0 ? a[0] : slot == 1 ? a[1] : slot == 2 ? a[2] : a[3];
    return __shfl(mine, src, kWave);
}

// pairs of an image as the offsets on the device give them: -1 for a pair of offsets that is no count
__device__ __forceinline__ int pairs_of(const int *off, int m, int Q, int Gmax) {
    const int64_t lo = off[m], g = (int64_t)off[m + 1] - lo;
    if (lo < 0 || g < 0 || g > Gmax) return -1;
    return g < Q ? (int)g : Q;
}

__global__ __launch_bounds__(kWave) void assign_solve_kernel(const float *__restrict__ cost, const int *__restrict__ off, int N, int Q, int Gmax,
                                                             int64_t *__restrict__ table, int *__restrict__ status) {
    extern __shared__ double lds[];
    double *u = lds;                                                // [kMaxDim]
    int *col4row = reinterpret_cast<int *>(u + kMaxDim);            // [kMaxDim]
    float *C = reinterpret_cast<float *>(col4row + kMaxDim);        // [nr][nc], nr * nc <= Q * Gmax
    const int lane = (int)threadIdx.x, prob = (int)blockIdx.x, out = prob / N, n = prob - out * N;

    int base = 0, K = 0;
    for (int m = lane; m < N; m += kWave) {
        const int k = pairs_of(off, m, Q, Gmax);
        if (k > 0) {
            K += k;
            if (m < n) base += k;
        }
    }
    base = wave_sum_int(base), K = wave_sum_int(K);
    const int mine = pairs_of(off, n, Q, Gmax);
    if (mine <= 0) {                                                // no count: infeasible, no pair; no target: solved, no pair
        if (lane == 0) status[prob] = mine < 0 ? 2 : 0;
        return;
    }
    const int o0 = off[n], G = off[n + 1] - o0;                     // 1 <= G <= Gmax, base + min(Q, G) <= K
    int64_t *t0 = table + (int64_t)out * 2 * K + base, *t1 = t0 + K;
    const bool tr = Q > G;
    const int nr = tr ? G : Q, nc = tr ? Q : G;                     // nr <= nc <= kMaxDim

    // stage the block in solver orientation; scipy's validity test on the way
    const float *blk = cost + (int64_t)prob * Q * Gmax;
    bool bad = false;
    for (int idx = lane; idx < Q * G; idx += kWave) {
        const int q = idx / G, g = idx - q * G;
        const float c = blk[q * Gmax + g];
        bad |= c != c || c == -INFINITY;
        C[tr ? g * Q + q : idx] = c;
    }
    for (int r = lane; r < nr; r += kWave) u[r] = 0.0, col4row[r] = -1;
    int code = __ballot(bad) != 0 ? 1 : 0;

    double v[kSlots], sp[kSlots];
    int path[kSlots], row4col[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) v[s] = 0.0, row4col[s] = -1;

    for (int cur = 0; cur < nr && code == 0; ++cur) {
        __syncthreads();                                            // the block; u and col4row of the row before
#pragma unroll
        for (int s = 0; s < kSlots; ++s) sp[s] = INFINITY, path[s] = -1;
        unsigned scanned = 0;
        double min_val = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step < nc && sink < 0; ++step) {         // a step scans one column
            const double ui = u[i];
            const float *row = C + i * nc;
            Key best = {INFINITY, INT_MAX};
#pragma unroll
            for (int s = 0; s < kSlots; ++s) {
                const int c = lane + kWave * s;
                if (c < nc && !((scanned >> s) & 1u)) {
                    const double r = min_val + (double)row[c] - ui - v[s];
                    if (r < sp[s]) sp[s] = r, path[s] = i;
                    const Key k = {sp[s], (row4col[s] >= 0 ? kAssignedBit : 0) | c};
                    if (before(k, best)) best = k;
                }
            }
            best = wave_min(best);
            if (!(best.val < INFINITY)) break;                      // nothing reachable: infeasible
            min_val = best.val;
            const int j = best.tie & (kAssignedBit - 1);
            if (lane == (j & 63)) scanned |= 1u << (j >> 6);
            if (!(best.tie & kAssignedBit)) {
                sink = j;
            } else {
                i = pick(row4col, j >> 6, j & 63);
                if ((unsigned)i >= (unsigned)nr) break;             // cannot happen; never index with it
            }
        }
        if (sink < 0) {
            code = 2;
            break;
        }
        // duals: scipy's u[i] += minVal - shortest[col4row[i]], v[j] -= minVal - shortest[j], from the column's side
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            if ((scanned >> s) & 1u) {
                const double d = min_val - sp[s];
                v[s] -= d;
                if (row4col[s] >= 0) u[row4col[s]] += d;            // < nr: only rows are ever stored there
            }
        }
        if (lane == 0) u[cur] += min_val;
        // flip the path from the sink back to cur; every lane stores the same word
        int j = sink;
        for (int step = 0; step <= nr; ++step) {
            const int slot = j >> 6, src = j & 63;
            const int pi = pick(path, slot, src);
            if ((unsigned)pi >= (unsigned)nr) {                     // cannot happen
                code = 2;
                break;
            }
#pragma unroll
            for (int s = 0; s < kSlots; ++s)
                if (s == slot && lane == src) row4col[s] = pi;
            const int prev = col4row[pi];
            col4row[pi] = j;
            if (pi == cur) break;
            j = prev;
            if ((unsigned)j >= (unsigned)nc) {                      // cannot happen
                code = 2;
                break;
            }
        }
    }
    __syncthreads();

    if (lane == 0) status[prob] = code;
    const int64_t q0 = (int64_t)n * Q;
    if (code != 0) {
        for (int k = lane; k < nr; k += kWave) t0[k] = q0 + k, t1[k] = (int64_t)o0 + k;
    } else if (!tr) {                                               // rows are the queries: all matched, already in order
        for (int q = lane; q < nr; q += kWave) {
            const int g = col4row[q];
            t0[q] = q0 + q, t1[q] = (int64_t)o0 + ((unsigned)g < (unsigned)nc ? g : 0);
        }
    } else {                                                        // columns are the queries: the assigned ones, ascending
        int done = 0;
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const int c = lane + kWave * s;
            const bool has = c < nc && row4col[s] >= 0;
            const uint64_t bits = __ballot(has);
            const int k = done + __popcll(bits & ((1ull << lane) - 1ull));
            if (has && k < nr) t0[k] = q0 + c, t1[k] = (int64_t)o0 + row4col[s];
            done += __popcll(bits);
        }
    }
}

int ptr_check(const char *fn, const char *name, const void *p, int align) {
    if (!p) return fail(VAH_E_NULL, "%s: null pointer (%s)", fn, name);
    if ((uintptr_t)p % align) return fail(VAH_E_ALIGN, "%s: %s misaligned (%d-byte pointer)", fn, name, align);
    return 0;
}

}  // namespace
}  // namespace vah

extern "C" {

int vah_assign_solve(const void *cost, const void *gt_offsets, int64_t L, int64_t N, int64_t Q, int64_t Gmax, void *table,
                     void *status, void *stream) {
    using namespace vah;
    const char *fn = "vah_assign_solve";
    clear_error();
    if (L < 0 || N < 0 || N > kMaxN || L >= ((int64_t)1 << 31) || L * N >= ((int64_t)1 << 31))
        return fail(VAH_E_SHAPE, "%s: bad dims (L %lld, N %lld; at most %lld images and fewer than 2^31 problems)", fn, (long long)L,
                    (long long)N, (long long)kMaxN);
    if (Q < 1 || Q > kMaxDim || Gmax < 0 || Gmax > kMaxDim || Q * Gmax > kMaxCells)
        return fail(VAH_E_UNSUPPORTED, "%s: Q %lld, Gmax %lld (1 <= Q <= %d, 0 <= Gmax <= %d, Q * Gmax <= %lld)", fn, (long long)Q,
                    (long long)Gmax, kMaxDim, kMaxDim, (long long)kMaxCells);
    if (L * N == 0 || Gmax == 0) return VAH_OK;
    if (int rc = ptr_check(fn, "cost", cost, 4)) return rc;
    if (int rc = ptr_check(fn, "gt_offsets", gt_offsets, 4)) return rc;
    if (int rc = ptr_check(fn, "table", table, 8)) return rc;
    if (int rc = ptr_check(fn, "status", status, 4)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int lds = kRowBytes + (int)(Q * Gmax) * 4;
    if (int rc = allow_dynamic_lds((const void *)assign_solve_kernel, lds, fn)) return rc;
    {
        LaunchScope scope("assign_solve", L * N * (Q * Gmax * 4 + 2 * Gmax * 8 + 4), st);
        hipLaunchKernelGGL(assign_solve_kernel, dim3((unsigned)(L * N)), dim3(kWave), lds, st, (const float *)cost, (const int *)gt_offsets,
                           (int)N, (int)Q, (int)Gmax, (int64_t *)table, (int *)status);
    }
    return check_launch(fn);
}

}  // extern "C"
