// The class counts of the mIoU evaluation (include/vitadapter_hip_seg_eval.h): predicted labels and ground truth in, 3 x C
// int64 totals added to, in two launches.
//   * seg_eval_count: a workgroup of 256 lanes walks a contiguous range of the N * H * W pixels, 512 at a step.  A lane owns
//     two consecutive pixels, so pred is one 16-byte load per lane and a wave reads 1 KiB at a time; kDepth steps are loaded
//     before the first is counted.  The kernel computes nothing, so what it costs beyond the loads is the LDS adds, three a
//     pixel if every pixel made its own.  Label maps are piecewise constant: the even pixels of a step and the odd ones are
//     each a sequence of 64 (pred, label) keys across the wave, one DPP shift and one ballot find the lanes where a run of
//     equal keys starts, and only those lanes add, the run's length.  One class everywhere is 6 adds per 128 pixels, a blob
//     map a few more, i.i.d. labels three per pixel (the worst case, bounded by the LDS atomic rate).  With 3 * C <= 1024
//     every wave counts into a histogram of its own, so the waves of a workgroup do not meet on one counter either.
//   * seg_eval_merge: 16 columns a workgroup, 64 lanes of partial rows per column, int64 sums, totals += .
// A value outside [0, C) becomes key part 0 before anything is indexed with it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vitadapter_hip_seg_eval.h"
#include "common.h"

namespace vah {
namespace {

constexpr int kThreads = 256;
constexpr int kStep = 2 * kThreads;         // pixels of a workgroup step
constexpr int kDepth = 4;                   // steps loaded before the first is counted
constexpr int64_t kMinChunk = 4096;         // pixels of a workgroup at least; a multiple of kStep * kDepth
constexpr int64_t kMaxChunk = (int64_t)1 << 30;
constexpr int kMaxParts = 1024, kMinParts = 64;
constexpr int64_t kRowBudget = (int64_t)1 << 21;    // counters in ws that the workgroup count aims to stay below
constexpr int kMaxC = 4096;                 // 13 bits of a key; 3 * C * 4 bytes of LDS
constexpr int kWaveCopies = 1024;           // 3 * C up to which every wave has a histogram of its own
constexpr int kMergeCols = 16, kMergeThreads = 1024;

struct Pos {
    unsigned n, y, x;
};

struct CountArgs {
    const int64_t *pred;
    int64_t pis, prs;
    const void *label;
    int64_t lis, lrs;
    const int64_t *map;
    int map_len;
    int *ws;
    int64_t total, chunk, ignore;
    unsigned H, W, HW;
    unsigned sn, sy, sx;        // kStep = sn * HW + sy * W + sx
    int C, reduce_zero, copies;
};

template <typename T>
using Two = T __attribute__((ext_vector_type(2)));

__device__ __forceinline__ Pos after(Pos q, unsigned H, unsigned W) {
    if (++q.x == W) {
        q.x = 0;
        if (++q.y == H) q.y = 0, ++q.n;
    }
    return q;
}

// the two pixels at q and after it; one load where they share a row.  A pixel past the range is not read
template <typename T>
__device__ __forceinline__ void load2(const T *base, int64_t is, int64_t rs, Pos q, unsigned H, unsigned W, bool v0, bool v1,
                                      int64_t &a, int64_t &b) {
    a = b = 0;
    if (!v0) return;
    const T *p = base + q.n * is + q.y * rs + q.x;
    if (v1 && q.x + 1 < W && (uintptr_t)p % sizeof(Two<T>) == 0) {       // pred: 16 bytes; an odd address takes the path below
        const Two<T> t = *reinterpret_cast<const Two<T> *>(p);
        a = (int64_t)t.x, b = (int64_t)t.y;
    } else {
        a = (int64_t)*p;
        if (v1) {
            const Pos r = after(q, H, W);
            b = (int64_t)base[r.n * is + r.y * rs + r.x];
        }
    }
}

// (class of pred + 1) << 13 | (class of label + 1), 0 in a part for a value outside [0, C); 0 for a pixel that counts for nothing
__device__ __forceinline__ int key_of(const CountArgs &a, int64_t p, int64_t g, bool valid) {
    if (a.map && (uint64_t)g < (uint64_t)a.map_len) g = a.map[g];
    if (a.reduce_zero) g = (g == 0 || g == 255) ? 255 : (int64_t)((uint64_t)g - 1);
    if (!valid || g == a.ignore) return 0;
    const int pi = (uint64_t)p < (uint64_t)a.C ? (int)p + 1 : 0;
    const int gi = (uint64_t)g < (uint64_t)a.C ? (int)g + 1 : 0;
    return pi << 13 | gi;
}

// the wave's 64 keys as runs of equal ones: the first lane of a run adds its length.  Called by whole waves only
__device__ __forceinline__ void count_runs(int *h, int C, int key) {
    const int prev = __builtin_amdgcn_update_dpp(-1, key, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);     // lane 0 keeps -1: no key
    const bool head = key != prev;
    const uint64_t heads = __ballot(head);
    if (head && key) {
        const int lane = (int)(threadIdx.x & 63);
        const uint64_t later = lane == 63 ? 0 : heads >> (lane + 1);
        const int len = later ? __builtin_ctzll(later) + 1 : 64 - lane;
        const int pi = key >> 13, gi = key & 0x1fff;
        if (pi) atomicAdd(&h[C + pi - 1], len);
        if (gi) atomicAdd(&h[2 * C + gi - 1], len);
        if (pi && pi == gi) atomicAdd(&h[pi - 1], len);
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void seg_eval_count_kernel(const CountArgs a) {
    extern __shared__ int hist[];
    const int cols = 3 * a.C, tid = (int)threadIdx.x;
    for (int k = tid; k < cols * a.copies; k += kThreads) hist[k] = 0;
    __syncthreads();
    int *h = hist + (a.copies > 1 ? (tid >> 6) * cols : 0);

    const int64_t base = (int64_t)blockIdx.x * a.chunk;
    const int64_t end = base + a.chunk < a.total ? base + a.chunk : a.total;
    int64_t idx = base + 2 * tid;
    Pos q;
    {
        const int64_t n = idx / a.HW;
        const unsigned r = (unsigned)(idx - n * a.HW);
        q.n = (unsigned)n, q.y = r / a.W, q.x = r - q.y * a.W;
    }
    const T *label = static_cast<const T *>(a.label);
    for (int64_t at = base; at < end; at += kStep * kDepth) {          // uniform over the workgroup
        int64_t p[kDepth][2], g[kDepth][2];
        bool v[kDepth][2];
#pragma unroll
        for (int d = 0; d < kDepth; ++d) {
            v[d][0] = idx < end, v[d][1] = idx + 1 < end;
            load2(a.pred, a.pis, a.prs, q, a.H, a.W, v[d][0], v[d][1], p[d][0], p[d][1]);
            load2(label, a.lis, a.lrs, q, a.H, a.W, v[d][0], v[d][1], g[d][0], g[d][1]);
            idx += kStep;
            q.x += a.sx;
            if (q.x >= a.W) q.x -= a.W, ++q.y;
            q.y += a.sy;
            if (q.y >= a.H) q.y -= a.H, ++q.n;
            q.n += a.sn;
        }
#pragma unroll
        for (int d = 0; d < kDepth; ++d) {
            count_runs(h, a.C, key_of(a, p[d][0], g[d][0], v[d][0]));
            count_runs(h, a.C, key_of(a, p[d][1], g[d][1], v[d][1]));
        }
    }
    __syncthreads();
    int *row = a.ws + (int64_t)blockIdx.x * cols;
    for (int k = tid; k < cols; k += kThreads) {
        int s = hist[k];
        for (int c = 1; c < a.copies; ++c) s += hist[c * cols + k];
        row[k] = s;
    }
}

__global__ __launch_bounds__(kMergeThreads) void seg_eval_merge_kernel(const int *ws, int64_t parts, int cols, int64_t *totals) {
    __shared__ int64_t s[kMergeThreads];
    const int tid = (int)threadIdx.x, col = (int)blockIdx.x * kMergeCols + (tid & (kMergeCols - 1));
    int64_t acc = 0;
    if (col < cols) {
#pragma unroll 4
        for (int64_t part = tid / kMergeCols; part < parts; part += kMergeThreads / kMergeCols) acc += ws[part * cols + col];
    }
    s[tid] = acc;
    __syncthreads();
    for (int step = kMergeThreads / 2; step >= kMergeCols; step >>= 1) {
        if (tid < step) s[tid] += s[tid + step];
        __syncthreads();
    }
    if (tid < kMergeCols && col < cols) totals[col] += s[tid];
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
constexpr int64_t kLim = (int64_t)1 << 31;

bool bad_size(int64_t v) { return v < 0 || v >= kLim; }

// pixels of a workgroup: a multiple of kStep * kDepth below 2^31
int64_t chunk_of(int64_t total, int64_t C) {
    int64_t cap = kRowBudget / (3 * C);
    cap = cap > kMaxParts ? kMaxParts : cap < kMinParts ? kMinParts : cap;
    const int64_t unit = (int64_t)kStep * kDepth;
    int64_t chunk = ((total + cap - 1) / cap + unit - 1) / unit * unit;
    return chunk < kMinChunk ? kMinChunk : chunk > kMaxChunk ? kMaxChunk : chunk;
}

int64_t parts_of(int64_t total, int64_t C) {
    const int64_t chunk = chunk_of(total, C);
    return (total + chunk - 1) / chunk;
}

int map_check(const char *fn, const char *name, const void *p, int align, int64_t is, int64_t rs, int64_t H, int64_t W) {
    if (!p) return fail(VAH_E_NULL, "%s: null pointer (%s)", fn, name);
    if ((uintptr_t)p % align) return fail(VAH_E_ALIGN, "%s: %s misaligned (%d-byte pointer)", fn, name, align);
    if (rs < W || is < (H - 1) * rs + W)
        return fail(VAH_E_SHAPE, "%s: %s strides (row stride >= width, images that do not overlap)", fn, name);
    return 0;
}

}  // namespace
}  // namespace vah

extern "C" {

int64_t vah_segeval_ws_bytes(int64_t N, int64_t H, int64_t W, int64_t C) {
    using namespace vah;
    if (N < 1 || H < 1 || W < 1 || C < 1 || C > kMaxC || N > 65535 || bad_size(H) || bad_size(W) || H * W >= kLim) return 0;
    return parts_of(N * H * W, C) * 3 * C * 4;
}

int vah_segeval_update(const void *pred, int64_t pred_img_stride, int64_t pred_row_stride, const void *label, int label_dtype,
                       int64_t label_img_stride, int64_t label_row_stride, int64_t N, int64_t H, int64_t W, int64_t C,
                       int64_t ignore_index, int reduce_zero_label, const void *label_map, int64_t label_map_len, void *totals,
                       void *ws, int64_t ws_bytes, void *stream) {
    using namespace vah;
    const char *fn = "vah_segeval_update";
    clear_error();
    if (bad_size(N) || bad_size(H) || bad_size(W) || N > 65535 || H * W >= kLim || C < 1)
        return fail(VAH_E_SHAPE, "%s: bad dims (N %lld, %lld x %lld, C %lld; an image has fewer than 2^31 pixels)", fn, (long long)N,
                    (long long)H, (long long)W, (long long)C);
    if (C > kMaxC) return fail(VAH_E_UNSUPPORTED, "%s: C %lld (at most %d classes)", fn, (long long)C, kMaxC);
    if (label_dtype < 0 || label_dtype > 1)
        return fail(VAH_E_UNSUPPORTED, "%s: label dtype codes are 0 (int64) and 1 (uint8), not %d", fn, label_dtype);
    if (label_map_len < 0 || label_map_len > 256)
        return fail(VAH_E_SHAPE, "%s: label_map_len %lld (a table of at most 256 entries)", fn, (long long)label_map_len);
    if (N * H * W == 0) return VAH_OK;
    if (int rc = map_check(fn, "pred", pred, 8, pred_img_stride, pred_row_stride, H, W)) return rc;
    if (int rc = map_check(fn, "label", label, label_dtype == 0 ? 8 : 1, label_img_stride, label_row_stride, H, W)) return rc;
    if ((uintptr_t)label_map % 8) return fail(VAH_E_ALIGN, "%s: label_map misaligned (8-byte pointer)", fn);
    if (!totals) return fail(VAH_E_NULL, "%s: null pointer (totals)", fn);
    if ((uintptr_t)totals % 8) return fail(VAH_E_ALIGN, "%s: totals misaligned (8-byte pointer)", fn);
    if (!ws) return fail(VAH_E_NULL, "%s: null pointer (ws)", fn);
    if ((uintptr_t)ws % 16) return fail(VAH_E_ALIGN, "%s: ws misaligned (16-byte pointer)", fn);
    const int64_t total = N * H * W, chunk = chunk_of(total, C), parts = (total + chunk - 1) / chunk, cols = 3 * C;
    if (ws_bytes < parts * cols * 4)
        return fail(VAH_E_SHAPE, "%s: workspace too small (%lld bytes, vah_segeval_ws_bytes says %lld)", fn, (long long)ws_bytes,
                    (long long)(parts * cols * 4));
    hipStream_t st = (hipStream_t)stream;
    CountArgs a;
    a.pred = (const int64_t *)pred, a.pis = pred_img_stride, a.prs = pred_row_stride;
    a.label = label, a.lis = label_img_stride, a.lrs = label_row_stride;
    a.map = label_map_len ? (const int64_t *)label_map : nullptr, a.map_len = (int)label_map_len;
    a.ws = (int *)ws;
    a.total = total, a.chunk = chunk, a.ignore = ignore_index;
    a.H = (unsigned)H, a.W = (unsigned)W, a.HW = (unsigned)(H * W);
    a.sn = (unsigned)(kStep / (H * W)), a.sy = (unsigned)(kStep % (H * W) / W), a.sx = (unsigned)(kStep % (H * W) % W);
    a.C = (int)C, a.reduce_zero = reduce_zero_label ? 1 : 0, a.copies = cols <= kWaveCopies ? kThreads / kWave : 1;
    const int64_t lbytes = label_dtype == 0 ? 8 : 1;
    {
        LaunchScope scope("seg_eval_count", total * (8 + lbytes) + parts * cols * 4, st);
        const dim3 grid((unsigned)parts), block(kThreads);
        const size_t lds = (size_t)a.copies * cols * 4;
        if (label_dtype == 0) hipLaunchKernelGGL(seg_eval_count_kernel<int64_t>, grid, block, lds, st, a);
        else hipLaunchKernelGGL(seg_eval_count_kernel<uint8_t>, grid, block, lds, st, a);
    }
    {
        LaunchScope scope("seg_eval_merge", parts * cols * 4 + cols * 16, st);
        hipLaunchKernelGGL(seg_eval_merge_kernel, dim3((unsigned)((cols + kMergeCols - 1) / kMergeCols)), dim3(kMergeThreads), 0, st,
                           (const int *)ws, parts, (int)cols, (int64_t *)totals);
    }
    return check_launch(fn);
}

}  // extern "C"
