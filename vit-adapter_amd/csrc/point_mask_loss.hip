// The sampled mask losses of the matched queries of Mask2Former's training head and their backward into mask_pred
// (include/vitadapter_hip_point_mask_loss.h): the reference's segmentation/mmseg_custom/models/decode_heads/mask2former_head.py:338-356.
//
// Like point_loss.hip these are gather and latency kernels, nothing here is near a bandwidth or a matrix limit; what they
// replace is several dozen small launches per decoder output and a backward that scatters with float atomics.
//   * forward: the sampling of point_sample.h on both maps (prediction rows read in place through `rows`), all 32 taps of a
//     thread's four points loaded before the first is used, the four sums of a chunk of 1024 points in the order of
//     vah_pts_match_cost, a merge launch that adds the chunks in ascending order (the chunk + merge pattern of masked_attn.hip):
//     24 rows alone cannot fill 256 CUs, 24 x 13 chunks do.
//   * backward in gather form, as resize_rows.hip: points are binned by cell with INTEGER counts (a count does not depend on
//     the order of its increments), each list is sorted by point index, one thread per pixel adds the lists of its four cells
//     in a fixed order.  Float sums never meet an atomic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/vitadapter_hip_point_mask_loss.h"
#include "point_sample.h"

namespace vah {
namespace {

constexpr int kU = 4;                       // points per thread of the forward
constexpr int kChunk = 256 * kU;            // points per workgroup of the forward

// ---------------------------------------------------------------------------------------
// forward: block b -> row b / chunks, points [(b % chunks) * 1024, +1024): 4 per thread, 256 apart
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pml_forward_kernel(const float *__restrict__ pred, int64_t pms, int prs, int Mp, int h, int w,
                                                          const T *__restrict__ tgt, int64_t tms, int trs, int Mt, int H, int W,
                                                          const float2 *__restrict__ points, int P, const int *__restrict__ rows,
                                                          const int *__restrict__ tgt_rows, unsigned chunks,
                                                          float *__restrict__ xs, float *__restrict__ ts, float *__restrict__ part) {
    __shared__ float slot[4];
    const unsigned k = blockIdx.x / chunks, chunk = blockIdx.x - k * chunks;
    const int m = rows ? rows[k] : (int)k, mt = tgt_rows ? tgt_rows[k] : (int)k;
    const int p0 = (int)chunk * kChunk + (int)threadIdx.x;
    float *xo = xs + (int64_t)k * P, *to = ts + (int64_t)k * P;
    float *po = part + (int64_t)blockIdx.x * 4;
    if (m < 0 || m >= Mp || mt < 0 || mt >= Mt) {       // block-uniform
#pragma unroll
        for (int u = 0; u < kU; ++u)
            if (p0 + u * 256 < P) xo[p0 + u * 256] = to[p0 + u * 256] = quiet_nan();
        if (threadIdx.x < 4) po[threadIdx.x] = quiet_nan();
        return;
    }
    const float *pmap = pred + (int64_t)m * pms;
    const T *tmap = tgt + (int64_t)mt * tms;
    const float2 *pts = points + (int64_t)k * P;
    Taps tp[kU], tt[kU];
    Quad qp[kU], qt[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        const float2 pt = pts[min(p0 + u * 256, P - 1)];
        tp[u] = taps_of(pt, h, w);
        tt[u] = taps_of(pt, H, W);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        qp[u] = load_quad(pmap, prs, h, w, tp[u]);
        qt[u] = load_quad(tmap, trs, H, W, tt[u]);
    }
    float bce = 0.f, a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        if (p0 + u * 256 < P) {
            const float x = combine(qp[u], tp[u], h, w), t = combine(qt[u], tt[u], H, W);
            xo[p0 + u * 256] = x;
            to[p0 + u * 256] = t;
            const Terms e = terms_of(x);
            bce += e.sp_pos - x * t;
            a += e.s * t;
            b += e.s;
            c += t;
        }
    }
    a = block_sum<4>(a, slot);
    b = block_sum<4>(b, slot);
    c = block_sum<4>(c, slot);
    bce = block_sum<4>(bce, slot);
    if (threadIdx.x == 0) {
        po[0] = a;
        po[1] = b;
        po[2] = c;
        po[3] = bce;
    }
}

// one thread per row: the chunks in ascending order
__global__ __launch_bounds__(64) void pml_merge_kernel(const float *__restrict__ part, int K, int chunks, float eps,
                                                       float *__restrict__ bce, float *__restrict__ dice, float *__restrict__ sums) {
    const int k = (int)(blockIdx.x * 64 + threadIdx.x);
    if (k >= K) return;
    const float *p = part + (int64_t)k * chunks * 4;
    float a = p[0], b = p[1], c = p[2], e = p[3];
    for (int i = 1; i < chunks; ++i) {
        a += p[4 * i];
        b += p[4 * i + 1];
        c += p[4 * i + 2];
        e += p[4 * i + 3];
    }
    float *s = sums + (int64_t)k * 4;
    s[0] = a;
    s[1] = b;
    s[2] = c;
    s[3] = e;
    bce[k] = e;
    dice[k] = 1.f - (2.f * a + eps) / ((b + c) + eps);
}

// ---------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------
// cell of a point, or -1 when none of its taps is in range
__device__ __forceinline__ int cell_of(const Taps t, int h, int w) {
    if (t.x0 < -1 || t.x0 > w - 1 || t.y0 < -1 || t.y0 > h - 1) return -1;
    return (t.y0 + 1) * (w + 1) + (t.x0 + 1);
}

// thread -> (k, p): gx and the count of the point's cell
__global__ __launch_bounds__(256) void pml_bwd_gx_kernel(const float2 *__restrict__ points, const float *__restrict__ xs,
                                                         const float *__restrict__ ts, const float *__restrict__ sums,
                                                         const float *__restrict__ g_bce, const float *__restrict__ g_dice, int P,
                                                         int h, int w, int cells, unsigned blocks, float eps, float *__restrict__ gx,
                                                         int *__restrict__ off) {
    const unsigned k = blockIdx.x / blocks;
    const int p = (int)(blockIdx.x - k * blocks) * 256 + (int)threadIdx.x;
    if (p >= P) return;
    const int64_t i = (int64_t)k * P + p;
    const float *s4 = sums + (int64_t)k * 4;
    const float A = s4[0], D = (s4[1] + s4[2]) + eps;
    const float x = xs[i], t = ts[i];
    const Terms e = terms_of(x);
    gx[i] = g_bce[k] * (e.s - t) + g_dice[k] * (e.s * (1.f - e.s)) * ((2.f * A + eps) / (D * D) - 2.f * t / D);
    const int c = cell_of(taps_of(points[i], h, w), h, w);
    if (c >= 0) atomicAdd(off + (int64_t)k * cells + c, 1);
}

// workgroup -> row: counts to exclusive starts, in place
__global__ __launch_bounds__(1024) void pml_bwd_scan_kernel(int *__restrict__ off, int cells) {
    __shared__ int part[1024];
    int *o = off + (int64_t)blockIdx.x * cells;
    const int tid = (int)threadIdx.x, seg = (cells + 1023) / 1024;
    const int lo = (int)min((int64_t)tid * seg, (int64_t)cells), hi = (int)min((int64_t)lo + seg, (int64_t)cells);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += o[i];
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - s;
    for (int i = lo; i < hi; ++i) {
        const int c = o[i];
        o[i] = run;
        run += c;
    }
}

// thread -> (k, p): the point takes the next place of its cell's list; afterwards off[c] is the END of cell c
__global__ __launch_bounds__(256) void pml_bwd_fill_kernel(const float2 *__restrict__ points, int P, int h, int w, int cells,
                                                           unsigned blocks, int *__restrict__ off, int *__restrict__ list) {
    const unsigned k = blockIdx.x / blocks;
    const int p = (int)(blockIdx.x - k * blocks) * 256 + (int)threadIdx.x;
    if (p >= P) return;
    const int c = cell_of(taps_of(points[(int64_t)k * P + p], h, w), h, w);
    if (c < 0) return;
    const int pos = atomicAdd(off + (int64_t)k * cells + c, 1);
    if (pos >= 0 && pos < P) list[(int64_t)k * P + pos] = p;
}

struct Span {
    int lo, hi;
};

__device__ __forceinline__ Span span_of(const int *__restrict__ o, int c, int P) {
    Span s;
    s.lo = c ? o[c - 1] : 0;
    s.hi = o[c];
    s.lo = clampi(s.lo, 0, P);
    s.hi = clampi(s.hi, s.lo, P);
    return s;
}

// thread -> (k, cell): the cell's list into ascending point index
__global__ __launch_bounds__(256) void pml_bwd_sort_kernel(const int *__restrict__ off, int P, int cells, unsigned blocks,
                                                           int *__restrict__ list) {
    const unsigned k = blockIdx.x / blocks;
    const int c = (int)(blockIdx.x - k * blocks) * 256 + (int)threadIdx.x;
    if (c >= cells) return;
    const Span s = span_of(off + (int64_t)k * cells, c, P);
    int *l = list + (int64_t)k * P;
    for (int i = s.lo + 1; i < s.hi; ++i) {
        const int v = l[i];
        int j = i - 1;
        while (j >= s.lo && l[j] > v) {
            l[j + 1] = l[j];
            --j;
        }
        l[j + 1] = v;
    }
}

// thread -> (k, y, x): the four cells in ascending cell number, each list in ascending p
__global__ __launch_bounds__(256) void pml_bwd_gather_kernel(const float2 *__restrict__ points, const float *__restrict__ gx,
                                                             const int *__restrict__ off, const int *__restrict__ list, int P, int h,
                                                             int w, int cells, unsigned blocks, float *__restrict__ dmaps) {
    const unsigned k = blockIdx.x / blocks;
    const int px = (int)(blockIdx.x - k * blocks) * 256 + (int)threadIdx.x;
    if (px >= h * w) return;
    const int y = px / w, x = px - y * w;
    const int *o = off + (int64_t)k * cells, *l = list + (int64_t)k * P;
    const float2 *pts = points + (int64_t)k * P;
    const float *g = gx + (int64_t)k * P;
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int dy = 1 - (q >> 1), dx = 1 - (q & 1);            // the pixel is tap (dy, dx) of cell (y - dy, x - dx)
        const Span s = span_of(o, (y + 1 - dy) * (w + 1) + (x + 1 - dx), P);
        for (int i = s.lo; i < s.hi; ++i) {
            const int p = clampi(l[i], 0, P - 1);
            const Taps t = taps_of(pts[p], h, w);
            const float wy = dy ? t.fy : 1.f - t.fy, wx = dx ? t.fx : 1.f - t.fx;
            acc += (wy * wx) * g[p];
        }
    }
    dmaps[(int64_t)k * h * w + px] = acc;
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
int64_t chunks_of(int64_t P) { return (P + kChunk - 1) / kChunk; }

int64_t ws_bytes_of(int64_t K, int64_t P, int64_t h, int64_t w) {
    const int64_t fwd = 4 * K * chunks_of(P) * 4, bwd = 4 * K * (2 * P + (h + 1) * (w + 1));
    return ((fwd > bwd ? fwd : bwd) + 15) / 16 * 16;
}

int dims_check(const char *fn, int64_t K, int64_t P, int64_t h, int64_t w) {
    if (K < 0 || K >= kLim || P >= kLim || h >= kLim || w >= kLim)
        return fail(VAH_E_SHAPE, "%s: bad dims (K %lld, P %lld, h %lld, w %lld)", fn, (long long)K, (long long)P, (long long)h, (long long)w);
    if (P <= 0) return fail(VAH_E_SHAPE, "%s: P must be positive (P %lld)", fn, (long long)P);
    return 0;
}

int size_check(const char *fn, int64_t K, int64_t P, int64_t h, int64_t w) {
    const int64_t cells = (h + 1) * (w + 1);
    if (K * (P > cells ? P : cells) >= kLim)
        return fail(VAH_E_SHAPE, "%s: bad dims (K * max(P, (h + 1) * (w + 1)) must stay below 2^31)", fn);
    return 0;
}

int ws_check(const char *fn, const void *ws, int64_t ws_bytes, int64_t need) {
    if (!ws) return fail(VAH_E_NULL, "%s: null pointer (ws)", fn);
    if ((uintptr_t)ws % 16) return fail(VAH_E_ALIGN, "%s: ws misaligned (16-byte pointer)", fn);
    if (ws_bytes < need) return fail(VAH_E_SHAPE, "%s: workspace too small (%lld bytes, vah_pml_ws_bytes says %lld)", fn,
                                     (long long)ws_bytes, (long long)need);
    return 0;
}

}  // namespace
}  // namespace vah

extern "C" {

int64_t vah_pml_ws_bytes(int64_t K, int64_t P, int64_t h, int64_t w) {
    using namespace vah;
    if (K < 1 || P < 1 || h < 1 || w < 1 || K >= kLim || P >= kLim || h >= kLim || w >= kLim || (h + 1) * (w + 1) >= kLim) return 0;
    if (K * (P > (h + 1) * (w + 1) ? P : (h + 1) * (w + 1)) >= kLim) return 0;
    return ws_bytes_of(K, P, h, w);
}

int vah_pml_forward(const void *pred, int64_t pred_map_stride, int64_t pred_row_stride, int64_t Mp, int64_t h, int64_t w,
                    const void *tgt, int tgt_dtype, int64_t tgt_map_stride, int64_t tgt_row_stride, int64_t Mt, int64_t H, int64_t W,
                    const void *points, int64_t P, const void *rows, const void *tgt_rows, int64_t K, float dice_eps, void *bce,
                    void *dice, void *xs, void *ts, void *sums, void *ws, int64_t ws_bytes, void *stream) {
    using namespace vah;
    const char *fn = "vah_pml_forward";
    clear_error();
    if (int rc = dims_check(fn, K, P, h, w)) return rc;
    if (tgt_dtype != 0 && tgt_dtype != 3) return fail(VAH_E_UNSUPPORTED, "%s: dtype codes of a map are 0 (fp32) and 3 (uint8) (tgt)", fn);
    if (K == 0) return VAH_OK;
    if (int rc = map_check(fn, "pred", pred, 0, pred_map_stride, pred_row_stride, Mp, h, w)) return rc;
    if (int rc = map_check(fn, "tgt", tgt, tgt_dtype, tgt_map_stride, tgt_row_stride, Mt, H, W)) return rc;
    if (int rc = size_check(fn, K, P, h, w)) return rc;
    if ((!rows && K > Mp) || (!tgt_rows && K > Mt))
        return fail(VAH_E_SHAPE, "%s: index out of range (identity rows: K %lld, Mp %lld, Mt %lld)", fn, (long long)K, (long long)Mp, (long long)Mt);
    const Arr arrs[] = {{"points", points, 8, false}, {"rows", rows, 4, true}, {"tgt_rows", tgt_rows, 4, true}, {"bce", bce, 4, false},
                        {"dice", dice, 4, false},     {"xs", xs, 4, false},    {"ts", ts, 4, false},            {"sums", sums, 4, false}};
    if (int rc = arr_check(fn, arrs)) return rc;
    if (int rc = ws_check(fn, ws, ws_bytes, ws_bytes_of(K, P, h, w))) return rc;
    const int64_t chunks = chunks_of(P);
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope("pml_forward", K * P * (8 + 8 + 4 * 4 + 4 * (tgt_dtype ? 1 : 4)), st);
    const dim3 grid((unsigned)(K * chunks)), block(256);
    float *part = (float *)ws;
    if (tgt_dtype == 0)
        hipLaunchKernelGGL(pml_forward_kernel<float>, grid, block, 0, st, (const float *)pred, pred_map_stride, (int)pred_row_stride, (int)Mp,
                           (int)h, (int)w, (const float *)tgt, tgt_map_stride, (int)tgt_row_stride, (int)Mt, (int)H, (int)W,
                           (const float2 *)points, (int)P, (const int *)rows, (const int *)tgt_rows, (unsigned)chunks, (float *)xs,
                           (float *)ts, part);
    else
        hipLaunchKernelGGL(pml_forward_kernel<uint8_t>, grid, block, 0, st, (const float *)pred, pred_map_stride, (int)pred_row_stride,
                           (int)Mp, (int)h, (int)w, (const uint8_t *)tgt, tgt_map_stride, (int)tgt_row_stride, (int)Mt, (int)H, (int)W,
                           (const float2 *)points, (int)P, (const int *)rows, (const int *)tgt_rows, (unsigned)chunks, (float *)xs,
                           (float *)ts, part);
    hipLaunchKernelGGL(pml_merge_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, st, (const float *)part, (int)K, (int)chunks,
                       dice_eps, (float *)bce, (float *)dice, (float *)sums);
    return check_launch(fn);
}

int vah_pml_backward(const void *points, const void *xs, const void *ts, const void *sums, const void *g_bce, const void *g_dice,
                     int64_t K, int64_t P, int64_t h, int64_t w, float dice_eps, void *dmaps, void *ws, int64_t ws_bytes,
                     void *stream) {
    using namespace vah;
    const char *fn = "vah_pml_backward";
    clear_error();
    if (int rc = dims_check(fn, K, P, h, w)) return rc;
    if (K == 0) return VAH_OK;
    if (h < 1 || w < 1 || (h + 1) * (w + 1) >= kLim)
        return fail(VAH_E_SHAPE, "%s: bad dims (maps of %lld x %lld)", fn, (long long)h, (long long)w);
    if (int rc = size_check(fn, K, P, h, w)) return rc;
    const Arr arrs[] = {{"points", points, 8, false}, {"xs", xs, 4, false},         {"ts", ts, 4, false},      {"sums", sums, 4, false},
                        {"g_bce", g_bce, 4, false},   {"g_dice", g_dice, 4, false}, {"dmaps", dmaps, 4, false}};
    if (int rc = arr_check(fn, arrs)) return rc;
    if (int rc = ws_check(fn, ws, ws_bytes, ws_bytes_of(K, P, h, w))) return rc;
    const int64_t cells = (h + 1) * (w + 1);
    const int64_t bp = (P + 255) / 256, bc = (cells + 255) / 256, bx = (h * w + 255) / 256;
    float *gx = (float *)ws;
    int *list = (int *)ws + K * P, *off = (int *)ws + 2 * K * P;
    hipStream_t st = (hipStream_t)stream;
    LaunchScope scope("pml_backward", 4 * (K * P * (2 + 2 + 1 + 2 + 4) + K * cells * 4 + K * h * w), st);
    if (hipMemsetAsync(off, 0, (size_t)(4 * K * cells), st) != hipSuccess) return check_launch(fn);
    const dim3 block(256);
    hipLaunchKernelGGL(pml_bwd_gx_kernel, dim3((unsigned)(K * bp)), block, 0, st, (const float2 *)points, (const float *)xs,
                       (const float *)ts, (const float *)sums, (const float *)g_bce, (const float *)g_dice, (int)P, (int)h, (int)w,
                       (int)cells, (unsigned)bp, dice_eps, gx, off);
    hipLaunchKernelGGL(pml_bwd_scan_kernel, dim3((unsigned)K), dim3(1024), 0, st, off, (int)cells);
    hipLaunchKernelGGL(pml_bwd_fill_kernel, dim3((unsigned)(K * bp)), block, 0, st, (const float2 *)points, (int)P, (int)h, (int)w,
                       (int)cells, (unsigned)bp, off, list);
    hipLaunchKernelGGL(pml_bwd_sort_kernel, dim3((unsigned)(K * bc)), block, 0, st, (const int *)off, (int)P, (int)cells, (unsigned)bc,
                       list);
    hipLaunchKernelGGL(pml_bwd_gather_kernel, dim3((unsigned)(K * bx)), block, 0, st, (const float2 *)points, (const float *)gx,
                       (const int *)off, (const int *)list, (int)P, (int)h, (int)w, (int)cells, (unsigned)bx, (float *)dmaps);
    return check_launch(fn);
}

}  // extern "C"
