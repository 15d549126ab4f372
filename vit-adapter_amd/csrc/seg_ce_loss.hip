// The training loss of the UperNet heads (include/vitadapter_hip_seg_loss.h): mmseg's BaseDecodeHead.losses - bilinear
// resize of the logits to the label map, cross-entropy with an ignore index, top-1 count - and its backward into the
// low-resolution logits, without a tensor of N * C * H * W elements.
//   * forward: a thread owns an output pixel, consecutive lanes consecutive x (seg_finish's layout, and its tap function).
//     The classes are walked once, kU at a time with 4 kU loads of the small, cached source in flight: running maximum, sum
//     rescaled when the maximum moves, running argmax, the label's logit.  One fp32 lse per pixel is all that stays.  A
//     workgroup leaves one partial (loss, valid, correct); a one-workgroup merge launch adds them in a fixed order.
//   * backward in gather form, as resize_rows.hip: a tables launch writes the taps of every output row / column and, per
//     source row / column, the range [lo, hi) of output positions whose taps name it.  A workgroup of one wave owns a
//     kTH x kTW tile of source pixels for a run of R classes and stages the tile with a one-pixel halo in LDS (every tap of
//     an output pixel that names a tile pixel lies inside the halo).  A lane owns a source pixel and walks its output rows
//     and columns in ascending order; per output pixel it reads lse and the label once, per class four LDS words, the
//     forward's blend (the same bits), one expf and one multiply-add into an fp32 accumulator.  R is 16, 8 or 4: the largest
//     run that still leaves a workgroup for every SIMD (a 16x upsample from a 32 x 32 map has 32 tiles only).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/vitadapter_hip_seg_loss.h"
#include "common.h"
#include "elem16.h"
#include "resize_tap.h"

namespace vah {
namespace {

constexpr int kU = 4;                   // classes in flight in the forward: 16 loads per thread
constexpr int kTH = 4, kTW = 16;        // the backward's tile of source pixels: one wave
constexpr int kPH = kTH + 2, kPW = kTW + 2, kPlane = kPH * kPW;
constexpr int kMerge = 256;             // threads of the merge launch

struct Logits {                 // an (N, C, h, w) tensor of T
    const void *p;
    int64_t is, ps, rs;
};

struct Labels {
    const int64_t *p;
    int64_t is, rs;
};

struct FwdArgs {
    Logits x;
    Labels y;
    const float *cw;
    float *lse, *part_loss;
    int *part_cnt;              // [partials][2]: valid, correct
    Axis ay, ax;
    int C, W;
    unsigned items;             // H * W
    int64_t ignore;
};

// sum over the 256 threads: wave_sum, then the four waves in ascending order; valid in thread 0
__device__ __forceinline__ float block_sum256(float v, float *slot) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

template <typename T>
__global__ __launch_bounds__(256) void sce_fwd_kernel(const FwdArgs a) {
    __shared__ float slot[4];
    __shared__ int cnt[4][2];
    const unsigned pix0 = blockIdx.x * 256 + threadIdx.x;
    const bool live = pix0 < a.items;
    const unsigned pix = live ? pix0 : a.items - 1;         // a spare thread repeats the last pixel and stores nothing
    const int oy = (int)(pix / (unsigned)a.W), ox = (int)(pix - (unsigned)oy * (unsigned)a.W);
    const Tap ty = tap_of(a.ay, oy), tx = tap_of(a.ax, ox);
    const int64_t o00 = ty.i0 * a.x.rs + tx.i0, o01 = ty.i0 * a.x.rs + tx.i1, o10 = ty.i1 * a.x.rs + tx.i0,
                  o11 = ty.i1 * a.x.rs + tx.i1;
    const T *xp = (const T *)a.x.p + blockIdx.y * a.x.is;
    const int C = a.C;
    const int64_t label = a.y.p[blockIdx.y * a.y.is + (int64_t)oy * a.y.rs + ox];
    const bool valid = live && label != a.ignore && label >= 0 && label < C;
    const int yi = valid ? (int)label : -1;

    // m, s: running maximum and sum exp(v - m); bad: where torch's log_softmax is NaN for the whole pixel;
    // best, arg, nan: the first NaN wins and ends the search, otherwise the first strictly larger value (seg_argmax's rule)
    float m = -INFINITY, s = 0.f, vy = 0.f, best = 0.f;
    int arg = -1;
    bool bad = false, nan = false;
    for (int c = 0; c < C; c += kU) {
        float t[kU][4];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const T *q = xp + min(c + u, C - 1) * a.x.ps;           // a clamped class: loaded, never used
            t[u][0] = (float)q[o00], t[u][1] = (float)q[o01], t[u][2] = (float)q[o10], t[u][3] = (float)q[o11];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (c + u >= C) break;
            const float v = blend_rn(ty, tx, t[u][0], t[u][1], t[u][2], t[u][3]);
            bad |= !(v < INFINITY);             // NaN or +inf
            if (c + u == yi) vy = v;
            if (!nan && (arg < 0 || v > best || v != v)) best = v, arg = c + u, nan = v != v;
            if (v > m) {
                s = s * expf(m - v) + 1.f;      // m == -inf: s is 0 and stays 0 before the 1
                m = v;
            } else if (v > -INFINITY) {
                s += expf(v - m);
            }
        }
    }
    bad |= m == -INFINITY;                      // all -inf (then s == 0)
    const float lse = bad ? NAN : m + logf(s);
    if (live) a.lse[(int64_t)blockIdx.y * a.items + pix] = lse;
    const float loss = valid ? (a.cw ? a.cw[yi] : 1.f) * (lse - vy) : 0.f;
    const int nv = __popcll(__ballot(valid)), nc = __popcll(__ballot(valid && arg == yi));
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6][0] = nv, cnt[threadIdx.x >> 6][1] = nc;
    const float total = block_sum256(loss, slot);           // its barrier covers cnt as well
    if (threadIdx.x == 0) {
        const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        a.part_loss[b] = total;
        a.part_cnt[2 * b] = cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0];
        a.part_cnt[2 * b + 1] = cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1];
    }
}

// one workgroup: thread t adds partials t, t + 256, ... in ascending order, then the workgroup's sum as above
__global__ __launch_bounds__(kMerge) void sce_merge_kernel(const float *__restrict__ part_loss, const int *__restrict__ part_cnt,
                                                           int64_t parts, float *__restrict__ loss_sum, int64_t *__restrict__ counts) {
    __shared__ float slot[4];
    __shared__ long long cv[kMerge], cc[kMerge];
    float s = 0.f;
    long long v = 0, c = 0;
    for (int64_t i = threadIdx.x; i < parts; i += kMerge) {
        s += part_loss[i];
        v += part_cnt[2 * i];
        c += part_cnt[2 * i + 1];
    }
    cv[threadIdx.x] = v, cc[threadIdx.x] = c;
    s = block_sum256(s, slot);
    if (threadIdx.x == 0) {
        for (int i = 1; i < kMerge; ++i) v += cv[i], c += cc[i];
        *loss_sum = s;
        counts[0] = v;
        counts[1] = c;
    }
}

// workspace: float part_loss[parts], int part_cnt[parts][2], then (16-byte aligned) Tap ty[H], Tap tx[W], int2 ry[h], int2 rx[w]
struct Tables {
    Tap *ty, *tx;
    int2 *ry, *rx;
};

int64_t parts_of(int64_t N, int64_t H, int64_t W) { return N * ((H * W + 255) / 256); }

int64_t tables_offset(int64_t N, int64_t H, int64_t W) { return (12 * parts_of(N, H, W) + 15) / 16 * 16; }

int64_t ws_bytes_of(int64_t N, int64_t h, int64_t w, int64_t H, int64_t W) {
    return (tables_offset(N, H, W) + 16 * (H + W) + 8 * (h + w) + 15) / 16 * 16;
}

Tables tables_in(void *ws, int64_t N, int64_t h, int64_t H, int64_t W) {
    Tables t;
    t.ty = (Tap *)((char *)ws + tables_offset(N, H, W));
    t.tx = t.ty + H;
    t.ry = (int2 *)(t.tx + W);
    t.rx = t.ry + h;
    return t;
}

__global__ __launch_bounds__(256) void sce_tables_kernel(Axis ay, Axis ax, Tables tb) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < ay.out) tb.ty[t] = tap_of(ay, t);
    if (t < ax.out) tb.tx[t] = tap_of(ax, t);
    if (t < ay.in) tb.ry[t] = make_int2(bisect<false>(ay, t), bisect<true>(ay, t));
    if (t < ax.in) tb.rx[t] = make_int2(bisect<false>(ax, t), bisect<true>(ax, t));
}

struct BwdArgs {
    Logits x;
    Labels y;
    const float *cw, *lse, *scale;
    void *dx;
    int64_t dis, dps, drs;
    Tables tb;
    int C, h, w, W, tiles_x;
    unsigned items;             // H * W
    int64_t ignore;
};

template <typename T, int R>
__global__ __launch_bounds__(64) void sce_bwd_kernel(const BwdArgs a) {
    __shared__ float tile[R * kPlane];
    const int tyi = (int)blockIdx.x / a.tiles_x, txi = (int)blockIdx.x - tyi * a.tiles_x;
    const int y0 = tyi * kTH, x0 = txi * kTW, c0 = (int)blockIdx.y * R;
    const T *xp = (const T *)a.x.p + blockIdx.z * a.x.is;
    // the tile and its halo, coordinates clamped into the map (a clamped cell is one no tap names); classes past C repeat the last
    for (int i = (int)threadIdx.x; i < R * kPlane; i += 64) {
        const int r = i / kPlane, cell = i - r * kPlane, hy = cell / kPW, hx = cell - hy * kPW;
        const int sy = min(max(y0 + hy - 1, 0), a.h - 1), sx = min(max(x0 + hx - 1, 0), a.w - 1);
        tile[i] = (float)xp[min(c0 + r, a.C - 1) * a.x.ps + sy * a.x.rs + sx];
    }
    __syncthreads();
    const int iy = y0 + (int)threadIdx.x / kTW, ix = x0 + (int)threadIdx.x % kTW;
    if (iy >= a.h || ix >= a.w) return;
    const int2 ry = a.tb.ry[iy], rx = a.tb.rx[ix];
    const float scale = *a.scale;
    const float *lse = a.lse + (int64_t)blockIdx.z * a.items;
    const int64_t *lab = a.y.p + blockIdx.z * a.y.is;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    for (int oy = ry.x; oy < ry.y; ++oy) {
        const Tap ty = a.tb.ty[oy];
        const float wy = weight_of(ty, iy);
        const int r0 = (ty.i0 - y0 + 1) * kPW - x0 + 1, r1 = (ty.i1 - y0 + 1) * kPW - x0 + 1;
        const float *lrow = lse + (int64_t)oy * a.W;
        const int64_t *yrow = lab + (int64_t)oy * a.y.rs;
        if (rx.x >= rx.y) break;
        float l_next = lrow[rx.x];
        int64_t y_next = yrow[rx.x];
        for (int ox = rx.x; ox < rx.y; ++ox) {
            const float l = l_next;
            const int64_t label = y_next;
            const int nx = min(ox + 1, rx.y - 1);           // the next pixel's loads go out before this one's arithmetic
            l_next = lrow[nx];
            y_next = yrow[nx];
            const bool valid = label != a.ignore && label >= 0 && label < a.C;
            if (!valid && fabsf(l) < INFINITY) continue;    // ignored, finite lse: exactly nothing
            const Tap tx = a.tb.tx[ox];
            // an ignored pixel whose lse is not finite: NaN to every class it taps
            const float coef = valid ? (wy * weight_of(tx, ix)) * (scale * (a.cw ? a.cw[label] : 1.f)) : NAN;
            const int yl = valid ? (int)label - c0 : -1;
            const int o00 = r0 + tx.i0, o01 = r0 + tx.i1, o10 = r1 + tx.i0, o11 = r1 + tx.i1;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float *t = tile + r * kPlane;
                const float v = blend_rn(ty, tx, t[o00], t[o01], t[o10], t[o11]);
                acc[r] += coef * (expf(v - l) - (r == yl ? 1.f : 0.f));
            }
        }
    }
    T *dp = (T *)a.dx + blockIdx.z * a.dis + (int64_t)iy * a.drs + ix;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (c0 + r < a.C) dp[(c0 + r) * a.dps] = (T)acc[r];
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
constexpr int64_t kLim = (int64_t)1 << 31;

bool bad_size(int64_t v) { return v < 0 || v >= kLim; }

// pointer, alignment and stride rules of one (N, C, H, W) tensor (C == 0: a label map, one plane per image)
int planes_check(const char *fn, const char *name, const void *p, int align, int64_t is, int64_t ps, int64_t rs, int64_t C,
                 int64_t H, int64_t W) {
    if (!p) return fail(VAH_E_NULL, "%s: null pointer (%s)", fn, name);
    if ((uintptr_t)p % align) return fail(VAH_E_ALIGN, "%s: %s misaligned (%d-byte pointer)", fn, name, align);
    const int64_t plane = (H - 1) * rs + W;
    if (rs < W || (C && ps < plane) || is < (C ? (C - 1) * ps + plane : plane))
        return fail(VAH_E_SHAPE, "%s: %s strides (row stride >= width, planes and images that do not overlap)", fn, name);
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

// what the two calls check alike, up to the empty problem: 0 go on, 1 empty (VAH_OK), < 0 an error
int problem_check(const char *fn, int dtype, int64_t N, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W) {
    if (bad_size(N) || bad_size(C) || bad_size(h) || bad_size(w) || bad_size(H) || bad_size(W) || N > 65535 || C > 65535 * 4)
        return fail(VAH_E_SHAPE, "%s: bad dims (N %lld, C %lld, %lld x %lld -> %lld x %lld)", fn, (long long)N, (long long)C,
                    (long long)h, (long long)w, (long long)H, (long long)W);
    if (dtype < 0 || dtype > 2) return fail(VAH_E_UNSUPPORTED, "%s: dtype codes are 0 (fp32), 1 (bf16) and 2 (fp16), not %d", fn, dtype);
    if (N * C * H * W == 0) return 1;
    if (h < 1 || w < 1 || H * W >= kLim || h * w >= kLim)
        return fail(VAH_E_SHAPE, "%s: bad dims (an empty source, or a plane of 2^31 pixels or more)", fn);
    return 0;
}

int ws_check(const char *fn, const void *ws, int64_t ws_bytes, int64_t need) {
    if (!ws) return fail(VAH_E_NULL, "%s: null pointer (ws)", fn);
    if ((uintptr_t)ws % 16) return fail(VAH_E_ALIGN, "%s: ws misaligned (16-byte pointer)", fn);
    if (ws_bytes < need)
        return fail(VAH_E_SHAPE, "%s: workspace too small (%lld bytes, vah_sce_ws_bytes says %lld)", fn, (long long)ws_bytes,
                    (long long)need);
    return 0;
}

// the class run of the backward: the largest that leaves a workgroup (one wave) for each of the 4 * kCUs SIMDs, else 4
int run_of(int64_t N, int64_t tiles, int64_t C) {
    for (int R : {16, 8})
        if (N * tiles * ((C + R - 1) / R) >= 4 * kCUs) return R;
    return 4;
}

}  // namespace
}  // namespace vah

extern "C" {

int64_t vah_sce_ws_bytes(int64_t N, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W) {
    using namespace vah;
    if (N < 1 || C < 1 || h < 1 || w < 1 || H < 1 || W < 1 || N > 65535 || bad_size(C) || bad_size(h) || bad_size(w) || bad_size(H) ||
        bad_size(W) || H * W >= kLim || h * w >= kLim)
        return 0;
    return ws_bytes_of(N, h, w, H, W);
}

int vah_sce_forward(const void *logits, int logits_dtype, int64_t logits_img_stride, int64_t logits_plane_stride,
                    int64_t logits_row_stride, int64_t N, int64_t C, int64_t h, int64_t w, const void *labels,
                    int64_t labels_img_stride, int64_t labels_row_stride, int64_t H, int64_t W, int align_corners,
                    int64_t ignore_index, const void *class_weight, void *lse, void *loss_sum, void *counts, void *ws,
                    int64_t ws_bytes, void *stream) {
    using namespace vah;
    const char *fn = "vah_sce_forward";
    clear_error();
    if (int rc = problem_check(fn, logits_dtype, N, C, h, w, H, W)) return rc < 0 ? rc : VAH_OK;
    if (int rc = planes_check(fn, "logits", logits, (int)esize(logits_dtype), logits_img_stride, logits_plane_stride,
                              logits_row_stride, C, h, w))
        return rc;
    if (int rc = planes_check(fn, "labels", labels, 8, labels_img_stride, 0, labels_row_stride, 0, H, W)) return rc;
    const Arr arrs[] = {{"class_weight", class_weight, 4, true}, {"lse", lse, 4, false}, {"loss_sum", loss_sum, 4, false},
                        {"counts", counts, 8, false}};
    if (int rc = arr_check(fn, arrs)) return rc;
    if (int rc = ws_check(fn, ws, ws_bytes, ws_bytes_of(N, h, w, H, W))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t parts = parts_of(N, H, W);
    FwdArgs a;
    a.x = {logits, logits_img_stride, logits_plane_stride, logits_row_stride};
    a.y = {(const int64_t *)labels, labels_img_stride, labels_row_stride};
    a.cw = (const float *)class_weight, a.lse = (float *)lse;
    a.part_loss = (float *)ws, a.part_cnt = (int *)ws + parts;
    a.ay = axis_of(h, H, align_corners), a.ax = axis_of(w, W, align_corners);
    a.C = (int)C, a.W = (int)W, a.items = (unsigned)(H * W), a.ignore = ignore_index;
    // the taps read h x w once at most (upsampling: each element by several pixels, from the cache)
    const int64_t touched = h * w < 4 * H * W ? h * w : 4 * H * W;
    LaunchScope scope("sce_forward", N * (C * touched * esize(logits_dtype) + H * W * (8 + 4)), st);
    const dim3 grid((unsigned)(parts / N), (unsigned)N), block(256);
    with_type(logits_dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(sce_fwd_kernel<T>, grid, block, 0, st, a);
        return 0;
    });
    hipLaunchKernelGGL(sce_merge_kernel, dim3(1), dim3(kMerge), 0, st, (const float *)a.part_loss, (const int *)a.part_cnt, parts,
                       (float *)loss_sum, (int64_t *)counts);
    return check_launch(fn);
}

int vah_sce_backward(const void *logits, int logits_dtype, int64_t logits_img_stride, int64_t logits_plane_stride,
                     int64_t logits_row_stride, int64_t N, int64_t C, int64_t h, int64_t w, const void *labels,
                     int64_t labels_img_stride, int64_t labels_row_stride, int64_t H, int64_t W, int align_corners,
                     int64_t ignore_index, const void *class_weight, const void *lse, const void *scale, void *dlogits,
                     int64_t dlogits_img_stride, int64_t dlogits_plane_stride, int64_t dlogits_row_stride, void *ws,
                     int64_t ws_bytes, void *stream) {
    using namespace vah;
    const char *fn = "vah_sce_backward";
    clear_error();
    if (int rc = problem_check(fn, logits_dtype, N, C, h, w, H, W)) return rc < 0 ? rc : VAH_OK;
    const int es = (int)esize(logits_dtype);
    if (int rc = planes_check(fn, "logits", logits, es, logits_img_stride, logits_plane_stride, logits_row_stride, C, h, w)) return rc;
    if (int rc = planes_check(fn, "labels", labels, 8, labels_img_stride, 0, labels_row_stride, 0, H, W)) return rc;
    if (int rc = planes_check(fn, "dlogits", dlogits, es, dlogits_img_stride, dlogits_plane_stride, dlogits_row_stride, C, h, w)) return rc;
    const Arr arrs[] = {{"class_weight", class_weight, 4, true}, {"lse", lse, 4, false}, {"scale", scale, 4, false}};
    if (int rc = arr_check(fn, arrs)) return rc;
    if (int rc = ws_check(fn, ws, ws_bytes, ws_bytes_of(N, h, w, H, W))) return rc;
    hipStream_t st = (hipStream_t)stream;
    BwdArgs a;
    a.x = {logits, logits_img_stride, logits_plane_stride, logits_row_stride};
    a.y = {(const int64_t *)labels, labels_img_stride, labels_row_stride};
    a.cw = (const float *)class_weight, a.lse = (const float *)lse, a.scale = (const float *)scale;
    a.dx = dlogits, a.dis = dlogits_img_stride, a.dps = dlogits_plane_stride, a.drs = dlogits_row_stride;
    a.tb = tables_in(ws, N, h, H, W);
    const int64_t tiles_x = (w + kTW - 1) / kTW, tiles = tiles_x * ((h + kTH - 1) / kTH);
    a.C = (int)C, a.h = (int)h, a.w = (int)w, a.W = (int)W, a.tiles_x = (int)tiles_x, a.items = (unsigned)(H * W);
    a.ignore = ignore_index;
    const Axis ay = axis_of(h, H, align_corners), ax = axis_of(w, W, align_corners);
    int64_t longest = h > w ? h : w;
    longest = H > longest ? H : longest;
    longest = W > longest ? W : longest;
    LaunchScope scope("sce_backward", N * (2 * C * h * w * es + H * W * (8 + 4)), st);
    hipLaunchKernelGGL(sce_tables_kernel, dim3((unsigned)((longest + 255) / 256)), dim3(256), 0, st, ay, ax, a.tb);
    const int R = run_of(N, tiles, C);
    const dim3 grid((unsigned)tiles, (unsigned)((C + R - 1) / R), (unsigned)N), block(64);
    with_type(logits_dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        if (R == 16) hipLaunchKernelGGL((sce_bwd_kernel<T, 16>), grid, block, 0, st, a);
        else if (R == 8) hipLaunchKernelGGL((sce_bwd_kernel<T, 8>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((sce_bwd_kernel<T, 4>), grid, block, 0, st, a);
        return 0;
    });
    return check_launch(fn);
}

}  // extern "C"
