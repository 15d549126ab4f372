// The logit tail of the Mask2Former segmentor (include/vitadapter_hip_seg.h): what the reference's
// segmentation/mmseg_custom/models/segmentors/encoder_decoder_mask2former[_aug].py does between decode_head.forward_test and
// the label map, as three launches over fp32 NCHW planes.
//   * seg_resize_add: resize(out, size=img.shape[2:]) and preds += F.pad(...) in one pass.  A thread owns one pixel of the
//     window for a run of kRaRun classes: the taps are computed once, each class costs four loads of the (small, cached)
//     source and one dword store - or load and store - of dst.  Grid (pixel blocks, class runs, N).
//   * seg_finish: preds / count_mat, un-pad, resize to ori_shape, softmax over the classes, flip, (+)= into the probability
//     sum and / or argmax.  A thread owns one output pixel, consecutive lanes consecutive x, so each class plane is read in
//     coalesced (or, downsampling, nearly coalesced) dwords.  The classes are walked twice: the first walk keeps a running
//     maximum and a sum rescaled when the maximum moves, the second recomputes v[c] from the same taps and writes
//     exp(v - max) / sum.  C = 150 values per lane do not fit in registers; the alternative, a column of C floats per lane
//     in LDS, costs 600 bytes a lane at C = 150 - one wave per SIMD - and bounds C; see DESIGN.md.
//   * seg_argmax: first index of the largest sum / divisor.
// Window offsets and widths are arbitrary (x0 = 299 at ADE20K sizes), so every access is a dword.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/vitadapter_hip_seg.h"
#include "common.h"
#include "resize_tap.h"

namespace vah {
namespace {

constexpr int kRaRun = 8;       // classes per thread of seg_resize_add
constexpr int kRaU = 4;         // of which in flight at a time

struct Planes {                 // an fp32 (N, C, H, W) tensor
    float *p;
    int64_t is, ps, rs;
};

struct ResizeAddArgs {
    Planes src, dst;
    Axis ay, ax;
    int C, Wc;
    unsigned items;             // Hc * Wc
    int accumulate;
};

__global__ __launch_bounds__(256) void seg_resize_add_kernel(const ResizeAddArgs a) {
    const unsigned pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= a.items) return;
    const int oy = (int)(pix / (unsigned)a.Wc), ox = (int)(pix - (unsigned)oy * (unsigned)a.Wc);
    const Tap ty = tap_of(a.ay, oy), tx = tap_of(a.ax, ox);
    const int c0 = blockIdx.y * kRaRun, c1 = min(c0 + kRaRun, a.C);
    const float *sp = a.src.p + blockIdx.z * a.src.is;
    float *dp = a.dst.p + blockIdx.z * a.dst.is + (int64_t)oy * a.dst.rs + ox;         // dst.p is the window's corner
    const int64_t o00 = ty.i0 * a.src.rs + tx.i0, o01 = ty.i0 * a.src.rs + tx.i1, o10 = ty.i1 * a.src.rs + tx.i0,
                  o11 = ty.i1 * a.src.rs + tx.i1;
    for (int c = c0; c < c1; c += kRaU) {
        float v[kRaU][4], old[kRaU];
#pragma unroll
        for (int u = 0; u < kRaU; ++u) {
            const int cc = min(c + u, c1 - 1);          // a clamped class: loaded, never stored
            const float *q = sp + cc * a.src.ps;
            v[u][0] = q[o00], v[u][1] = q[o01], v[u][2] = q[o10], v[u][3] = q[o11];
            old[u] = a.accumulate ? dp[cc * a.dst.ps] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kRaU; ++u) {
            if (c + u >= c1) break;
            const float r = blend_rn(ty, tx, v[u][0], v[u][1], v[u][2], v[u][3]);
            dp[(c + u) * a.dst.ps] = a.accumulate ? old[u] + r : r;
        }
    }
}

struct FinishArgs {
    Planes acc, prob;
    const int *cy, *cx;
    int64_t *labels;
    int64_t lis, lrs;
    Axis ay, ax;
    int C, Ho, Wo;
    unsigned items;             // Ho * Wo
    int flip, accumulate;
};

// what a pixel needs to evaluate v[c]: tap offsets inside a plane, the taps and 1 / nothing - the four counts
template <bool RESIZE, bool COUNTS>
struct Pixel {
    Tap ty, tx;
    int64_t o[RESIZE ? 4 : 1];
    float d[RESIZE ? 4 : 1];

    __device__ __forceinline__ void load(const float *plane, float (&t)[RESIZE ? 4 : 1]) const {
#pragma unroll
        for (int k = 0; k < (RESIZE ? 4 : 1); ++k) t[k] = plane[o[k]];
    }
    // divide, then resize; the same instructions in both walks, so the second walk meets the first's maximum again
    __device__ __forceinline__ float value(float (&t)[RESIZE ? 4 : 1]) const {
        if (COUNTS) {
#pragma unroll
            for (int k = 0; k < (RESIZE ? 4 : 1); ++k) t[k] = t[k] / d[k];
        }
        if (RESIZE) return blend_rn(ty, tx, t[0], t[RESIZE ? 1 : 0], t[RESIZE ? 2 : 0], t[RESIZE ? 3 : 0]);
        return t[0];
    }
};

template <bool RESIZE, bool COUNTS>
__global__ __launch_bounds__(256) void seg_finish_kernel(const FinishArgs a) {
    constexpr int U = RESIZE ? 4 : 8;           // classes in flight: 16 / 8 loads per thread
    constexpr int T = RESIZE ? 4 : 1;
    const unsigned pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= a.items) return;
    const int oy = (int)(pix / (unsigned)a.Wo), ox = (int)(pix - (unsigned)oy * (unsigned)a.Wo);
    Pixel<RESIZE, COUNTS> px;
    if (RESIZE) {
        px.ty = tap_of(a.ay, oy), px.tx = tap_of(a.ax, ox);
        const int ys[2] = {px.ty.i0, px.ty.i1}, xs[2] = {px.tx.i0, px.tx.i1};
#pragma unroll
        for (int k = 0; k < T; ++k) {
            px.o[k] = ys[k >> 1] * a.acc.rs + xs[k & 1];
            px.d[k] = COUNTS ? (float)(a.cy[ys[k >> 1]] * a.cx[xs[k & 1]]) : 1.f;
        }
    } else {
        px.o[0] = oy * a.acc.rs + ox;
        px.d[0] = COUNTS ? (float)(a.cy[oy] * a.cx[ox]) : 1.f;
    }
    const float *ap = a.acc.p + blockIdx.y * a.acc.is;
    const int C = a.C;

    // first walk: running maximum m and s = sum exp(v - m); `bad` where torch's softmax gives NaN for the whole pixel
    float m = -INFINITY, s = 0.f;
    bool bad = false;
    for (int c = 0; c < C; c += U) {
        float t[U][T];
#pragma unroll
        for (int u = 0; u < U; ++u) px.load(ap + min(c + u, C - 1) * a.acc.ps, t[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u >= C) break;
            const float v = px.value(t[u]);
            bad |= !(v < INFINITY);             // NaN or +inf
            if (v > m) {
                s = s * expf(m - v) + 1.f;      // m == -inf: s is 0 and stays 0 before the 1
                m = v;
            } else if (v > -INFINITY) {
                s += expf(v - m);
            }
        }
    }
    bad |= m == -INFINITY;                      // all -inf (then s == 0)

    // second walk: p[c], the outputs, and the first index of the largest p (a NaN pixel: index 0).  Labels alone take it
    // too: the label is argmax of the rounded probabilities, as in the reference, and exp and the division can round a
    // logit just below the maximum, at a lower index, to the same p
    const int sy = a.flip == 2 ? a.Ho - 1 - oy : oy, sx = a.flip == 1 ? a.Wo - 1 - ox : ox;
    float *pp = a.prob.p ? a.prob.p + blockIdx.y * a.prob.is + (int64_t)sy * a.prob.rs + sx : nullptr;
    float best = -1.f;
    int arg = 0;
    for (int c = 0; c < C; c += U) {
        float t[U][T], old[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int cc = min(c + u, C - 1);
            px.load(ap + cc * a.acc.ps, t[u]);
            old[u] = pp && a.accumulate ? pp[cc * a.prob.ps] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u >= C) break;
            const float v = px.value(t[u]);
            const float p = bad ? NAN : expf(v - m) / s;
            if (p > best) best = p, arg = c + u;          // p >= 0 > -1: class 0 always enters; NaN never does: arg stays 0
            if (pp) pp[(c + u) * a.prob.ps] = a.accumulate ? old[u] + p : p;
        }
    }
    if (a.labels) a.labels[blockIdx.y * a.lis + (int64_t)sy * a.lrs + sx] = arg;
}

struct ArgmaxArgs {
    Planes sum;
    int64_t *labels;
    int64_t lis, lrs;
    int C, W;
    unsigned items;
    float divisor;
};

__global__ __launch_bounds__(256) void seg_argmax_kernel(const ArgmaxArgs a) {
    constexpr int U = 8;
    const unsigned pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= a.items) return;
    const int y = (int)(pix / (unsigned)a.W), x = (int)(pix - (unsigned)y * (unsigned)a.W);
    const float *sp = a.sum.p + blockIdx.y * a.sum.is + (int64_t)y * a.sum.rs + x;
    float best = 0.f;
    int arg = -1;
    bool nan = false;
    for (int c = 0; c < a.C; c += U) {
        float t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] = sp[min(c + u, a.C - 1) * a.sum.ps];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u >= a.C) break;
            const float v = t[u] / a.divisor;
            // the first NaN wins and ends the search; otherwise the first strictly larger value
            if (!nan && (arg < 0 || v > best || v != v)) best = v, arg = c + u, nan = v != v;
        }
    }
    a.labels[blockIdx.y * a.lis + (int64_t)y * a.lrs + x] = arg;
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
constexpr int64_t kLim = (int64_t)1 << 31;

bool bad_size(int64_t v) { return v < 0 || v >= kLim; }

// pointer, alignment and stride rules of one (N, C, H, W) tensor (C == 0: a label map, one plane per image)
int planes_check(const char *fn, const char *name, const void *p, int align, int64_t is, int64_t ps, int64_t rs, int64_t N,
                 int64_t C, int64_t H, int64_t W) {
    if (!p) return fail(VAH_E_NULL, "%s: null pointer (%s)", fn, name);
    if ((uintptr_t)p % align) return fail(VAH_E_ALIGN, "%s: %s misaligned (%d-byte pointer)", fn, name, align);
    const int64_t plane = (H - 1) * rs + W;
    if (rs < W || (C && ps < plane) || is < (C ? (C - 1) * ps + plane : plane))
        return fail(VAH_E_SHAPE, "%s: %s strides (row stride >= width, planes and images that do not overlap)", fn, name);
    return 0;
}

unsigned pixel_blocks(int64_t items) { return (unsigned)((items + 255) / 256); }

}  // namespace
}  // namespace vah

extern "C" {

int vah_seg_resize_add(const void *src, int64_t src_img_stride, int64_t src_plane_stride, int64_t src_row_stride, int64_t N,
                       int64_t C, int64_t hs, int64_t ws, int64_t Hc, int64_t Wc, int align_corners, void *dst,
                       int64_t dst_img_stride, int64_t dst_plane_stride, int64_t dst_row_stride, int64_t Hd, int64_t Wd,
                       int64_t y0, int64_t x0, int accumulate, void *stream) {
    using namespace vah;
    const char *fn = "vah_seg_resize_add";
    clear_error();
    if (bad_size(N) || bad_size(C) || bad_size(hs) || bad_size(ws) || bad_size(Hc) || bad_size(Wc) || bad_size(Hd) || bad_size(Wd) ||
        N > 65535 || C > 65535 * kRaRun)
        return fail(VAH_E_SHAPE, "%s: bad dims (N %lld, C %lld, %lld x %lld -> %lld x %lld in %lld x %lld)", fn, (long long)N,
                    (long long)C, (long long)hs, (long long)ws, (long long)Hc, (long long)Wc, (long long)Hd, (long long)Wd);
    if (y0 < 0 || x0 < 0 || y0 + Hc > Hd || x0 + Wc > Wd)
        return fail(VAH_E_SHAPE, "%s: the window leaves dst (%lld x %lld at (%lld, %lld) in %lld x %lld)", fn, (long long)Hc,
                    (long long)Wc, (long long)y0, (long long)x0, (long long)Hd, (long long)Wd);
    if (N * C * Hc * Wc == 0) return VAH_OK;
    if (hs < 1 || ws < 1 || Hc * Wc >= kLim || hs * ws >= kLim)
        return fail(VAH_E_SHAPE, "%s: bad dims (an empty source, or a plane of 2^31 pixels or more)", fn);
    if (int rc = planes_check(fn, "src", src, 4, src_img_stride, src_plane_stride, src_row_stride, N, C, hs, ws)) return rc;
    if (int rc = planes_check(fn, "dst", dst, 4, dst_img_stride, dst_plane_stride, dst_row_stride, N, C, Hd, Wd)) return rc;
    hipStream_t st = (hipStream_t)stream;
    ResizeAddArgs a;
    a.src = {(float *)src, src_img_stride, src_plane_stride, src_row_stride};
    a.dst = {(float *)dst + y0 * dst_row_stride + x0, dst_img_stride, dst_plane_stride, dst_row_stride};
    a.ay = axis_of(hs, Hc, align_corners), a.ax = axis_of(ws, Wc, align_corners);
    a.C = (int)C, a.Wc = (int)Wc, a.items = (unsigned)(Hc * Wc), a.accumulate = accumulate ? 1 : 0;
    LaunchScope scope("seg_resize_add", N * C * (hs * ws + Hc * Wc * (accumulate ? 2 : 1)) * 4, st);
    hipLaunchKernelGGL(seg_resize_add_kernel, dim3(pixel_blocks(Hc * Wc), (unsigned)((C + kRaRun - 1) / kRaRun), (unsigned)N),
                       dim3(256), 0, st, a);
    return check_launch(fn);
}

int vah_seg_finish(const void *acc, int64_t acc_img_stride, int64_t acc_plane_stride, int64_t acc_row_stride, int64_t N,
                   int64_t C, int64_t Hs, int64_t Ws, const void *cy, const void *cx, int resize, int64_t Ho, int64_t Wo,
                   int align_corners, int flip, void *prob, int64_t prob_img_stride, int64_t prob_plane_stride,
                   int64_t prob_row_stride, int accumulate, void *labels, int64_t labels_img_stride, int64_t labels_row_stride,
                   void *stream) {
    using namespace vah;
    const char *fn = "vah_seg_finish";
    clear_error();
    if (bad_size(N) || bad_size(C) || bad_size(Hs) || bad_size(Ws) || bad_size(Ho) || bad_size(Wo) || N > 65535)
        return fail(VAH_E_SHAPE, "%s: bad dims (N %lld, C %lld, %lld x %lld -> %lld x %lld)", fn, (long long)N, (long long)C,
                    (long long)Hs, (long long)Ws, (long long)Ho, (long long)Wo);
    if (!resize && (Ho != Hs || Wo != Ws))
        return fail(VAH_E_SHAPE, "%s: resize == 0 needs (Ho, Wo) == (Hs, Ws) (%lld x %lld, %lld x %lld)", fn, (long long)Ho,
                    (long long)Wo, (long long)Hs, (long long)Ws);
    if (flip < 0 || flip > 2) return fail(VAH_E_SHAPE, "%s: flip is 0 (none), 1 (horizontal) or 2 (vertical), not %d", fn, flip);
    if (N * C * Ho * Wo == 0) return VAH_OK;
    if (Hs < 1 || Ws < 1 || Ho * Wo >= kLim || Hs * Ws >= kLim)
        return fail(VAH_E_SHAPE, "%s: bad dims (an empty source, or a plane of 2^31 pixels or more)", fn);
    if (int rc = planes_check(fn, "acc", acc, 4, acc_img_stride, acc_plane_stride, acc_row_stride, N, C, Hs, Ws)) return rc;
    if (!cy != !cx) return fail(VAH_E_NULL, "%s: null pointer (one of cy, cx; both null means count 1)", fn);
    if ((uintptr_t)cy % 4 || (uintptr_t)cx % 4) return fail(VAH_E_ALIGN, "%s: cy / cx misaligned (4-byte pointer)", fn);
    if (!prob && !labels) return fail(VAH_E_NULL, "%s: null pointer (prob and labels: nothing to write)", fn);
    if (prob)
        if (int rc = planes_check(fn, "prob", prob, 4, prob_img_stride, prob_plane_stride, prob_row_stride, N, C, Ho, Wo)) return rc;
    if (labels)
        if (int rc = planes_check(fn, "labels", labels, 8, labels_img_stride, 0, labels_row_stride, N, 0, Ho, Wo)) return rc;
    hipStream_t st = (hipStream_t)stream;
    FinishArgs a;
    a.acc = {(float *)acc, acc_img_stride, acc_plane_stride, acc_row_stride};
    a.prob = {(float *)prob, prob_img_stride, prob_plane_stride, prob_row_stride};
    a.cy = (const int *)cy, a.cx = (const int *)cx;
    a.labels = (int64_t *)labels, a.lis = labels_img_stride, a.lrs = labels_row_stride;
    a.ay = axis_of(Hs, Ho, align_corners), a.ax = axis_of(Ws, Wo, align_corners);
    a.C = (int)C, a.Ho = (int)Ho, a.Wo = (int)Wo, a.items = (unsigned)(Ho * Wo), a.flip = flip, a.accumulate = accumulate ? 1 : 0;
    // the taps read Hs x Ws once per walk at most (upsampling: each element by several pixels, from the cache)
    const int64_t touched = resize ? (Hs * Ws < 4 * Ho * Wo ? Hs * Ws : 4 * Ho * Wo) : Ho * Wo;
    LaunchScope scope("seg_finish",
                      N * (C * (touched + (prob ? Ho * Wo * (accumulate ? 2 : 1) : 0)) * 4 + (labels ? Ho * Wo * 8 : 0)), st);
    const dim3 grid(pixel_blocks(Ho * Wo), (unsigned)N), block(256);
    if (resize && cy) hipLaunchKernelGGL((seg_finish_kernel<true, true>), grid, block, 0, st, a);
    else if (resize) hipLaunchKernelGGL((seg_finish_kernel<true, false>), grid, block, 0, st, a);
    else if (cy) hipLaunchKernelGGL((seg_finish_kernel<false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((seg_finish_kernel<false, false>), grid, block, 0, st, a);
    return check_launch(fn);
}

int vah_seg_argmax(const void *sum, int64_t sum_img_stride, int64_t sum_plane_stride, int64_t sum_row_stride, int64_t N,
                   int64_t C, int64_t H, int64_t W, float divisor, void *labels, int64_t labels_img_stride,
                   int64_t labels_row_stride, void *stream) {
    using namespace vah;
    const char *fn = "vah_seg_argmax";
    clear_error();
    if (bad_size(N) || bad_size(C) || bad_size(H) || bad_size(W) || N > 65535 || H * W >= kLim)
        return fail(VAH_E_SHAPE, "%s: bad dims (N %lld, C %lld, %lld x %lld)", fn, (long long)N, (long long)C, (long long)H,
                    (long long)W);
    if (N * C * H * W == 0) return VAH_OK;
    if (int rc = planes_check(fn, "sum", sum, 4, sum_img_stride, sum_plane_stride, sum_row_stride, N, C, H, W)) return rc;
    if (int rc = planes_check(fn, "labels", labels, 8, labels_img_stride, 0, labels_row_stride, N, 0, H, W)) return rc;
    hipStream_t st = (hipStream_t)stream;
    ArgmaxArgs a;
    a.sum = {(float *)sum, sum_img_stride, sum_plane_stride, sum_row_stride};
    a.labels = (int64_t *)labels, a.lis = labels_img_stride, a.lrs = labels_row_stride;
    a.C = (int)C, a.W = (int)W, a.items = (unsigned)(H * W), a.divisor = divisor;
    LaunchScope scope("seg_argmax", N * H * W * (C * 4 + 8), st);
    hipLaunchKernelGGL(seg_argmax_kernel, dim3(pixel_blocks(H * W), (unsigned)N), dim3(256), 0, st, a);
    return check_launch(fn);
}

}  // extern "C"
