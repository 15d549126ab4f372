// Bilinear resize on channels-last rows and its ordered adjoint (include/vitadapter_hip_resize.h): the
// F.interpolate(outs[-1], size=..., mode='bilinear', align_corners=False) of the FPN tail of Mask2Former's pixel decoder
// (the reference's segmentation/mmseg_custom/models/plugins/msdeformattn_pixel_decoder.py:258-262), which torch runs as
// an fp32 NCHW operator whose backward accumulates with float atomics.
//
// Element [n][t][c] sits at n * img_stride + t * row_stride + c (the GroupNorm convention), so the forward reads a level's
// rows of the encoder's (Lq, N, C) buffer in place.  An item is one 16-byte piece - 8 channels - of one pixel; items are
// numbered pixel-major (item = pixel * C / 8 + piece), so consecutive lanes move consecutive 16 bytes of a row.  Grid
// (blocks, N), items strided over the blocks.
//   * forward: an item is a piece of an OUTPUT pixel: four taps, four products, one store; 16 16-byte loads in flight per
//     thread (4 items of 16-bit data, 2 of fp32).  The taps are computed in registers by tap_of().
//   * adjoint: an item is a piece of an INPUT pixel.  A table launch writes tap_of() of every output row and column and,
//     per input row and column, the range [lo, hi) of output rows / columns whose taps name it (the tap indices are
//     monotone, so the range is contiguous; found by bisection on tap_of() itself).  The gather launch walks
//     rows [lo, hi) x columns [lo, hi) in order with fp32 accumulators and stores once - zeros where the range is empty.
//     No atomics, counters or flags; the weights are the forward's own numbers, so the operator is its exact transpose.
// The element types are template parameters (float, __bf16, _Float16): they appear in loads, stores and converts only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vitadapter_hip_resize.h"
#include "common.h"
#include "elem16.h"
#include "resize_tap.h"           // Tap, Axis, tap_of(), axis_of(), weight_of(), bisect(): shared with seg_logits.hip, seg_ce_loss.hip

namespace vah {
namespace {

constexpr int kRsBlocks = 2048;         // per call

// workspace: Tap ty[Ho], Tap tx[Wo], int2 ry[Hi], int2 rx[Wi]
struct Tables {
    Tap *ty, *tx;
    int2 *ry, *rx;
};

__host__ __device__ inline Tables tables_in(void *ws, int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo) {
    Tables t;
    t.ty = (Tap *)ws;
    t.tx = t.ty + Ho;
    t.ry = (int2 *)(t.tx + Wo);
    t.rx = t.ry + Hi;
    return t;
}

__global__ __launch_bounds__(256) void resize_tables_kernel(Axis ay, Axis ax, Tables tb) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < ay.out) tb.ty[t] = tap_of(ay, t);
    if (t < ax.out) tb.tx[t] = tap_of(ax, t);
    if (t < ay.in) tb.ry[t] = make_int2(bisect<false>(ay, t), bisect<true>(ay, t));
    if (t < ax.in) tb.rx[t] = make_int2(bisect<false>(ax, t), bisect<true>(ax, t));
}

template <typename TX, typename TY, int U>
__global__ __launch_bounds__(256) void resize_rows_fwd_kernel(const TX *__restrict__ x, int64_t xrs, int64_t xis, Axis ay, Axis ax,
                                                              unsigned C8, unsigned items, TY *__restrict__ y, int64_t yrs,
                                                              int64_t yis) {
    const TX *xp = x + blockIdx.y * xis;
    TY *yp = y + blockIdx.y * yis;
    const unsigned step = gridDim.x * 256;
    struct Item {
        Tap ty, tx;
        int64_t off;      // of the output piece
        int c0;
    };
    auto locate = [&](unsigned it) {
        const unsigned o = it / C8, oy = o / (unsigned)ax.out;
        Item m;
        m.c0 = (int)(it - o * C8) * 8;
        m.ty = tap_of(ay, (int)oy);
        m.tx = tap_of(ax, (int)(o - oy * (unsigned)ax.out));
        m.off = (int64_t)o * yrs + m.c0;
        return m;
    };
    auto load = [&](const Item &m, float (&v)[4][8]) {
        const TX *r0 = xp + (int64_t)m.ty.i0 * ax.in * xrs + m.c0, *r1 = xp + (int64_t)m.ty.i1 * ax.in * xrs + m.c0;
        load8_f32(r0 + m.tx.i0 * xrs, v[0]);
        load8_f32(r0 + m.tx.i1 * xrs, v[1]);
        load8_f32(r1 + m.tx.i0 * xrs, v[2]);
        load8_f32(r1 + m.tx.i1 * xrs, v[3]);
    };
    auto finish = [&](const Item &m, const float (&v)[4][8]) {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)       // all four products, whatever the weights: 0 * inf = NaN as in torch
            r[j] = m.ty.l0 * (m.tx.l0 * v[0][j] + m.tx.l1 * v[1][j]) + m.ty.l1 * (m.tx.l0 * v[2][j] + m.tx.l1 * v[3][j]);
        store8_f32(yp + m.off, r);
    };
    unsigned it = blockIdx.x * 256 + threadIdx.x;
    // items < 2^31 and step * U <= 2^21 * U: `it + (U - 1) * step` stays below 2^32
    for (; it + (U - 1) * step < items; it += U * step) {
        Item m[U];
        float v[U][4][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            m[u] = locate(it + u * step);
            load(m[u], v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) finish(m[u], v[u]);
    }
    for (; it < items; it += step) {
        float v[4][8];
        const Item m = locate(it);
        load(m, v);
        finish(m, v);
    }
}

template <typename TD, typename TG>
__global__ __launch_bounds__(256) void resize_rows_bwd_kernel(const TD *__restrict__ dy, int64_t drs, int64_t dis, int Wi, int Wo,
                                                              Tables tb, unsigned C8, unsigned items, TG *__restrict__ dx,
                                                              int64_t grs, int64_t gis) {
    const TD *dp = dy + blockIdx.y * dis;
    TG *gp = dx + blockIdx.y * gis;
    const unsigned step = gridDim.x * 256;
    for (unsigned it = blockIdx.x * 256 + threadIdx.x; it < items; it += step) {
        const unsigned i = it / C8, iy = i / (unsigned)Wi, ix = i - iy * (unsigned)Wi;
        const int c0 = (int)(it - i * C8) * 8;
        const int2 ry = tb.ry[iy], rx = tb.rx[ix];
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        for (int oy = ry.x; oy < ry.y; ++oy) {
            const float wy = weight_of(tb.ty[oy], (int)iy);
            const TD *row = dp + (int64_t)oy * Wo * drs + c0;
#pragma unroll 4
            for (int ox = rx.x; ox < rx.y; ++ox) {
                const float w = wy * weight_of(tb.tx[ox], (int)ix);
                float g[8];
                load8_f32(row + ox * drs, g);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += w * g[j];
            }
        }
        store8_f32(gp + (int64_t)i * grs + c0, acc);
    }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
int64_t rs_ws_bytes(int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo) {
    return (Ho + Wo) * (int64_t)sizeof(Tap) + (Hi + Wi) * (int64_t)sizeof(int2);
}

unsigned rs_blocks(int64_t N, int64_t items, int per_thread) {
    int64_t cap = kRsBlocks / N;
    cap = cap < 1 ? 1 : cap;
    const int64_t want = (items + 256 * per_thread - 1) / (256 * per_thread);
    return (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
}

// the checks both entry points share; `a` is the tensor read (x / dy), `b` the one written (y / dx); pix_b = pixels of b
int rs_check(const char *fn, const char *an, const void *a, int a_dt, int64_t a_rs, int64_t a_is, const char *bn, const void *b,
             int b_dt, int64_t b_rs, int64_t b_is, int64_t N, int64_t C, int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo,
             int64_t pix_b, const void *ws, int64_t ws_bytes, bool *empty) {
    const int64_t lim = (int64_t)1 << 31;
    *empty = false;
    if (N < 0 || C < 1 || Hi < 0 || Wi < 0 || Ho < 0 || Wo < 0 || N > 65535 || Hi >= lim || Wi >= lim || Ho >= lim || Wo >= lim)
        return fail(VAH_E_SHAPE, "%s: bad dims (N %lld, C %lld, %lld x %lld -> %lld x %lld)", fn, (long long)N, (long long)C,
                    (long long)Hi, (long long)Wi, (long long)Ho, (long long)Wo);
    if (C % 8) return fail(VAH_E_UNSUPPORTED, "%s: C must be a multiple of 8 (C %lld)", fn, (long long)C);
    bool bf = false, fp = false;
    for (int d : {a_dt, b_dt}) {
        if (d < 0 || d > 2) return fail(VAH_E_UNSUPPORTED, "%s: dtype codes are 0 (fp32), 1 (bf16), 2 (fp16)", fn);
        bf |= d == 1, fp |= d == 2;
    }
    if (bf && fp) return fail(VAH_E_UNSUPPORTED, "%s: fp16 mixed with bf16", fn);
    if (N * pix_b == 0) {
        *empty = true;
        return 0;
    }
    if (Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || Hi * Wi * (C / 8) >= lim || Ho * Wo * (C / 8) >= lim)
        return fail(VAH_E_SHAPE, "%s: bad dims (an empty side, or an image of 2^31 pieces or more: %lld x %lld -> %lld x %lld, C %lld)", fn,
                    (long long)Hi, (long long)Wi, (long long)Ho, (long long)Wo, (long long)C);
    const struct { const char *name; const void *ptr; int64_t rs, is; } ts[2] = {{an, a, a_rs, a_is}, {bn, b, b_rs, b_is}};
    for (const auto &t : ts) {
        if (!t.ptr) return fail(VAH_E_NULL, "%s: null pointer (%s)", fn, t.name);
        if ((uintptr_t)t.ptr % 16 || t.rs % 8 || t.is % 8)
            return fail(VAH_E_ALIGN, "%s: %s misaligned (16-byte pointer, strides in multiples of 8)", fn, t.name);
        if (t.rs < C || t.is < 0) return fail(VAH_E_SHAPE, "%s: %s strides (row stride >= C)", fn, t.name);
    }
    if (!ws) return fail(VAH_E_NULL, "%s: null pointer (ws)", fn);
    if ((uintptr_t)ws % 16) return fail(VAH_E_ALIGN, "%s: ws misaligned (16-byte pointer)", fn);
    if (ws_bytes < rs_ws_bytes(Hi, Wi, Ho, Wo)) return fail(VAH_E_SHAPE, "%s: workspace too small", fn);
    return 0;
}

}  // namespace
}  // namespace vah

extern "C" {

int64_t vah_resize_rows_ws_bytes(int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo) {
    if (Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1) return 0;
    return vah::rs_ws_bytes(Hi, Wi, Ho, Wo);
}

int vah_resize_rows_forward(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride, int64_t N, int64_t C, int64_t Hi,
                            int64_t Wi, int64_t Ho, int64_t Wo, int align_corners, void *y, int y_dtype, int64_t y_row_stride,
                            int64_t y_img_stride, void *ws, int64_t ws_bytes, void *stream) {
    using namespace vah;
    const char *fn = "vah_resize_rows_forward";
    clear_error();
    bool empty;
    if (int rc = rs_check(fn, "x", x, x_dtype, x_row_stride, x_img_stride, "y", y, y_dtype, y_row_stride, y_img_stride, N, C, Hi, Wi, Ho,
                          Wo, Ho * Wo, ws, ws_bytes, &empty))
        return rc;
    if (empty) return VAH_OK;
    hipStream_t st = (hipStream_t)stream;
    const Axis ay = axis_of(Hi, Ho, align_corners), ax = axis_of(Wi, Wo, align_corners);
    const unsigned C8 = (unsigned)(C / 8), items = (unsigned)(Ho * Wo * (C / 8));
    LaunchScope scope(x_dtype == 2 || y_dtype == 2 ? "resize_rows_fwd_f16" : "resize_rows_fwd",
                      N * C * (Hi * Wi * esize(x_dtype) + Ho * Wo * esize(y_dtype)), st, N * C * (Hi * Wi + Ho * Wo) * 4);
    return with_type(x_dtype, [&](auto tx) {
        return with_type(y_dtype, [&](auto ty) {
            typedef typename decltype(tx)::type TX;
            typedef typename decltype(ty)::type TY;
            constexpr int U = sizeof(TX) == 4 ? 2 : 4;          // 4 taps x 16 (32) bytes x U in flight per thread
            if constexpr (!mixed16<TX, TY>())
                hipLaunchKernelGGL((resize_rows_fwd_kernel<TX, TY, U>), dim3(rs_blocks(N, items, U), (unsigned)N), dim3(256), 0, st,
                                   (const TX *)x, x_row_stride, x_img_stride, ay, ax, C8, items, (TY *)y, y_row_stride, y_img_stride);
            return check_launch(fn);
        });
    });
}

int vah_resize_rows_backward(const void *dy, int dy_dtype, int64_t dy_row_stride, int64_t dy_img_stride, int64_t N, int64_t C,
                             int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo, int align_corners, void *dx, int dx_dtype,
                             int64_t dx_row_stride, int64_t dx_img_stride, void *ws, int64_t ws_bytes, void *stream) {
    using namespace vah;
    const char *fn = "vah_resize_rows_backward";
    clear_error();
    bool empty;
    if (int rc = rs_check(fn, "dy", dy, dy_dtype, dy_row_stride, dy_img_stride, "dx", dx, dx_dtype, dx_row_stride, dx_img_stride, N, C,
                          Hi, Wi, Ho, Wo, Hi * Wi, ws, ws_bytes, &empty))
        return rc;
    if (empty) return VAH_OK;
    hipStream_t st = (hipStream_t)stream;
    const Axis ay = axis_of(Hi, Ho, align_corners), ax = axis_of(Wi, Wo, align_corners);
    const Tables tb = tables_in(ws, Hi, Wi, Ho, Wo);
    const unsigned C8 = (unsigned)(C / 8), items = (unsigned)(Hi * Wi * (C / 8));
    int64_t longest = Hi > Wi ? Hi : Wi;
    longest = Ho > longest ? Ho : longest;
    longest = Wo > longest ? Wo : longest;
    LaunchScope scope(dy_dtype == 2 || dx_dtype == 2 ? "resize_rows_bwd_f16" : "resize_rows_bwd",
                      N * C * (Ho * Wo * esize(dy_dtype) + Hi * Wi * esize(dx_dtype)), st, N * C * (Hi * Wi + Ho * Wo) * 4);
    hipLaunchKernelGGL(resize_tables_kernel, dim3((unsigned)((longest + 255) / 256)), dim3(256), 0, st, ay, ax, tb);
    if (int rc = check_launch(fn)) return rc;
    return with_type(dy_dtype, [&](auto td) {
        return with_type(dx_dtype, [&](auto tg) {
            typedef typename decltype(td)::type TD;
            typedef typename decltype(tg)::type TG;
            if constexpr (!mixed16<TD, TG>())
                hipLaunchKernelGGL((resize_rows_bwd_kernel<TD, TG>), dim3(rs_blocks(N, items, 1), (unsigned)N), dim3(256), 0, st,
                                   (const TD *)dy, dy_row_stride, dy_img_stride, (int)Wi, (int)Wo, tb, C8, items, (TG *)dx, dx_row_stride,
                                   dx_img_stride);
            return check_launch(fn);
        });
    });
}

}  // extern "C"
