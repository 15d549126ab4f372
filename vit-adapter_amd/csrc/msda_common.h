// Helpers shared by the MSDA kernels (msda.hip, msda_fused.hip): bilinear tap, level geometry read
// with the window guard, XCD-chunked block order.
#pragma once
#include "common.h"

namespace vah {
namespace msda {

template <typename T>
struct Tap {
    int row[4];     // token index inside the level (clamped to 0 when the corner is invalid)
    bool ok[4];     // corner inside the map and sample inside the gate
    T cw[4];        // hh*hw, hh*lw, lh*hw, lh*lw
    T lh, lw, hh, hw;
};

template <typename T>
__device__ __forceinline__ Tap<T> make_tap(T lx, T ly, int H, int W) {
    Tap<T> t;
    const T h_im = ly * (T)H - (T)0.5;
    const T w_im = lx * (T)W - (T)0.5;
    // strict gate of the reference (cuh:288); NaN and +-inf locations fail it.  They are not dropped as a sample outside
    // the map is: `bad` is 0 for finite coordinates and NaN otherwise, such a sample sits on pixel (0, 0) - an address
    // that exists - with NaN fractions, so its four weights, the output and every gradient it feeds are NaN, as
    // torch's grid_sample makes them (GradScaler has to see an overflowed offset).
    const bool gate = h_im > (T)-1 && w_im > (T)-1 && h_im < (T)H && w_im < (T)W;
    const T bad = (h_im - h_im) + (w_im - w_im);
    const bool inside = gate || bad != bad;
    const T hs = gate ? h_im : (T)0;
    const T ws = gate ? w_im : (T)0;
    const T hf = floor(hs), wf = floor(ws);
    const int h_low = (int)hf, w_low = (int)wf;
    const int h_high = h_low + 1, w_high = w_low + 1;
    t.lh = hs - hf + bad;
    t.lw = ws - wf + bad;
    t.hh = (T)1 - t.lh;
    t.hw = (T)1 - t.lw;
    t.cw[0] = t.hh * t.hw;
    t.cw[1] = t.hh * t.lw;
    t.cw[2] = t.lh * t.hw;
    t.cw[3] = t.lh * t.lw;
    const bool hl = h_low >= 0, hh_ = h_high <= H - 1, wl = w_low >= 0, wh = w_high <= W - 1;
    t.ok[0] = inside && hl && wl;
    t.ok[1] = inside && hl && wh;
    t.ok[2] = inside && hh_ && wl;
    t.ok[3] = inside && hh_ && wh;
    t.row[0] = t.ok[0] ? h_low * W + w_low : 0;
    t.row[1] = t.ok[1] ? h_low * W + w_high : 0;
    t.row[2] = t.ok[2] ? h_high * W + w_low : 0;
    t.row[3] = t.ok[3] ? h_high * W + w_high : 0;
    return t;
}

// Reference of one (image, query, level) as the fused core reads it: a point (x, y), or - BOX - a box (cx, cy, w, h).
// The reference module forms the sampling location of offset `off` as (detection/ops/modules/ms_deform_attn.py:117-122)
//     point  loc = ref + off / (W, H)
//     box    loc = ref[:2] + off / P * ref[2:] * 0.5
// box_loc is the one spelling of the second line that the forward, the binning pass, the tile pass and the gather
// kernels share (the tile pass owns a sample by its location: they have to agree to the bit); box_grad_scale is
// d(off) / d(pixel coordinate), the factor that turns the pixel-space gradient the kernels accumulate into d(offsets):
// d off.x = d out / d loc.x * w * 0.5 / P = gx * W * w * 0.5 / P (point form: gx, the level size cancels).
template <bool BOX> struct RefRaw { typedef float2 type; };
template <> struct RefRaw<true> { typedef float4 type; };

template <int P>
__device__ __forceinline__ float2 box_loc(const float4 &b, float ox, float oy) {
    // an explicit fma: what -ffp-contract=fast makes of c + (o * 0.5 / P) * wh where it can, spelled so that it does everywhere
    return make_float2(__builtin_fmaf(ox * (0.5f / P), b.z, b.x), __builtin_fmaf(oy * (0.5f / P), b.w, b.y));
}
template <int P>
__device__ __forceinline__ float2 box_grad_scale(const float4 &b, int H, int W) {
    return make_float2((float)W * ((0.5f / P) * b.z), (float)H * ((0.5f / P) * b.w));
}

struct Level {
    int H, W;
    int64_t start;
    bool valid;
};

// Scalar (SGPR) read of one level's geometry, with the window guard described in the ABI.
__device__ __forceinline__ Level read_level(const int64_t *__restrict__ shapes,
                                            const int64_t *__restrict__ lsi, int l, int64_t S) {
    Level lv;
    const int64_t H = shapes[2 * l], W = shapes[2 * l + 1], st = lsi[l];
    lv.valid = H >= 1 && W >= 1 && st >= 0 && H <= S && W <= S && st + H * W <= S;
    lv.H = (int)H;
    lv.W = (int)W;
    lv.start = st;
    return lv;
}

// Each XCD (observed: blockIdx % 8) gets one contiguous chunk of the logical blocks.
// Placement only affects speed, never results.
__device__ __forceinline__ int64_t xcd_chunked_block(int64_t nblocks) {
    const int64_t b = blockIdx.x;
    const int64_t chunk = (nblocks + 7) / 8;
    return (b % 8) * chunk + b / 8;
}

constexpr int kBlock = 256;

}  // namespace msda
}  // namespace vah
