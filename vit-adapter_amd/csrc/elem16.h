// The 16-bit element types of the kernels and their MFMA / LDS primitives (gfx950).
//
// Every fast kernel family is a template on the 16-bit element type T of its operands: __bf16 (bf16 autocast) or
// _Float16 (fp16 autocast).  v_mfma_f32_32x32x16_bf16 and _f16 share operand layout and cycles, ds_read_b64_tr_b16
// reads either type: only the typedefs, mfma() and the float <-> T conversions differ.  Accumulators are fp32 for both.
//
// 32x32x16 MFMA, lane l = (r = l & 31, h = l >> 5):
//   A operand element j : A[row r][k = 8h + j]         (8 x T)
//   B operand element j : B[k = 8h + j][col r]         (8 x T)
//   C/D register i      : C[row (i&3) + 8(i>>2) + 4h][col r]
//
// Only what two or more files use lives here; a conversion helper with one user stays in its file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace vah {

typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 bf16x4;
typedef __attribute__((__vector_size__(2 * sizeof(__bf16)))) __bf16 bf16x2;
typedef __attribute__((__vector_size__(8 * sizeof(_Float16)))) _Float16 f16x8;
typedef __attribute__((__vector_size__(4 * sizeof(_Float16)))) _Float16 f16x4;
typedef __attribute__((__vector_size__(2 * sizeof(_Float16)))) _Float16 f16x2;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float f32x16;
typedef __attribute__((__vector_size__(4 * sizeof(short)))) short s16x4;     // what the transposed LDS read returns
typedef __attribute__((__vector_size__(8 * sizeof(short)))) short s16x8;

// vectors of 8 / 4 / 2 elements of the kernels' 16-bit type T
template <typename T> struct Vec16;
template <> struct Vec16<__bf16> { typedef bf16x8 x8; typedef bf16x4 x4; typedef bf16x2 x2; };
template <> struct Vec16<_Float16> { typedef f16x8 x8; typedef f16x4 x4; typedef f16x2 x2; };
template <typename T> using vec8 = typename Vec16<T>::x8;
template <typename T> using vec4 = typename Vec16<T>::x4;
template <typename T> using vec2 = typename Vec16<T>::x2;

// profiler row / launch name of the instantiation: the bf16 name or its _f16 twin
template <typename T> constexpr const char *tname(const char *bf16_name, const char *f16_name);
template <> constexpr const char *tname<__bf16>(const char *bf16_name, const char *) { return bf16_name; }
template <> constexpr const char *tname<_Float16>(const char *, const char *f16_name) { return f16_name; }

// The dtype codes of the entry points whose element types are arguments (0 fp32, 1 bf16, 2 fp16): element size in bytes,
// f(Tag<element type>) for a code, and "a bf16 operand beside an fp16 one" (never instantiated)
inline int64_t esize(int dt) { return dt == 0 ? 4 : 2; }

template <typename T> struct Tag { typedef T type; };

template <typename F>
int with_type(int dt, F &&f) {
    switch (dt) {
        case 0: return f(Tag<float>{});
        case 1: return f(Tag<__bf16>{});
        default: return f(Tag<_Float16>{});
    }
}

template <typename A, typename B>
constexpr bool mixed16() { return sizeof(A) == 2 && sizeof(B) == 2 && !std::is_same<A, B>::value; }

#if defined(__HIPCC__)
__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// row of a C/D tile held in register i by lane half h
__device__ __forceinline__ int crow(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

// Transposed fragment of a row-major LDS tile, two ds_read_b64_tr_b16: lane 4q+p of a 16-lane group names row q,
// columns 4p..4p+3 of a 4 x 16 block at p0 and receives column (lane & 15) of its 4 rows (checked on the GPU:
// tools/ubench/tr_read.hip); p1 names the block 8 rows further, which fills elements 4..7.  With rows 4h + q the lane
// holds column (lane & 31) of 8 rows in the k order of a fragment pair (4h.., 8 + 4h..).
template <typename T>
__device__ __forceinline__ vec8<T> tr_frag(const void *p0, const void *p1) {
    const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3))) *)p0);
    const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3))) *)p1);
    return __builtin_bit_cast(vec8<T>, __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7));
}

// element i of an array of T (float, _Float16 or __bf16) packed in 32-bit words, as fp32
template <typename T>
__device__ __forceinline__ float word_elem(const uint32_t *w, int i) {
    if constexpr (sizeof(T) == 4) return __builtin_bit_cast(float, w[i]);
    else if constexpr (std::is_same<T, _Float16>::value)                      // v_cvt_f32_f16: exact, subnormals kept
        return (float)__builtin_bit_cast(_Float16, (unsigned short)((i & 1) ? w[i >> 1] >> 16 : w[i >> 1] & 0xFFFFu));
    else return __builtin_bit_cast(float, (i & 1) ? (w[i >> 1] & 0xFFFF0000u) : (w[i >> 1] << 16));
}

// 8 consecutive elements of T (float, _Float16 or __bf16) at a 16-byte aligned address, as fp32: one 16-byte load of
// 16-bit data, two of fp32 (the channels-last row kernels: group_norm.hip, resize_rows.hip)
template <typename T>
__device__ __forceinline__ void load8_f32(const T *p, float (&v)[8]) {
    if constexpr (sizeof(T) == 4) {
        const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
        const vec8<T> t = *reinterpret_cast<const vec8<T> *>(p);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
    }
}

// the store to match: each element rounded once, to nearest even (fp16 overflows to inf and keeps subnormals)
template <typename T>
__device__ __forceinline__ void store8_f32(T *p, const float (&v)[8]) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4 *>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        vec8<T> t;
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = (T)v[j];
        *reinterpret_cast<vec8<T> *>(p) = t;
    }
}
#endif

}  // namespace vah
