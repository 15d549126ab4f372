// The 16-bit working copies of a forward's fp32 parameters in one launch (include/vitadapter_hip_epoch.h).
//
// Before this kernel a step made them with a multi-tensor cast for the nn.Linear parameters (6 launches) and, per use,
// cat + index_select + cast (the head-interleaved MSDeformAttn pair weights), permute + cast + copy (the tap-major 3x3
// weights, the transposed-convolution matrix) or a plain cast (1x1 / patch weights): ~100 launches of 3-6 us that only
// re-type or re-lay out parameters.  Every one of them is a strided gather of fp32 elements written contiguously in the
// destination's order, so one table of such jobs, cut into 2048-element chunks, describes them all and one grid runs it.
//
// A workgroup owns one chunk, a thread 8 consecutive destination elements (32 bytes read, 16 written).  A dense job
// (flag 1) moves them with two 16-byte loads and one 16-byte store; a strided job decomposes each element's index
// (uniform divisors from the job) - those are the small layouts (2.4 M elements for `up`, 0.6 M per 3x3 weight), whose
// strided reads stay in L2.  The table is data: every destination is checked against the buffer's capacity and every
// source offset against the job's own extent before it is used.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vitadapter_hip_epoch.h"
#include "common.h"
#include "elem16.h"

namespace vah {
namespace {

constexpr int kChunk = 2048;            // elements per workgroup: 256 threads x 8
constexpr int64_t kDense = 1, kToF32 = 2;

struct EpochJob {
    int64_t src, dst, n, d1, d2, d3, s[4], l[4], flags, src_elems;
};
static_assert(sizeof(EpochJob) == 128, "the job layout is part of the ABI");

template <typename T>
__global__ __launch_bounds__(256) void epoch_copies_kernel(const EpochJob *__restrict__ jobs, int njobs,
                                                           const int2 *__restrict__ chunks, T *__restrict__ out16,
                                                           int64_t cap16, float *__restrict__ out32, int64_t cap32) {
    const int2 ch = chunks[blockIdx.x];
    if (ch.x < 0 || ch.x >= njobs || ch.y < 0) return;
    const EpochJob &j = jobs[ch.x];
    const int64_t n = j.n;
    const int64_t e0 = (int64_t)ch.y * kChunk + threadIdx.x * 8;
    if (e0 >= n) return;
    const int cnt = (int)(n - e0 < 8 ? n - e0 : 8);
    const float *src = reinterpret_cast<const float *>(j.src);
    const int64_t src_elems = j.src_elems;
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = 0.f;
    if (j.flags & kDense) {
        const float *p = src + e0;
        if (e0 + cnt > src_elems) return;
        if (cnt == 8 && ((uintptr_t)p & 15) == 0) {
            const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < cnt) v[u] = p[u];
        }
    } else {
        const unsigned d1 = (unsigned)j.d1, d2 = (unsigned)j.d2, d3 = (unsigned)j.d3;
        if (d1 == 0 || d2 == 0 || d3 == 0) return;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (u < cnt) {
                unsigned t = (unsigned)(e0 + u);
                const unsigned i3 = t % d3;
                t /= d3;
                const unsigned i2 = t % d2;
                t /= d2;
                const unsigned i1 = t % d1;
                const unsigned i0 = t / d1;
                const int64_t off = i0 * j.s[0] + i1 * j.s[1] + i2 * j.s[2] + i3 * j.s[3];
                if (i0 < j.l[0] && i1 < j.l[1] && i2 < j.l[2] && i3 < j.l[3] && off >= 0 && off < src_elems) v[u] = src[off];
            }
        }
    }
    const int64_t o = j.dst + e0;
    if (j.flags & kToF32) {
        if (j.dst < 0 || o + cnt > cap32) return;
        float *q = out32 + o;
        if (cnt == 8 && ((uintptr_t)q & 15) == 0) {
            *reinterpret_cast<float4 *>(q) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4 *>(q + 4) = make_float4(v[4], v[5], v[6], v[7]);
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < cnt) q[u] = v[u];
        }
    } else {
        if (j.dst < 0 || o + cnt > cap16) return;
        T *q = out16 + o;
        if (cnt == 8 && ((uintptr_t)q & 15) == 0) {
            store8_f32<T>(q, v);
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < cnt) q[u] = (T)v[u];
        }
    }
}

}  // namespace
}  // namespace vah

extern "C" {

int64_t vah_epoch_job_bytes(void) { return (int64_t)sizeof(vah::EpochJob); }

int64_t vah_epoch_chunk_elems(void) { return vah::kChunk; }

int vah_epoch_copies(const void *jobs, int64_t njobs, const void *chunks, int64_t nchunks, int dtype16, void *out16,
                     int64_t cap16, float *out32, int64_t cap32, void *stream) {
    using namespace vah;
    const char *fn = "vah_epoch_copies";
    clear_error();
    if (njobs < 0 || nchunks < 0 || cap16 < 0 || cap32 < 0 || njobs > (1 << 24) || nchunks > (int64_t)0x7fffffff)
        return fail(VAH_E_SHAPE, "%s: bad dims", fn);
    if (dtype16 != 1 && dtype16 != 2) return fail(VAH_E_UNSUPPORTED, "%s: dtype16 is 1 (bf16) or 2 (fp16)", fn);
    if (nchunks == 0) return VAH_OK;
    if (njobs == 0) return fail(VAH_E_SHAPE, "%s: chunks without jobs", fn);
    if (!jobs || !chunks || (cap16 > 0 && !out16) || (cap32 > 0 && !out32)) return fail(VAH_E_NULL, "%s: null pointer", fn);
    if ((uintptr_t)jobs % 8 || (uintptr_t)chunks % 8 || (uintptr_t)out16 % 16 || (uintptr_t)out32 % 16)
        return fail(VAH_E_ALIGN, "%s: misaligned pointer (tables 8 bytes, buffers 16)", fn);
    hipStream_t st = (hipStream_t)stream;
    // the chunks cover every destination element once (the host's table): 4 bytes read per element, 2 (or 4) written
    LaunchScope scope(dtype16 == 2 ? "epoch_copies_f16" : "epoch_copies", cap16 * 6 + cap32 * 8, st, (cap16 + cap32) * 8);
    if (dtype16 == 2)
        hipLaunchKernelGGL(epoch_copies_kernel<_Float16>, dim3((unsigned)nchunks), dim3(256), 0, st, (const EpochJob *)jobs, (int)njobs,
                           (const int2 *)chunks, (_Float16 *)out16, cap16, out32, cap32);
    else
        hipLaunchKernelGGL(epoch_copies_kernel<__bf16>, dim3((unsigned)nchunks), dim3(256), 0, st, (const EpochJob *)jobs, (int)njobs,
                           (const int2 *)chunks, (__bf16 *)out16, cap16, out32, cap32);
    return check_launch(fn);
}

}  // extern "C"
