// The training targets of Mask2Former from a label map (include/vitadapter_hip_seg_target.h): per image the distinct labels
// without ignore_index, ascending, and one 0 / 1 mask per label, in three launches.
//   * seg_target_scan: a workgroup of 256 lanes reads a contiguous pixel range of one image, 16 bytes a lane and load, and
//     marks what it meets in 256 LDS flags (plain stores of 1: every writer writes the same).  Label maps are piecewise
//     constant, so a lane marks only where the value differs from the one before.  Where the rows of an image follow each
//     other without a gap the range is one run for the whole workgroup; otherwise every wave takes a row of the range at a
//     time.  The remap table is applied to the 256 flags at the end, not to the pixels.  The flags leave as a 256-bit row.
//   * seg_target_finish: one workgroup; per image 32 lanes OR each of the 8 words of its rows, the set bits are ranked by a
//     popcount prefix, and labels / slot / meta are written (the header describes them).
//   * seg_target_masks: a wave per 1024 pixels of one image.  A lane turns its 16 labels into the image's local target
//     indices (one LDS lookup each: remap and slot folded into one table), packed four to a dword, and compares all four with
//     a target's index in a handful of integer operations; one 16-byte store per target and lane.  The launch is a streaming
//     write of G_total * H * W bytes next to H * W labels read once.
// A value outside [0, 256) sets the out-of-range word before anything is indexed with it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vitadapter_hip_seg_target.h"
#include "common.h"

namespace vah {
namespace {

constexpr int kValues = 256;                // label values the kernels handle
constexpr int kScanThreads = 256;
constexpr int kDepth = 4;                   // 16-byte loads of a lane in flight
constexpr int64_t kMinChunk = 4096;         // pixels of a scan workgroup at least; chunks are multiples of it
constexpr int kMaxParts = 256;              // scan workgroups per image at most
constexpr int kRowWords = 16;               // a workspace row: 8 words of bits, the out-of-range word, 64 bytes in all
constexpr int kMaskThreads = 64, kGroup = 16;
constexpr int64_t kMaxN = 4096;

template <typename T>
using Two = T __attribute__((ext_vector_type(2)));

struct ScanArgs {
    const void *label;
    int64_t is, rs;
    const uint8_t *remap;
    unsigned *ws;
    unsigned H, W, HW, chunk, parts;
};

// flags[v] = 1 for a value in [0, 256), flags[256] = 1 for any other; nothing where the flag is the lane's previous one (-1: none)
__device__ __forceinline__ void mark(int *flags, int64_t v, int &prev) {
    const int key = (uint64_t)v < (uint64_t)kValues ? (int)v : kValues;
    if (key == prev) return;
    prev = key;
    flags[key] = 1;
}

__device__ __forceinline__ void mark16(int *flags, const uint4 q, int &prev) {
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) mark(flags, (int64_t)((w[j >> 2] >> (8 * (j & 3))) & 255u), prev);
}

// one run of `len` labels at p, by lanes t = 0 .. G - 1 (G >= 16): scalar loads up to the first 16-byte boundary, 16-byte loads,
// scalar loads for what is left
template <typename T>
__device__ __forceinline__ void scan_run(int *flags, const T *p, unsigned len, unsigned t, unsigned G, int &prev) {
    constexpr unsigned per = 16 / sizeof(T);
    unsigned head = (unsigned)((16 - (uintptr_t)p % 16) % 16 / sizeof(T));
    if (head > len) head = len;
    if (t < head) mark(flags, (int64_t)p[t], prev);
    const T *body = p + head;
    const unsigned nvec = (len - head) / per;
    for (unsigned k = t; k < nvec; k += kDepth * G) {
        if constexpr (sizeof(T) == 1) {
            uint4 q[kDepth];
#pragma unroll
            for (int d = 0; d < kDepth; ++d)
                if (k + d * G < nvec) q[d] = reinterpret_cast<const uint4 *>(body)[k + d * G];
#pragma unroll
            for (int d = 0; d < kDepth; ++d)
                if (k + d * G < nvec) mark16(flags, q[d], prev);
        } else {
            Two<int64_t> q[kDepth];
#pragma unroll
            for (int d = 0; d < kDepth; ++d)
                if (k + d * G < nvec) q[d] = reinterpret_cast<const Two<int64_t> *>(body)[k + d * G];
#pragma unroll
            for (int d = 0; d < kDepth; ++d)
                if (k + d * G < nvec) mark(flags, q[d].x, prev), mark(flags, q[d].y, prev);
        }
    }
    const unsigned done = head + nvec * per;
    if (t < len - done) mark(flags, (int64_t)p[done + t], prev);
}

template <typename T>
__global__ __launch_bounds__(kScanThreads) void seg_target_scan_kernel(const ScanArgs a) {
    __shared__ int raw[kValues + 1], out[kValues];
    const unsigned tid = threadIdx.x, part = blockIdx.x, n = blockIdx.y;
    raw[tid] = 0, out[tid] = 0;
    if (tid == 0) raw[kValues] = 0;
    __syncthreads();
    const T *img = static_cast<const T *>(a.label) + (int64_t)n * a.is;
    const unsigned p0 = part * a.chunk, p1 = a.HW - p0 > a.chunk ? p0 + a.chunk : a.HW;       // p0 < HW: parts = ceil(HW / chunk)
    int prev = -1;
    if (a.rs == (int64_t)a.W || a.H == 1) {
        scan_run(raw, img + p0, p1 - p0, tid, kScanThreads, prev);
    } else {
        const unsigned y0 = p0 / a.W, y1 = (p1 - 1) / a.W, lane = tid & 63;
        for (unsigned y = y0 + (tid >> 6); y <= y1; y += kScanThreads / kWave) {
            const unsigned xa = y == y0 ? p0 - y0 * a.W : 0, xb = y == y1 ? p1 - y1 * a.W : a.W;
            scan_run(raw, img + (int64_t)y * a.rs + xa, xb - xa, lane, kWave, prev);
        }
    }
    __syncthreads();
    if (raw[tid]) out[a.remap ? (int)a.remap[tid] : (int)tid] = 1;
    __syncthreads();
    const uint64_t bits = __ballot(out[tid] != 0);
    unsigned *row = a.ws + ((int64_t)n * a.parts + part) * kRowWords;
    if ((tid & 63) == 0) row[2 * (tid >> 6)] = (unsigned)bits, row[2 * (tid >> 6) + 1] = (unsigned)(bits >> 32);
    if (tid == 0) row[8] = raw[kValues] ? 1u : 0u;
}

__global__ __launch_bounds__(kValues) void seg_target_finish_kernel(const unsigned *ws, int N, int parts, int64_t ignore, int64_t *labels,
                                                                    int *slot, int *meta) {
    __shared__ unsigned part_or[kValues], set[8], oor_s[kValues];
    const int tid = (int)threadIdx.x, w = tid & 7;
    unsigned oor = 0;
    int first = 0;
    for (int n = 0; n < N; ++n) {
        const unsigned *rows = ws + (int64_t)n * parts * kRowWords;
        unsigned acc = 0;
        for (int p = tid >> 3; p < parts; p += kValues / 8) acc |= rows[(int64_t)p * kRowWords + w];
        for (int p = tid; p < parts; p += kValues) oor |= rows[(int64_t)p * kRowWords + 8];
        part_or[tid] = acc;
        __syncthreads();
        if (tid < 8) {
            unsigned s = 0;
            for (int j = 0; j < kValues / 8; ++j) s |= part_or[8 * j + tid];
            if ((uint64_t)ignore < (uint64_t)kValues && (int)(ignore >> 5) == tid) s &= ~(1u << (ignore & 31));
            set[tid] = s;
        }
        __syncthreads();
        int rank = 0, count = 0;
        for (int k = 0; k < 8; ++k) {
            const int c = __popc(set[k]);
            if (k < (tid >> 5)) rank += c;
            count += c;
        }
        const unsigned word = set[tid >> 5];
        const bool present = (word >> (tid & 31)) & 1u;
        rank += __popc(word & ((1u << (tid & 31)) - 1u));
        slot[n * kValues + tid] = present ? first + rank : -1;
        if (present) labels[n * kValues + rank] = tid;             // rank < count
        if (tid >= count) labels[n * kValues + tid] = -1;
        if (tid == 0) meta[n] = first;
        first += count;
        __syncthreads();                                            // part_or and set are written again for the next image
    }
    oor_s[tid] = oor;
    __syncthreads();
    if (tid == 0) {
        unsigned s = 0;
        for (int j = 0; j < kValues; ++j) s |= oor_s[j];
        meta[N] = first;
        meta[N + 1] = s ? 1 : 0;
    }
}

struct MaskArgs {
    const void *label;
    int64_t is, rs;
    const uint8_t *remap;
    const int *slot;
    const int64_t *labels;
    const int *meta;
    int64_t G;
    uint8_t *masks;
    int *image_of;
    int64_t *labels_out;
    unsigned W, HW;
};

// 0x01 in every byte of x that is zero, 0x00 in the others (exact: no carry leaves a byte)
__device__ __forceinline__ unsigned zero_bytes(unsigned x) {
    return (~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu)) >> 7;
}

// kAligned: H * W is a multiple of 16, so every lane holds 16 pixels and every target plane starts on a 16-byte boundary
template <typename T, bool kAligned>
__global__ __launch_bounds__(kMaskThreads) void seg_target_masks_kernel(const MaskArgs a) {
    __shared__ short lidx[kValues];
    const unsigned tid = threadIdx.x, n = blockIdx.y;
    int64_t first = a.meta[n], last = a.meta[n + 1];
    if (first < 0) first = 0;
    if (last > a.G) last = a.G;
    if (last - first > kValues) last = first + kValues;
    if (last <= first) return;                                      // the whole workgroup: no target, nothing to write
    const int count = (int)(last - first);
    for (unsigned v = tid; v < (unsigned)kValues; v += kMaskThreads) {
        const unsigned r = a.remap ? a.remap[v] : v;
        const int64_t s = a.slot[n * kValues + r];
        lidx[v] = s >= first && s < last ? (short)(s - first) : (short)-1;
    }
    if (blockIdx.x == 0) {
        for (int t = (int)tid; t < count; t += kMaskThreads) {
            a.image_of[first + t] = (int)n;
            a.labels_out[first + t] = a.labels[n * kValues + t];
        }
    }
    __syncthreads();
    const int64_t p0 = ((int64_t)blockIdx.x * kMaskThreads + tid) * kGroup;
    if (p0 >= a.HW) return;
    const unsigned cnt = a.HW - p0 >= kGroup ? kGroup : (unsigned)(a.HW - p0);
    unsigned y = (unsigned)p0 / a.W, x = (unsigned)p0 - y * a.W;
    const T *img = static_cast<const T *>(a.label) + (int64_t)n * a.is;
    const T *p = img + (int64_t)y * a.rs + x;

    unsigned idx[4] = {0, 0, 0, 0}, ok[4] = {0, 0, 0, 0};          // local target index and 0x01 per pixel that has one
    auto put = [&](int j, int64_t v) {
        if ((uint64_t)v < (uint64_t)kValues) {
            const int li = lidx[v];
            if (li >= 0) idx[j >> 2] |= (unsigned)li << (8 * (j & 3)), ok[j >> 2] |= 1u << (8 * (j & 3));
        }
    };
    if (cnt == kGroup && x + kGroup <= a.W && (uintptr_t)p % 16 == 0) {
        if constexpr (sizeof(T) == 1) {
            const uint4 q = *reinterpret_cast<const uint4 *>(p);
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) put(j, (int64_t)((w[j >> 2] >> (8 * (j & 3))) & 255u));
        } else {
            Two<int64_t> q[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = reinterpret_cast<const Two<int64_t> *>(p)[j];
#pragma unroll
            for (int j = 0; j < 8; ++j) put(2 * j, q[j].x), put(2 * j + 1, q[j].y);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if ((unsigned)j < cnt) {
                put(j, (int64_t)img[(int64_t)y * a.rs + x]);
                if (++x == a.W) x = 0, ++y;
            }
        }
    }
    uint8_t *o = a.masks + first * (int64_t)a.HW + p0;
    for (int g = 0; g < count; ++g, o += a.HW) {
        const unsigned gg = (unsigned)g * 0x01010101u;
        unsigned m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = zero_bytes(idx[k] ^ gg) & ok[k];
        if constexpr (kAligned) {
            *reinterpret_cast<uint4 *>(o) = make_uint4(m[0], m[1], m[2], m[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if ((unsigned)j < cnt) o[j] = (uint8_t)((m[j >> 2] >> (8 * (j & 3))) & 1u);
        }
    }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
constexpr int64_t kLim = (int64_t)1 << 31;

bool bad_size(int64_t v) { return v < 0 || v >= kLim; }

bool bad_dims(int64_t N, int64_t H, int64_t W) { return bad_size(N) || bad_size(H) || bad_size(W) || N > kMaxN || H * W >= kLim; }

// pixels of a scan workgroup: a multiple of kMinChunk that leaves at most kMaxParts workgroups per image
int64_t chunk_of(int64_t HW) {
    const int64_t per = (HW + kMaxParts - 1) / kMaxParts;
    const int64_t chunk = (per + kMinChunk - 1) / kMinChunk * kMinChunk;
    return chunk < kMinChunk ? kMinChunk : chunk;
}

int64_t parts_of(int64_t HW) { return (HW + chunk_of(HW) - 1) / chunk_of(HW); }

int dims_check(const char *fn, int64_t N, int64_t H, int64_t W, int dtype) {
    if (bad_dims(N, H, W))
        return fail(VAH_E_SHAPE, "%s: bad dims (N %lld, %lld x %lld; at most %lld images of fewer than 2^31 pixels)", fn, (long long)N,
                    (long long)H, (long long)W, (long long)kMaxN);
    if (dtype < 0 || dtype > 1) return fail(VAH_E_UNSUPPORTED, "%s: label dtype codes are 0 (int64) and 1 (uint8), not %d", fn, dtype);
    return 0;
}

int ptr_check(const char *fn, const char *name, const void *p, int align) {
    if (!p) return fail(VAH_E_NULL, "%s: null pointer (%s)", fn, name);
    if ((uintptr_t)p % align) return fail(VAH_E_ALIGN, "%s: %s misaligned (%d-byte pointer)", fn, name, align);
    return 0;
}

int map_check(const char *fn, const void *p, int dtype, int64_t is, int64_t rs, int64_t H, int64_t W) {
    if (int rc = ptr_check(fn, "label", p, dtype == 0 ? 8 : 1)) return rc;
    if (rs < W || is < (H - 1) * rs + W)
        return fail(VAH_E_SHAPE, "%s: label strides (row stride >= width, images that do not overlap)", fn);
    return 0;
}

}  // namespace
}  // namespace vah

extern "C" {

int64_t vah_segtgt_ws_bytes(int64_t N, int64_t H, int64_t W) {
    using namespace vah;
    if (N < 1 || H < 1 || W < 1 || bad_dims(N, H, W)) return 0;
    return N * parts_of(H * W) * kRowWords * 4;
}

int vah_segtgt_scan(const void *label, int label_dtype, int64_t label_img_stride, int64_t label_row_stride, int64_t N, int64_t H,
                    int64_t W, int64_t ignore_index, const void *remap, void *labels, void *slot, void *meta, void *ws,
                    int64_t ws_bytes, void *stream) {
    using namespace vah;
    const char *fn = "vah_segtgt_scan";
    clear_error();
    if (int rc = dims_check(fn, N, H, W, label_dtype)) return rc;
    if (N * H * W == 0) return VAH_OK;
    if (int rc = map_check(fn, label, label_dtype, label_img_stride, label_row_stride, H, W)) return rc;
    if (int rc = ptr_check(fn, "labels", labels, 8)) return rc;
    if (int rc = ptr_check(fn, "slot", slot, 4)) return rc;
    if (int rc = ptr_check(fn, "meta", meta, 4)) return rc;
    if (int rc = ptr_check(fn, "ws", ws, 16)) return rc;
    const int64_t HW = H * W, chunk = chunk_of(HW), parts = parts_of(HW), need = N * parts * kRowWords * 4;
    if (ws_bytes < need)
        return fail(VAH_E_SHAPE, "%s: workspace too small (%lld bytes, vah_segtgt_ws_bytes says %lld)", fn, (long long)ws_bytes,
                    (long long)need);
    hipStream_t st = (hipStream_t)stream;
    ScanArgs a;
    a.label = label, a.is = label_img_stride, a.rs = label_row_stride, a.remap = (const uint8_t *)remap, a.ws = (unsigned *)ws;
    a.H = (unsigned)H, a.W = (unsigned)W, a.HW = (unsigned)HW, a.chunk = (unsigned)chunk, a.parts = (unsigned)parts;
    {
        LaunchScope scope("seg_target_scan", N * HW * (label_dtype == 0 ? 8 : 1) + need, st);
        const dim3 grid((unsigned)parts, (unsigned)N), block(kScanThreads);
        if (label_dtype == 0) hipLaunchKernelGGL(seg_target_scan_kernel<int64_t>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(seg_target_scan_kernel<uint8_t>, grid, block, 0, st, a);
    }
    {
        LaunchScope scope("seg_target_finish", need + N * kValues * 12 + (N + 2) * 4, st);
        hipLaunchKernelGGL(seg_target_finish_kernel, dim3(1), dim3(kValues), 0, st, (const unsigned *)ws, (int)N, (int)parts, ignore_index,
                           (int64_t *)labels, (int *)slot, (int *)meta);
    }
    return check_launch(fn);
}

int vah_segtgt_masks(const void *label, int label_dtype, int64_t label_img_stride, int64_t label_row_stride, int64_t N, int64_t H,
                     int64_t W, const void *remap, const void *slot, const void *labels, const void *meta, int64_t G_total,
                     void *masks, void *image_of, void *labels_out, void *stream) {
    using namespace vah;
    const char *fn = "vah_segtgt_masks";
    clear_error();
    if (int rc = dims_check(fn, N, H, W, label_dtype)) return rc;
    if (G_total < 0 || G_total > N * kValues)
        return fail(VAH_E_SHAPE, "%s: G_total %lld (0 .. %d targets an image)", fn, (long long)G_total, kValues);
    if (N * H * W == 0 || G_total == 0) return VAH_OK;
    if (int rc = map_check(fn, label, label_dtype, label_img_stride, label_row_stride, H, W)) return rc;
    if (int rc = ptr_check(fn, "slot", slot, 4)) return rc;
    if (int rc = ptr_check(fn, "labels", labels, 8)) return rc;
    if (int rc = ptr_check(fn, "meta", meta, 4)) return rc;
    if (int rc = ptr_check(fn, "masks", masks, 16)) return rc;
    if (int rc = ptr_check(fn, "image_of", image_of, 4)) return rc;
    if (int rc = ptr_check(fn, "labels_out", labels_out, 8)) return rc;
    const int64_t HW = H * W;
    hipStream_t st = (hipStream_t)stream;
    MaskArgs a;
    a.label = label, a.is = label_img_stride, a.rs = label_row_stride, a.remap = (const uint8_t *)remap;
    a.slot = (const int *)slot, a.labels = (const int64_t *)labels, a.meta = (const int *)meta, a.G = G_total;
    a.masks = (uint8_t *)masks, a.image_of = (int *)image_of, a.labels_out = (int64_t *)labels_out;
    a.W = (unsigned)W, a.HW = (unsigned)HW;
    {
        LaunchScope scope("seg_target_masks", G_total * HW + N * HW * (label_dtype == 0 ? 8 : 1) + G_total * 12, st);
        const int64_t per = (int64_t)kMaskThreads * kGroup;
        const dim3 grid((unsigned)((HW + per - 1) / per), (unsigned)N), block(kMaskThreads);
        const bool aligned = HW % kGroup == 0;
        if (label_dtype == 0) {
            if (aligned) hipLaunchKernelGGL((seg_target_masks_kernel<int64_t, true>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((seg_target_masks_kernel<int64_t, false>), grid, block, 0, st, a);
        } else {
            if (aligned) hipLaunchKernelGGL((seg_target_masks_kernel<uint8_t, true>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((seg_target_masks_kernel<uint8_t, false>), grid, block, 0, st, a);
        }
    }
    return check_launch(fn);
}

}  // extern "C"
