/*
 * vitadapter_hip_epoch.h -- C ABI of libvitadapter_hip.so: the per-step parameter work of a training step
 * (csrc/epoch_copies.hip, csrc/gemm.hip, csrc/tail_ops.hip).  Conventions, error codes and the ABI version are those of
 * vitadapter_hip.h (adding symbols does not move the version).
 *
 * 1. vah_epoch_copies: every 16-bit working copy of fp32 parameters that one forward needs, in ONE launch driven by a
 *    device-resident job table (vitadapter/fused.py::_EpochCopies builds it once per model and 16-bit type).
 *
 *    A JOB is a strided gather-and-cast: vah_epoch_job_bytes() = 128 bytes, sixteen int64 fields
 *        src          address of the fp32 source (4-byte aligned)
 *        dst          element offset of the job's first element in out16 (or out32, flag 2)
 *        n            elements written, = d0 * d1 * d2 * d3; 1 <= n < 2^31
 *        d1, d2, d3   sizes of the destination's dims 1..3 (dim 0 is n / (d1 * d2 * d3)); the job writes its elements
 *                     contiguously in destination order, element e <-> (i0, i1, i2, i3) row-major
 *        s0..s3       element strides of the SOURCE for those four indices
 *        l0..l3       extents of the source along them: an index i_k >= l_k reads as 0.0f (zero padding, e.g. a 3-channel
 *                     stem weight laid out for a 16-channel input)
 *        flags        1: the source is dense in destination order (s3 = 1, no padding) - 16-byte loads; 2: the destination is
 *                     out32 and the elements are copied, not cast
 *        src_elems    elements readable behind src: an offset >= src_elems is never read (the element is 0)
 *    A CHUNK is (int32 job, int32 k): elements [k * C, min(n, (k + 1) * C)) of that job, C = vah_epoch_chunk_elems() = 2048.
 *    One workgroup of 256 threads runs one chunk, 8 consecutive elements per thread; the chunk table lists every chunk of
 *    every job, so one grid covers all jobs at streaming rate.
 *
 *    cast       (__bf16) / (_Float16) of the fp32 value: round to nearest even, what torch's .to() gives; fp16 overflow goes
 *               to +-inf, subnormals are kept; a NaN stays a NaN.
 *    dtype16    1 bf16, 2 fp16 (the codes of vitadapter_hip_group_norm.h); anything else is VAH_E_UNSUPPORTED.
 *    bounds     a chunk that names a job >= njobs, and an element whose destination lies outside [0, cap16) / [0, cap32),
 *               is skipped: a damaged table cannot write outside the two buffers.
 *    alignment  jobs, chunks 8-byte aligned, out16 and out32 16-byte aligned (VAH_E_ALIGN).  A thread whose 8 elements start
 *               16-byte aligned on both sides moves them with 16-byte accesses, any other thread one element at a time.
 *    order      argument checks come before any device work; nchunks == 0 returns VAH_OK and reads no pointer.  Nothing is
 *               allocated, copied from the host or synchronised: the call captures into a graph as one kernel node.
 *    profile    row epoch_copies (epoch_copies_f16).
 *
 * 2. vah_gemm_bf16_fin_rowmap / vah_gemm_f16_fin_rowmap: vah_gemm_bf16_fin / vah_gemm_f16_fin (vitadapter_hip.h) with an
 *    int32 row map of M entries for the reduction launch: row r of the product is stored to row row_map[r] of D and the
 *    finalize job's sum k to fin_out[row_map[k]] (fin_C must equal M; an entry outside [0, M) drops its row).  The
 *    slices are loaded and added exactly as without a map: every bit is what index_select of the unmapped result by the
 *    inverse map gives.  The map can only ride on a reduction launch: where the dispatcher runs the product with split 1
 *    hipBLASLt writes D itself, the map is NOT applied to D or fin_out, and *applied is 0 (else 1) - the caller reorders.
 *    row_map null: VAH_E_NULL.  applied is a host pointer and may be null.
 *
 * 3. vah_bn_finalize_stats_book: vah_bn_finalize_stats (vitadapter_hip.h) with BatchNorm's bookkeeping in the same launch:
 *    the element count is an ARGUMENT (not read from sums[2 * C]) and is also stored to sums[2 * C], where the backward
 *    reads it; num_batches_tracked (int64, may be null) is incremented by one.  mean, rstd and the running statistics
 *    are computed by the same expressions as vah_bn_finalize_stats.  For a BatchNorm without a process group: with one, the
 *    count has to be in sums before the all-reduce.
 */
#ifndef VITADAPTER_HIP_EPOCH_H
#define VITADAPTER_HIP_EPOCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t vah_epoch_job_bytes(void);
int64_t vah_epoch_chunk_elems(void);
int vah_epoch_copies(const void *jobs, int64_t njobs, const void *chunks, int64_t nchunks, int dtype16,
                     void *out16, int64_t cap16, float *out32, int64_t cap32, void *stream);

int vah_gemm_bf16_fin_rowmap(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda,
                             const void *B, int64_t ldb, void *D, int64_t ldd, int d_is_f32, void *workspace,
                             int64_t workspace_bytes, const float *fin_part, int64_t fin_nparts, int64_t fin_C,
                             float *fin_out, const int32_t *row_map, int *applied, void *stream);
int vah_gemm_f16_fin_rowmap(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda,
                            const void *B, int64_t ldb, void *D, int64_t ldd, int d_is_f32, void *workspace,
                            int64_t workspace_bytes, const float *fin_part, int64_t fin_nparts, int64_t fin_C,
                            float *fin_out, const int32_t *row_map, int *applied, void *stream);

int vah_bn_finalize_stats_book(float *sums, int64_t C, float count, float eps, float momentum, float *running_mean,
                               float *running_var, float *mean, float *rstd, int64_t *num_batches_tracked,
                               void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_EPOCH_H */
