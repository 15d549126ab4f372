/*
 * vitadapter_hip_masked_attn.h -- C ABI of libvitadapter_hip.so, fifth part: masked cross-attention of Mask2Former's query
 * decoder (csrc/masked_attn.hip).  Conventions, error codes and the ABI version are those of vitadapter_hip.h (adding symbols
 * does not move the version); dtype codes and the (pointer, dtype, stride, stride) form of a tensor operand are those of
 * vitadapter_hip_group_norm.h.
 *
 * Replaces the cross-attention of the reference's Mask2FormerHead (segmentation/mmseg_custom/models/decode_heads/
 * mask2former_head.py:404-525): Lq <= 128 queries attend to the Lk keys of one pyramid level, H heads of 32 channels, under a
 * boolean mask derived from the previous layer's mask prediction:
 *     out = softmax(scale q k^T + (-inf where the key is excluded)) v
 * The reference repeats an (N, Lq, Lk) bool mask over the heads, materialises (N * H, Lq, Lk) scores and repairs rows that
 * exclude every key with a torch.where (a host synchronisation).  Here the mask is one bit per (image, query, key), shared by
 * the heads, the "keep everything" repair is part of packing it, and nothing is read back to the host.
 *
 * vah_mca_pack_mask   x[n][q][j] (mask logits: the interpolated mask_pred; dtype code 0 fp32, 1 bf16, 2 fp16; element
 *                     [n][q][j] at n * x_img_stride + q * x_row_stride + j, strides in ELEMENTS, no alignment asked)
 *                     -> bits[n][q][w], uint32, contiguous, W = ceil(Lk / 32) words per row: bit (j & 31) of word (j >> 5)
 *                     is set when key j is KEPT.
 *                       - a key is kept iff !(x < 0): -0.0, +0.0 and NaN are kept;
 *                       - a row that keeps no key keeps every key (the reference's :502-503);
 *                       - bits at positions >= Lk of the last word are 0.
 *                     Deviation from the reference: it tests sigmoid(x) < 0.5 with torch's rounded sigmoid, which is x < 0
 *                     in exact arithmetic but differs from it in a thin band below zero (about -2e-7 < x < 0 in fp32, -1e-3
 *                     in fp16, -4e-3 in bf16: there the rounded sigmoid is exactly 0.5 and the reference keeps the key, the
 *                     sign test excludes it).  The torch expression of this project uses x < 0 too.
 *                     One workgroup owns a row.  N * Q * Lk == 0 returns VAH_OK and reads no pointer; bits needs 4-byte
 *                     alignment only.
 *
 * vah_mca_forward / vah_mca_backward
 *   operands   q, out, d_out, dq: (Lq, N, H * 32); k, v, dk, dv: (Lk, N, H * 32); element [t][n][c] at
 *              t * tok_stride + n * img_stride + c (strides in ELEMENTS), so k and v may be column slices of a packed
 *              projection or a level's rows of a larger buffer.  Dtype code 1 (bf16) or 2 (fp16), the same for every operand
 *              of a call: fp32 (0) and bf16 beside fp16 are VAH_E_UNSUPPORTED.  bits as written by vah_mca_pack_mask for
 *              (N, Lq, Lk).  lse: fp32 (N, H, Lq), log2 domain (log2 of the sum of exp2(scale * log2(e) * s)), as in the
 *              other attention kernels.  scale: the factor of q k^T (1 / sqrt(32) in the head).
 *   shapes     head_dim must be 32 and 1 <= Lq <= 128 (else VAH_E_UNSUPPORTED); H >= 1; any Lk >= 1 (below 2^30); N, H <= 65535.
 *              Lk == 0 with Lq > 0 is VAH_E_SHAPE.  N * H * Lq == 0 returns VAH_OK and reads no pointer.
 *   alignment  every tensor pointer 16-byte aligned, every stride a multiple of 8 elements (VAH_E_ALIGN); bits 4-byte,
 *              lse 4-byte, ws 16-byte aligned.
 *   numerics   the contract of the other attention kernels: scores, max, sum, lse, delta and every accumulator
 *              are fp32; P (forward, backward) and dS (backward) are rounded to T once each as MFMA operands, every output
 *              once at its store.  Excluded keys contribute exactly 0 (P and dS are set to 0, not multiplied by it).  A row of
 *              bits with no bit set (never produced by vah_mca_pack_mask) gives NaN, as softmax over -inf does.
 *   chunks     the keys are cut into vah_mca_splits(Lk) chunks of whole 64-key tiles:
 *                  tiles = ceil(Lk / 64),  tiles_per_chunk = ceil(tiles / min(16, tiles)),
 *                  splits = ceil(tiles / tiles_per_chunk),  chunk = 64 * tiles_per_chunk keys (the last one shorter).
 *              Up to Lk = 1024 a chunk is one tile.  At N * H = 16 the three levels of a 640 x 640 image give 7 x 16 = 112
 *              (Lk 400), 13 x 16 = 208 (1600) and 15 x 16 = 240 (6400) workgroups on 256 CUs.  The rule is chosen by that
 *              count alone; no other rule has been timed against it.
 *   forward    a workgroup owns (chunk, head, image) and all Lq queries (4 waves x 32 query rows; rows >= Lq are clamped when
 *              loaded and never stored) and loops over the 64-key tiles of its chunk.  A chunk that holds no kept key for a
 *              row leaves that row's running max at -inf and its sum at 0.  With more than one chunk each workgroup writes
 *              an fp32 partial (unnormalised o, m, l) to the workspace and a second launch merges the chunks in ascending
 *              order into out and lse; a single-chunk call writes them directly.
 *   backward   a small launch forms delta = rowsum(d_out o out) in the workspace; the main launch has the forward's grid,
 *              keeps every query's q and d_out in registers and recomputes P from lse.  dv and dk of a chunk's keys are
 *              complete inside the workgroup: the four waves' parts are summed through LDS, wave 0 first, and stored once.
 *              The chunk's part of dq goes to the workspace in fp32 and a last launch sums the chunks in ascending order
 *              (a single-chunk call stores dq directly).  The mask gets no gradient (the reference detaches it, :442).
 *   ordering   between launches by kernel boundaries on the stream only: no atomics, no counters or flags between workgroups,
 *              no last-arriver reductions, nothing read back to the host.  The same inputs give the same bits, and the
 *              calls capture into a graph.
 *   workspace  vah_mca_ws_bytes(N, H, Lq, Lk) bytes, 16-byte aligned, for either direction: with R = N * H * Lq rows and
 *              S = vah_mca_splits(Lk), 4 * (4 * ceil(R / 4) + 34 * R * S) rounded up to a multiple of 16 (delta, then per row
 *              and chunk 32 fp32 of o or dq, m and l).  A smaller ws_bytes is VAH_E_SHAPE ("workspace too small").
 *              0 for a non-positive dimension.
 *   order      argument checks come before any device work.
 *   profile    rows mca_pack, mca_fwd, mca_fwd_merge, mca_bwd (delta and the main launch), mca_dq_reduce, with `_f16`
 *              appended where the 16-bit operands are fp16 (mca_pack: where the logits are fp16).
 */
#ifndef VITADAPTER_HIP_MASKED_ATTN_H
#define VITADAPTER_HIP_MASKED_ATTN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t vah_mca_splits(int64_t Lk);
int64_t vah_mca_ws_bytes(int64_t N, int64_t H, int64_t Lq, int64_t Lk);
int vah_mca_pack_mask(const void *x, int x_dtype, int64_t x_row_stride, int64_t x_img_stride, int64_t N, int64_t Q, int64_t Lk,
                      void *bits, void *stream);
int vah_mca_forward(const void *q, int q_dtype, int64_t q_tok_stride, int64_t q_img_stride,
                    const void *k, int k_dtype, int64_t k_tok_stride, int64_t k_img_stride,
                    const void *v, int v_dtype, int64_t v_tok_stride, int64_t v_img_stride,
                    const void *bits, int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t head_dim, float scale,
                    void *out, int out_dtype, int64_t out_tok_stride, int64_t out_img_stride,
                    void *lse, void *ws, int64_t ws_bytes, void *stream);
int vah_mca_backward(const void *q, int q_dtype, int64_t q_tok_stride, int64_t q_img_stride,
                     const void *k, int k_dtype, int64_t k_tok_stride, int64_t k_img_stride,
                     const void *v, int v_dtype, int64_t v_tok_stride, int64_t v_img_stride,
                     const void *bits,
                     const void *out, int out_dtype, int64_t out_tok_stride, int64_t out_img_stride,
                     const void *d_out, int d_out_dtype, int64_t d_out_tok_stride, int64_t d_out_img_stride,
                     const void *lse, int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t head_dim, float scale,
                     void *dq, int dq_dtype, int64_t dq_tok_stride, int64_t dq_img_stride,
                     void *dk, int dk_dtype, int64_t dk_tok_stride, int64_t dk_img_stride,
                     void *dv, int dv_dtype, int64_t dv_tok_stride, int64_t dv_img_stride,
                     void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_MASKED_ATTN_H */
