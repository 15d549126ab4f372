/*
 * vitadapter_hip_seg_eval.h -- C ABI of libvitadapter_hip.so, eleventh part: the class counts of the mIoU evaluation
 * (csrc/seg_eval.hip).  Conventions, error codes and the ABI version are those of vitadapter_hip.h (adding symbols does not
 * move the version): argument checks come before any device work, strides are in ELEMENTS, an empty problem returns VAH_OK
 * and reads no pointer.  The entry points are spelled vah_segeval_* (the prefix vah_seg_ belongs to the seventh part).
 *
 * Replaces mmseg's intersect_and_union (mmseg/core/evaluation/metrics.py of mmseg 0.20: three torch.histc calls on float
 * copies of boolean-masked maps, on the CPU) for label maps that are already on the device: the predicted labels that
 * vah_seg_finish / vah_seg_argmax write and the ground truth go into one counting pass, and the 3 x C int64 totals of a whole
 * validation set stay on the device.
 *
 *   pred       int64 (N, H, W), [n][y][x] at n * img_stride + y * row_stride + x (column stride 1): what the seventh part writes.
 *   label      the same addressing with strides of its own; dtype code 0 int64, 1 uint8 (VAH_E_UNSUPPORTED otherwise).
 *              For both maps row_stride >= W and img_stride >= (H - 1) * row_stride + W: rows and images never overlap
 *              (VAH_E_SHAPE), the stride rules of the seventh part's label maps.
 *   rule       for every pixel, in this order (mmseg's):
 *                1. g = label
 *                2. if label_map != NULL and 0 <= g < label_map_len: g = label_map[g].  label_map is an int64 table of
 *                   label_map_len <= 256 entries (more, or a negative length: VAH_E_SHAPE); every entry applies to the
 *                   ORIGINAL value, all at once
 *                3. if reduce_zero_label: g = 255 if g == 0 or g == 255, else g - 1
 *                4. if g == ignore_index the pixel counts for nothing
 *                5. otherwise, with p = pred: area_pred[p]++ if 0 <= p < C; area_label[g]++ if 0 <= g < C;
 *                   area_intersect[p]++ if p == g and 0 <= p < C
 *              A predicted or ground-truth value outside [0, C), a negative one included, indexes nothing: the range test
 *              comes before every table or counter access.
 *   totals     int64 [3][C]: intersect, pred, label.  ADDED to (+=).  The union is pred + label - intersect, formed by the
 *              caller.
 *   mmseg 0.20 differs in two places.  For C == 1 its torch.histc(min=0, max=0) falls back to the data's own range and counts
 *              everything; here C == 1 follows the rule above.  It applies the label_map entries one after another in place,
 *              so a chain a -> b, b -> c sends a to c; here the mapping is simultaneous (mmseg's later, fixed behaviour).
 *   order      all counts are integers, so any order gives the same bits.  Integer LDS atomics inside a workgroup; global
 *              memory sees plain vector stores only: no global atomics, counters or flags, nothing read back to the host,
 *              and the call captures into a graph.  Launch one (profile row seg_eval_count): a workgroup counts a
 *              contiguous range of fewer than 2^31 pixels into LDS and stores its [3][C] row of 32-bit counts into ws.  A
 *              lane owns two consecutive pixels (one 16-byte load of pred); consecutive lanes that hold the same
 *              (pred, label) pair are found with one ballot and only the first lane of such a run adds, the run's length.
 *              Launch two (profile row seg_eval_merge) adds the rows into totals as int64.
 *   limits     1 <= C <= 4096 (C < 1: VAH_E_SHAPE, above: VAH_E_UNSUPPORTED).  N, H, W >= 0 and < 2^31, N <= 65535, an image
 *              of fewer than 2^31 pixels (VAH_E_SHAPE).  pred, int64 labels, label_map and totals 8-byte, ws 16-byte aligned
 *              (VAH_E_ALIGN); uint8 labels may have any alignment and any row stride >= W.  Empty: N * H * W == 0 (sizes,
 *              C, the dtype code and label_map_len are still checked).
 *
 * vah_segeval_ws_bytes  bytes of workspace for vah_segeval_update (0 for an empty or impossible problem):
 *                       workgroups * 3 * C * 4, at most 1024 workgroups of at least 4096 pixels (fewer workgroups for a
 *                       large C, so the rows stay within a few MB).
 * vah_segeval_update    the two launches above.  ws_bytes below vah_segeval_ws_bytes: VAH_E_SHAPE.
 */
#ifndef VITADAPTER_HIP_SEG_EVAL_H
#define VITADAPTER_HIP_SEG_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t vah_segeval_ws_bytes(int64_t N, int64_t H, int64_t W, int64_t C);
int vah_segeval_update(const void *pred, int64_t pred_img_stride, int64_t pred_row_stride, const void *label, int label_dtype,
                       int64_t label_img_stride, int64_t label_row_stride, int64_t N, int64_t H, int64_t W, int64_t C,
                       int64_t ignore_index, int reduce_zero_label, const void *label_map, int64_t label_map_len, void *totals,
                       void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_SEG_EVAL_H */
