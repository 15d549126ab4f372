/*
 * vitadapter_hip_seg_target.h -- C ABI of libvitadapter_hip.so, twelfth part: the training targets of Mask2Former from a
 * label map (csrc/seg_target.hip).  Conventions, error codes and the ABI version are those of vitadapter_hip.h (adding
 * symbols does not move the version): argument checks come before any device work, strides are in ELEMENTS, an empty
 * problem returns VAH_OK and reads no pointer.  The entry points are spelled vah_segtgt_* (vah_seg_ and vah_segeval_ belong
 * to the seventh and the eleventh part).
 *
 * Replaces the ToMask step of the reference's training pipeline (mmseg_custom/datasets/pipelines/formatting.py:52-82:
 * np.unique of the label map and one comparison per class, stacked as int64 on a data-loader core) for label maps that are
 * already on the device: the class labels and the binary masks of every image of a batch are built where the loss reads
 * them, as uint8, and the host learns the number of targets from one small copy.
 *
 *   label      (N, H, W), [n][y][x] at n * img_stride + y * row_stride + x (column stride 1); dtype code 0 int64, 1 uint8
 *              (VAH_E_UNSUPPORTED otherwise).  row_stride >= W and img_stride >= (H - 1) * row_stride + W: rows and images
 *              never overlap (VAH_E_SHAPE), the stride rules of the eleventh part.  Every image of a call is H x W.
 *   remap      NULL, or a table of 256 uint8 entries (any alignment) applied to the ORIGINAL value first, all entries at
 *              once: g = remap[label].  It expresses mmseg's reduce_zero_label and the reference's MapillaryHack.
 *   rule       per image, the one of formatting.py:58-77: the labels are the distinct values of the (remapped) map,
 *              ascending, without ignore_index; mask g is 1 where the map equals label g, else 0.  An image whose pixels are
 *              all ignored has no label and no mask.  ignore_index is an int64; a value outside [0, 256) removes nothing.
 *   range      values in [0, 256) are handled (mmseg label maps are 8-bit images).  An int64 value outside that range sets
 *              the "out of range" flag, contributes to nothing and indexes nothing: the range test comes before every table
 *              access.  The caller then has to build that call's targets by other means.
 *   order      everything is an integer, so the same input gives the same bits.  Global memory sees plain vector stores
 *              only: no global atomics, counters or flags.  Three launches:
 *              one (profile row seg_target_scan): a workgroup owns a contiguous pixel range of one image, marks the values
 *                it meets in 256 LDS flags and stores its 256-bit row (and an out-of-range word) into ws.  A lane loads 16
 *                bytes: 16 uint8 labels or 2 int64 ones; the unaligned head and tail of a row or range take scalar loads.
 *              two (profile row seg_target_finish): one workgroup, image after image: ORs the image's rows, clears
 *                ignore_index, ranks the set bits by a popcount prefix and writes
 *                  labels  int64 [N][256]  the image's labels ascending, -1 past its count
 *                  slot    int32 [N][256]  for value v of image n the global target index first_n + rank, or -1
 *                  meta    int32 [N + 2]   the exclusive offsets first_0 .. first_N (meta[N] is G_total), then the
 *                                          out-of-range flag (0 / 1): one small copy carries all the host needs
 *              three (profile row seg_target_masks): G_total comes from the host, for bounds: a slot outside [0, G_total)
 *                writes nothing.  A lane loads 16 labels once, looks their targets up in a per-image table in LDS and stores,
 *                for every target of its image, 16 bytes of 0 / 1: masks uint8 (G_total, H, W) contiguous is written in full
 *                lines, every byte exactly once (the caller need not clear it).  With H * W no multiple of 16 the planes
 *                start at odd addresses and the bytes are stored one by one.  Also written: image_of int32 (G_total,) and
 *                the compact labels int64 (G_total,).
 *   limits     N, H, W >= 0 and < 2^31, an image of fewer than 2^31 pixels, N <= 4096 (VAH_E_SHAPE).  int64 label maps,
 *              labels and labels_out 8-byte, slot, meta and image_of 4-byte, ws and masks 16-byte aligned (VAH_E_ALIGN); uint8
 *              label maps may have any alignment and any row stride >= W.  0 <= G_total <= 256 * N (VAH_E_SHAPE).  Empty:
 *              N * H * W == 0, for vah_segtgt_masks also G_total == 0 (sizes and the dtype code are still checked).
 *
 * vah_segtgt_ws_bytes  bytes of workspace for vah_segtgt_scan (0 for an empty or impossible problem): 64 bytes for each of
 *                      at most 256 workgroups per image, of at least 4096 pixels each.
 * vah_segtgt_scan      launches one and two.  ws_bytes below vah_segtgt_ws_bytes: VAH_E_SHAPE.
 * vah_segtgt_masks     launch three; slot, labels and meta are what vah_segtgt_scan wrote for the same label map and remap.
 */
#ifndef VITADAPTER_HIP_SEG_TARGET_H
#define VITADAPTER_HIP_SEG_TARGET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t vah_segtgt_ws_bytes(int64_t N, int64_t H, int64_t W);
int vah_segtgt_scan(const void *label, int label_dtype, int64_t label_img_stride, int64_t label_row_stride, int64_t N, int64_t H,
                    int64_t W, int64_t ignore_index, const void *remap, void *labels, void *slot, void *meta, void *ws,
                    int64_t ws_bytes, void *stream);
int vah_segtgt_masks(const void *label, int label_dtype, int64_t label_img_stride, int64_t label_row_stride, int64_t N, int64_t H,
                     int64_t W, const void *remap, const void *slot, const void *labels, const void *meta, int64_t G_total,
                     void *masks, void *image_of, void *labels_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_SEG_TARGET_H */
