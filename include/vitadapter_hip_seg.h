/*
 * vitadapter_hip_seg.h -- C ABI of libvitadapter_hip.so, seventh part: the logit tail of the Mask2Former segmentor
 * (csrc/seg_logits.hip).  Conventions, error codes and the ABI version are those of vitadapter_hip.h (adding symbols does not
 * move the version): argument checks come before any device work, strides are in ELEMENTS, an empty problem returns VAH_OK
 * and reads no pointer.
 *
 * Replaces, in the reference's segmentation/mmseg_custom/models/segmentors/encoder_decoder_mask2former[_aug].py, everything
 * between decode_head.forward_test and the label map: resize(out, size=img.shape[2:]) and preds += F.pad(...) of
 * encode_decode / slide_inference (:75-79, :181-183), preds / count_mat, the un-padding of the Aug class, the resize to
 * ori_shape, F.softmax(dim=1), the flip, the sum over the views of aug_test and argmax(dim=1) (:191-285).
 *
 *   layout     fp32 NCHW planes: element [n][c][y][x] sits at n * img_stride + c * plane_stride + y * row_stride + x (column
 *              stride 1), so a call addresses a window of `preds`, or its un-padded corner, in place.  labels are int64,
 *              [n][y][x] at n * img_stride + y * row_stride + x.  For every tensor row_stride >= width,
 *              plane_stride >= (height - 1) * row_stride + width and img_stride >= (C - 1) * plane_stride + that (labels:
 *              img_stride >= the plane extent): planes never overlap.  VAH_E_SHAPE otherwise.
 *   resize     R is torch's upsample_bilinear2d for size=, by exactly the tap rule of vitadapter_hip_resize.h (indices and
 *              fractions from un-contracted fp32 operations, one function shared with csrc/resize_rows.hip), and
 *                y = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11)
 *              with every product and sum rounded on its own and all four products always taken: a zero weight times inf
 *              is NaN, as in torch.
 *   order      no atomics, counters or flags, nothing read back to the host.  One thread owns every output element of a
 *              call, so the same inputs give the same bits and the calls capture into a graph.
 *   limits     sizes >= 0 and < 2^31, N <= 65535, a plane of fewer than 2^31 pixels (VAH_E_SHAPE); an empty source for a
 *              non-empty result is VAH_E_SHAPE.  fp32 and int32 pointers 4-byte, labels 8-byte aligned (VAH_E_ALIGN).
 *
 * vah_seg_resize_add  dst[n][c][y0 + oy][x0 + ox] (= | +=) R(src[n][c])[oy][ox] for oy < Hc, ox < Wc, with R from (hs, ws) to
 *                     (Hc, Wc); accumulate == 0 stores, != 0 adds to what dst holds.  dst is (N, C, Hd, Wd); a window that
 *                     leaves it (y0 < 0, x0 < 0, y0 + Hc > Hd, x0 + Wc > Wd) is VAH_E_SHAPE.  Elements of dst outside the
 *                     window are neither read nor written.  Neither the upsampled nor the padded tensor of the reference is
 *                     formed.  Empty: N * C * Hc * Wc == 0.  A thread owns a pixel of the window for a run of classes (the
 *                     taps are computed once); stores are dwords, the window's offset and width being arbitrary.
 *                     Profile row seg_resize_add.
 * vah_seg_finish      the rest of one view in one launch.  For each output pixel (oy, ox) of (Ho, Wo), over the C classes:
 *                       t[c][y][x] = acc[n][c][y][x] / (float)(cy[y] * cx[x])   a true fp32 division; cy (Hs) and cx (Ws)
 *                                    int32 vectors (the windows are a grid product, so count_mat is cy x cx); both NULL:
 *                                    count 1, no division (whole mode); one NULL: VAH_E_NULL
 *                       v[c]       = t[c][oy][ox] (resize == 0, which needs Ho == Hs and Wo == Ws: VAH_E_SHAPE) or
 *                                    R(t[c])[oy][ox] from the read region (Hs, Ws) - the corner of acc, smaller than its
 *                                    buffer for the Aug class - to (Ho, Wo): divide, then resize, as in the reference
 *                       p[c]       = exp(v[c] - max v) / sum_c exp(v[c] - max v), fp32 with the accurate expf; as in torch, a NaN
 *                                    or +inf logit makes the whole pixel NaN, -inf gives 0, all -inf gives NaN
 *                     The output position is (oy, ox) (flip 0), (oy, Wo - 1 - ox) (flip 1, horizontal) or (Ho - 1 - oy, ox)
 *                     (flip 2, vertical); any other flip is VAH_E_SHAPE.  Outputs, each of which may be NULL (both NULL:
 *                     VAH_E_NULL):
 *                       prob[n][c][.][.] (= | +=) p[c]    by `accumulate`: the output of `inference`, or the sum of aug_test
 *                       labels[n][.][.] = the first index of the largest p[c]; a NaN counts as largest, as in torch's argmax
 *                     Empty: N * C * Ho * Wo == 0.  A lane owns a pixel and consecutive lanes consecutive x, so every class
 *                     plane is read coalesced; the classes are walked twice (maximum and sum, then p), see DESIGN.md.
 *                     Profile row seg_finish.
 * vah_seg_argmax      labels[n][y][x] = the first index of the largest sum[n][c][y][x] / divisor (a true fp32 division), a
 *                     NaN counting as largest: the last lines of aug_test.  Empty: N * C * H * W == 0.  Profile row seg_argmax.
 */
#ifndef VITADAPTER_HIP_SEG_H
#define VITADAPTER_HIP_SEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int vah_seg_resize_add(const void *src, int64_t src_img_stride, int64_t src_plane_stride, int64_t src_row_stride, int64_t N,
                       int64_t C, int64_t hs, int64_t ws, int64_t Hc, int64_t Wc, int align_corners, void *dst,
                       int64_t dst_img_stride, int64_t dst_plane_stride, int64_t dst_row_stride, int64_t Hd, int64_t Wd,
                       int64_t y0, int64_t x0, int accumulate, void *stream);
int vah_seg_finish(const void *acc, int64_t acc_img_stride, int64_t acc_plane_stride, int64_t acc_row_stride, int64_t N,
                   int64_t C, int64_t Hs, int64_t Ws, const void *cy, const void *cx, int resize, int64_t Ho, int64_t Wo,
                   int align_corners, int flip, void *prob, int64_t prob_img_stride, int64_t prob_plane_stride,
                   int64_t prob_row_stride, int accumulate, void *labels, int64_t labels_img_stride, int64_t labels_row_stride,
                   void *stream);
int vah_seg_argmax(const void *sum, int64_t sum_img_stride, int64_t sum_plane_stride, int64_t sum_row_stride, int64_t N,
                   int64_t C, int64_t H, int64_t W, float divisor, void *labels, int64_t labels_img_stride,
                   int64_t labels_row_stride, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_SEG_H */
