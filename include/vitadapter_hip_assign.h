/*
 * vitadapter_hip_assign.h -- C ABI of libvitadapter_hip.so, thirteenth part: the assignment step of Mask2Former's matching
 * (csrc/assign.hip).  Conventions, error codes and the ABI version are those of vitadapter_hip.h (adding symbols does not
 * move the version): argument checks come before any device work, a zero-size call returns VAH_OK and reads no pointer.
 *
 * Replaces, in the reference's MaskHungarianAssigner (segmentation/mmseg_custom/models/utils/assigner.py:147-160: the cost
 * matrix goes to the host, scipy.optimize.linear_sum_assignment solves it, the two index arrays go back) and its
 * MaskPseudoSampler (segmentation/mmseg_custom/core/box/samplers/mask_pseudo_sampler.py: the positives in query order), the
 * trip to the host per (decoder output, image): every problem of a training step is solved where its costs were written,
 * and the matched pairs are stored in the form the losses index with.
 *
 * vah_assign_solve
 *   cost        (L, N, Q, Gmax) fp32 contiguous: what L calls of vah_pts_match_cost write, stacked.  Columns g >= G_n of
 *               image n are padding and are never read.
 *   gt_offsets  [N + 1] int32 on the device, the array vah_pts_match_cost takes; G_n = gt_offsets[n + 1] - gt_offsets[n].
 *   problem     (i, n) is the rectangular assignment of the Q x G_n block cost[i][n][:, :G_n]: min(Q, G_n) pairs (q, g), no q
 *               and no g twice, of the least total cost.
 *   method      the shortest-augmenting-path method of scipy's linear_sum_assignment (rectangular Jonker-Volgenant, restated
 *               from the published description of rectangular_lsap.cpp): the smaller dimension is the row set, rows are added
 *               one at a time by a Dijkstra search over reduced costs, then the duals are updated and the path is flipped.
 *               Duals and path costs are fp64 over the fp32 costs widened to fp64, with scipy's expressions, so that where the
 *               optimum is unique in fp64 the pairs are scipy's.  A tie for the lowest reduced cost is broken by (an unassigned
 *               column first, then the lowest column index): on ties the result is an optimal assignment, not necessarily
 *               scipy's.
 *   table       (L, 2, K) int64, K = sum_n min(Q, G_n).  The pairs of image n start at base_n = sum_{m < n} min(Q, G_m), in
 *               ascending query order (MaskPseudoSampler's): table[i][0][base_n + k] = n * Q + q, table[i][1][base_n + k] =
 *               gt_offsets[n] + g.  Each workgroup derives base_n and K from gt_offsets itself.
 *   status      (L, N) int32, every element written: 0 solved (also G_n = 0: no pairs); 1 the block holds a NaN or -inf
 *               (scipy: "matrix contains invalid numeric entries"); 2 infeasible (scipy: "cost matrix is infeasible": no
 *               complete assignment over finite entries, for one when a row has only +inf).  With status 1 or 2 the problem's
 *               pairs are the identity pairing (q = k, g = k), k < min(Q, G_n): always in range, so that nothing downstream
 *               forms an address from a bad index.
 *   bad offsets a pair read on the device with G_n < 0 or G_n > Gmax gives status 2, writes no pair and counts as G_n = 0 in
 *               every base and in K; table has to hold the K of the offsets it is called with.
 *   limits      1 <= Q <= 256, 0 <= Gmax <= 256, Q * Gmax <= 32768 (the staged block is at most 128 KiB of the 160 KiB of
 *               LDS a workgroup may take; it is requested as dynamic LDS): VAH_E_UNSUPPORTED otherwise.  0 <= L, 0 <= N <= 4096,
 *               L * N < 2^31 (VAH_E_SHAPE).  cost and status 4-byte, gt_offsets 4-byte, table 8-byte aligned (VAH_E_ALIGN).
 *               Zero size: L * N == 0 or Gmax == 0 (K is then 0): nothing is launched and nothing written, status included.
 *   kernel      one launch (profile row assign_solve), one workgroup of 64 lanes per problem.  The block is staged once into
 *               LDS as fp32 in solver orientation (transposed while staging when Q > G_n, so that a row read is consecutive
 *               words).  Lane l owns columns l, l + 64, l + 128, l + 192 and keeps their shortest-path cost, predecessor,
 *               assigned row, dual and "scanned" bit in registers; the row duals and the rows' columns are in LDS.  A step of
 *               the search is one row read, up to four fp64 candidates per lane, and a 6-level wave reduction of the key
 *               (value, assigned, column).  No atomics, no communication between workgroups, nothing read back: the launch can
 *               be captured in a graph, and the same inputs give the same bits.
 */
#ifndef VITADAPTER_HIP_ASSIGN_H
#define VITADAPTER_HIP_ASSIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int vah_assign_solve(const void *cost, const void *gt_offsets, int64_t L, int64_t N, int64_t Q, int64_t Gmax, void *table,
                     void *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VITADAPTER_HIP_ASSIGN_H */
