/* gp_meanshift.h -- flat-kernel mean-shift clustering of per-point features on the device: the C entry points of
 * csrc/meanshift_kernels.hip, a part of libgp_hip.so with an ABI number of its own.  (The header lives beside the sources, not in
 * include/: see DESIGN sections 22 and 23.)
 *
 * What it replaces: the MeanShift branch of cluster() of [REF utils/visualizer_utils.py:35-44] -- sklearn's MeanShift() on the host,
 * which seeds every point and is O(N^2) per iteration -- and sklearn's estimate_bandwidth that it calls.
 *
 * THE DEFINITION.  X: float32 [N][D], row-major and contiguous; seeds: float32 [S][D] (X itself by default).  Refused, with a message
 * that names the argument: anything outside 1 <= D <= 64 (the bound of gp_kmeans_assign, which labels the rows), 1 <= N, S < 2^31,
 * N*D and S*D < 2^31, 0 <= max_iter <= 10000, 0 < quantile <= 1, bandwidth finite and > 0 (a bandwidth is read on the device: a bad
 * one sets status word GP_MEANSHIFT_ST_BAD_BANDWIDTH and nothing else is computed), and more than 4096 kept centres (status word
 * GP_MEANSHIFT_ST_OVERFLOW).
 *  Distance.  d(a, b) = sqrtf(sum_j (a_j - b_j)^2) in float32, j ascending from 0; the subtraction, the multiplication and the addition
 *     each rounded once (no contraction: the file is compiled with -ffp-contract=off); square root and division are the correctly
 *     rounded ones.  A point is WITHIN a radius when d <= (float)bandwidth.  The kernels compare the squared sum against t, the largest
 *     float32 with sqrtf(t) <= (float)bandwidth: sqrtf is monotone, so the result is the same.
 *  Bandwidth (sklearn's estimate_bandwidth).  k = max(1, (int)(N * quantile)).  For every row i the k-th smallest of
 *     d(x_i, x_0 .. x_{N-1}), self included, in float32 order: exact, a radix select over the bits of the row's squared distances, four
 *     8-bit passes, the distances recomputed each pass; nothing of size N^2 is stored.  bandwidth = (those N values added in float64
 *     in ascending i) / N, a float64 written to the device.
 *  Shift.  Every seed starts with m = the seed, it = 0, unfinished.  One step, for every unfinished seed: the members are the rows of X
 *     within the radius of m, n of them.  n = 0: count = 0 and the seed is finished (it is dropped by the merge).  Otherwise
 *     m_new_j = (float)((sum over the members of (double)x_ij, ascending i) / n); shift = sqrt(sum_j ((double)m_new_j - (double)m_j)^2)
 *     in float64, j ascending; m = m_new, count = n; the seed is finished when shift <= 1e-3 * bandwidth (in float64) or it == max_iter,
 *     otherwise it += 1.  This is sklearn's _mean_shift_single_seed with its off-by-one: max_iter = 0 still moves every seed once.
 *     n_iter is the largest `it` over the seeds.  A seed's result depends on nothing but the seed, X and the bandwidth.
 *  Merge.  Seeds with count 0 are dropped.  Precedence: count descending, then the centre as a tuple compared lexicographically, larger
 *     first (the reference's sorted(..., key=(count, centre), reverse=True)); seeds equal in both are taken in ascending index.
 *     Walking in that order, a centre is kept unless a kept centre that precedes it is within the radius.  The kept centres, in
 *     precedence order, are the cluster centres.  sklearn keys a dict by the centre first, which drops exact duplicates; a duplicate
 *     is at distance 0 of its twin, so whether it is dropped first does not change the kept coordinates.
 *  Labels are not an entry here: gp_kmeans_assign over the kept centres (nearest in squared float32 distance, ties to the lower index).
 *  Non-finite input: every entry terminates, the results are unspecified, nothing outside the arrays is touched.
 *
 * Launches.  gp_meanshift_bandwidth: four select passes and one sum.  gp_meanshift_run: one launch does ONE step for all unfinished
 *     seeds (a workgroup whose seeds are all finished returns at once); the entry issues max_iter + 1 of them in stream order and never
 *     reads the device.  gp_meanshift_merge: two launches per round of pick-and-suppress (the first live centre in precedence order by a
 *     two-level reduction of the comparator, kept; every live centre within its radius killed); the caller asks for `rounds` rounds per
 *     call and may read status word GP_MEANSHIFT_ST_LIVE between calls: 0 means that no live centre is left.
 *
 * Conventions are those of gp_hip.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), every argument validated before
 * any launch, a gp_stream_t last.  No entry synchronises or reads the device; every array is on the device.  No kernel uses a
 * floating-point atomic: two calls with equal inputs give equal bytes. */
#ifndef GP_MEANSHIFT_H
#define GP_MEANSHIFT_H

#include "../../include/gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_MEANSHIFT_ABI_VERSION 1

#define GP_MEANSHIFT_MAX_D 64
#define GP_MEANSHIFT_MAX_CENTRES 4096
#define GP_MEANSHIFT_MAX_ITER 10000

/* the status block: int32 words on the device */
#define GP_MEANSHIFT_STATUS_WORDS 8
#define GP_MEANSHIFT_ST_UNFINISHED 0      /* seeds not yet finished (run) */
#define GP_MEANSHIFT_ST_KEPT 1            /* K, the kept centres (merge) */
#define GP_MEANSHIFT_ST_EMPTY 2           /* seeds with count 0 (run) */
#define GP_MEANSHIFT_ST_OVERFLOW 3        /* 1: a centre beyond the 4096th would have been kept (merge) */
#define GP_MEANSHIFT_ST_N_ITER 4          /* the largest `it` (run) */
#define GP_MEANSHIFT_ST_BAD_BANDWIDTH 5   /* 1: the bandwidth read on the device is not finite and > 0 (run, merge) */
#define GP_MEANSHIFT_ST_LIVE 6            /* 1: the last merge round issued found a live centre */

int gp_meanshift_abi_version(void);

/* Bytes of scratch that any entry needs for these sizes; -1: refused. */
int64_t gp_meanshift_scratch_size(int64_t N, int64_t S, int64_t D);

/* bandwidth [1] float64, written.  kth [N] float32 or NULL: every row's k-th smallest distance.  scratch: 256-byte aligned. */
int gp_meanshift_bandwidth(const float* X, int64_t N, int64_t D, double quantile, double* bandwidth, float* kth, void* scratch,
                           int64_t scratch_bytes, gp_stream_t stream);

/* Shift.  seed_centers [S][D] float32, seed_counts [S], seed_iterations [S], status [GP_MEANSHIFT_STATUS_WORDS]: written (the status
 * block is reset here).  bandwidth [1] float64. */
int gp_meanshift_run(const float* X, int64_t N, int64_t D, const float* seeds, int64_t S, const double* bandwidth, int32_t max_iter,
                     float* seed_centers, int32_t* seed_counts, int32_t* seed_iterations, int32_t* status, void* scratch,
                     int64_t scratch_bytes, gp_stream_t stream);

/* Merge.  first != 0 starts the walk (K = 0, every seed with count > 0 live) before `rounds` rounds (1 .. 4096) are issued; first == 0
 * continues with the same scratch.  centres [GP_MEANSHIFT_MAX_CENTRES][D] and counts [GP_MEANSHIFT_MAX_CENTRES]: rows 0 .. K - 1 are
 * written; K is status[GP_MEANSHIFT_ST_KEPT]. */
int gp_meanshift_merge(const float* seed_centers, const int32_t* seed_counts, int64_t S, int64_t D, const double* bandwidth, int32_t first,
                       int32_t rounds, float* centres, int32_t* counts, int32_t* status, void* scratch, int64_t scratch_bytes,
                       gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
