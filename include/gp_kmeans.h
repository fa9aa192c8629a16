/* gp_kmeans.h -- deterministic Lloyd k-means on the device, for the keypoint extraction at second_stage_iter + 1: the C entry points
 * of csrc/kmeans_kernels.hip, a part of libgp_hip.so with an ABI number of its own.
 *
 * Conventions are those of gp_hip.h: plain device pointers and sizes, a return code != 0 (or -1 from the int64_t query) plus
 * gp_last_error(), no synchronisation and no host read inside any entry, a gp_stream_t last.  No kernel uses a float atomic: two
 * calls on equal inputs give the same bits.
 *
 * What they replace [REF utils/visualizer_utils.py:84-93, scene/gaussian_model.py:128-136]: kmeans_pytorch.kmeans and
 * torch_scatter.scatter(reduce="mean").
 *
 * X [N][D] and centres [K][D] are fp32, contiguous, row-major.
 *
 * The distance:  d2(i, k) = sum over d = 0 .. D-1, in that order, of (X[i][d] - centres[k][d])^2, every operation rounded to fp32 (no
 * inner-product expansion, no contraction: the library is built with -ffp-contract=off).  This is gp_knn_points' distance.
 *
 * The summation order of the per-cluster sums (doubles):  the rows are cut into contiguous ranges of R rows, R a multiple of
 * GP_KMEANS_BLOCK fixed by (N, D, K) alone; workgroup b adds the rows of range b, in ascending row order, into a partial sum of its
 * own; the partial sums are added in ascending b.  The sum is divided by the count in double and rounded once to fp32. */
#ifndef GP_KMEANS_H
#define GP_KMEANS_H

#include "gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_KMEANS_ABI_VERSION 1

#define GP_KMEANS_BLOCK 256       /* rows per batch of a workgroup */
#define GP_KMEANS_MAX_D 64        /* gp_knn_points' limit */
#define GP_KMEANS_MAX_K 4096
#define GP_KMEANS_MAX_ROWS 2147483647 /* N < 2^31 */
#define GP_KMEANS_MAX_ITERS 1000

/* the status block (uint32 words on the device, 8-byte aligned) */
#define GP_KMEANS_STATUS_WORDS 4
#define GP_KMEANS_ST_ITERATIONS 0 /* Lloyd iterations run */
#define GP_KMEANS_ST_CONVERGED 1  /* 1 once shift^2 <= tol */
#define GP_KMEANS_ST_SHIFT2 2     /* .. 3: the last shift^2, a double */

int gp_kmeans_abi_version(void);

/* Bytes of `scratch` (256-byte aligned) for gp_cluster_mean and gp_kmeans_run; -1 for an argument outside the limits
 * (1 <= N <= GP_KMEANS_MAX_ROWS, 1 <= D <= GP_KMEANS_MAX_D, 1 <= K <= GP_KMEANS_MAX_K). */
int64_t gp_kmeans_scratch_bytes(int64_t N, int32_t D, int32_t K);

/* ids[i] = the k with the smallest d2(i, k); ties go to the lower k; a row whose distances are all NaN gets 0.  d2 (optional):
 * the distance to that centre.  One launch. */
int gp_kmeans_assign(int64_t N, int32_t D, const float* X, int32_t K, const float* centres, int32_t* ids, float* d2, gp_stream_t stream);

/* mean[k] = the mean of the rows with ids[i] == k (zeros for a cluster without rows), counts[k] their number.  An id outside [0, K)
 * is ignored.  Sums in double, in the order stated above.  Two launches. */
int gp_cluster_mean(int64_t N, int32_t D, const float* X, const int32_t* ids, int32_t K, float* mean, int32_t* counts, void* scratch,
                    gp_stream_t stream);

/* Up to max_iters (1 .. GP_KMEANS_MAX_ITERS) Lloyd iterations from `centres` (in: initial, out: final).  One iteration: assign; per-cluster
 * double sums; new centre = mean, or the previous centre for a cluster without rows; shift s = sum over k, in order, of
 * ||new_k - old_k||_2 in double; converged once s^2 <= tol (tol = 0: an exact fixed point only; a NaN never converges).  The flag is
 * a word of `status`: all max_iters iterations are enqueued, and the launches after convergence return at once.  After the loop one
 * more assignment runs against the FINAL centres: ids [N], counts [K] and aux_mean describe the centres returned.
 * aux [N][aux_dim] (optional, 1 <= aux_dim <= D): aux_mean [K][aux_dim] = its per-cluster mean by the final ids, as gp_cluster_mean.
 * status[GP_KMEANS_STATUS_WORDS] is written from its first word on; scratch: gp_kmeans_scratch_bytes(N, D, K). */
int gp_kmeans_run(int64_t N, int32_t D, const float* X, int32_t K, float* centres, int32_t max_iters, double tol, int32_t* ids,
                  int32_t* counts, const float* aux, int32_t aux_dim, float* aux_mean, uint32_t* status, void* scratch, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
