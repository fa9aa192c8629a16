/* gp_pca.h -- PCA colouring of per-point features on the device, and a jet colour map: the C entry points of csrc/pca_kernels.hip, a
 * part of libgp_hip.so with an ABI number of its own.  (The header lives beside the sources, not in include/: see DESIGN section 22.)
 *
 * What it replaces: PCA_vis, draw_weights and draw_motion_feature of [REF utils/visualizer_utils.py:46-82, 95-102] -- sklearn's PCA,
 * np.percentile over 3*N values and matplotlib's jet on the host, after a copy of the features off the device.
 *
 * THE DEFINITION.  X: float32 [N][D], row-major and contiguous; dim components.  Refused: anything outside N >= 2, 1 <= D <= 128,
 * 1 <= dim <= min(8, D, N), N*dim < 2^31.  Rows are dealt in CHUNKS of GP_PCA_CHUNK_ROWS = 1024 rows (the last one shorter);
 * parts = min(chunks, 256) workers, worker b taking chunks b, b + parts, ... in ascending order.
 *  1. Mean.  Every worker adds its rows per column in float64, in a fixed order; mean_j = (the workers' sums added in float64 in
 *     ascending b) / N, kept in float64 for step 2 and rounded to float32 once for the output.
 *  2. Covariance.  d_ij = (float)((double)x_ij - mean_j): the difference against the float64 mean, rounded to float32 once.  Every
 *     worker adds the products d_ij * d_ik -- exact in float64 -- in float64 in ascending row order; C_jk = (the workers' sums added in
 *     ascending b) / (N - 1).  C is symmetric bit for bit.  There is no floating-point atomic anywhere.
 *  3. Eigenvectors.  Cyclic Jacobi on C in float64, one workgroup: sweeps of D - 1 (D odd: D) steps of disjoint rotations in
 *     round-robin order, a rotation applied where |c_pq| > 1e-14 * ||C||_F / D, until a sweep applies none or 30 sweeps have run -- so
 *     non-finite input terminates; the results are then unspecified and nothing outside the arrays is touched.  On finite input
 *     ||C v - lambda v||_2 <= 1e-12 * ||C||_F for every returned pair.
 *  4. Order and sign.  Eigenvalues descending (equal ones: the lower column of the iteration first); each component times +-1 so that
 *     its entry of largest magnitude is positive, the first such entry on a tie, decided on the float64 vector -- what sklearn 1.7's
 *     PCA does (svd_flip decided on the components).  components [dim][D] and explained_variance [dim] are float32, each rounded from
 *     float64 once.
 *  5. Projection.  y_ik = sum_j (x_ij - mean_j) * c_kj in float32 with the float32 mean, j ascending from y = 0, the subtraction, the
 *     multiplication and the addition each rounded once (no contraction).
 *  6. Percentiles, over all M = N*dim values of Y together (the reference's np.percentile(transformed, [1, 99]) on the whole array):
 *     pos = q / 100 * (M - 1) in float64, lo = floor(pos), hi = ceil(pos), value = (float)(v_lo + (v_hi - v_lo) * (pos - lo)) in
 *     float64, v_k the k-th smallest value in float32 total order (-0 below +0; a NaN sorts by its bits, which is NOT numpy's order:
 *     unpinned).  v_k is exact: a radix select over the value bits, four 8-bit passes, up to four ranks at once.
 *  7. Colours.  vis = (y - q1) / (q99 - q1) in float32; q99 == q1 gives the IEEE result (inf or NaN), as in the reference: there is no
 *     special case.  dim == 3: colours clip(vis, 0, 1).  dim == 5 (the reference fits [xyz, features], D = 3 + feature_dim): positions
 *     (vis_0, vis_1, 1) unclipped, colours clip(vis_2 .. vis_4, 0, 1).  clip leaves a NaN a NaN.
 *  8. Colour map.  lut: [256][3] float32.  x -> row (int)(x * 256) for 0 <= x < 1, row 255 for x >= 1, row 0 for x < 0, (0, 0, 0) for
 *     a NaN.
 *
 * Conventions are those of gp_hip.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a gp_stream_t last.  No entry
 * synchronises or reads the device; every array is on the device unless it says HOST.  Two calls with equal inputs give equal bytes. */
#ifndef GP_PCA_H
#define GP_PCA_H

#include "../../include/gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_PCA_ABI_VERSION 1

#define GP_PCA_MAX_D 128
#define GP_PCA_MAX_DIM 8
#define GP_PCA_MAX_Q 2            /* percentiles per call: two ranks each, four tracked at once */
#define GP_PCA_CHUNK_ROWS 1024

int gp_pca_abi_version(void);

/* Bytes of scratch that gp_pca_fit needs for [N][D], and that gp_pca_percentiles needs for any M; -1: refused (N < 2 or D outside 1 .. 128). */
int64_t gp_pca_scratch_size(int64_t N, int64_t D);

/* Steps 1 to 4.  mean [D], components [dim][D], explained_variance [dim]: float32, written.  scratch: 256-byte aligned. */
int gp_pca_fit(const float* X, int64_t N, int64_t D, int32_t dim, float* mean, float* components, float* explained_variance, void* scratch,
               int64_t scratch_bytes, gp_stream_t stream);

/* Step 5 with any mean and components (a frozen basis): Y [N][dim].  N >= 1 here; the other bounds are those of the fit. */
int gp_pca_project(const float* X, int64_t N, int64_t D, const float* mean, const float* components, int32_t dim, float* Y, gp_stream_t stream);

/* Step 6.  qs: nq percentiles in 0 .. 100, on the HOST, nq 1 or 2; 1 <= M < 2^31.  out [nq]: the percentiles.  selected [nq][2], or
 * NULL: the order statistics v_lo and v_hi each was interpolated from. */
int gp_pca_percentiles(const float* values, int64_t M, const double* qs, int32_t nq, float* out, float* selected, void* scratch,
                       int64_t scratch_bytes, gp_stream_t stream);

/* Step 7.  q: {q1, q99}.  colors [N][3]; positions [N][3] for dim == 5, or NULL (dim == 3 writes none).  Refused: dim not 3 or 5. */
int gp_pca_colorize(const float* Y, int64_t N, int32_t dim, const float* q, float* positions, float* colors, gp_stream_t stream);

/* Step 8.  out [n][3].  n == 0 launches nothing. */
int gp_colormap_lut(const float* values, int64_t n, const float* lut, float* out, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
