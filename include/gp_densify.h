/* gp_densify.h -- densify (clone + split), opacity reset and prune of the per-Gaussian tensors on the device: the C entry points of
 * csrc/densify_kernels.hip, a part of libgp_hip.so with an ABI number of its own.
 *
 * Conventions are those of gp_hip.h: plain device pointers and sizes, a return code != 0 (or -1 from the int64_t query) plus
 * gp_last_error(), no synchronisation, a gp_stream_t last.  No entry reads the device; no kernel uses an atomic: two calls on equal
 * inputs give the same bits.
 *
 * What they replace [REF train.py:164-177, scene/gaussian_model.py:526-760]:
 *   gp_densify_stats    max_radii2D update + add_densification_stats of one view                        [REF train.py:166-167, :755-760]
 *   gp_densify_plan     every selection of densify_and_clone, densify_and_split, reset_opacity, prune   [REF :663-718, :745-753]
 *   gp_densify_apply    cat_tensors_to_optimizer / _prune_optimizer / replace_tensor_to_optimizer       [REF :547-661]
 *
 * The plan decides, from the state BEFORE any of the three operations, what "densify -> reset_opacity -> prune" leaves.  Output row order:
 *   segment 0   the original rows that are neither split sources nor pruned, in order
 *   segment 1   the clones that survive the prune, in source order
 *   segment 2   the first split copies that survive
 *   segment 3   the second split copies that survive
 * The prune tests of a new row run on the values that row would have: the source's opacity (after the reset, if any), the shrunk
 * scaling of a split copy, and max_radii2D = 0 after a densify (the live value when GP_DENSIFY_DENSIFY is not set). */
#ifndef GP_DENSIFY_H
#define GP_DENSIFY_H

#include "gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_DENSIFY_ABI_VERSION 1

#define GP_DENSIFY_BLOCK 256       /* rows per workgroup of the plan and the apply */
#define GP_DENSIFY_MAX_TENSORS 8
#define GP_DENSIFY_MAX_ROWS 1073741824 /* 2^30: 2 N output rows stay inside 32 bits */

/* flags */
#define GP_DENSIFY_DENSIFY 1u /* clone + split */
#define GP_DENSIFY_RESET 2u   /* opacity <- logit(min(sigmoid(opacity), 0.01)), its moments zero */
#define GP_DENSIFY_PRUNE 4u
#define GP_DENSIFY_SCREEN 8u  /* max_screen_size is given: the screen-size AND the world-size test run [REF :748-751] */

/* the status block (uint32 words on the device) */
#define GP_DENSIFY_STATUS_WORDS 8
#define GP_DENSIFY_ST_CLONED 0  /* rows selected for cloning */
#define GP_DENSIFY_ST_SPLIT 1   /* split sources */
#define GP_DENSIFY_ST_PRUNED 2  /* rows the prune removes, counted as prune() counts them (new rows included, split sources not) */
#define GP_DENSIFY_ST_ROWS 3    /* output rows */
#define GP_DENSIFY_ST_BASE 4    /* .. 7: first output row of segments 0 .. 3 */

/* what a table entry is to the apply */
#define GP_DENSIFY_ROLE_NONE 0
#define GP_DENSIFY_ROLE_XYZ 1      /* width 3; split copies: R(normalize(rotation)) (exp(scaling) * z) + xyz */
#define GP_DENSIFY_ROLE_SCALING 2  /* width 3; split copies: log(exp(scaling) / 1.6) */
#define GP_DENSIFY_ROLE_ROTATION 3 /* width 4 */
#define GP_DENSIFY_ROLE_OPACITY 4  /* width 1 */

/* One per-Gaussian tensor, [N][width] floats in, [rows][width] out.  The moment pointers are all NULL or all set. */
typedef struct gp_densify_tensor {
    const float* in;
    const float* in_exp_avg;
    const float* in_exp_avg_sq;
    float* out;
    float* out_exp_avg;
    float* out_exp_avg_sq;
    int32_t width;
    int32_t role;
} gp_densify_tensor;

int gp_densify_abi_version(void);

/* One launch over N rows.  Rows with visible[i] != 0:  max_radii2D = max(max_radii2D, (float)radii),  s = sqrt(gx^2 + gy^2) of
 * grad [N][3],  accum += s,  denom += 1,  accum_max = s > accum_max ? s : accum_max  (a NaN never replaces a number).  Other rows
 * are not written. */
int gp_densify_stats(int64_t N, const uint8_t* visible, const int32_t* radii, const float* grad, float* max_radii2D, float* accum,
                     float* denom, float* accum_max, gp_stream_t stream);

/* Bytes of `scratch` for N rows (keep bytes + per-block class counts); -1 for N outside [1, GP_DENSIFY_MAX_ROWS]. */
int64_t gp_densify_scratch_bytes(int64_t N);

/* scaling [N][3] and opacity [N] are the raw parameters.  grad_threshold <= 0 (or NaN) is refused: the split pass relies on the
 * zero gradient of the cloned rows failing `>= grad_threshold`.  dense_extent = percent_dense * extent, world_extent = 0.1 * extent.
 * Writes scratch (256-byte aligned, gp_densify_scratch_bytes) and status[GP_DENSIFY_STATUS_WORDS].  Two launches. */
int gp_densify_plan(int64_t N, const float* accum, const float* denom, const float* max_radii2D, const float* scaling, const float* opacity,
                    float grad_threshold, float dense_extent, float min_opacity, float max_screen_size, float world_extent, uint32_t flags,
                    void* scratch, uint32_t* status, gp_stream_t stream);

/* One launch that writes every output tensor from the plan in `scratch` / `status` (both read on the device).  `tensors`: a HOST array
 * of num_tensors <= GP_DENSIFY_MAX_TENSORS entries; with GP_DENSIFY_DENSIFY it must hold the XYZ, SCALING and ROTATION roles, with
 * GP_DENSIFY_RESET the OPACITY role.  normals [2][N][3]: the split draws, read at split sources only (NULL without
 * GP_DENSIFY_DENSIFY).  stats_in / stats_out: HOST arrays of four device pointers (accum, denom, accum_max, max_radii2D), [N] in and
 * [out_rows] out: zero for every output row with GP_DENSIFY_DENSIFY, else compacted.  out_rows: the rows every output holds; rows the
 * plan places at or beyond it are not written (status[GP_DENSIFY_ST_ROWS] <= 2 N always). */
int gp_densify_apply(int64_t N, int32_t num_tensors, const gp_densify_tensor* tensors, const float* normals, const float* const* stats_in,
                     float* const* stats_out, int64_t out_rows, uint32_t flags, const void* scratch, const uint32_t* status,
                     gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
