/* gp_mesh_simplify.h -- simplification of a triangle mesh on the device: welding of bit-equal vertices and vertex clustering on a
 * grid.  The C entry points of csrc/mesh_simplify_kernels.hip, a part of libgp_hip.so with an ABI number of its own.  (The header
 * lives beside the sources, not in include/, like gp_mesh.h: see DESIGN section 28.)
 *
 * What it adds: gp_tsdf.h's extraction puts the crossing vertices of several lattice edges on one grid point where a sample equals
 * iso, and keeps the zero-area triangles this gives; gp_mesh.h cleans the mesh and leaves its weight as it is.  Here the vertices
 * are clustered, every cluster is contracted to one vertex, the faces are carried over, and what collapsed or doubled is dropped,
 * all in a stated order: two runs give equal bytes.
 *
 * A mesh: vertices [nv][3] float32, faces [nf][3] int32, on the device.  Refused: nv >= 2^31; 3*nf >= 2^31.  nv = 0 and nf = 0
 * are accepted.  Any [nv][k] float32 array (colours, attributes), 1 <= k <= 1024, follows the vertices through
 * gp_mesh_simplify_rows.
 *
 * 1. The cluster key of a vertex: three 32-bit words.  Two vertices are in one cluster iff their keys are equal.
 *      GP_MESH_SIMPLIFY_WELD   the three words of the position, the word of -0.0 replaced by that of +0.0.  NaNs of equal bits
 *                              weld; NaNs of different bits do not.
 *      GP_MESH_SIMPLIFY_GRID   all in float64: origin_a = min_a - voxel_size / 2, idx_a = (int32)floor((double(p_a) - origin_a) /
 *                              voxel_size) -- that subtraction and that IEEE division, no reciprocal (gp_voxel.h's rule) --
 *                              dims_a = floor((max_a + voxel_size / 2 - origin_a) / voxel_size) + 1.  min and max: bounds[0 .. 3)
 *                              and bounds[3 .. 6), a HOST array: the exact bounds of the vertices as gp_mesh_simplify_bounds
 *                              leaves them, or whatever box the caller chooses.  Refused: a voxel_size that is not finite or
 *                              <= 0; bounds that are not finite or have min > max; any dims_a > 2^21 ("voxel_size is too small").
 *                              A vertex whose index leaves [0, dims_a) -- a coordinate that is not finite among them: the
 *                              comparison is made in float64 and such a value never reaches a conversion to an integer --
 *                              raises the status word and takes index 0.  The sort runs on the bits dims_a - 1 needs.
 *    gp_mesh_simplify_bounds leaves record[8] float64 on the device: min xyz, max xyz over the finite coordinates (as float64 of
 *    the float32 values, a zero always +0.0), then != 0 iff some coordinate is not finite, then 0.  Partial results per workgroup,
 *    one workgroup folds them: no float atomics (and min and max do not depend on the order).
 *
 * 2. Numbering.  Clusters are numbered 0 .. C-1 in ascending order of their SMALLEST member (old vertex index), not in key order:
 *    the mesh keeps its memory order, the result does not depend on how the sort orders unequal keys, and a mesh with nothing to
 *    merge comes back unchanged.  Mechanism: a stable radix sort of (key, vertex) pairs, a word at a time; the head of every run
 *    of equal keys is the run's smallest vertex and is flagged at that vertex; an ordered compaction (gp_mesh.h's: tile sums,
 *    ONE workgroup scans the tiles, ballot ranks) over the vertices numbers the heads.  The members of a cluster are its run, in
 *    ascending old index.
 *
 * 3. Contraction, per column of the positions and of any rows:
 *      GP_MESH_SIMPLIFY_AVERAGE   the float64 sum of double(row) over the members, one after the other in ascending old index from
 *                                 +0.0, divided by double(count), rounded to float32 once
 *      GP_MESH_SIMPLIFY_FIRST     the smallest member's row, bits unchanged
 *    Weld mode is always FIRST.  One lane walks one cluster's members: a cluster of 5000 members is 5000 dependent additions on
 *    one lane, correct and as slow as that sounds.
 *
 * 4. Faces.  A face with an index outside [0, nv) is skipped and raises the status word (mesh_core.h's ms_face).  g =
 *    cluster[face].  In this order:
 *      COLLAPSED   two of g are equal: always dropped
 *      ZERO-AREA   (drop_zero_area) the three components of (b - a) x (c - a) of the CONTRACTED positions (ms_face_vector, float32,
 *                  no contraction) all compare equal to 0: dropped.  A NaN component is not zero: that face stays.
 *      DUPLICATE   (drop_duplicates) g rotated so that its smallest index comes first; among the faces that survived so far with
 *                  equal rotated triples all but the one of the smallest old face index are dropped (a stable sort of the triples).
 *                  The oppositely wound triple is another face and stays.
 *    Kept faces stay in ascending old index, in their corner order, renumbered.
 *
 * 5. Unreferenced clusters.  Unless keep_unreferenced, a cluster stays iff a kept face names it (plain byte stores of 1).  The
 *    final vertices are the kept clusters in ascending cluster number; vertex_map[v] = -1 for the members of a dropped cluster.
 *
 * gp_mesh_simplify_plan leaves counts[GP_MESH_SIMPLIFY_COUNT_WORDS] int32 on the device: status, vertices kept, faces kept,
 * clusters, collapsed, zero-area, duplicates, 0 (integer atomicAdd, one per wave).  The caller reads them, allocates, and calls
 * gp_mesh_simplify_apply and gp_mesh_simplify_rows, which read what the plan left in the scratch (the same stream, vertices,
 * faces and scratch).  The scratch of every entry: gp_mesh_simplify_scratch_bytes(nv, nf) bytes, 256-byte aligned.  Conventions
 * are those of gp_hip.h and gp_mesh.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a gp_stream_t last.  No
 * entry synchronises or reads the device.  Refused everywhere, before any pointer is looked at: the sizes above, a null or
 * unaligned (8 bytes) scratch, a null array that the sizes make non-empty. */
#ifndef GP_MESH_SIMPLIFY_H
#define GP_MESH_SIMPLIFY_H

#include "../../include/gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_MESH_SIMPLIFY_ABI_VERSION 1

#define GP_MESH_SIMPLIFY_WELD 0              /* mode */
#define GP_MESH_SIMPLIFY_GRID 1
#define GP_MESH_SIMPLIFY_FIRST 0             /* contraction */
#define GP_MESH_SIMPLIFY_AVERAGE 1
#define GP_MESH_SIMPLIFY_MAX_DIM 2097152     /* 2^21: the cells of an axis at the most */

#define GP_MESH_SIMPLIFY_STATUS 0            /* counts[]: != 0 iff a face index or a cell index was out of range */
#define GP_MESH_SIMPLIFY_VERTICES 1          /*           nv', the vertices kept */
#define GP_MESH_SIMPLIFY_FACES 2             /*           nf', the faces kept */
#define GP_MESH_SIMPLIFY_CLUSTERS 3          /*           C */
#define GP_MESH_SIMPLIFY_COLLAPSED 4         /*           faces dropped because two of their clusters are equal */
#define GP_MESH_SIMPLIFY_ZERO_AREA 5         /*           faces dropped for a zero face vector */
#define GP_MESH_SIMPLIFY_DUPLICATES 6        /*           faces dropped as copies of an earlier face */
#define GP_MESH_SIMPLIFY_COUNT_WORDS 8
#define GP_MESH_SIMPLIFY_RECORD_WORDS 8      /* float64: min xyz, max xyz, not-finite flag, 0 */

int gp_mesh_simplify_abi_version(void);

/* The bytes of the scratch.  -1 (and gp_last_error()) where the sizes are refused. */
int64_t gp_mesh_simplify_scratch_bytes(int64_t nv, int64_t nf);

/* Grid mode without bounds of the caller's.  nv >= 1.  record: [GP_MESH_SIMPLIFY_RECORD_WORDS] float64 on the device. */
int gp_mesh_simplify_bounds(const float* vertices, int64_t nv, void* scratch, double* record, gp_stream_t stream);

/* bounds: [6] float64 on the HOST, read in grid mode only (may be null in weld mode, where voxel_size and contraction are not
 * looked at either); counts: [GP_MESH_SIMPLIFY_COUNT_WORDS] int32 on the device. */
int gp_mesh_simplify_plan(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, int32_t mode, double voxel_size, const double* bounds,
                          int32_t contraction, int32_t drop_zero_area, int32_t drop_duplicates, int32_t keep_unreferenced, void* scratch, int32_t* counts,
                          gp_stream_t stream);

/* After gp_mesh_simplify_plan.  vertices_out: [nv'][3]; faces_out: [nf'][3]; vertex_map: [nv]; face_index: [nf'] (the old ids);
 * vertex_counts: [nv'] (the members of every kept vertex). */
int gp_mesh_simplify_apply(const int32_t* faces, int64_t nv, int64_t nf, const void* scratch, float* vertices_out, int32_t* faces_out, int32_t* vertex_map,
                           int32_t* face_index, int32_t* vertex_counts, gp_stream_t stream);

/* After gp_mesh_simplify_plan.  dst[new v][0 .. k) = the contraction of src[member][0 .. k) over the members of every kept vertex:
 * src [nv][k], dst [nv'][k] float32, 1 <= k <= 1024, nv*k below 2^31. */
int gp_mesh_simplify_rows(const float* src, int64_t nv, int64_t nf, int32_t k, int32_t contraction, const void* scratch, float* dst, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
