/* gp_volume.h -- signed-distance volumes on the device: a bounding-volume tree over the triangles of a mesh that answers
 * gp_surface.h's query anywhere in space, the signed distance of a mesh on the lattice of a TSDF volume, and the counts of a volumetric
 * IoU.  The C entry points of csrc/volume_kernels.hip, a part of libgp_hip.so with an ABI number of its own.  (The header lives beside
 * the sources, not in include/, as gp_surface.h, gp_mesh_smooth.h and gp_sdf.h do: see DESIGN section 34.)
 *
 * What it adds: gp_surface.h's grid pays for every empty ring between a query and the surface, O(r^3) lookups to reach ring r, so a
 * query deep inside or far outside a mesh is slow.  A tree skips empty space a box at a time.
 *
 * The library is built without contraction: every operation below rounds once, in the stated order.
 *
 * 1. THE RESULT is gp_surface.h section 1, unchanged: the lexicographic minimum over the usable faces f of (d_f, f), d_f the float64
 *    distance of that section, with its five outputs (dist2, face, region, closest, bary) and its empty row (+inf, -1, 0, NaN, 0) for a
 *    query with a non-finite coordinate and where no face is usable.  The distance arithmetic is surface_core.h's own functions: the
 *    same operations give the same bytes as gp_surface_grid_query.  Nothing depends on the tree, on the leaf size or on the run.
 *
 * 2. THE TREE (gp_volume_tree).  No result depends on any of this; only the cost does.
 *    A record (gp_surface.h's: nine floats and the face number, -1 where the face is not usable) per face.  lo, hi: the bounds of the
 *    corners of the usable faces (x + 0.f first); M: the largest |coordinate| among them; all by integer atomic minima and maxima of
 *    order-preserving bits.  No float atomics anywhere.
 *    A sort key per face: the 30-bit Morton code (x the lowest bit of every triple) of the cells t_k = min(1023, (int)floor(((c_k -
 *    lo_k) / (hi_k - lo_k)) * 1024.0)) in float64, c_k = 0.5 * (min + max of the three corners) the centre of the face's box, t_k = 0
 *    where hi_k = lo_k; 2^30 for a face that is not usable, so that those sort last.  ONE stable radix sort of (key, face); the records
 *    are copied into sorted order, so that a leaf is contiguous memory.
 *    A leaf holds GP_VOLUME_LEAF consecutive sorted records (the last one fewer).  Level 0 holds the leaves' boxes: the float32 minimum
 *    and maximum of the corners of the leaf's usable records, exact; a leaf without a usable record is marked EMPTY (lo = +inf, hi =
 *    -inf) and so is a union of empty boxes.  Level k box i is the union of level k - 1 boxes 2i and 2i + 1 (the second where it
 *    exists); level k has ceil(n_{k-1} / 2) boxes, the last level one.  One launch a level, bottom-up.  At most GP_VOLUME_MAX_LEVELS = 27 levels (nf < 2^26 with one record a leaf; 26 with two).
 *    Every size is a function of nf alone: the build reads nothing back.
 *
 * 3. THE WALK, a lane per query, with an explicit stack of GP_VOLUME_STACK entries (a pop pushes at most two boxes of the level below:
 *    the stack never holds more than one box per level and one: 28 at the most); no recursion; every loop is bounded by the number of boxes.
 *    The bound of a box for the query q, in float64:
 *        g_k = max(lo_k - q_k, q_k - hi_k, 0) - 2^-47 * M, floored at 0;      lb = (g_x*g_x + g_y*g_y) + g_z*g_z
 *    A box is SKIPPED iff it is empty, or  lb >= 2^-100  and  lb * (1 - 2^-40) > best  (best: the float64 minimum so far), strictly.
 *    The rule is applied when a box is made a candidate and again when it is popped (best has only shrunk).  The children of a box are
 *    pushed farther first: the nearer one is popped first, equal bounds go to the lower index.  A leaf that is not skipped tests all
 *    its records with surface_core.h's sf_test.
 *    Why the rule is exact.  Take a usable face under a skipped box and any candidate p of it with its computed d.
 *    (i)   gp_surface.h section 2 bounds the computed p: |p_k - p*_k| <= 2^-48 * M_k <= 2^-48 * M for a real point p* of the triangle.
 *    (ii)  The triangle lies inside its leaf's box and every box above it, whose bounds are float32 minima and maxima: exact.  So
 *          lo_k <= p*_k <= hi_k and |q_k - p*_k| >= G_k := max(lo_k - q_k, q_k - hi_k, 0) in real numbers.
 *    (iii) lo_k - q_k and q_k - hi_k are differences of two float32 in float64: one rounding, relative 2^-53, and 2^-47 * M is exact (a
 *          power of two times a float32), t for short.  With s_k the computed maximum before t is taken off: s_k <= G_k * (1 + 2^-53)
 *          (and s_k = 0 where G_k = 0), and where g_k > 0:  g_k = fl(s_k - t) <= (s_k - t) * (1 + 2^-53).  From (i) and (ii),
 *          |q_k - p_k| >= G_k - 2^-48 * M >= s_k * (1 - 2^-53) - t / 2 = (s_k - t) + (t / 2 - 2^-53 * s_k).  The bracket is >= 0 where
 *          s_k <= 32 * M; where s_k > 32 * M it is >= -2^-53 * s_k >= -2^-52 * (s_k - t).  Either way
 *          |q_k - p_k| >= (s_k - t) * (1 - 2^-52) >= g_k * (1 - 2^-51): half of the 2^-47 * M pays for (i), the other half for the roundings.
 *    (iv)  d = fl(dot(r, r)), r_k = fl(q_k - p_k): d >= sum (q_k - p_k)^2 * (1 - 2^-53)^5 up to underflow (r_k twice, its square, two
 *          sums); lb <= sum g_k^2 * (1 + 2^-53)^3.  So d >= lb * (1 - 2^-51)^2 * (1 - 2^-53)^8 > lb * (1 - 2^-49): the factor
 *          (1 - 2^-40), itself exact, leaves 2^9 times that for the dozen roundings and for the one of the product lb * (1 - 2^-40).
 *    (v)   Underflow.  A square of d that underflows loses at most 2^-1074 a term against lb >= 2^-100: relative 2^-970.  A square of
 *          lb that underflows only lowers lb.  Below 2^-100 nothing is skipped.
 *    So lb * (1 - 2^-40) > best gives d > best, strictly, for every candidate of every face under the box: such a face can neither
 *    win nor tie, whatever its number.  An overflow makes lb = +inf > best only where best is finite, and then d, which is >= the real
 *    distance up to the roundings above, is +inf or beyond the largest finite best too.
 *    The worst case visits every box: fewer than 2 * ceil(nf / GP_VOLUME_LEAF) of them and every record once -- under twice a brute
 *    force, with no sweep rule.
 *    stats [GP_VOLUME_STAT_WORDS] int64 on the device, zeroed by the entry: EXCLUDED_FACES, EXCLUDED_QUERIES, NODES (boxes whose bound
 *    was computed), CANDIDATES (records handed to sf_test), MAX_STACK (the deepest stack of any query), LEVELS, LEAVES, STATUS (!= 0:
 *    the stack overflowed, which the argument above excludes).  Tallied by wave ballots and reductions; integer atomics, one per
 *    workgroup and word.
 *
 * 4. THE LATTICE (gp_volume_lattice).  sdf [nz][ny][nx] float32, a lane per lattice point, x fastest.  The point (i, j, k) is
 *    (fmaf((float)i, voxel, ox), fmaf((float)j, voxel, oy), fmaf((float)k, voxel, oz)): tsdf_core.h's ts_coord, the lattice of a
 *    gp_tsdf.h volume.  Per point the walk of 3, then gp_sdf.h section 2 (sd_sign) on the float32-rounded dist2, the face and the region
 *    -- what gp_sdf_sign computes from gp_surface_grid_query's row for that point.  4 bytes are written a point; no query array and no
 *    row of the walk is materialised.  The value is +inf where there is no usable face and for a point whose coordinate is not finite.
 *    stats [GP_VOLUME_LATTICE_WORDS] int64: the walk's eight words, then gp_sdf.h's eight STAT words.
 *
 * 5. THE COMPARISON (gp_volume_compare) of two volumes of n values: counts [GP_VOLUME_COUNT_WORDS] int64 = inside_a, inside_b, both,
 *    either, undetermined, n.  "Inside": a finite value < 0.  "Undetermined": a value that is not finite in either volume; such a point
 *    counts in none of the first four.  Integer arithmetic only: ballots and one integer atomic per workgroup and word.
 *
 * Conventions are those of gp_hip.h and gp_surface.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a gp_stream_t
 * last.  No entry synchronises or reads the device.  Refused everywhere, before any pointer is looked at: sizes outside the ranges
 * (nv < 2^31, nf < 2^26, nq and n 0 .. 2^31 - 1, 0 <= n_edges <= 3*nf), an origin or a voxel that is not finite, voxel <= 0, a
 * dimension < 1, nx*ny*nz >= 2^31; then a null or unaligned (16 bytes) scratch; then a null array that the sizes make non-empty.
 * gp_volume_query and gp_volume_lattice read what gp_volume_tree left in the scratch (the same nf). */
#ifndef GP_VOLUME_H
#define GP_VOLUME_H

#include "gp_sdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_VOLUME_ABI_VERSION 1

#ifndef GP_VOLUME_LEAF
#define GP_VOLUME_LEAF 2                     /* records a leaf (DESIGN section 34 measured 2, 4 and 8; a build may set another: no result depends on it) */
#endif
#define GP_VOLUME_STACK 32                   /* entries of a lane's stack: 28 at the most are ever used */
#define GP_VOLUME_MAX_LEVELS 27

#define GP_VOLUME_EXCLUDED_FACES 0           /* stats[] of gp_volume_query; the first words of gp_volume_lattice's */
#define GP_VOLUME_EXCLUDED_QUERIES 1
#define GP_VOLUME_NODES 2
#define GP_VOLUME_CANDIDATES 3
#define GP_VOLUME_MAX_STACK 4
#define GP_VOLUME_LEVELS 5
#define GP_VOLUME_LEAVES 6
#define GP_VOLUME_STATUS 7
#define GP_VOLUME_STAT_WORDS 8
#define GP_VOLUME_LATTICE_WORDS 16           /* the eight above, then gp_sdf.h's GP_SDF_STAT_WORDS */

#define GP_VOLUME_INSIDE_A 0                 /* counts[] of gp_volume_compare */
#define GP_VOLUME_INSIDE_B 1
#define GP_VOLUME_BOTH 2
#define GP_VOLUME_EITHER 3
#define GP_VOLUME_UNDETERMINED 4
#define GP_VOLUME_POINTS 5
#define GP_VOLUME_COUNT_WORDS 6

int gp_volume_abi_version(void);

/* The bytes of the scratch of gp_volume_tree.  -1 (and gp_last_error()) where nf is refused. */
int64_t gp_volume_tree_scratch_bytes(int64_t nf);

/* The tree of the mesh into `scratch`, which gp_volume_query and gp_volume_lattice then read. */
int gp_volume_tree(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, void* scratch, gp_stream_t stream);

/* dist2: [nq] float32; face, region: [nq] int32; closest: [nq][3] float32; bary: [nq][2] float32; stats: [GP_VOLUME_STAT_WORDS] int64. */
int gp_volume_query(const float* queries, int64_t nq, const void* scratch, int64_t nf, float* dist2, int32_t* face, int32_t* region, float* closest, float* bary,
                    int64_t* stats, gp_stream_t stream);

/* The mesh, its tree and its gp_sdf_tables; sdf: [nz][ny][nx] float32; stats: [GP_VOLUME_LATTICE_WORDS] int64. */
int gp_volume_lattice(const void* scratch, const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const int32_t* face_edges, const double* edge_normal,
                      int64_t n_edges, const double* vertex_normal, float ox, float oy, float oz, float voxel, int32_t nx, int32_t ny, int32_t nz, float* sdf,
                      int64_t* stats, gp_stream_t stream);

/* sdf_a, sdf_b: [n] float32; counts: [GP_VOLUME_COUNT_WORDS] int64 on the device. */
int gp_volume_compare(const float* sdf_a, const float* sdf_b, int64_t n, int64_t* counts, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
