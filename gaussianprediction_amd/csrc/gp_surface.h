/* gp_surface.h -- the exact distance from a point to a mesh surface on the device: the closest point on the nearest triangle, found on
 * a uniform grid over the triangles.  The C entry points of csrc/surface_kernels.hip, a part of libgp_hip.so with an ABI number of its
 * own.  (The header lives beside the sources, not in include/, as gp_geometry.h does: see DESIGN sections 30 and 31.)
 *
 * What it adds: every measure of gp_geometry.h is sample to sample, so a mesh against itself measures the spacing of the samples.  Here
 * a point is measured against the surface itself.
 *
 * The library is built without contraction: every operation below rounds once, in the stated order.
 *
 * 1. THE DEFINITION.  vertices [nv][3] float32, faces [nf][3] int32, queries [nq][3] float32; nv < 2^31, nf < GP_GEOMETRY_MAX_FACES =
 *    2^26, nq < 2^31 (gp_geometry.h's limits).  The result is defined without the grid.
 *    Usable faces.  A face with an index outside [0, nv) or a non-finite corner coordinate is never a candidate
 *    (stats[EXCLUDED_FACES]).  A face of zero area IS usable: it is a point or a segment, and its edge candidates give its distance.
 *    Notation, everything in float64 from the float32 inputs ((double)x first), per component unless said otherwise:
 *      dot(x, y) = (x_0*y_0 + x_1*y_1) + x_2*y_2
 *      cross(x, y) = (x_1*y_2 - x_2*y_1,  x_2*y_0 - x_0*y_2,  x_0*y_1 - x_1*y_0)
 *    The distance of q to a usable face (a, b, c):
 *      edge candidates k = 1, 2, 3 on the segments (s, t) = (a, b), (b, c), (c, a):
 *        e = t - s;  l2 = dot(e, e);  w = q - s;  tau = l2 > 0 ? clamp(dot(w, e) / l2, 0, 1) : 0   (clamp(x) = x < 0 ? 0 : (x > 1 ? 1 : x))
 *        p = s + e*tau;  r = q - p;  d_k = dot(r, r)
 *      the interior candidate k = 0:  e1 = b - a, e2 = c - a, n = cross(e1, e2), nn = dot(n, n); only where nn > 0:  w = q - a,
 *        u = dot(cross(w, e2), n) / nn,  v = dot(cross(e1, w), n) / nn;  a candidate iff u >= 0 and v >= 0 and u + v <= 1;
 *        p = (a + e1*u) + e2*v;  r = q - p;  d_0 = dot(r, r)
 *      the face's (d, region) = the lexicographic minimum of (d_k, k) over its candidates (the three edges always are).
 *    No denominator is zero for any usable face, and every candidate p is, up to its own rounding, a real point of the triangle (tau in
 *    [0, 1], or u, v >= 0 with u + v <= 1 as computed): a computed distance is never meaningfully below the true one.
 *    The result of a query with finite coordinates: the lexicographic minimum over the usable faces f of (d_f, f) -- a tie between
 *    faces goes to the smaller face number.  Nothing depends on the order of the faces, of the cells or of the run.
 *      dist2 [nq] float32       (float)d, the float64 minimum rounded once
 *      face [nq] int32          f
 *      region [nq] int32        k: 0 the interior, 1 the edge (a, b), 2 (b, c), 3 (c, a)
 *      closest [nq][3] float32  (float)p of the winning candidate
 *      bary [nq][2] float32     (float)(u1, u2) in gp_geometry_interpolate's convention, point = a + (b - a)*u1 + (c - a)*u2:
 *                               k = 0: (u, v);  k = 1: (tau, 0);  k = 2: (1.0 - tau, tau);  k = 3: (0, 1.0 - tau)   (1.0 - tau in float64)
 *    Where there is no usable face, and for a query with a non-finite coordinate (stats[EXCLUDED_QUERIES]):
 *      dist2 = +inf, face = -1, region = 0, closest = (NaN, NaN, NaN), bary = (0, 0).
 *
 * 2. THE GRID.  gp_surface_grid_count, then gp_surface_grid_fill; no entry synchronises or reads the device.
 *    A face record: the nine corner floats and the face number (-1: not usable), 48 bytes, three 16-byte loads -- a candidate costs
 *    one dependent gather, not four.  lo, hi: the bounds of the corners of the usable faces (x + 0.f first), by integer atomic minima
 *    and maxima of order-preserving bits.  One lane derives gp_geometry.h's grid record from them with gp_geometry.h's formulas
 *    (inv, size, dims, the halving to GP_GEOMETRY_MAX_CELLS, ONE CELL in the degenerate ranges) and gp_geometry.h's cell function
 *    (a monotone clamp; x fastest), with `usable` the number of usable faces and the automatic
 *      R = clamp(round(sqrt(usable) / 4), 1, 1024) in integers: r = the largest integer with 16*r*r <= usable, plus 1 where 4*(2r+1)^2 <= usable
 *    (a measured choice, DESIGN section 31: a cell of about one and a half face edges on an extracted surface; no result depends on it).
 *    A face is registered in every cell of its box, cell(min corner) .. cell(max corner) per axis (the cell function is monotone: the
 *    smallest and largest of the three corner cells).  A face whose box holds more than W cells, 1 <= W <= GP_SURFACE_MAX_WIDE_CELLS,
 *    goes to the WIDE LIST instead, which every query tests first (GP_SURFACE_WIDE_CELLS = 64 is the measured choice).
 *    gp_surface_grid_count: the records, the bounds, the grid, the wide list, the per-cell pair counts by integer atomic adds and
 *    their exclusive scan start[cells + 1]; sizes[0] = the number of (cell, face) pairs (at most nf * W < 2^32), sizes[1] = the wide
 *    faces, int64 on the device.  The CALLER reads those 16 bytes to size `pairs` -- the one read the data's own size forces.
 *    gp_surface_grid_fill(pairs, pair_capacity): the face numbers scattered to cell order.  pair_capacity < sizes[0] is refused on
 *    the device: nothing is written to `pairs`, stats[STATUS] of every later query is GP_SURFACE_REFUSED_CAPACITY and every result is
 *    the (+inf, -1, ..) row.  The order inside a cell and inside the wide list may depend on the run; no result does.
 *    Query (gp_surface_grid_query), a lane per query.  The wide list, then rings r = 0, 1, 2, ... in Chebyshev distance around the
 *    cell h of q, clamped to the grid, with gp_geometry.h's spans: the cells [h_x - r, h_x + r] of one (y, z) are one span of pairs.
 *    Every face of a visited pair is a candidate; a face met twice costs time only (a minimum is idempotent).  After ring r the walk
 *    stops when (a) the ring has covered the grid, or (b) B = (r * size * (1 - 2^-10))^2 in float64 is >= 2^-100 and best <= B (best:
 *    the float64 minimum so far), or (c) the spans and cells looked up so far are >= usable: then ONE pass over all nf records
 *    (stats[SWEPT]) -- a query costs at most about twice a brute force, however sparse the grid and however far away the query.
 *    Why (b) is exact.  A face not met after ring r is not wide and its box misses the cube [h - r, h + r]^3, so on some axis k the
 *    whole box lies beyond: the cells of all three corners are >= h_k + r + 1 (the other side mirrors).  gp_geometry.h's argument,
 *    corner by corner (its p is a corner coordinate c_k, its x the real point between q_k and the corner with cell(x) = h_k), gives
 *    c_k - x > size * (r - 2^-12 * (1 + 2^-21)) for each corner, and a real point of the triangle is a convex combination of the
 *    corners: every real point p* of the face has p*_k - x > size * (r - 2^-12 * (1 + 2^-21)), and |q_k - p*_k| >= |x - p*_k|.
 *    The ONE new term: the computed candidate p is not p* but its float64 evaluation.  With M_k the largest |coordinate| on axis k
 *    among the usable corners: |e| <= 2 M_k, |a + e1*u| <= 3 M_k, |p| <= 5 M_k, so the five roundings of the interior candidate move
 *    p_k by at most (2 + 2 + 3 + 2*2 + 5) * 2^-53 * M_k = 2^-49 * M_k, the three of an edge candidate by less, and u + v <= 1 as
 *    computed allows a real u + v <= 1 + 2^-53, another 2^-52 * M_k outside the triangle: |p_k - p*_k| <= 2^-48 * M_k.
 *    An axis that can separate has dims_k >= 2, hence ext_k > 0: lo_k and hi_k are different float32 values, so ext_k >= 2^-24 * M_k
 *    (an ulp of the larger, or more), and size >= (E / 1024) * (1 - 2^-24) >= ext_k / 1024 * (1 - 2^-24).  So M_k <= 2^34 * size *
 *    (1 + 2^-23) and |p_k - p*_k| <= 2^-14 * size * (1 + 2^-23) -- also for a mesh far from the origin: the rounding of p is small
 *    against a cell because a cell is at least 2^-34 of the largest coordinate.  It is bounded with the (1 - 2^-10) margin already
 *    there; the margin does not change.  |q_k - p_k| > size * (r - 2^-12 * (1 + 2^-21) - 2^-14 * (1 + 2^-23)) > size * (r - 2^-11),
 *    d >= fl(r_k * r_k) >= (q_k - p_k)^2 * (1 - 2^-53)^3, and for r >= 1:  (r - 2^-11)^2 * (1 - 2^-53)^3 >= r^2 * (1 - 2^-11)^2 *
 *    (1 - 2^-51) > (r * (1 - 2^-10))^2 * (1 + 2^-11), which leaves room for the float64 roundings of B and of size.  So every
 *    candidate of a face not met has d > B >= best, strictly: the face can neither win nor tie.  For r = 0, B = 0 < 2^-100.
 *    stats: [GP_SURFACE_STAT_WORDS] int64 on the device, zeroed by gp_surface_grid_query: EXCLUDED_FACES, EXCLUDED_QUERIES,
 *    CANDIDATES (face records tested, in all), MAX_RING, DIM_X, DIM_Y, DIM_Z, SWEPT, PAIRS, WIDE, STATUS.  Tallied by wave ballots and
 *    reductions; integer atomics, one per workgroup and word.  No float atomics anywhere.
 *
 * Conventions are those of gp_hip.h and gp_geometry.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a
 * gp_stream_t last.  Refused everywhere, before any pointer is looked at: sizes outside the ranges above, a cell that is NaN,
 * negative or infinite, W outside 1 .. 64, a negative pair_capacity; then a null or unaligned (16 bytes) scratch, a null array that
 * the sizes make non-empty.  The scratch (gp_surface_scratch_bytes): 52 bytes a face plus 8 bytes for every cell the record may choose
 * -- min(R^3, 2^24) of the automatic rule, ALL 2^24 cells, 128 MiB, where the caller passes a cell, as in gp_geometry.h.  gp_surface_grid_fill
 * and gp_surface_grid_query read what the entry before them left (the same nf and cell). */
#ifndef GP_SURFACE_H
#define GP_SURFACE_H

#include "gp_geometry.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_SURFACE_ABI_VERSION 1

#define GP_SURFACE_WIDE_CELLS 64             /* W: a face whose box holds more cells goes to the wide list */
#define GP_SURFACE_MAX_WIDE_CELLS 64         /* W at the most: nf * W stays below 2^32 */

#define GP_SURFACE_EXCLUDED_FACES 0          /* stats[] of gp_surface_grid_query */
#define GP_SURFACE_EXCLUDED_QUERIES 1
#define GP_SURFACE_CANDIDATES 2
#define GP_SURFACE_MAX_RING 3
#define GP_SURFACE_DIM_X 4
#define GP_SURFACE_DIM_Y 5
#define GP_SURFACE_DIM_Z 6
#define GP_SURFACE_SWEPT 7
#define GP_SURFACE_PAIRS 8
#define GP_SURFACE_WIDE 9
#define GP_SURFACE_STATUS 10
#define GP_SURFACE_STAT_WORDS 12
#define GP_SURFACE_REFUSED_CAPACITY 1        /* pair_capacity below the number of pairs */

int gp_surface_abi_version(void);

/* The bytes of the scratch.  -1 (and gp_last_error()) where the arguments are refused. */
int64_t gp_surface_scratch_bytes(int64_t nf, float cell);

/* cell: the size of a cell, or 0 for the automatic rule.  wide_cells: W.  sizes: [2] int64 on the device: pairs, wide faces. */
int gp_surface_grid_count(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, float cell, int32_t wide_cells, void* scratch, int64_t* sizes,
                          gp_stream_t stream);

/* After gp_surface_grid_count with the same nf, cell and wide_cells.  pairs: [pair_capacity] int32 on the device. */
int gp_surface_grid_fill(int64_t nf, float cell, int32_t wide_cells, void* scratch, int32_t* pairs, int64_t pair_capacity, gp_stream_t stream);

/* After gp_surface_grid_fill.  dist2: [nq] float32; face, region: [nq] int32; closest: [nq][3] float32; bary: [nq][2] float32;
 * stats: [GP_SURFACE_STAT_WORDS] int64. */
int gp_surface_grid_query(const float* queries, int64_t nq, const void* scratch, const int32_t* pairs, int64_t nf, float cell, float* dist2, int32_t* face,
                          int32_t* region, float* closest, float* bary, int64_t* stats, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
