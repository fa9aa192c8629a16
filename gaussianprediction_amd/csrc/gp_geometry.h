/* gp_geometry.h -- geometry metrics on the device: area-weighted samples of a mesh surface, an exact nearest neighbour on a uniform
 * grid, and the accuracy / completeness / Chamfer / F-score / Hausdorff table of two clouds.  The C entry points of
 * csrc/geometry_kernels.hip, a part of libgp_hip.so with an ABI number of its own.  (The header lives beside the sources, not in
 * include/: see DESIGN section 30.)
 *
 * What it adds: gp_mesh_render.h compares a mesh with a depth map, one camera at a time; nothing measured geometry in three
 * dimensions.  All the standard measures reduce to "sample the surfaces, find every sample's nearest neighbour in the other set,
 * reduce"; the only nearest neighbour of the library, gp_knn_points, is a brute force.
 *
 * The library is built without contraction: every operation below rounds once, in the stated order.
 *
 * 1. SAMPLES.  A mesh: vertices [nv][3] float32, faces [nf][3] int32, nv < 2^31, nf < GP_GEOMETRY_MAX_FACES = 2^26; n samples,
 *    1 <= n < 2^31; a seed, uint64.
 *    Face weight.  A face with an index outside [0, nv) (counts[BAD_INDEX]) or a non-finite corner coordinate (counts[NON_FINITE])
 *    has A_f = 0.  Otherwise, in float64 from the float32 corners a, b, c:  e = b - a, g = c - a (per component, (double)b - (double)a),
 *      n = (e_y*g_z - e_z*g_y,  e_z*g_x - e_x*g_z,  e_x*g_y - e_y*g_x);   A_f = sqrt((n_x*n_x + n_y*n_y) + n_z*n_z)
 *    (twice the area; only ratios matter).  m = max_f A_f (a maximum does not depend on order);  E = the binary exponent of m
 *    (m = 1.xxx * 2^E; m is never subnormal);  w_f = (uint64)(A_f * 2^(36 - E)), truncated: the scale is a power of two, so the
 *    product is exact, w_f < 2^37 and T = sum_f w_f < 2^63.  m == 0 gives every w_f = 0.  counts[ZERO_WEIGHT]: the faces that are
 *    neither BAD_INDEX nor NON_FINITE and have w_f == 0.
 *    P_f = w_0 + ... + w_f in uint64 (integer sums are exact in any order).
 *    Refusals on the device: counts[STATUS] = GP_GEOMETRY_REFUSED_EMPTY where T == 0, GP_GEOMETRY_REFUSED_TOO_MANY where 0 < T < n,
 *    0 otherwise (a T > 0 is at least 2^36 > n: TOO_MANY is a guard that these sizes cannot reach).  A refused call writes
 *    point = (NaN, NaN, NaN), face = -1, bary = (0, 0) for every sample; nothing is read by the host.
 *    Choice of face.  q = T / n (integer division; the tail T - q*n is never hit: a bias below n / T).
 *      h(seed, i, k) = mix(seed + 0x9E3779B97F4A7C15 * (3*i + k + 1))   mod 2^64, k = 0, 1, 2
 *      mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)    (splitmix64's)
 *      t_i = i*q + (h(seed, i, 0) mod q);  face_i = the first f with P_f > t_i (a binary search).  One sample per stratum
 *      [i*q, (i+1)*q): a face meets between w_f/q - 2 and w_f/q + 2 strata.
 *    Barycentrics.  k1 = h(seed, i, 1) >> 40, k2 = h(seed, i, 2) >> 40 (24 bits each); where k1 + k2 > 2^24: k1 = 2^24 - k1 and
 *    k2 = 2^24 - k2 (an integer test).  u1 = k1 * 2^-24, u2 = k2 * 2^-24 (exact); bary_i = (u1, u2).
 *    The point, per component in float32, in this order:  ((b - a) * u1 + a) + (c - a) * u2.
 *    gp_geometry_interpolate gives attributes [nv][C] float32, 1 <= C <= GP_GEOMETRY_MAX_CHANNELS, the same formula with the
 *    attribute rows of the corners of face_i; zeros where face_i is not a face with indices in range.
 *    The bytes depend on nothing but the arguments: not on the run, not on the launch shape.
 *
 * 2. NEAREST.  points [np][3], queries [nq][3] float32, np < 2^31 - 1, nq < 2^31.
 *    The result is defined without the grid.  d(q, p) = ((dx*dx + dy*dy) + dz*dz) in float32 with dx = q.x - p.x (knn_kernels.hip's
 *    own distance).  A point with a non-finite coordinate is never a neighbour (stats[EXCLUDED_POINTS]).  For a query with finite
 *    coordinates (dist2, index) is the lexicographic minimum over the usable points j of (d(q, p_j), j); (+inf, -1) where there is
 *    no usable point, and for a query with a non-finite coordinate (stats[EXCLUDED_QUERIES]).  Index -1 means exactly that: where
 *    there are usable points but every d overflows to +inf, the minimum is (+inf, the smallest usable index), as defined.
 *    For finite inputs this is gp_knn_points with K = 1 bit for bit, and the same for every cell size.
 *    Build (gp_geometry_grid_build; nothing is read by the host).  lo, hi: the bounds of the usable points (x + 0.f first, so a
 *    bound is never -0).  One lane derives the record, in float64: ext_a = hi_a - lo_a, E = max ext_a;
 *      R = ceil(E / cell) clamped to 1 .. 1024 where the caller passes cell > 0, else the automatic
 *      R = clamp(round(1.5 * cbrt(usable)), 1, 1024) in integers: r = the largest integer >= 1 with 8*r^3 <= 27*usable, plus 1 where
 *      (2r+1)^3 <= 27*usable (the 1.5 is a measured choice; no result depends on it);
 *      inv = (float)(R / E); size = 1.0 / (double)inv; dims_a = clamp((int)floor(ext_a / size) + 1, 1, R);
 *      while dims_x*dims_y*dims_z > GP_GEOMETRY_MAX_CELLS = 2^24: R = (R + 1) / 2 and again.
 *    ONE CELL (dims = 1, inv = 0, size = +inf) where E == 0, where there is no usable point, and where inv is outside
 *    [2^-96, 2^96] (clouds so small or so large that float32 would lose the argument below).
 *    The cell of x on an axis: t = floorf((x - lo) * inv); cell = t > 0 ? (t < dims - 1 ? (int)t : dims - 1) : 0 (a NaN t is cell 0):
 *    a clamp, monotone in x.  The linear key is (z*dims_y + y)*dims_x + x: x fastest.  Per-cell counts by integer atomic adds
 *    (order-free totals), an exclusive scan to start[cells + 1], then the usable points go to cell order as 16-byte records
 *    (x, y, z, index).  The order inside a cell may depend on the run; no result does (the explicit (d, j) comparison).
 *    Query (gp_geometry_grid_query), a lane per query.  h = the cell of q.  Rings r = 0, 1, 2, ... in Chebyshev distance around h,
 *    clamped to the grid.  Because x is fastest the cells [h_x - r, h_x + r] of one (y, z) are one span of records, start[first] to
 *    start[last + 1]: the rows of the two z faces and the two y faces of the shell are whole spans, only the x faces are single
 *    cells (ring 1 is 9 spans).  Every record of a visited span is a candidate.
 *    Stopping.  After ring r the walk stops when (a) the ring has covered the grid, or (b) B = (r * size * (1 - 2^-10))^2 in float64
 *    is >= 2^-100 and (double)best <= B, or (c) the spans and cells looked up so far are >= usable: the walk then ends with ONE
 *    pass over all the records (stats[SWEPT]) -- a query never costs more than about twice a brute force, however sparse the grid
 *    and however far outside the query (ring r costs up to (2r + 1)^2 + (2r - 1)^2 lookups, empty cells or not; a query far
 *    outside would otherwise walk the whole grid).
 *    Why (b) is exact.  Write g(x) = fl(fl(x - lo) * inv) for a real x, so cell(x) = clamp(floor(g(x))); g is monotone.  A point p
 *    not visited after ring r has on some axis |cell(p) - h| >= r + 1; say cell(p) >= h + r + 1 (the other side mirrors).  Take the
 *    real x nearest to q in [p, q] with cell(x) = h and inv*|x - lo| <= 1024 * (1 + 2^-22): x = q where q lies inside the bounds;
 *    x = lo where q < lo (cell(lo) = 0 = h, g(lo) = 0); where g(q) >= dims (q beyond the last cell, clamped) an x below q with g(x)
 *    in [dims - 1, dims), which exists because between 0 and ext the values of g are at most 2^-13 apart (an ulp of x - lo is at most
 *    2^-23 * E, times inv <= 1024 / E); p < x as g(p) < dims - 1.  |q - p| >= |x - p|.  floor(g(p)) >= cell(p) (the upper clamp only
 *    lowers) and g(x) < h + 1, so g(p) - g(x) > r.  Each fl is a relative error of at most 2^-24 (no underflow: inv >= 2^-96 and
 *    a product below 2^-126 is below one cell), so g(y) = inv * (y - lo) * (1 + e), |e| <= 2^-23 * (1 + 2^-25), and
 *      inv * (p - x) >= g(p) - g(x) - |e|*(inv*(p - lo) + inv*(x - lo)) > r - 2^-23 * 2 * 1024 * (1 + 2^-21) = r - 2^-12 * (1 + 2^-21),
 *    that is p - x > size * (r - 2^-12 * (1 + 2^-21)) with size = 1/inv the real size of a cell as the cell function sees it --
 *    also for a cloud far from the origin, where an ulp of x exceeds a cell: only x - lo enters, and Sterbenz or not, it is one
 *    rounding.  d(q, p) >= fl(dx*dx) >= (q - p)^2 * (1 - 2^-24)^3 (rounding is monotone, the other terms are >= 0, B >= 2^-100 keeps
 *    dx*dx far from underflow).  For r >= 1: (r - 2^-12*(1 + 2^-21))^2 * (1 - 2^-24)^3 > (r * (1 - 2^-10))^2 * (1 + 2^-11), which
 *    leaves room for the float64 roundings of B and of size.  So every point not visited has d > B >= best, strictly: it can neither
 *    win nor tie.  For r = 0, B = 0 < 2^-100: ring 1 is always walked unless (a) or (c) holds.
 *    stats: [GP_GEOMETRY_STAT_WORDS] int64 on the device, zeroed by gp_geometry_grid_query: EXCLUDED_POINTS, EXCLUDED_QUERIES,
 *    CANDIDATES (records compared, in all), MAX_RING, DIM_X, DIM_Y, DIM_Z, SWEPT.  Tallied by wave ballots and reductions; integer
 *    atomics, one per workgroup and word.
 *
 * 3. METRICS.  gp_geometry_metrics on dist2_ab [n_ab] (a's points to their nearest in b) and dist2_ba [n_ba]; thresholds: up to
 *    GP_GEOMETRY_MAX_THRESHOLDS float32 on the HOST.  An entry COUNTS iff it is finite; dist = sqrt((double)dist2).  Per direction
 *    twelve terms in float64: 1, dist, (double)dist2, dist (a maximum), and for k < 8: dist <= (double)tau_k (0 for k >= nt).
 *    Reduced exactly as gp_depth_metrics reduces: tile t holds the elements t*1024 + u*256 + lane, u = 0 .. 3, added per lane in
 *    that order; the 64 lanes of a wave by the butterfly x += x[lane ^ s], s = 32, 16, .., 1; the four waves as (w0 + w1) + (w2 + w3);
 *    a slot of twelve float64 per tile, stored plainly; ONE workgroup, a direction after the other: lane l adds the slots l,
 *    l + 256, .. in ascending order, then the tree s[l] += s[l + stride], stride = 128, .., 1; its first lane writes the table.
 *    (For the maximum every + is a max.)  No float atomics: equal bytes from run to run.
 *    table: [GP_GEOMETRY_COLUMNS] float64.  Conventions (the literature has several): distances, not squared, for accuracy and
 *    completeness; a is the prediction, b the ground truth.
 *      COUNT_AB, SUM_AB, SUM2_AB, MAX_AB, COUNT_BA, SUM_BA, SUM2_BA, MAX_BA       the totals
 *      ACCURACY = SUM_AB / COUNT_AB;  COMPLETENESS = SUM_BA / COUNT_BA            (0 / 0 = NaN)
 *      CHAMFER_L1 = (ACCURACY + COMPLETENESS) / 2;  CHAMFER_L2 = SUM2_AB / COUNT_AB + SUM2_BA / COUNT_BA
 *      HAUSDORFF = max(MAX_AB, MAX_BA), NaN unless both counts are > 0
 *      PRECISION + k = within_ab_k / COUNT_AB;  RECALL + k = within_ba_k / COUNT_BA;  FSCORE + k = 2pr / (p + r) where p + r > 0, else 0
 *      (k < 8; the columns of k >= nt are 0).
 *
 * Conventions are those of gp_hip.h and gp_mesh.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a gp_stream_t
 * last.  No entry synchronises or reads the device.  Refused everywhere, before any pointer is looked at: sizes outside the ranges
 * above; then a null or unaligned (16 bytes) scratch, a null array that the sizes make non-empty, a cell that is NaN, negative or
 * infinite, C outside 1 .. 8, nt outside 0 .. 8, a threshold that is NaN.  The scratch of each family is stated by its
 * gp_geometry_*_scratch_bytes entry; gp_geometry_grid_query reads what gp_geometry_grid_build left (the same np and cell).
 * The grid's scratch: 16 bytes a point plus 8 bytes for every cell the record may choose -- R^3 of the automatic rule (3.4 cells a point: about 43
 * bytes a point in all), but ALL 2^24 cells, 128 MiB, cleared and scanned by every build, where the caller passes a cell: the grid is derived on
 * the device, so the host cannot size for less.  A caller who passes a cell pays that for any cloud, however small. */
#ifndef GP_GEOMETRY_H
#define GP_GEOMETRY_H

#include "../../include/gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_GEOMETRY_ABI_VERSION 1

#define GP_GEOMETRY_MAX_FACES 67108864       /* 2^26: nf below this */
#define GP_GEOMETRY_MAX_CHANNELS 8
#define GP_GEOMETRY_MAX_AXIS 1024            /* cells along an axis at the most */
#define GP_GEOMETRY_MAX_CELLS 16777216       /* 2^24: cells in all at the most */
#define GP_GEOMETRY_MAX_THRESHOLDS 8
#define GP_GEOMETRY_WEIGHT_BITS 36           /* the largest face weight lies in [2^36, 2^37) */

#define GP_GEOMETRY_STATUS 0                 /* counts[] of gp_geometry_sample: 0, or why every sample was refused */
#define GP_GEOMETRY_BAD_INDEX 1              /*           faces with an index out of range */
#define GP_GEOMETRY_NON_FINITE 2             /*           faces with a non-finite corner */
#define GP_GEOMETRY_ZERO_WEIGHT 3            /*           other faces of weight 0 */
#define GP_GEOMETRY_COUNT_WORDS 8
#define GP_GEOMETRY_REFUSED_EMPTY 1          /* T == 0 */
#define GP_GEOMETRY_REFUSED_TOO_MANY 2       /* n > T */

#define GP_GEOMETRY_EXCLUDED_POINTS 0        /* stats[] of gp_geometry_grid_query */
#define GP_GEOMETRY_EXCLUDED_QUERIES 1
#define GP_GEOMETRY_CANDIDATES 2
#define GP_GEOMETRY_MAX_RING 3
#define GP_GEOMETRY_DIM_X 4
#define GP_GEOMETRY_DIM_Y 5
#define GP_GEOMETRY_DIM_Z 6
#define GP_GEOMETRY_SWEPT 7
#define GP_GEOMETRY_STAT_WORDS 8

#define GP_GEOMETRY_COUNT_AB 0               /* table[] of gp_geometry_metrics */
#define GP_GEOMETRY_SUM_AB 1
#define GP_GEOMETRY_SUM2_AB 2
#define GP_GEOMETRY_MAX_AB 3
#define GP_GEOMETRY_COUNT_BA 4
#define GP_GEOMETRY_SUM_BA 5
#define GP_GEOMETRY_SUM2_BA 6
#define GP_GEOMETRY_MAX_BA 7
#define GP_GEOMETRY_ACCURACY 8
#define GP_GEOMETRY_COMPLETENESS 9
#define GP_GEOMETRY_CHAMFER_L1 10
#define GP_GEOMETRY_CHAMFER_L2 11
#define GP_GEOMETRY_HAUSDORFF 12
#define GP_GEOMETRY_PRECISION 13             /* + k */
#define GP_GEOMETRY_RECALL 21                /* + k */
#define GP_GEOMETRY_FSCORE 29                /* + k */
#define GP_GEOMETRY_COLUMNS 37

int gp_geometry_abi_version(void);

/* The bytes of a scratch.  -1 (and gp_last_error()) where the sizes are refused. */
int64_t gp_geometry_sample_scratch_bytes(int64_t nf);
int64_t gp_geometry_grid_scratch_bytes(int64_t np, float cell);
int64_t gp_geometry_metrics_scratch_bytes(int64_t n_ab, int64_t n_ba);

/* points: [n][3] float32; face: [n] int32; bary: [n][2] float32; counts: [GP_GEOMETRY_COUNT_WORDS] int32, on the device. */
int gp_geometry_sample(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, int64_t n, uint64_t seed, void* scratch, float* points,
                       int32_t* face, float* bary, int32_t* counts, gp_stream_t stream);

/* attributes: [nv][C]; face, bary: as gp_geometry_sample left them; out: [n][C]. */
int gp_geometry_interpolate(const float* attributes, int32_t C, const int32_t* faces, int64_t nv, int64_t nf, const int32_t* face, const float* bary, int64_t n,
                            float* out, gp_stream_t stream);

/* cell: the size of a cell, or 0 for the automatic rule. */
int gp_geometry_grid_build(const float* points, int64_t np, float cell, void* scratch, gp_stream_t stream);

/* After gp_geometry_grid_build with the same np and cell.  dist2: [nq] float32; index: [nq] int32; stats: [GP_GEOMETRY_STAT_WORDS] int64. */
int gp_geometry_grid_query(const float* queries, int64_t nq, const void* scratch, int64_t np, float cell, float* dist2, int32_t* index, int64_t* stats,
                           gp_stream_t stream);

/* thresholds: [nt] float32 on the HOST; table: [GP_GEOMETRY_COLUMNS] float64 on the device. */
int gp_geometry_metrics(const float* dist2_ab, int64_t n_ab, const float* dist2_ba, int64_t n_ba, const float* thresholds, int32_t nt, void* scratch,
                        double* table, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
