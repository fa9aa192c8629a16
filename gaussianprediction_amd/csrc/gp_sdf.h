/* gp_sdf.h -- the SIGNED distance from a point to a mesh on the device: angle-weighted pseudonormals at faces, edges and vertices, and
 * the sign of a query from the normal of its closest feature (Baerentzen and Aanaes, "Signed distance computation using the angle
 * weighted pseudonormal", 2005).  The C entry points of csrc/sdf_kernels.hip, a part of libgp_hip.so with an ABI number of its own.
 * (The header lives beside the sources, not in include/, as gp_surface.h and gp_mesh_smooth.h do: see DESIGN section 33.)
 *
 * What it adds: gp_surface.h gives the closest point, its face and its Voronoi region, exactly; gp_mesh_smooth.h gives the unique edges
 * in ascending order.  Here the two are joined: the sign cannot be taken from the winning face's own normal (a query whose closest
 * point lies on an edge or a vertex sees the wrong side of a face at a sharp fold), the closest FEATURE's pseudonormal can.
 *
 * The library is built without contraction: every operation below rounds once, in the stated order.  All arithmetic is float64 from the
 * float32 inputs ((double)x first), with gp_surface.h's
 *      dot(x, y) = (x_0*y_0 + x_1*y_1) + x_2*y_2
 *      cross(x, y) = (x_1*y_2 - x_2*y_1,  x_2*y_0 - x_0*y_2,  x_0*y_1 - x_1*y_0)
 *
 * 1. THE TABLES (gp_sdf_tables).  vertices [nv][3] float32, faces [nf][3] int32, edge [E][2] int32: gp_mesh_smooth_edges_apply's unique
 *    pairs (lo, hi), lo < hi, in ascending lexicographic order.  nv < 2^31, nf < 2^26 (gp_surface.h's limits), 0 <= E <= 3*nf.
 *    A CONTRIBUTING face: its three indices lie in [0, nv) and are three different numbers.  A face with an index out of range raises
 *    counts[STATUS] and, like a face with a repeated index, contributes nothing anywhere (counts[SKIPPED] counts both).
 *    Face normal.  For a contributing face f = (a, b, c):  n_f = cross(b - a, c - a);  nn = dot(n_f, n_f);  u_f = n_f / sqrt(nn) per
 *      component where nn > 0, else (0, 0, 0) (counts[ZERO_AREA]; a NaN nn is not > 0).
 *    face_edges [nf][3] int32.  The number in `edge` of the sides (a, b), (b, c), (c, a) of face f, found by bisection on (min, max) of
 *      the two ends; -1 for a side with equal ends, for every side of a face with an index out of range, and for a side that `edge` does
 *      not hold (counts[MISSING]: `edge` is not this mesh's).  A face with a repeated index still names the edges of its other sides.
 *    edge_normal [E][3] float64.  The sum of u_f over the sides (f, k) of contributing faces with face_edges[f][k] = e, in ascending
 *      (face number, side number), starting from +0.0:  sum = sum + u_f per component.  A duplicated face counts twice, as face_count does.
 *    vertex_normal [nv][3] float64.  The sum over the corners (f, k) of contributing faces at the vertex, in ascending (face number,
 *      corner number), starting from +0.0, of angle * u_f:  t = angle * u_f per component;  sum = sum + t.
 *      angle = atan2(sqrt(dot(x, x)), dot(e1, e2)),  x = cross(e1, e2),  e1 = (next corner) - (this corner),  e2 = (previous corner) -
 *      (this corner): the two sides leaving that corner; corner 0 is a with e1 = b - a, e2 = c - a; corner 1 is b with e1 = c - b,
 *      e2 = a - b; corner 2 is c with e1 = a - c, e2 = b - c.  A corner of a face with nn > 0 false adds nothing.
 *    A sum is never split over lanes and nothing is added by float atomics: the 3*nf corner entries are sorted by vertex and the 3*nf
 *    side entries by edge number with the stable radix sort (entry 3f + k ascends inside every run), and ONE lane walks each run -- a
 *    hub of 2000 faces is 2000 dependent additions on one lane.  That is the definition's price.
 *    sqrt and division are IEEE; atan2 is the platform's libm (a host's and the device's may differ in the last bits: DESIGN section 33
 *    measures by how much).
 *    volume [1] float64.  term_f = dot(a, cross(b, c)) / 6.0 for a contributing face, +0.0 for any other.  Faces in blocks of 256:
 *      x[i] = term of face 256*block + i (+0.0 beyond nf);  for d = 128, 64, ..., 1:  x[i] = x[i] + x[i + d] for every i < d;  the
 *      block's partial is x[0], a plain store.  volume = the partials added in ascending block from +0.0 by one lane.  No float atomics.
 *    counts [GP_SDF_COUNT_WORDS] int32: STATUS (!= 0 iff a face index was out of range), SKIPPED, ZERO_AREA, MISSING.  Integer
 *      atomicAdd, one per wave and word.
 *
 * 2. THE SIGN OF A QUERY (gp_sdf_sign), defined from gp_surface_grid_query's own (dist2, face, region) for that query.
 *    face = -1 (an excluded query, or no usable face):  sdf = +inf, sign = 0, kind = -1, element = -1  (stats[EXCLUDED]).
 *    Otherwise, with f = face = (a, b, c) and q the query:
 *    (1) the winning candidate again, in float64, with surface_core.h's own functions -- the same operations give the same tau and p:
 *        region 0: the interior candidate p = (a + e1*u) + e2*v;  region k >= 1 on the segment (s, t) = (a, b), (b, c), (c, a):
 *        e = t - s, l2 = dot(e, e), tau, p = s + e*tau.
 *    (2) the closest feature:  region 0 is the face: kind 0, element f, N = u_f.  Region k >= 1 is
 *          vertex s  where l2 > 0 is false, or tau = 0, or the indices of s and t are equal;
 *          vertex t  where tau = 1;                                    (kind 2, element the vertex number, N = vertex_normal[element])
 *          otherwise the edge face_edges[f][k - 1]                    (kind 1, element that number, N = edge_normal[element];
 *                                                                      where it is -1: element -1 and N = (0, 0, 0))
 *    (3) r = q - p per component;  g = dot(r, N).
 *    (4) sign = -1 where g < 0, +1 where g > 0, 0 otherwise: a query on the surface, a zero N (two faces wound against each other
 *        cancel on their edge), a NaN, and face_edges = -1.  (stats[INSIDE], [OUTSIDE], [UNDETERMINED].)
 *    (5) sdf = (float)sqrt((double)dist2), negated where sign < 0.
 *    With the faces wound outward on a watertight mesh, sign < 0 is "inside"; on an open sheet it is the side the normals point away from.
 *    Foreign input.  A face outside [0, nf), a region outside 0 .. 3, a region 0 whose interior candidate does not exist, a face index
 *    outside [0, nv), a face_edges entry outside [-1, E): nothing is read through it; the row is sdf = (float)sqrt((double)dist2),
 *    sign 0, kind -1, element -1, counted UNDETERMINED, and stats[STATUS] is raised.
 *    stats [GP_SDF_STAT_WORDS] int64 on the device, zeroed by gp_sdf_sign: FACE, EDGE, VERTEX (queries by kind), INSIDE, OUTSIDE,
 *    UNDETERMINED, EXCLUDED, STATUS.  Tallied by wave ballots; integer atomics, one per workgroup and word.
 *    closest and bary of the query are taken for the caller's convenience and never read (they may be null): p is recomputed in float64.
 *
 * 3. THE MEANS (gp_sdf_means) of n signed distances: out [4] float64 = the number of finite sdf, their float64 sum, how many of those
 *    have sign > 0, how many sign < 0.  Entries in blocks of 256 with the tree of 1's volume, per word; one lane adds the partials in
 *    ascending block.  Two runs give equal bytes.
 *
 * Nothing depends on the run: two runs give equal bytes in every table and every output.
 *
 * Conventions are those of gp_hip.h and gp_surface.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a gp_stream_t
 * last.  No entry synchronises or reads the device.  Refused everywhere, before any pointer is looked at: sizes outside the ranges
 * above (nq and n: 0 .. 2^31 - 1); then a null or unaligned (8 bytes) scratch; then a null array that the sizes make non-empty. */
#ifndef GP_SDF_H
#define GP_SDF_H

#include "gp_surface.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_SDF_ABI_VERSION 1

#define GP_SDF_KIND_FACE 0                   /* kind[] */
#define GP_SDF_KIND_EDGE 1
#define GP_SDF_KIND_VERTEX 2

#define GP_SDF_COUNT_STATUS 0                /* counts[] of gp_sdf_tables: != 0 iff a face index was out of range */
#define GP_SDF_COUNT_SKIPPED 1               /*   faces that contribute nothing: an index out of range or repeated */
#define GP_SDF_COUNT_ZERO_AREA 2             /*   contributing faces with nn > 0 false */
#define GP_SDF_COUNT_MISSING 3               /*   sides with different ends that `edge` does not hold */
#define GP_SDF_COUNT_WORDS 4

#define GP_SDF_FACE 0                        /* stats[] of gp_sdf_sign: queries whose closest feature is a face */
#define GP_SDF_EDGE 1
#define GP_SDF_VERTEX 2
#define GP_SDF_INSIDE 3                      /*   sign < 0 */
#define GP_SDF_OUTSIDE 4                     /*   sign > 0 */
#define GP_SDF_UNDETERMINED 5                /*   sign = 0 with a face */
#define GP_SDF_EXCLUDED 6                    /*   face = -1 */
#define GP_SDF_STATUS 7                      /*   != 0 iff foreign input was met */
#define GP_SDF_STAT_WORDS 8

#define GP_SDF_MEAN_WORDS 4                  /* out[] of gp_sdf_means: count, sum, outside, inside */

int gp_sdf_abi_version(void);

/* The bytes of the scratch of gp_sdf_tables.  -1 (and gp_last_error()) where the sizes are refused. */
int64_t gp_sdf_tables_scratch_bytes(int64_t nv, int64_t nf, int64_t n_edges);

/* face_edges: [nf][3] int32; edge_normal: [n_edges][3] float64; vertex_normal: [nv][3] float64; volume: [1] float64; counts:
 * [GP_SDF_COUNT_WORDS] int32, all on the device. */
int gp_sdf_tables(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const int32_t* edge, int64_t n_edges, void* scratch, int32_t* face_edges,
                  double* edge_normal, double* vertex_normal, double* volume, int32_t* counts, gp_stream_t stream);

/* queries [nq][3]; dist2, face, region, closest, bary: gp_surface_grid_query's outputs for them; the mesh and its tables.
 * sdf: [nq] float32; sign: [nq] int8; kind, element: [nq] int32; stats: [GP_SDF_STAT_WORDS] int64. */
int gp_sdf_sign(const float* queries, int64_t nq, const float* dist2, const int32_t* face, const int32_t* region, const float* closest, const float* bary,
                const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const int32_t* face_edges, const double* edge_normal, int64_t n_edges,
                const double* vertex_normal, float* sdf, int8_t* sign, int32_t* kind, int32_t* element, int64_t* stats, gp_stream_t stream);

/* The bytes of the scratch of gp_sdf_means.  -1 where n is refused. */
int64_t gp_sdf_means_scratch_bytes(int64_t n);

/* sdf [n] float32, sign [n] int8 -> out [GP_SDF_MEAN_WORDS] float64 on the device. */
int gp_sdf_means(const float* sdf, const int8_t* sign, int64_t n, void* scratch, double* out, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
