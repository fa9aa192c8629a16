/* gp_mesh_smooth.h -- the topology of a triangle mesh on the device (unique edges, vertex adjacency, a report) and Laplacian /
 * Taubin smoothing of any per-vertex rows over it.  The C entry points of csrc/mesh_smooth_kernels.hip, a part of libgp_hip.so
 * with an ABI number of its own.  (The header lives beside the sources, not in include/, like gp_mesh.h: see DESIGN section 32.)
 *
 * What it adds: gp_mesh.h finds components by hooking face corners and gp_mesh_simplify.h sorts vertex keys; neither knows an edge.
 * Here the edges of a mesh, the faces on each, every vertex's neighbours and the boundary are built in a stated order, and one
 * smoothing step is a gather over the neighbour lists: two runs give equal bytes.
 *
 * A mesh: faces [nf][3] int32 over nv vertices, on the device.  Refused: gp_mesh.h's sizes (nv >= 2^31, 3*nf >= 2^31) and
 * 6*nf >= 2^31.  nv = 0 and nf = 0 are accepted.
 *
 * 1. Half-edges.  A face with an index outside [0, nv) is skipped and raises the status word (mesh_core.h's ms_face).  A kept face
 *    (a, b, c) gives the half-edges a->b, b->c, c->a.  A half-edge with equal ends is dropped and counted (degenerate).
 * 2. Edges.  The unique pairs (lo, hi), lo < hi, over all half-edges, in ascending lexicographic order: edge [E][2] int32.
 *      face_count[e]   the half-edges on edge e (a duplicated face counts twice, as it is)
 *      wind[e]         the half-edges running lo->hi minus those running hi->lo: a consistently oriented interior edge has
 *                      face_count 2 and wind 0
 * 3. Adjacency, in CSR form: offsets [nv + 1], neighbors [2E] int32.  The neighbours of v are the other ends of its edges, each once,
 *    in ascending index: neighbors[offsets[v] .. offsets[v + 1]).  degree(v) = offsets[v + 1] - offsets[v].
 * 4. vertex_flags [nv] uint8: GP_MESH_SMOOTH_FLAG_BOUNDARY (1) v ends an edge with face_count == 1; GP_MESH_SMOOTH_FLAG_NONMANIFOLD
 *    (2) v ends an edge with face_count > 2; GP_MESH_SMOOTH_FLAG_ISOLATED (4) degree 0.  Marks are plain byte stores of 1 into two
 *    arrays of the scratch (every writer stores the same byte); one lane a vertex puts the three bits together.
 * 5. counts [GP_MESH_SMOOTH_COUNT_WORDS] int32: status, E, boundary edges (face_count == 1), non-manifold edges (> 2), inconsistent
 *    edges (face_count == 2 and wind != 0), degenerate half-edges, vertices of degree > 0, kept faces.  Integer atomicAdd, one per
 *    wave.
 *
 * Mechanism.  Every half-edge u->v is entered twice, as (u, v) and as (v, u) with its direction bit: 6*nf directed entries, those of
 * skipped faces and dropped half-edges with the key (nv, nv), which sorts behind everything.  A stable radix sort by (first, second),
 * a word at a time on the bits nv needs; the head of every run of equal pairs is flagged; the ordered compaction of gp_mesh.h numbers
 * the heads: they are the neighbour lists in order, and the heads with first < second are the edges in order.  The lane of an edge's
 * head walks its run for face_count and wind (an edge of 5000 faces is 5000 steps on one lane).  offsets[v]: the first position of
 * the heads' first ends that is not below v, by bisection.
 *
 * gp_mesh_smooth_edges_plan leaves the counts on the device; the caller reads them (the one read), allocates, and calls
 * gp_mesh_smooth_edges_apply with the E it read (the same stream, sizes and scratch), which writes nothing beyond E edges and 2E
 * neighbours.
 *
 * 6. One step with factor s on rows [nv][k] float32, 1 <= k <= 1024, nv*k below 2^31, reading src and writing dst (Jacobi: a step
 *    never reads what it writes).  For vertex v and column a, all in float64, one operation at a time (no contraction):
 *      sum = +0.0;  for u in the neighbours of v, ascending:  sum = sum + double(src[u][a])
 *      m = sum / double(degree)                             (IEEE division, no reciprocal)
 *      t = m - double(src[v][a]);  t = s * t;  r = double(src[v][a]) + t;  dst[v][a] = float(r)       (one rounding)
 *    A vertex of degree 0 keeps its bits; so does a pinned vertex: pinned[v] & mask != 0, where mask is 3 under
 *    GP_MESH_SMOOTH_FIXED (with vertex_flags as `pinned`: the ends of boundary and non-manifold edges stay) and 0 under
 *    GP_MESH_SMOOTH_FREE (pinned is not read and may be null).  Non-finite values go through the arithmetic as IEEE has them: where
 *    that makes a NaN, the result is a NaN, of a sign and payload IEEE 754 does not state (a host's and the device's differ).
 *    One lane walks one vertex's list for one column: a hub of 2000 neighbours is 2000 dependent additions.  A list that leaves
 *    [0, n_neighbors) or names a vertex outside [0, nv) -- not one gp_mesh_smooth_edges_apply wrote -- leaves its vertex unchanged.
 *    GP_MESH_SMOOTH_LAPLACIAN   `iterations` steps with lambda_
 *    GP_MESH_SMOOTH_TAUBIN      per iteration one step with lambda_, then one with mu: 2 * iterations steps
 *    One launch per step, ping-pong between two buffers of the scratch; the last step writes dst; src is never written.
 *    iterations = 0 copies src to dst.  Refused: lambda_ or mu not finite, iterations outside [0, GP_MESH_SMOOTH_MAX_ITERATIONS],
 *    a method or boundary that is none of the above.  pinned_count (may be null): one int32 on the device, the pinned vertices.
 * 7. gp_mesh_smooth_umbrella writes float(m - double(src[v][a])) for every vertex and column, +0.0 where the degree is 0 (or the
 *    list is refused as in 6).
 *
 * Conventions are those of gp_hip.h and gp_mesh.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a gp_stream_t
 * last.  No entry synchronises or reads the device.  No float atomics anywhere.  Refused everywhere, before any pointer is looked
 * at: the sizes above, a null or unaligned (8 bytes) scratch, a null array that the sizes make non-empty. */
#ifndef GP_MESH_SMOOTH_H
#define GP_MESH_SMOOTH_H

#include "../../include/gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_MESH_SMOOTH_ABI_VERSION 1

#define GP_MESH_SMOOTH_LAPLACIAN 0           /* method */
#define GP_MESH_SMOOTH_TAUBIN 1
#define GP_MESH_SMOOTH_FREE 0                /* boundary */
#define GP_MESH_SMOOTH_FIXED 1
#define GP_MESH_SMOOTH_MAX_ITERATIONS 10000

#define GP_MESH_SMOOTH_FLAG_BOUNDARY 1       /* vertex_flags */
#define GP_MESH_SMOOTH_FLAG_NONMANIFOLD 2
#define GP_MESH_SMOOTH_FLAG_ISOLATED 4

#define GP_MESH_SMOOTH_STATUS 0              /* counts[]: != 0 iff a face index was out of range */
#define GP_MESH_SMOOTH_EDGES 1               /*           E */
#define GP_MESH_SMOOTH_BOUNDARY 2            /*           edges with face_count == 1 */
#define GP_MESH_SMOOTH_NONMANIFOLD 3         /*           edges with face_count > 2 */
#define GP_MESH_SMOOTH_INCONSISTENT 4        /*           edges with face_count == 2 and wind != 0 */
#define GP_MESH_SMOOTH_DEGENERATE 5          /*           half-edges with equal ends */
#define GP_MESH_SMOOTH_VERTICES 6            /*           vertices of degree > 0 */
#define GP_MESH_SMOOTH_FACES 7               /*           kept faces */
#define GP_MESH_SMOOTH_COUNT_WORDS 8

int gp_mesh_smooth_abi_version(void);

/* The bytes of the scratch of the two edges entries.  -1 (and gp_last_error()) where the sizes are refused. */
int64_t gp_mesh_smooth_scratch_bytes(int64_t nv, int64_t nf);

/* counts: [GP_MESH_SMOOTH_COUNT_WORDS] int32 on the device. */
int gp_mesh_smooth_edges_plan(const int32_t* faces, int64_t nv, int64_t nf, void* scratch, int32_t* counts, gp_stream_t stream);

/* After gp_mesh_smooth_edges_plan.  n_edges: counts[GP_MESH_SMOOTH_EDGES] as the caller read it.  edge: [E][2]; face_count, wind:
 * [E]; offsets: [nv + 1]; neighbors: [2E]; vertex_flags: [nv]. */
int gp_mesh_smooth_edges_apply(int64_t nv, int64_t nf, int64_t n_edges, const void* scratch, int32_t* edge, int32_t* face_count, int32_t* wind, int32_t* offsets,
                               int32_t* neighbors, uint8_t* vertex_flags, gp_stream_t stream);

/* The bytes of the scratch of gp_mesh_smooth_steps (two buffers of nv*k float32).  -1 where nv or k are refused. */
int64_t gp_mesh_smooth_rows_bytes(int64_t nv, int32_t k);

/* src, dst: [nv][k] float32 (dst may not overlap src); offsets [nv + 1], neighbors [n_neighbors]; pinned [nv] (see 6). */
int gp_mesh_smooth_steps(const float* src, int64_t nv, int32_t k, const int32_t* offsets, const int32_t* neighbors, int64_t n_neighbors, const uint8_t* pinned,
                         int32_t method, int32_t boundary, int32_t iterations, double lambda_, double mu, void* scratch, float* dst, int32_t* pinned_count,
                         gp_stream_t stream);

int gp_mesh_smooth_umbrella(const float* src, int64_t nv, int32_t k, const int32_t* offsets, const int32_t* neighbors, int64_t n_neighbors, float* dst,
                            gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
