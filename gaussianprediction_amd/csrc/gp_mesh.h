/* gp_mesh.h -- cleanup of a triangle mesh on the device: connected components, removal of small components, vertex normals.  The C
 * entry points of csrc/mesh_kernels.hip, a part of libgp_hip.so with an ABI number of its own.  (The header lives beside the
 * sources, not in include/: see DESIGN sections 26 and 27.)
 *
 * What it adds: gp_tsdf.h ends at the extracted mesh.  A mesh fused from a trained scene carries small closed shells (one per stray
 * blob that two views agree on) and no normals.  Both need the connectivity of the mesh on the device.
 *
 * A mesh: vertices [nv][3] float32, faces [nf][3] int32, on the device.  Refused: nv >= 2^31; 3*nf >= 2^31 (incidence ids 3f + corner
 * are int32).  nv = 0 and nf = 0 are accepted.  A face with an index outside [0, nv) is SKIPPED by every kernel -- every index is
 * checked where it is dereferenced -- and raises state[GP_MESH_STATUS]; the caller finds it at its next read.
 *
 * 1. Components.  The graph has the vertices as nodes and an edge between any two indices of one face: triangles that share only a
 *    vertex are connected.  vertex_label[v]: the SMALLEST vertex index of v's component, so the result is unique.  face_label[f] =
 *    vertex_label[faces[f][0]] (-1 for a skipped face).  The table, in ascending label, C rows: labels, vertex_counts, face_counts
 *    (int32; table = [3][nv], the first C of each row).  A vertex no face names is a component of its own with face count 0.
 *    Degenerate faces are ordinary faces.
 *    The scheme is monotone: parent[v] starts as v and only ever decreases, through integer atomicMin; parent[v] <= v and parent[v] is
 *    a vertex of v's component, always.  A stale plain load therefore costs a round and never a result.  One ROUND is three launches:
 *      hook    per face, its edges (a, b), (b, c): with gu = parent[parent[u]], gv likewise, the smaller of the two goes by atomicMin
 *              onto the other side's parent and onto the other vertex itself (FastSV's stochastic and aggressive hooking)
 *      jump    per vertex, parent[v] = its ancestor up to GP_MESH_HOPS pointers up (a plain store to its own word)
 *      settle  changes nothing and, behind the launch boundary, sees everything: unless every face has one parent on its three
 *              indices and every parent is a root, the next round's flag is raised
 *    A round whose flag is down returns at once.  When a settle launch finds nothing, every component is a star on one root r <= all
 *    of its vertices, r one of them: its smallest index.  The answer does not depend on the rounds granted: gp_mesh_components runs
 *    `rounds` of them (first != 0: from parent[v] = v; first == 0: on from where the last call stopped), then the table, and leaves
 *    state = (status, converged, C, rounds used); table, face_label and C mean something only where converged != 0.
 *    Rounds: the hooks at least halve the number of trees that still have a neighbour tree in every round in which the loads are
 *    fresh, and the jumps halve (here: divide by GP_MESH_HOPS + 1) every height: logarithmic in practice, never proportional to the
 *    diameter.  No proof of the worst case is claimed; the tests cap a path of 4098 vertices under a seeded numbering at
 *    4 ceil(log2 nv) + 8 rounds, on the CPU with synchronous rounds (every load of a round as stale as it can be) and on the device.
 *    The table counts with integer atomicAdd (one per wave where the wave's labels agree) and numbers the roots by an ordered
 *    compaction: per tile of GP_MESH_TILE elements a sum, ONE workgroup scans the tiles, then ballot ranks inside the tile.
 *
 * 2. Filter.  A component is kept iff its face count is >= 1, and >= min_triangles where min_triangles >= 0, and it is among the
 *    keep_largest components with the most faces where keep_largest >= 0, ties to the smaller label (a stable radix sort of
 *    0x7fffffff - face_count over the table).  A vertex is kept iff its component is, a face iff its three vertices are.  Kept
 *    vertices and faces keep their ascending order (ordered compaction as above; no atomics), the faces' indices are renumbered.
 *    gp_mesh_filter_plan leaves counts = (vertices kept, faces kept, status); gp_mesh_filter_apply writes vertex_index, face_index
 *    (the old ids) and the new faces; gp_mesh_gather_rows carries any [nv][k] float32 array along (positions, colours, attributes).
 *
 * 3. Normals, float32, one operation at a time (the library is built without contraction):
 *      face vector   e1 = b - a, e2 = c - a, n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x)      (area-weighted)
 *      vertex        x, y, z = the sums of its incidences' face vectors, one after the other in ascending 3f + corner, from +0
 *                    len = sqrtf((x*x + y*y) + z*z);  (x / len, y / len, z / len) if len is finite and > 0, else (0, 0, 0)
 *    The incidence lists come from a stable radix sort of (vertex, 3f + corner) pairs; the corners of a skipped face sort behind
 *    every vertex and contribute nothing.  One lane walks one vertex's list: a vertex of several thousand faces is correct and as
 *    slow as that sounds.  No float atomics: two runs give equal bytes.
 *
 * The scratch of every entry: gp_mesh_scratch_bytes(nv, nf) bytes, 256-byte aligned; gp_mesh_filter_apply and gp_mesh_gather_rows
 * read what gp_mesh_filter_plan left in it.  Conventions are those of gp_hip.h: plain pointers and sizes, a return code != 0 plus
 * gp_last_error(), a gp_stream_t last.  No entry synchronises or reads the device.  Refused everywhere: the sizes above, a null or
 * unaligned (4 bytes) scratch, a null array that the sizes make non-empty. */
#ifndef GP_MESH_H
#define GP_MESH_H

#include "../../include/gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_MESH_ABI_VERSION 1

#define GP_MESH_TILE 1024            /* elements per workgroup of the ordered compactions */
#define GP_MESH_HOPS 4               /* pointers a jump follows */
#define GP_MESH_MAX_ROUNDS 64        /* the rounds of one gp_mesh_components call at the most */

#define GP_MESH_STATUS 0             /* state[]: != 0 iff a face index (or a label handed in) was out of range */
#define GP_MESH_CONVERGED 1          /*          != 0 iff the last settle launch found nothing */
#define GP_MESH_COUNT 2              /*          C, the rows of the table */
#define GP_MESH_ROUNDS 3             /*          the rounds that ran since first != 0 */
#define GP_MESH_STATE_WORDS 4

int gp_mesh_abi_version(void);

/* The bytes of the scratch.  -1 (and gp_last_error()) where the sizes are refused. */
int64_t gp_mesh_scratch_bytes(int64_t nv, int64_t nf);

/* rounds: 1 .. GP_MESH_MAX_ROUNDS.  vertex_label: [nv], the parents between calls; face_label: [nf]; table: [3][nv]; state:
 * [GP_MESH_STATE_WORDS] int32, all on the device. */
int gp_mesh_components(const int32_t* faces, int64_t nv, int64_t nf, int32_t rounds, int32_t first, int32_t* vertex_label, int32_t* face_label,
                       int32_t* table, void* scratch, int32_t* state, gp_stream_t stream);

/* vertex_label: [nv]; labels, face_counts: [components], as gp_mesh_components left them; min_triangles, keep_largest: < 0 for "not
 * given"; counts: [3] int32 on the device. */
int gp_mesh_filter_plan(const int32_t* faces, int64_t nv, int64_t nf, const int32_t* vertex_label, const int32_t* labels, const int32_t* face_counts,
                        int64_t components, int32_t min_triangles, int32_t keep_largest, void* scratch, int32_t* counts, gp_stream_t stream);

/* After gp_mesh_filter_plan on the same stream with the same faces and scratch.  vertex_index: [counts[0]]; face_index: [counts[1]];
 * faces_out: [counts[1]][3]. */
int gp_mesh_filter_apply(const int32_t* faces, int64_t nv, int64_t nf, const void* scratch, int32_t* vertex_index, int32_t* face_index,
                         int32_t* faces_out, gp_stream_t stream);

/* dst[new v][0 .. k) = src[old v][0 .. k) for every kept vertex: src [nv][k], dst [counts[0]][k] float32, 1 <= k <= 1024. */
int gp_mesh_gather_rows(const float* src, int64_t nv, int32_t k, const void* scratch, float* dst, gp_stream_t stream);

/* normals: [nv][3] float32; state: [GP_MESH_STATE_WORDS] int32 (only GP_MESH_STATUS is written, and only raised). */
int gp_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, void* scratch, float* normals, int32_t* state,
                           gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
