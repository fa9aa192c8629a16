// mesh_core.h -- the per-face, per-vertex and per-component programs of mesh cleanup (csrc/gp_mesh.h), shared by the kernels of
// mesh_kernels.hip and by the stand-alone CPU build the tests run under the sanitizers (tests/mesh_emulate.cpp).
//
//   ms_face            the three indices of a face, bound-checked: every program that dereferences a face index goes through it
//   ms_hook_face       one face's two edges hooked (FastSV: the smaller grandparent onto the other side's parent and vertex)
//   ms_jump            one vertex's pointer jumped, up to GP_MESH_HOPS steps
//   ms_unsettled_face, ms_unsettled_vertex     what the convergence launch looks for
//   ms_keep_component, ms_keep_vertex, ms_keep_face, ms_remap_face     the filter
//   ms_face_vector, ms_incidence_key, ms_vertex_normal                 the normals
//   ms_tile_elem, ms_chunk                     the order of the tiled scans;  ms_refuse_sizes, ms_scratch_layout
// `pr` and `pw` of the hooking programs are the SAME array on the device (a stale load costs a round, never a result: labels only
// decrease); the CPU build hands them a snapshot and the live array, the synchronous round that is the slowest a device can be.
// The file must be compiled with -ffp-contract=off: every operation rounds once.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gp_mesh.h"

#if defined(__HIPCC__)
#define MS_FN __host__ __device__ inline
#else
#define MS_FN inline
#endif

#define MS_BLOCK 256
#define MS_PER_LANE (GP_MESH_TILE / MS_BLOCK)
#define MS_CHUNKS (GP_MESH_TILE / 64)               // the 64-element chunks of a tile: one ballot each

MS_FN bool ms_finite(float v) { return fabsf(v) < INFINITY; }            // (false for a NaN)
MS_FN bool ms_index_ok(int64_t i, int64_t nv) { return i >= 0 && i < nv; }

MS_FN void ms_atomic_min(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
// *p = min(*p, v), the atomic left out where a load past the vector L1 already shows a value <= v: values only decrease, so the word
// is then <= v for good and the atomic would change nothing (the roots of large trees are named by many thousands of faces a round)
MS_FN void ms_lower(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, v);
#else
    ms_atomic_min(p, v);
#endif
}
MS_FN void ms_atomic_add(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

// the indices of face f into v; false, and the status word raised, where one lies outside [0, nv): the face is then skipped
MS_FN bool ms_face(const int32_t* faces, int64_t f, int64_t nv, int32_t* v, int32_t* state) {
    v[0] = faces[3 * f]; v[1] = faces[3 * f + 1]; v[2] = faces[3 * f + 2];
    if (ms_index_ok(v[0], nv) && ms_index_ok(v[1], nv) && ms_index_ok(v[2], nv)) return true;
    if (state) state[GP_MESH_STATUS] = 1;                               // (every writer stores the same word)
    return false;
}

// ---- components ----
// parent[x] <= x always, and parent[x] is a vertex of x's component: the pointers form a forest whose roots only ever get smaller
MS_FN void ms_hook_edge(const int32_t* pr, int32_t* pw, int32_t u, int32_t v) {
    const int32_t pu = pr[u], pv = pr[v];
    const int32_t gu = pr[pu], gv = pr[pv];
    if (gu < gv) { ms_lower(&pw[pv], gu); ms_lower(&pw[v], gu); }
    else if (gv < gu) { ms_lower(&pw[pu], gv); ms_lower(&pw[u], gv); }
}

MS_FN void ms_hook_face(const int32_t* pr, int32_t* pw, const int32_t* faces, int64_t f, int64_t nv, int32_t* state) {
    int32_t v[3];
    if (!ms_face(faces, f, nv, v, state)) return;
    ms_hook_edge(pr, pw, v[0], v[1]);
    ms_hook_edge(pr, pw, v[1], v[2]);
}

MS_FN void ms_jump(const int32_t* pr, int32_t* pw, int64_t v) {
    int32_t p = pr[v];
    for (int hop = 0; hop < GP_MESH_HOPS; ++hop) {
        const int32_t q = pr[p];
        if (q == p) break;
        p = q;
    }
    pw[v] = p;                                       // (an ancestor of v: never larger than before)
}

MS_FN bool ms_unsettled_face(const int32_t* parent, const int32_t* faces, int64_t f, int64_t nv) {
    int32_t v[3];
    if (!ms_face(faces, f, nv, v, nullptr)) return false;
    const int32_t a = parent[v[0]];
    return a != parent[v[1]] || a != parent[v[2]];
}
MS_FN bool ms_unsettled_vertex(const int32_t* parent, int64_t v) { const int32_t p = parent[v]; return parent[p] != p; }

// the label of a face, -1 for a skipped one
MS_FN int32_t ms_face_label(const int32_t* parent, const int32_t* faces, int64_t f, int64_t nv, int32_t* state) {
    int32_t v[3];
    return ms_face(faces, f, nv, v, state) ? parent[v[0]] : -1;
}

// ---- the filter ----
// component `c` of the table, standing at `pos` in the order most faces first, ties by label
MS_FN uint8_t ms_keep_component(int32_t face_count, int32_t min_triangles, int32_t keep_largest, int64_t pos) {
    return face_count >= 1 && (min_triangles < 0 || face_count >= min_triangles) && (keep_largest < 0 || pos < keep_largest);
}

MS_FN uint8_t ms_keep_vertex(const uint8_t* keep_label, const int32_t* vertex_label, int64_t v, int64_t nv, int32_t* state) {
    const int32_t l = vertex_label[v];
    if (!ms_index_ok(l, nv)) { state[GP_MESH_STATUS] = 1; return 0; }
    return keep_label[l];
}

// a face stays iff its three vertices stay (with the labels of this mesh: iff its component stays)
MS_FN uint8_t ms_keep_face(const uint8_t* keep_vertex, const int32_t* faces, int64_t f, int64_t nv, int32_t* state) {
    int32_t v[3];
    if (!ms_face(faces, f, nv, v, state)) return 0;
    return keep_vertex[v[0]] && keep_vertex[v[1]] && keep_vertex[v[2]];
}

MS_FN void ms_remap_face(const int32_t* faces, int64_t f, const uint32_t* rank_vertex, int32_t* out) {      // (a kept face: its indices were checked)
    for (int c = 0; c < 3; ++c) out[c] = (int32_t)rank_vertex[faces[3 * f + c]];
}

// ---- the normals ----
// (b - a) x (c - a); false and zeros for a skipped face
MS_FN bool ms_face_vector(const float* vertices, const int32_t* faces, int64_t f, int64_t nv, float* n, int32_t* state) {
    int32_t v[3];
    n[0] = n[1] = n[2] = 0.f;
    if (!ms_face(faces, f, nv, v, state)) return false;
    const float* a = vertices + 3 * (int64_t)v[0];
    const float* b = vertices + 3 * (int64_t)v[1];
    const float* c = vertices + 3 * (int64_t)v[2];
    const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    n[0] = e1y * e2z - e1z * e2y;
    n[1] = e1z * e2x - e1x * e2z;
    n[2] = e1x * e2y - e1y * e2x;
    return true;
}

// the sort key of incidence i = 3f + corner: its vertex, or nv for a corner of a skipped face (those sort behind every vertex)
MS_FN uint32_t ms_incidence_key(const int32_t* faces, int64_t i, int64_t nv) {
    int32_t v[3];
    return ms_face(faces, i / 3, nv, v, nullptr) ? (uint32_t)v[i % 3] : (uint32_t)nv;
}

// incidences: ids 3f + corner in ascending order, [begin, end) those of one vertex; face_vectors [nf][3]
MS_FN void ms_vertex_normal(const float* face_vectors, const uint32_t* incidences, int64_t begin, int64_t end, float* out) {
    float x = 0.f, y = 0.f, z = 0.f;
    for (int64_t i = begin; i < end; ++i) {
        const float* n = face_vectors + 3 * (int64_t)(incidences[i] / 3u);
        x = x + n[0]; y = y + n[1]; z = z + n[2];
    }
    const float len = sqrtf((x * x + y * y) + z * z);
    const bool ok = ms_finite(len) && len > 0.f;
    out[0] = ok ? x / len : 0.f;
    out[1] = ok ? y / len : 0.f;
    out[2] = ok ? z / len : 0.f;
}

// ---- the tile order (that of tsdf_core.h) ----
MS_FN int64_t ms_tile_elem(int64_t tile, int u, int t) { return tile * GP_MESH_TILE + (int64_t)u * MS_BLOCK + t; }
MS_FN int ms_chunk(int u, int t) { return u * (MS_BLOCK / 64) + t / 64; }

// ---- refusals and the scratch ----
inline const char* ms_refuse_sizes(int64_t nv, int64_t nf) {
    if (nv < 0 || nf < 0) return "nv and nf must be >= 0";
    if (nv >= 0x80000000LL) return "nv must be below 2^31";
    if (nf >= 0x80000000LL || 3 * nf >= 0x80000000LL) return "3*nf must be below 2^31";
    return nullptr;
}

inline int64_t ms_tiles(int64_t n) { return (n + GP_MESH_TILE - 1) / GP_MESH_TILE; }
inline int ms_bits(int64_t v) { int b = 0; while (v > 0) { ++b; v >>= 1; } return b < 1 ? 1 : b; }      // the bits of the largest key v

// byte offsets of the scratch's arrays, each 256-byte aligned.  sort_n: the pairs the sort buffers hold, max(3 nf, nv)
struct MsScratch {
    int64_t flags, vertex_count, face_count, keep_label, keep_vertex, keep_face, rank_vertex, rank_face, tile_vertex, tile_face, face_vectors, begin, end, sort_k[2], sort_v[2], sort_hist, sort_tmp, sort_n, sort_hist_elems, sort_tmp_elems, bytes;
};

inline MsScratch ms_scratch_layout(int64_t nv, int64_t nf, int64_t hist_elems, int64_t tmp_elems) {
    const auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    MsScratch s;
    int64_t at = 0;
    const auto take = [&](int64_t bytes) { const int64_t here = at; at += up(bytes); return here; };
    s.sort_n = 3 * nf > nv ? 3 * nf : nv;
    s.sort_hist_elems = hist_elems; s.sort_tmp_elems = tmp_elems;
    s.flags = take(4 * (GP_MESH_MAX_ROUNDS + 1));
    s.vertex_count = take(4 * nv);
    s.face_count = take(4 * nv);
    s.keep_label = take(nv);
    s.keep_vertex = take(nv);
    s.rank_vertex = take(4 * nv);
    s.tile_vertex = take(4 * ms_tiles(nv));
    s.begin = take(4 * nv);
    s.end = take(4 * nv);                            // (everything up to here lies where nv alone puts it: gp_mesh_gather_rows knows no nf)
    s.keep_face = take(nf);
    s.rank_face = take(4 * nf);
    s.tile_face = take(4 * ms_tiles(nf));
    s.face_vectors = take(12 * nf);
    for (int k = 0; k < 2; ++k) { s.sort_k[k] = take(4 * s.sort_n); s.sort_v[k] = take(4 * s.sort_n); }
    s.sort_hist = take(4 * hist_elems);
    s.sort_tmp = take(4 * tmp_elems);
    s.bytes = at;
    return s;
}
