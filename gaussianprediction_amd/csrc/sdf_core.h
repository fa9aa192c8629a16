// sdf_core.h -- the per-face, per-run and per-query programs of the signed distance (csrc/gp_sdf.h), shared by the kernels of
// sdf_kernels.hip and by the stand-alone CPU build the tests run under the sanitizers (tests/sdf_emulate.cpp).  Every formula of the
// header stands here once; the candidates of a face against a query are surface_core.h's own functions.
//
//   sd_refuse_*                        the refusals
//   sd_face, sd_find_edge              a contributing face; the number of a side among the ascending edges, by bisection
//   sd_face_program                    one face: its record (u_f and the three angles), face_edges, the keys of its six entries, its volume term
//   sd_is_head, sd_walk_vertex, sd_walk_edge       a sorted position begins a run; one lane's walk of a run, in ascending entry
//   sd_tree                            the fixed tree of a block of 256 terms
//   sd_sign                            one query: the candidate again, the closest feature, its normal, the sign
// The file must be compiled with -ffp-contract=off: every operation rounds once.
#pragma once
#include "gp_sdf.h"
#include "surface_core.h"

#define SD_FN SF_FN
#define SD_BLOCK 256

// what sd_sign says of its query (one of)
#define SD_ROW_EXCLUDED 0
#define SD_ROW_FOREIGN 1
#define SD_ROW_SIGNED 2

struct SdFace { double u[3], angle[3]; };              // u_f; the angle at each corner (only read where u_f was made)
static_assert(sizeof(SdFace) == 48, "a face's record");

inline const char* sd_refuse_tables(int64_t nv, int64_t nf, int64_t n_edges) {
    const char* why = gm_refuse_mesh(nv, nf);
    if (why) return why;
    if (n_edges < 0 || n_edges > 3 * nf) return "n_edges must be 0 .. 3*nf";
    return nullptr;
}
inline const char* sd_refuse_sign(int64_t nq, int64_t nv, int64_t nf, int64_t n_edges) {
    const char* why = gm_refuse_count(nq);
    if (why) return why;
    return sd_refuse_tables(nv, nf, n_edges);
}

// ---- the faces ----
// the indices of a contributing face; *bad: an index lies outside [0, nv)
SD_FN bool sd_face(const int32_t* faces, int64_t f, int64_t nv, int32_t* v, bool* bad) {
    const bool ok = ms_face(faces, f, nv, v, nullptr);
    *bad = !ok;
    return ok && v[0] != v[1] && v[1] != v[2] && v[2] != v[0];
}

// the number of the pair (a, b), a != b, in edge[n_edges][2] (ascending lexicographic pairs lo < hi); -1 where it is not there
SD_FN int32_t sd_find_edge(const int32_t* edge, int64_t n_edges, int32_t a, int32_t b) {
    const int32_t x = a < b ? a : b, y = a < b ? b : a;
    int64_t lo = 0, hi = n_edges;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        const int32_t ex = edge[2 * mid], ey = edge[2 * mid + 1];
        if (ex < x || (ex == x && ey < y)) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n_edges && edge[2 * lo] == x && edge[2 * lo + 1] == y) ? (int32_t)lo : -1;
}

SD_FN void sd_corner(const float* vertices, int32_t v, double* out) {
    out[0] = (double)vertices[3 * (int64_t)v]; out[1] = (double)vertices[3 * (int64_t)v + 1]; out[2] = (double)vertices[3 * (int64_t)v + 2];
}

// u_f of the corners a, b, c; false (and zeros) where nn > 0 is false
SD_FN bool sd_unit_normal(const double* a, const double* b, const double* c, double* u) {
    double e1[3], e2[3], n[3];
    for (int k = 0; k < 3; ++k) { e1[k] = b[k] - a[k]; e2[k] = c[k] - a[k]; }
    sf_cross(e1, e2, n);
    const double nn = sf_dot(n, n);
    u[0] = u[1] = u[2] = 0.0;
    if (!(nn > 0.0)) return false;
    const double len = sqrt(nn);
    for (int k = 0; k < 3; ++k) u[k] = n[k] / len;
    return true;
}

// the angle at corner `at` between the sides to `next` and to `prev`
SD_FN double sd_angle(const double* at, const double* next, const double* prev) {
    double e1[3], e2[3], x[3];
    for (int k = 0; k < 3; ++k) { e1[k] = next[k] - at[k]; e2[k] = prev[k] - at[k]; }
    sf_cross(e1, e2, x);
    return atan2(sqrt(sf_dot(x, x)), sf_dot(e1, e2));
}

// one face.  face_edges: its three words; corner_key, side_key: the keys of entries 3f .. 3f + 2 (nv and n_edges: no entry); *term: its
// volume term; *bad, *skipped, *zero_area; *missing: its sides that `edge` does not hold
SD_FN void sd_face_program(const float* vertices, const int32_t* faces, int64_t f, int64_t nv, const int32_t* edge, int64_t n_edges, int32_t* face_edges, SdFace* rec,
                           uint32_t* corner_key, uint32_t* side_key, double* term, bool* bad, bool* skipped, bool* zero_area, int32_t* missing) {
    int32_t v[3];
    const bool contributes = sd_face(faces, f, nv, v, bad);
    *skipped = !contributes; *zero_area = false; *missing = 0; *term = 0.0;
    for (int k = 0; k < 3; ++k) {
        rec->u[k] = 0.0; rec->angle[k] = 0.0;
        corner_key[k] = (uint32_t)nv; side_key[k] = (uint32_t)n_edges;
        face_edges[k] = -1;
        if (*bad) continue;
        const int32_t s = v[k], t = v[(k + 1) % 3];
        if (s == t) continue;
        face_edges[k] = sd_find_edge(edge, n_edges, s, t);
        if (face_edges[k] < 0) *missing += 1;
    }
    if (!contributes) return;
    double p[3][3], x[3];
    for (int k = 0; k < 3; ++k) sd_corner(vertices, v[k], p[k]);
    sf_cross(p[1], p[2], x);
    *term = sf_dot(p[0], x) / 6.0;
    if (!sd_unit_normal(p[0], p[1], p[2], rec->u)) { *zero_area = true; return; }
    for (int k = 0; k < 3; ++k) {
        rec->angle[k] = sd_angle(p[k], p[(k + 1) % 3], p[(k + 2) % 3]);
        corner_key[k] = (uint32_t)v[k];
        if (face_edges[k] >= 0) side_key[k] = (uint32_t)face_edges[k];
    }
}

// ---- the sorted entries: key[i] (limit: no entry), entry[i] = 3f + k, ascending inside a run ----
SD_FN bool sd_is_head(const uint32_t* key, int64_t i, uint32_t limit) { return key[i] < limit && (i == 0 || key[i - 1] != key[i]); }

SD_FN void sd_walk_vertex(const uint32_t* key, const uint32_t* entry, int64_t i, int64_t n, const SdFace* records, double* out) {
    const uint32_t v = key[i];
    double sum[3] = {0.0, 0.0, 0.0};
    for (int64_t p = i; p < n && key[p] == v; ++p) {
        const uint32_t e = entry[p] < (uint32_t)n ? entry[p] : 0u;          // (a permutation of 0 .. n - 1: the values the sort was handed)
        const SdFace& r = records[e / 3u];
        const double angle = r.angle[e % 3u];
        for (int k = 0; k < 3; ++k) {
            const double t = angle * r.u[k];
            sum[k] = sum[k] + t;
        }
    }
    out[0] = sum[0]; out[1] = sum[1]; out[2] = sum[2];
}

SD_FN void sd_walk_edge(const uint32_t* key, const uint32_t* entry, int64_t i, int64_t n, const SdFace* records, double* out) {
    const uint32_t v = key[i];
    double sum[3] = {0.0, 0.0, 0.0};
    for (int64_t p = i; p < n && key[p] == v; ++p) {
        const uint32_t e = entry[p] < (uint32_t)n ? entry[p] : 0u;
        const SdFace& r = records[e / 3u];
        for (int k = 0; k < 3; ++k) sum[k] = sum[k] + r.u[k];
    }
    out[0] = sum[0]; out[1] = sum[1]; out[2] = sum[2];
}

// x[0 .. SD_BLOCK): the block's terms; leaves the partial in x[0].  (The device runs every level on its lanes, a barrier between levels.)
SD_FN void sd_tree(double* x) {
    for (int d = SD_BLOCK / 2; d >= 1; d >>= 1)
        for (int i = 0; i < d; ++i) x[i] = x[i] + x[i + d];
}

// ---- one query ----
SD_FN float sd_root(float dist2) { return (float)sqrt((double)dist2); }

// returns SD_ROW_*; for SD_ROW_SIGNED *kind and *sign say which words of the stats the row counts in
SD_FN int sd_sign(const float* qf, float dist2, int32_t face, int32_t region, const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const int32_t* face_edges,
                  const double* edge_normal, int64_t n_edges, const double* vertex_normal, float* sdf, int8_t* sign, int32_t* kind, int32_t* element) {
    *sign = 0; *kind = -1; *element = -1;
    if (face == -1) { *sdf = INFINITY; return SD_ROW_EXCLUDED; }
    *sdf = sd_root(dist2);
    int32_t v[3];
    if (face < 0 || face >= nf || region < 0 || region > 3 || !ms_face(faces, face, nv, v, nullptr)) return SD_ROW_FOREIGN;
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    double c[3][3], p[3], N[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k) sd_corner(vertices, v[k], c[k]);
    if (region == 0) {
        double bu, bv, d;
        if (!sf_interior(q, c[0], c[1], c[2], p, &bu, &bv, &d)) return SD_ROW_FOREIGN;
        sd_unit_normal(c[0], c[1], c[2], N);
        *kind = GP_SDF_KIND_FACE; *element = face;
    } else {
        const int s = region - 1, t = region % 3;
        double tau, e[3];
        sf_edge(q, c[s], c[t], p, &tau);
        for (int k = 0; k < 3; ++k) e[k] = c[t][k] - c[s][k];
        const double l2 = sf_dot(e, e);
        if (!(l2 > 0.0) || tau == 0.0 || v[s] == v[t]) { *kind = GP_SDF_KIND_VERTEX; *element = v[s]; }
        else if (tau == 1.0) { *kind = GP_SDF_KIND_VERTEX; *element = v[t]; }
        else {
            const int32_t e_number = face_edges[3 * (int64_t)face + s];
            if (e_number < -1 || e_number >= n_edges) return SD_ROW_FOREIGN;
            *kind = GP_SDF_KIND_EDGE; *element = e_number;
        }
        const double* table = *kind == GP_SDF_KIND_VERTEX ? vertex_normal : edge_normal;
        if (*element >= 0)
            for (int k = 0; k < 3; ++k) N[k] = table[3 * (int64_t)*element + k];
    }
    double r[3];
    for (int k = 0; k < 3; ++k) r[k] = q[k] - p[k];
    const double g = sf_dot(r, N);
    *sign = g < 0.0 ? -1 : (g > 0.0 ? 1 : 0);
    if (*sign < 0) *sdf = -*sdf;
    return SD_ROW_SIGNED;
}

// ---- the scratch of gp_sdf_tables: byte offsets, each 256-byte aligned.  n3 = 3 nf ----
struct SdScratch { int64_t records, side_key, partials, sort_k[2], sort_v[2], sort_hist, sort_tmp, sort_hist_elems, sort_tmp_elems, blocks, bytes; };

inline int64_t sd_blocks(int64_t n) { return (n + SD_BLOCK - 1) / SD_BLOCK; }

inline SdScratch sd_scratch_layout(int64_t nf, int64_t hist_elems, int64_t tmp_elems) {
    SdScratch s;
    int64_t at = 0;
    const auto take = [&](int64_t bytes) { const int64_t here = at; at += gm_up(bytes); return here; };
    const int64_t n3 = 3 * nf;
    s.sort_hist_elems = hist_elems; s.sort_tmp_elems = tmp_elems;
    s.blocks = sd_blocks(nf);
    s.records = take((int64_t)sizeof(SdFace) * nf);
    s.side_key = take(4 * n3);
    s.partials = take(8 * (s.blocks > 0 ? s.blocks : 1));
    for (int k = 0; k < 2; ++k) { s.sort_k[k] = take(4 * n3); s.sort_v[k] = take(4 * n3); }
    s.sort_hist = take(4 * hist_elems);
    s.sort_tmp = take(4 * tmp_elems);
    s.bytes = at;
    return s;
}
