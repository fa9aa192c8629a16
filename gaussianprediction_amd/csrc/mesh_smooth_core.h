// mesh_smooth_core.h -- the per-entry, per-run and per-vertex programs of mesh topology and smoothing (csrc/gp_mesh_smooth.h), shared by
// the kernels of mesh_smooth_kernels.hip and by the stand-alone CPU build the tests run under the sanitizers
// (tests/mesh_smooth_emulate.cpp).  The checked face access and the size refusals are those of mesh_core.h.
//
//   mt_refuse_sizes                   gp_mesh.h's refusals and 6*nf below 2^31
//   mt_face_tally                     a face: kept or skipped (the status word), its degenerate half-edges
//   mt_entry, mt_sort_word            directed entry j = 6 f + 2 corner + direction: its two ends; the key word of a sort pass
//   mt_is_head, mt_starts_vertex      a sorted position begins a run of equal pairs; begins the entries of its first end
//   mt_run                            face_count and wind of the run that begins at a sorted position
//   mt_lower_bound                    offsets[v] among the first ends of the heads
//   mt_flags                          a vertex's three bits
//   mt_mean, mt_step, mt_umbrella     one vertex and column of a smoothing step
// The file must be compiled with -ffp-contract=off: every operation rounds once.
#pragma once
#include "gp_mesh_smooth.h"
#include "mesh_core.h"

#define MT_FN MS_FN
#define MT_DIRECTION 0x80000000u             // second[]: the entry is the reverse of its half-edge (it runs second -> first)

inline const char* mt_refuse_sizes(int64_t nv, int64_t nf) {
    const char* why = ms_refuse_sizes(nv, nf);
    if (why) return why;
    if (6 * nf >= 0x80000000LL) return "6*nf must be below 2^31";
    return nullptr;
}

inline const char* mt_refuse_rows(int64_t nv, int64_t k) {
    if (nv < 0 || nv >= 0x80000000LL) return "nv must be 0 .. 2^31 - 1";
    if (k < 1 || k > 1024) return "k must be 1 .. 1024";
    if (nv * k >= 0x80000000LL) return "nv*k must be below 2^31";
    return nullptr;
}

inline const char* mt_refuse_options(int32_t method, int32_t boundary, int32_t iterations, double lambda_, double mu) {
    if (method != GP_MESH_SMOOTH_LAPLACIAN && method != GP_MESH_SMOOTH_TAUBIN) return "method must be \"laplacian\" or \"taubin\"";
    if (boundary != GP_MESH_SMOOTH_FREE && boundary != GP_MESH_SMOOTH_FIXED) return "boundary must be \"fixed\" or \"free\"";
    if (iterations < 0 || iterations > GP_MESH_SMOOTH_MAX_ITERATIONS) return "iterations must be 0 .. 10000";
    if (!(fabs(lambda_) < INFINITY) || !(fabs(mu) < INFINITY)) return "lambda_ and mu must be finite";
    return nullptr;
}

// ---- faces and directed entries ----
// true for a kept face; *degenerate: its half-edges with equal ends
MT_FN bool mt_face_tally(const int32_t* faces, int64_t f, int64_t nv, int32_t* state, int32_t* degenerate) {
    int32_t v[3];
    *degenerate = 0;
    if (!ms_face(faces, f, nv, v, state)) return false;
    *degenerate = (v[0] == v[1]) + (v[1] == v[2]) + (v[2] == v[0]);
    return true;
}

// entry j: half-edge `corner` of face j / 6 as (from, to) for direction 0 and (to, from) for direction 1; (nv, nv) where the face is
// skipped or the half-edge dropped
MT_FN void mt_entry(const int32_t* faces, int64_t j, int64_t nv, uint32_t* first, uint32_t* second) {
    int32_t v[3];
    const int corner = (int)((j % 6) / 2);
    *first = *second = (uint32_t)nv;
    if (!ms_face(faces, j / 6, nv, v, nullptr)) return;
    const int32_t a = v[corner], b = v[(corner + 1) % 3];
    if (a == b) return;
    *first = (uint32_t)((j & 1) ? b : a);
    *second = (uint32_t)((j & 1) ? a : b);
}

// the key of sorted position i in the pass over word w (1: the second end, sorted first; 0: the first end): `before` is the order the
// earlier pass left (null: 0, 1, 2, ...)
MT_FN uint32_t mt_sort_word(const int32_t* faces, const uint32_t* before, int64_t i, int w, int64_t nv, uint32_t* element) {
    const uint32_t e = before ? before[i] : (uint32_t)i;
    uint32_t first, second;
    *element = e;
    mt_entry(faces, e, nv, &first, &second);
    return w == 0 ? first : second;
}

// ---- the sorted entries: first[i] (nv: not an entry), second[i] with MT_DIRECTION ----
MT_FN uint32_t mt_end(uint32_t second) { return second & ~MT_DIRECTION; }
MT_FN bool mt_is_head(const uint32_t* first, const uint32_t* second, int64_t i, int64_t nv) {
    if (first[i] >= (uint32_t)nv) return false;
    return i == 0 || first[i - 1] != first[i] || mt_end(second[i - 1]) != mt_end(second[i]);
}
MT_FN bool mt_starts_vertex(const uint32_t* first, int64_t i, int64_t nv) { return first[i] < (uint32_t)nv && (i == 0 || first[i - 1] != first[i]); }

// the run of equal pairs that begins at i, a head with first < second: lo = first, hi = second
MT_FN void mt_run(const uint32_t* first, const uint32_t* second, int64_t i, int64_t n, int32_t* face_count, int32_t* wind) {
    const uint32_t lo = first[i], hi = mt_end(second[i]);
    int32_t count = 0, w = 0;
    for (int64_t p = i; p < n && first[p] == lo && mt_end(second[p]) == hi; ++p) {
        count += 1;
        w += (second[p] & MT_DIRECTION) ? -1 : 1;
    }
    *face_count = count;
    *wind = w;
}
MT_FN bool mt_is_boundary(int32_t face_count) { return face_count == 1; }
MT_FN bool mt_is_nonmanifold(int32_t face_count) { return face_count > 2; }
MT_FN bool mt_is_inconsistent(int32_t face_count, int32_t wind) { return face_count == 2 && wind != 0; }

// the first position of src[0 .. n) (ascending) whose value is not below v
MT_FN int64_t mt_lower_bound(const uint32_t* src, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)src[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

MT_FN uint8_t mt_flags(uint8_t boundary, uint8_t nonmanifold, int64_t degree) {
    return (uint8_t)((boundary ? GP_MESH_SMOOTH_FLAG_BOUNDARY : 0) | (nonmanifold ? GP_MESH_SMOOTH_FLAG_NONMANIFOLD : 0) | (degree == 0 ? GP_MESH_SMOOTH_FLAG_ISOLATED : 0));
}

// ---- smoothing ----
MT_FN bool mt_is_pinned(const uint8_t* pinned, uint8_t mask, int64_t v) { return mask != 0 && (pinned[v] & mask) != 0; }

// the mean of column a over the neighbours of v, in their order; false for degree 0 and for a list that is not one of this mesh
MT_FN bool mt_mean(const float* src, int64_t nv, int64_t k, int64_t v, int64_t a, const int32_t* offsets, const int32_t* neighbors, int64_t n_neighbors, double* m) {
    const int64_t begin = offsets[v], end = offsets[v + 1];
    if (begin < 0 || end > n_neighbors || end <= begin) return false;
    double sum = 0.0;
    for (int64_t i = begin; i < end; ++i) {
        const int32_t u = neighbors[i];
        if (!ms_index_ok(u, nv)) return false;
        sum = sum + (double)src[(int64_t)u * k + a];
    }
    *m = sum / (double)(end - begin);
    return true;
}

MT_FN void mt_step(const float* src, int64_t nv, int64_t k, int64_t v, int64_t a, const int32_t* offsets, const int32_t* neighbors, int64_t n_neighbors,
                   const uint8_t* pinned, uint8_t mask, double s, float* dst) {
    const float* p = src + v * k + a;
    double m;
    if (mt_is_pinned(pinned, mask, v) || !mt_mean(src, nv, k, v, a, offsets, neighbors, n_neighbors, &m)) {
        memcpy(dst + v * k + a, p, 4);                // (bits unchanged, a signalling NaN included)
        return;
    }
    const double pd = (double)*p;
    double t = m - pd;
    t = s * t;
    dst[v * k + a] = (float)(pd + t);
}

MT_FN void mt_umbrella(const float* src, int64_t nv, int64_t k, int64_t v, int64_t a, const int32_t* offsets, const int32_t* neighbors, int64_t n_neighbors, float* dst) {
    double m;
    dst[v * k + a] = mt_mean(src, nv, k, v, a, offsets, neighbors, n_neighbors, &m) ? (float)(m - (double)src[v * k + a]) : 0.f;
}

// the factor of step `step` (0 ..) of a method
MT_FN double mt_factor(int32_t method, int64_t step, double lambda_, double mu) { return (method == GP_MESH_SMOOTH_TAUBIN && (step & 1)) ? mu : lambda_; }
MT_FN int64_t mt_steps(int32_t method, int64_t iterations) { return method == GP_MESH_SMOOTH_TAUBIN ? 2 * iterations : iterations; }

// ---- the scratch of the edges entries: byte offsets, each 256-byte aligned.  n6 = 6 nf ----
struct MtScratch {
    int64_t words, first, second, head_adj, head_edge, rank_adj, rank_edge, tile_adj, tile_edge, adj_src, mark_boundary, mark_nonmanifold, sort_k[2], sort_v[2], sort_hist,
        sort_tmp, sort_hist_elems, sort_tmp_elems, bytes;
};
#define MT_WORD_ADJ 0                        // words[]: 2E, the heads of all runs

inline MtScratch mt_scratch_layout(int64_t nv, int64_t nf, int64_t hist_elems, int64_t tmp_elems) {
    const auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    MtScratch s;
    int64_t at = 0;
    const auto take = [&](int64_t bytes) { const int64_t here = at; at += up(bytes); return here; };
    const int64_t n6 = 6 * nf;
    s.sort_hist_elems = hist_elems; s.sort_tmp_elems = tmp_elems;
    s.words = take(4 * 8);
    s.first = take(4 * n6);
    s.second = take(4 * n6);
    s.head_adj = take(n6);
    s.head_edge = take(n6);
    s.rank_adj = take(4 * n6);
    s.rank_edge = take(4 * n6);
    s.tile_adj = take(4 * ms_tiles(n6));
    s.tile_edge = take(4 * ms_tiles(n6));
    s.adj_src = take(4 * n6);
    s.mark_boundary = take(nv);
    s.mark_nonmanifold = take(nv);
    for (int k = 0; k < 2; ++k) { s.sort_k[k] = take(4 * n6); s.sort_v[k] = take(4 * n6); }
    s.sort_hist = take(4 * hist_elems);
    s.sort_tmp = take(4 * tmp_elems);
    s.bytes = at;
    return s;
}
