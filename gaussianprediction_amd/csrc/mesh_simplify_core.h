// mesh_simplify_core.h -- the per-vertex, per-cluster and per-face programs of mesh simplification (csrc/gp_mesh_simplify.h), shared
// by the kernels of mesh_simplify_kernels.hip and by the stand-alone CPU build the tests run under the sanitizers
// (tests/mesh_simplify_emulate.cpp).  The checked face access, the face vector, the tile order and the size refusals are those of
// mesh_core.h.
//
//   mz_plan_grid                      the grid of a box and a voxel size, or the refusal
//   mz_bounds_start, mz_bounds_fold, mz_bounds_merge, mz_bounds_record       the exact bounds of the finite coordinates
//   mz_key                            a vertex's three key words (weld: its bits, -0.0 as +0.0; grid: its cell)
//   mz_sort_word, mz_is_head          the key word of a sort pass; whether a sorted position begins a run of equal keys
//   mz_segment                        the run a sorted position lies in, from the exclusive ranks of the heads
//   mz_contract                       one column of one cluster: the first member's bits or the float64 mean in member order
//   mz_face_class, mz_is_duplicate    collapsed, zero-area, the rotated triple; a copy of the face before it in sorted order
// The file must be compiled with -ffp-contract=off: every operation rounds once.
#pragma once
#include "gp_mesh_simplify.h"
#include "mesh_core.h"

#define MZ_FN MS_FN
#define MZ_BOUNDS_BLOCKS 256                 // the workgroups of the bounds' first launch at the most
#define MZ_BOUNDS_WORDS 8                    // a partial result: min xyz, max xyz, flag, 0 (float32)

#define MZ_KEPT 0                            // mz_face_class
#define MZ_SKIPPED 1
#define MZ_COLLAPSED 2
#define MZ_ZERO_AREA 3

struct MzGrid {
    int32_t mode;                            // GP_MESH_SIMPLIFY_WELD: nothing else is read but bits
    double origin[3], voxel;
    int32_t dims[3], bits[3];                // bits: what the sort of word a runs on
};

// ---- the grid ----
inline const char* mz_plan_grid(MzGrid& g, int32_t mode, double voxel_size, const double* bounds) {
    g.mode = mode;
    g.voxel = 1.0;
    for (int a = 0; a < 3; ++a) { g.origin[a] = 0.0; g.dims[a] = 1; g.bits[a] = 32; }
    if (mode == GP_MESH_SIMPLIFY_WELD) return nullptr;
    if (mode != GP_MESH_SIMPLIFY_GRID) return "mode must be GP_MESH_SIMPLIFY_WELD or GP_MESH_SIMPLIFY_GRID";
    if (!(fabs(voxel_size) < INFINITY) || !(voxel_size > 0.0)) return "voxel_size must be finite and > 0";
    if (!bounds) return "null argument (bounds)";
    for (int a = 0; a < 3; ++a)
        if (!(fabs(bounds[a]) < INFINITY) || !(fabs(bounds[3 + a]) < INFINITY) || bounds[a] > bounds[3 + a]) return "bounds must be finite with min <= max";
    g.voxel = voxel_size;
    for (int a = 0; a < 3; ++a) {
        g.origin[a] = bounds[a] - voxel_size / 2;
        const double dims = floor((bounds[3 + a] + voxel_size / 2 - g.origin[a]) / voxel_size) + 1.0;
        if (!(dims <= (double)GP_MESH_SIMPLIFY_MAX_DIM)) return "voxel_size is too small";
        g.dims[a] = dims < 1.0 ? 1 : (int32_t)dims;
        g.bits[a] = ms_bits(g.dims[a] - 1);
    }
    return nullptr;
}

// ---- the bounds: acc = min xyz, max xyz, flag, 0 ----
MZ_FN void mz_bounds_start(float* acc) {
    for (int a = 0; a < 3; ++a) { acc[a] = INFINITY; acc[3 + a] = -INFINITY; }
    acc[6] = 0.f; acc[7] = 0.f;
}
MZ_FN void mz_bounds_fold(float* acc, const float* p) {
    for (int a = 0; a < 3; ++a) {
        const float v = p[a];
        if (!ms_finite(v)) { acc[6] = 1.f; continue; }
        if (v < acc[a]) acc[a] = v;
        if (v > acc[3 + a]) acc[3 + a] = v;
    }
}
MZ_FN void mz_bounds_merge(float* acc, const float* other) {
    for (int a = 0; a < 3; ++a) {
        if (other[a] < acc[a]) acc[a] = other[a];
        if (other[3 + a] > acc[3 + a]) acc[3 + a] = other[3 + a];
    }
    if (other[6] != 0.f) acc[6] = 1.f;
}
MZ_FN void mz_bounds_record(const float* acc, double* record) {
    for (int a = 0; a < 6; ++a) record[a] = (double)acc[a] + 0.0;            // (-0.0 + 0.0 = +0.0: which zero the comparisons kept does not show)
    record[6] = acc[6] != 0.f ? 1.0 : 0.0;
    record[7] = 0.0;
}

// ---- keys ----
MZ_FN void mz_key(const MzGrid& g, const float* p, uint32_t* key, int32_t* state) {
    for (int a = 0; a < 3; ++a) {
        if (g.mode == GP_MESH_SIMPLIFY_WELD) {
            uint32_t w;
            memcpy(&w, p + a, 4);
            key[a] = w == 0x80000000u ? 0u : w;
        } else {
            const double q = floor(((double)p[a] - g.origin[a]) / g.voxel);
            const bool inside = q >= 0.0 && q < (double)g.dims[a];          // (false for a NaN: it never reaches the conversion)
            if (!inside) state[GP_MESH_SIMPLIFY_STATUS] = 1;
            key[a] = inside ? (uint32_t)(int32_t)q : 0u;
        }
    }
}

// the key of sorted position i in the pass over word a: `before` is the order the earlier passes left (null: 0, 1, 2, ...)
MZ_FN uint32_t mz_sort_word(const uint32_t* keys, const uint32_t* before, int64_t i, int a, uint32_t* element) {
    const uint32_t e = before ? before[i] : (uint32_t)i;
    *element = e;
    return keys[3 * (int64_t)e + a];
}

MZ_FN bool mz_same_key(const uint32_t* keys, uint32_t u, uint32_t v) {
    const uint32_t* a = keys + 3 * (int64_t)u;
    const uint32_t* b = keys + 3 * (int64_t)v;
    return a[0] == b[0] && a[1] == b[1] && a[2] == b[2];
}
MZ_FN bool mz_is_head(const uint32_t* keys, const uint32_t* order, int64_t i) { return i == 0 || !mz_same_key(keys, order[i], order[i - 1]); }

// rank: the heads before position i; the run of i is the last head at or before it
MZ_FN uint32_t mz_segment(uint32_t rank, bool head) { return head ? rank : rank - 1u; }          // (position 0 is a head: rank >= 1 elsewhere)

// ---- contraction of column j of rows [..][k] over members[begin .. end), end > begin ----
MZ_FN void mz_contract(const float* rows, int64_t k, int64_t j, const uint32_t* members, int64_t begin, int64_t end, int32_t contraction, float* out) {
    if (contraction != GP_MESH_SIMPLIFY_AVERAGE) {
        memcpy(out, rows + (int64_t)members[begin] * k + j, 4);             // (bits unchanged, a signalling NaN included)
        return;
    }
    double sum = 0.0;
    for (int64_t i = begin; i < end; ++i) sum = sum + (double)rows[(int64_t)members[i] * k + j];
    *out = (float)(sum / (double)(end - begin));
}

// ---- faces ----
// cluster: [nv]; positions: the contracted positions [C][3].  rot: the triple of clusters with its smallest first, (nv, nv, nv)
// where the face does not survive: those sort behind every face that does
MZ_FN int mz_face_class(const int32_t* faces, int64_t f, int64_t nv, const int32_t* cluster, const float* positions, int32_t drop_zero_area, int32_t* rot,
                        int32_t* state) {
    int32_t v[3];
    rot[0] = rot[1] = rot[2] = (int32_t)nv;
    if (!ms_face(faces, f, nv, v, state)) return MZ_SKIPPED;
    const int32_t g[3] = {cluster[v[0]], cluster[v[1]], cluster[v[2]]};
    if (g[0] == g[1] || g[1] == g[2] || g[0] == g[2]) return MZ_COLLAPSED;
    if (drop_zero_area) {
        float n[3];
        (void)ms_face_vector(positions, g, 0, nv, n, nullptr);              // (cluster numbers lie below C <= nv)
        if (n[0] == 0.f && n[1] == 0.f && n[2] == 0.f) return MZ_ZERO_AREA;
    }
    const int s = (g[0] < g[1] && g[0] < g[2]) ? 0 : (g[1] < g[2] ? 1 : 2);
    rot[0] = g[s]; rot[1] = g[(s + 1) % 3]; rot[2] = g[(s + 2) % 3];
    return MZ_KEPT;
}

// sorted position i of the faces under their rotated triples: a surviving face with the triple of the face before it
MZ_FN bool mz_is_duplicate(const uint32_t* rot, const uint32_t* order, int64_t i, int64_t nv) {
    if (i == 0 || rot[3 * (int64_t)order[i]] == (uint32_t)nv) return false;
    return mz_same_key(rot, order[i], order[i - 1]);
}

// ---- the scratch: byte offsets, each 256-byte aligned ----
struct MzScratch {
    int64_t words, partial, keys, members, head_pos, head_vertex, rank_pos, rank_vertex, tile_a, tile_b, seg_begin, seg_cluster, cluster, begin, end, positions,
        keep_cluster, rank_cluster, rot, keep_face, rank_face, tile_face, sort_k[2], sort_v[2], sort_hist, sort_tmp, sort_n, sort_hist_elems, sort_tmp_elems, bytes;
};
#define MZ_WORD_CLUSTERS 0                   // words[]: C, as the compaction of the heads over the vertices counted it
#define MZ_WORD_SPARE 1                      //          the same count over the sorted positions

inline MzScratch mz_scratch_layout(int64_t nv, int64_t nf, int64_t hist_elems, int64_t tmp_elems) {
    const auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    MzScratch s;
    int64_t at = 0;
    const auto take = [&](int64_t bytes) { const int64_t here = at; at += up(bytes); return here; };
    s.sort_n = nf > nv ? nf : nv;
    s.sort_hist_elems = hist_elems; s.sort_tmp_elems = tmp_elems;
    s.words = take(4 * 8);
    s.partial = take(4 * MZ_BOUNDS_WORDS * MZ_BOUNDS_BLOCKS);
    s.keys = take(12 * nv);
    s.members = take(4 * nv);
    s.head_pos = take(nv);
    s.head_vertex = take(nv);
    s.rank_pos = take(4 * nv);
    s.rank_vertex = take(4 * nv);
    s.tile_a = take(4 * ms_tiles(nv));
    s.tile_b = take(4 * ms_tiles(nv));
    s.seg_begin = take(4 * nv);
    s.seg_cluster = take(4 * nv);
    s.cluster = take(4 * nv);
    s.begin = take(4 * nv);
    s.end = take(4 * nv);
    s.positions = take(12 * nv);
    s.keep_cluster = take(nv);
    s.rank_cluster = take(4 * nv);
    s.rot = take(12 * nf);
    s.keep_face = take(nf);
    s.rank_face = take(4 * nf);
    s.tile_face = take(4 * ms_tiles(nf));
    for (int k = 0; k < 2; ++k) { s.sort_k[k] = take(4 * s.sort_n); s.sort_v[k] = take(4 * s.sort_n); }
    s.sort_hist = take(4 * hist_elems);
    s.sort_tmp = take(4 * tmp_elems);
    s.bytes = at;
    return s;
}
