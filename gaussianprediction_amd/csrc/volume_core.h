// volume_core.h -- the per-face, per-box, per-query and per-point programs of the signed-distance volumes (csrc/gp_volume.h), shared by
// the kernels of volume_kernels.hip and by the stand-alone CPU build the tests run under the sanitizers (tests/volume_emulate.cpp).
// The distance of a face is surface_core.h's sf_test and the sign sdf_core.h's sd_sign: no distance or sign arithmetic stands here.
//
//   vl_tree                            the levels of the tree of nf faces: their sizes and offsets, from nf and the leaf size alone
//   vl_morton, vl_key                  a face's sort key on the bounds of the usable corners
//   vl_leaf_box, vl_union              a leaf's box; the box of two boxes
//   vl_bound, vl_skip                  the bound of a box for a query; the skipping rule
//   vl_walk, vl_query                  one query: the stack, nearer child first
//   vl_point, vl_lattice_point         a lattice point; its signed distance
//   vl_compare                         one pair of values of two volumes
//   vl_refuse_*, vl_layout             the refusals and the scratch
// The file must be compiled with -ffp-contract=off: every operation rounds once.
#pragma once
#include "gp_volume.h"
#include "sdf_core.h"

#define VL_FN SF_FN
#define VL_BLOCK 256

// words of the scratch's head (uint32): the ordered bits of lo[3] and hi[3], then
#define VL_WORD_USABLE 6
#define VL_WORD_M 7                  // the bits of the largest |coordinate| (non-negative floats order as their bits)
#define VL_WORDS 16
#define VL_KEY_UNUSABLE 0x40000000u  // 2^30: beyond every Morton code
#define VL_KEY_BITS 31

struct alignas(16) VlBox { float lo[3]; int32_t pad0; float hi[3]; int32_t pad1; };
static_assert(sizeof(VlBox) == 32, "a box is two 16-byte loads");

// count[k], offset[k]: the boxes of level k and where they begin; level `levels - 1` holds one box
struct VlTree { uint32_t nf, leaf, levels, pad; uint32_t count[GP_VOLUME_MAX_LEVELS], offset[GP_VOLUME_MAX_LEVELS]; uint32_t boxes; };

inline VlTree vl_tree(int64_t nf, int64_t leaf) {
    VlTree t;
    t.nf = (uint32_t)nf; t.leaf = (uint32_t)leaf; t.pad = 0;
    for (int k = 0; k < GP_VOLUME_MAX_LEVELS; ++k) t.count[k] = t.offset[k] = 0;
    int64_t n = (nf + leaf - 1) / leaf, at = 0;
    if (n < 1) n = 1;
    uint32_t k = 0;
    for (;;) {                                     // (nf < 2^26: at most 27 levels)
        t.count[k] = (uint32_t)n; t.offset[k] = (uint32_t)at;
        at += n; ++k;
        if (n == 1 || k == GP_VOLUME_MAX_LEVELS) break;
        n = (n + 1) / 2;
    }
    t.levels = k; t.boxes = (uint32_t)at;
    return t;
}

// ---- the keys ----
VL_FN uint32_t vl_spread(uint32_t v) {             // the 10 bits of v, two zeros between each
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
VL_FN uint32_t vl_morton(uint32_t x, uint32_t y, uint32_t z) { return vl_spread(x) | (vl_spread(y) << 1) | (vl_spread(z) << 2); }

// bounds: the ordered bits of lo[3] then hi[3] of the usable corners (a usable record exists: they are finite)
VL_FN uint32_t vl_key(const SfFace& r, const uint32_t* bounds) {
    if (r.face < 0) return VL_KEY_UNUSABLE;
    uint32_t t[3];
    for (int k = 0; k < 3; ++k) {
        const float mn = fminf(r.a[k], fminf(r.b[k], r.c[k])), mx = fmaxf(r.a[k], fmaxf(r.b[k], r.c[k]));
        const double lo = (double)gm_unordered(bounds[k]), hi = (double)gm_unordered(bounds[3 + k]);
        const double c = 0.5 * ((double)mn + (double)mx), ext = hi - lo;
        double x = ext > 0.0 ? floor(((c - lo) / ext) * 1024.0) : 0.0;
        x = x > 0.0 ? (x < 1023.0 ? x : 1023.0) : 0.0;          // (a NaN goes to 0)
        t[k] = (uint32_t)x;
    }
    return vl_morton(t[0], t[1], t[2]);
}

// ---- the boxes ----
VL_FN void vl_empty(VlBox* b) {
    b->lo[0] = b->lo[1] = b->lo[2] = INFINITY; b->hi[0] = b->hi[1] = b->hi[2] = -INFINITY;
    b->pad0 = b->pad1 = 0;
}
VL_FN bool vl_is_empty(const VlBox& b) { return !(b.lo[0] <= b.hi[0]); }

// leaf i of the sorted records
VL_FN void vl_leaf_box(const SfFace* sorted, const VlTree& t, uint32_t i, VlBox* out) {
    VlBox b;
    vl_empty(&b);
    const uint64_t begin = (uint64_t)i * t.leaf, end = begin + t.leaf < t.nf ? begin + t.leaf : t.nf;
    for (uint64_t k = begin; k < end; ++k) {
        const SfFace& r = sorted[k];
        if (r.face < 0) continue;
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = fminf(b.lo[a], fminf(r.a[a], fminf(r.b[a], r.c[a])));
            b.hi[a] = fmaxf(b.hi[a], fmaxf(r.a[a], fmaxf(r.b[a], r.c[a])));
        }
    }
    *out = b;
}

// box i of level k >= 1 from level k - 1
VL_FN void vl_union(const VlBox* boxes, const VlTree& t, uint32_t k, uint32_t i, VlBox* out) {
    const VlBox* below = boxes + t.offset[k - 1];
    VlBox b = below[2 * (uint64_t)i];
    if (2 * (uint64_t)i + 1 < t.count[k - 1]) {
        const VlBox c = below[2 * (uint64_t)i + 1];
        for (int a = 0; a < 3; ++a) { b.lo[a] = fminf(b.lo[a], c.lo[a]); b.hi[a] = fmaxf(b.hi[a], c.hi[a]); }          // (an empty box is the identity)
    }
    *out = b;
}

// ---- the walk ----
// margin: 2^-47 * M
VL_FN double vl_bound(const VlBox& b, const double* q, double margin) {
    double g[3];
    for (int k = 0; k < 3; ++k) {
        const double below = (double)b.lo[k] - q[k], above = q[k] - (double)b.hi[k];
        double s = below > above ? below : above;
        s = s > 0.0 ? s : 0.0;
        s = s - margin;
        g[k] = s > 0.0 ? s : 0.0;
    }
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}
VL_FN bool vl_skip(double lb, double best) { return lb >= 0x1p-100 && lb * (1.0 - 0x1p-40) > best; }

struct VlEntry { double lb; uint32_t level, index; };

// the tallies of one query
struct VlTally { uint64_t nodes, candidates; int32_t stack, overflow; };

VL_FN void vl_walk(const VlTree& t, const VlBox* boxes, const SfFace* sorted, double margin, const double* q, SfBest& best, VlTally* tally) {
    VlEntry stack[GP_VOLUME_STACK];
    int sp = 0;
    const VlBox root = boxes[t.offset[t.levels - 1]];
    tally->nodes += 1;
    if (vl_is_empty(root)) return;
    stack[sp].lb = vl_bound(root, q, margin); stack[sp].level = t.levels - 1; stack[sp].index = 0; ++sp;
    tally->stack = 1;
    for (uint64_t trip = 0; sp > 0 && trip < 2 * (uint64_t)t.boxes + 2; ++trip) {          // (a box is popped once at the most)
        const VlEntry e = stack[--sp];
        if (vl_skip(e.lb, best.d)) continue;
        if (e.level == 0) {
            const uint64_t begin = (uint64_t)e.index * t.leaf, end = begin + t.leaf < t.nf ? begin + t.leaf : t.nf;
            for (uint64_t k = begin; k < end; ++k) sf_test(sorted[k], q, best);
            tally->candidates += end - begin;
            continue;
        }
        const uint32_t level = e.level - 1;
        const uint64_t c0 = 2 * (uint64_t)e.index;
        const VlBox* below = boxes + t.offset[level];
        double lb[2] = {0.0, 0.0};
        bool take[2] = {false, false};
        for (int c = 0; c < 2; ++c) {
            if (c0 + c >= t.count[level]) continue;
            const VlBox b = below[c0 + c];
            tally->nodes += 1;
            if (vl_is_empty(b)) continue;
            lb[c] = vl_bound(b, q, margin);
            take[c] = !vl_skip(lb[c], best.d);
        }
        const int first = (take[0] && take[1] && lb[1] < lb[0]) ? 1 : 0;          // the nearer child; equal bounds: the lower index
        for (int n = 1; n >= 0; --n) {                                             // the farther one is pushed first
            const int c = n == 0 ? first : 1 - first;
            if (!take[c]) continue;
            if (sp >= GP_VOLUME_STACK) { tally->overflow = 1; continue; }          // (cannot be: one box per level and one)
            stack[sp].lb = lb[c]; stack[sp].level = level; stack[sp].index = (uint32_t)(c0 + c); ++sp;
        }
        tally->stack = sp > tally->stack ? sp : tally->stack;
    }
}

// one query: gp_surface.h's row.  usable: the number of usable faces; M: the largest |coordinate| among their corners
VL_FN void vl_query(const VlTree& t, const VlBox* boxes, const SfFace* sorted, uint32_t usable, float M, const float* qf, float* dist2, int32_t* face, int32_t* region,
                    float* closest, float* bary, VlTally* tally) {
    tally->nodes = 0; tally->candidates = 0; tally->stack = 0; tally->overflow = 0;
    *dist2 = INFINITY; *face = -1; *region = 0;
    closest[0] = closest[1] = closest[2] = NAN;
    bary[0] = bary[1] = 0.f;
    if (!gm_usable(qf) || usable == 0) return;
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    SfBest best;
    best.d = (double)INFINITY; best.face = 0x7FFFFFFF; best.region = 0; best.u1 = best.u2 = 0.0;
    best.p[0] = best.p[1] = best.p[2] = 0.0;
    vl_walk(t, boxes, sorted, 0x1p-47 * (double)M, q, best, tally);
    *dist2 = (float)best.d;
    *face = best.face;
    *region = best.region;
    for (int k = 0; k < 3; ++k) closest[k] = (float)best.p[k];
    bary[0] = (float)best.u1; bary[1] = (float)best.u2;
}

// ---- the lattice ----
VL_FN float vl_coord(int32_t i, float voxel, float origin) { return fmaf((float)i, voxel, origin); }          // tsdf_core.h's ts_coord

VL_FN void vl_point(int64_t at, int32_t nx, int32_t ny, float ox, float oy, float oz, float voxel, float* p) {
    const int32_t i = (int32_t)(at % nx), j = (int32_t)((at / nx) % ny), k = (int32_t)(at / ((int64_t)nx * ny));
    p[0] = vl_coord(i, voxel, ox); p[1] = vl_coord(j, voxel, oy); p[2] = vl_coord(k, voxel, oz);
}

// the signed distance of one point; returns sd_sign's row, *kind and *sign as sd_sign leaves them
VL_FN int vl_lattice_point(const VlTree& t, const VlBox* boxes, const SfFace* sorted, uint32_t usable, float M, const float* p, const float* vertices, const int32_t* faces,
                           int64_t nv, int64_t nf, const int32_t* face_edges, const double* edge_normal, int64_t n_edges, const double* vertex_normal, float* sdf,
                           int8_t* sign, int32_t* kind, VlTally* tally) {
    float dist2, closest[3], bary[2];
    int32_t face, region, element;
    vl_query(t, boxes, sorted, usable, M, p, &dist2, &face, &region, closest, bary, tally);
    return sd_sign(p, dist2, face, region, vertices, faces, nv, nf, face_edges, edge_normal, n_edges, vertex_normal, sdf, sign, kind, &element);
}

// ---- the comparison: which of the first five count words a pair of values adds to (bits 0 .. 4) ----
VL_FN uint32_t vl_compare(float a, float b) {
    if (!ms_finite(a) || !ms_finite(b)) return 1u << GP_VOLUME_UNDETERMINED;
    const bool ia = a < 0.f, ib = b < 0.f;
    return (ia ? 1u << GP_VOLUME_INSIDE_A : 0u) | (ib ? 1u << GP_VOLUME_INSIDE_B : 0u) | ((ia && ib) ? 1u << GP_VOLUME_BOTH : 0u) | ((ia || ib) ? 1u << GP_VOLUME_EITHER : 0u);
}

// ---- refusals and the scratch ----
inline const char* vl_refuse_lattice(float ox, float oy, float oz, float voxel, int64_t nx, int64_t ny, int64_t nz) {
    if (!(ms_finite(ox) && ms_finite(oy) && ms_finite(oz) && ms_finite(voxel))) return "origin and voxel must be finite";
    if (!(voxel > 0.f)) return "voxel must be > 0";
    if (nx < 1 || ny < 1 || nz < 1) return "nx, ny and nz must be >= 1";
    if (nx >= 0x80000000LL || ny >= 0x80000000LL || nz >= 0x80000000LL || nx * ny >= 0x80000000LL || nx * ny * nz >= 0x80000000LL) return "nx*ny*nz must be below 2^31";
    return nullptr;
}

// [words: VL_WORDS uint32] [records: nf] [sorted: nf] [boxes] [sort keys and values: 4 x nf uint32] [hist] [tmp]; 256-byte aligned each
struct VlScratch { int64_t words, records, sorted, boxes, sort_k[2], sort_v[2], sort_hist, sort_tmp, sort_hist_elems, sort_tmp_elems, bytes; };

inline VlScratch vl_layout(int64_t nf, int64_t leaf, int64_t hist_elems, int64_t tmp_elems) {
    VlScratch s;
    int64_t at = 0;
    const auto take = [&](int64_t bytes) { const int64_t here = at; at += gm_up(bytes > 0 ? bytes : 1); return here; };
    s.sort_hist_elems = hist_elems; s.sort_tmp_elems = tmp_elems;
    s.words = take(4 * VL_WORDS);
    s.records = take((int64_t)sizeof(SfFace) * nf);
    s.sorted = take((int64_t)sizeof(SfFace) * nf);
    s.boxes = take((int64_t)sizeof(VlBox) * vl_tree(nf, leaf).boxes);
    for (int k = 0; k < 2; ++k) { s.sort_k[k] = take(4 * nf); s.sort_v[k] = take(4 * nf); }
    s.sort_hist = take(4 * hist_elems);
    s.sort_tmp = take(4 * tmp_elems);
    s.bytes = at;
    return s;
}
