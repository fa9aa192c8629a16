// surface_core.h -- the per-face and per-query programs of the point-to-surface distance (csrc/gp_surface.h), shared by the kernels of
// surface_kernels.hip and by the stand-alone CPU build the tests run under the sanitizers (tests/surface_emulate.cpp).  Every formula
// of the header stands here once; the grid record, the cell function and the ordered bits are geometry_core.h's.
//
//   sf_record                          a face's record: nine floats and its number, or -1 where it is not usable
//   sf_auto_cells, sf_derive           round(sqrt(usable) / 4); the grid record (geometry_core.h's formulas with that rule)
//   sf_box, sf_box_cells               the cells a face is registered in
//   sf_edge, sf_interior, sf_test      the candidates of one face against one query; the lexicographic minimum
//   sf_query                           one query: the wide list, the rings, the spans, the stopping rule, the sweep
//   sf_refuse_*, sf_layout             the refusals and the scratch
// The file must be compiled with -ffp-contract=off: every operation rounds once.
#pragma once
#include "gp_surface.h"
#include "geometry_core.h"

#define SF_FN GM_FN
#define SF_BLOCK GM_BLOCK
#define SF_TILE GM_TILE
#define SF_PER_LANE GM_PER_LANE

// words of the scratch's head (uint32): the ordered bits of lo[3] and hi[3], then the counters
#define SF_WORD_USABLE 6
#define SF_WORD_WIDE 7
#define SF_WORD_STATUS 8
#define SF_WORD_PAIRS 9
#define SF_WORDS 16

struct alignas(16) SfFace { float a[3], b[3], c[3]; int32_t face; int32_t pad[2]; };
static_assert(sizeof(SfFace) == 48, "a candidate is three 16-byte loads");

// ---- the faces ----
SF_FN bool sf_record(const float* vertices, const int32_t* faces, int64_t f, int64_t nv, SfFace* r) {
    int32_t v[3];
    bool ok = ms_face(faces, f, nv, v, nullptr);
    for (int k = 0; k < 3; ++k) {
        r->a[k] = ok ? vertices[3 * (int64_t)v[0] + k] : 0.f;
        r->b[k] = ok ? vertices[3 * (int64_t)v[1] + k] : 0.f;
        r->c[k] = ok ? vertices[3 * (int64_t)v[2] + k] : 0.f;
    }
    ok = ok && gm_usable(r->a) && gm_usable(r->b) && gm_usable(r->c);
    r->face = ok ? (int32_t)f : -1;
    r->pad[0] = r->pad[1] = 0;
    return ok;
}

// round(sqrt(usable) / 4) in integers, clamped to 1 .. 1024: DESIGN section 31's measured choice
SF_FN int64_t sf_auto_cells(int64_t usable) {
    int64_t r = 0;
    while (16 * (r + 1) * (r + 1) <= usable) ++r;                       // (usable < 2^26: r < 2048)
    if (4 * (2 * r + 1) * (2 * r + 1) <= usable) ++r;
    return r < 1 ? 1 : (r > GP_GEOMETRY_MAX_AXIS ? GP_GEOMETRY_MAX_AXIS : r);
}

// gm_derive with the rule above.  bounds: the ordered bits of lo[3] then hi[3] (only read where usable > 0)
SF_FN void sf_derive(const uint32_t* bounds, int64_t usable, int64_t nf, float cell, GmGrid* g) {
    double ext[3] = {0.0, 0.0, 0.0}, E = 0.0;
    for (int a = 0; a < 3; ++a) {
        g->lo[a] = usable > 0 ? gm_unordered(bounds[a]) : 0.f;
        if (usable > 0) ext[a] = (double)gm_unordered(bounds[3 + a]) - (double)g->lo[a];
        if (ext[a] > E) E = ext[a];
    }
    g->usable = (int32_t)usable; g->excluded = (int32_t)(nf - usable); g->pad[0] = g->pad[1] = 0;
    g->dims[0] = g->dims[1] = g->dims[2] = 1; g->cells = 1; g->inv = 0.f; g->size = (double)INFINITY;
    if (!(E > 0.0)) return;
    int64_t R;
    if (cell > 0.f) {
        const double c = ceil(E / (double)cell);
        R = c < 1.0 ? 1 : (c > (double)GP_GEOMETRY_MAX_AXIS ? GP_GEOMETRY_MAX_AXIS : (int64_t)c);
    } else {
        R = sf_auto_cells(usable);
    }
    for (;;) {
        const float inv = (float)((double)R / E);
        if (!(inv >= 0x1p-96f && inv <= 0x1p96f)) return;          // (one cell)
        const double size = 1.0 / (double)inv;
        int64_t d[3], cells = 1;
        for (int a = 0; a < 3; ++a) {
            d[a] = (int64_t)floor(ext[a] / size) + 1;
            d[a] = d[a] < 1 ? 1 : (d[a] > R ? R : d[a]);
            cells *= d[a];
        }
        if (cells <= GP_GEOMETRY_MAX_CELLS) {
            for (int a = 0; a < 3; ++a) g->dims[a] = (int32_t)d[a];
            g->cells = (int32_t)cells; g->inv = inv; g->size = size;
            return;
        }
        R = (R + 1) / 2;
    }
}

// the box of a usable face: lo[3], hi[3] in cells
SF_FN void sf_box(const GmGrid& g, const SfFace& r, int32_t* lo, int32_t* hi) {
    for (int k = 0; k < 3; ++k) {
        const int32_t ca = gm_cell(r.a[k], g.lo[k], g.inv, g.dims[k]), cb = gm_cell(r.b[k], g.lo[k], g.inv, g.dims[k]), cc = gm_cell(r.c[k], g.lo[k], g.inv, g.dims[k]);
        lo[k] = ca < cb ? (ca < cc ? ca : cc) : (cb < cc ? cb : cc);
        hi[k] = ca > cb ? (ca > cc ? ca : cc) : (cb > cc ? cb : cc);
    }
}
SF_FN int64_t sf_box_cells(const int32_t* lo, const int32_t* hi) { return (int64_t)(hi[0] - lo[0] + 1) * (int64_t)(hi[1] - lo[1] + 1) * (int64_t)(hi[2] - lo[2] + 1); }
SF_FN uint32_t sf_key(const GmGrid& g, int32_t x, int32_t y, int32_t z) { return ((uint32_t)z * (uint32_t)g.dims[1] + (uint32_t)y) * (uint32_t)g.dims[0] + (uint32_t)x; }

// ---- one face against one query ----
struct SfBest { double d, p[3], u1, u2; int32_t face, region; };

SF_FN double sf_dot(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }
SF_FN void sf_cross(const double* x, const double* y, double* out) {
    out[0] = x[1] * y[2] - x[2] * y[1];
    out[1] = x[2] * y[0] - x[0] * y[2];
    out[2] = x[0] * y[1] - x[1] * y[0];
}

// the candidate of the segment (s, t): its distance, point and parameter
SF_FN double sf_edge(const double* q, const double* s, const double* t, double* p, double* tau) {
    double e[3], w[3], r[3];
    for (int k = 0; k < 3; ++k) { e[k] = t[k] - s[k]; w[k] = q[k] - s[k]; }
    const double l2 = sf_dot(e, e);
    double x = 0.0;
    if (l2 > 0.0) {
        x = sf_dot(w, e) / l2;
        x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
    }
    for (int k = 0; k < 3; ++k) { p[k] = s[k] + e[k] * x; r[k] = q[k] - p[k]; }
    *tau = x;
    return sf_dot(r, r);
}

// the interior candidate; false where there is none
SF_FN bool sf_interior(const double* q, const double* a, const double* b, const double* c, double* p, double* u, double* v, double* d) {
    double e1[3], e2[3], w[3], n[3], t[3], r[3];
    for (int k = 0; k < 3; ++k) { e1[k] = b[k] - a[k]; e2[k] = c[k] - a[k]; w[k] = q[k] - a[k]; }
    sf_cross(e1, e2, n);
    const double nn = sf_dot(n, n);
    if (!(nn > 0.0)) return false;
    sf_cross(w, e2, t);
    *u = sf_dot(t, n) / nn;
    sf_cross(e1, w, t);
    *v = sf_dot(t, n) / nn;
    if (!(*u >= 0.0 && *v >= 0.0 && *u + *v <= 1.0)) return false;
    for (int k = 0; k < 3; ++k) { p[k] = (a[k] + e1[k] * *u) + e2[k] * *v; r[k] = q[k] - p[k]; }
    *d = sf_dot(r, r);
    return true;
}

// the face's (d, region), joined into best by (d, face)
SF_FN void sf_test(const SfFace& rec, const double* q, SfBest& best) {
    if (rec.face < 0) return;
    const double a[3] = {(double)rec.a[0], (double)rec.a[1], (double)rec.a[2]};
    const double b[3] = {(double)rec.b[0], (double)rec.b[1], (double)rec.b[2]};
    const double c[3] = {(double)rec.c[0], (double)rec.c[1], (double)rec.c[2]};
    double p[3], pk[3], u = 0.0, v = 0.0, d = (double)INFINITY, tau;
    int32_t region = 0;
    const bool inside = sf_interior(q, a, b, c, p, &u, &v, &d);
    double dk = sf_edge(q, a, b, pk, &tau);
    if (!inside || dk < d) { d = dk; region = 1; u = tau; v = 0.0; p[0] = pk[0]; p[1] = pk[1]; p[2] = pk[2]; }
    dk = sf_edge(q, b, c, pk, &tau);
    if (dk < d) { d = dk; region = 2; u = 1.0 - tau; v = tau; p[0] = pk[0]; p[1] = pk[1]; p[2] = pk[2]; }
    dk = sf_edge(q, c, a, pk, &tau);
    if (dk < d) { d = dk; region = 3; u = 0.0; v = 1.0 - tau; p[0] = pk[0]; p[1] = pk[1]; p[2] = pk[2]; }
    if (d < best.d || (d == best.d && rec.face < best.face)) {
        best.d = d; best.face = rec.face; best.region = region; best.u1 = u; best.u2 = v;
        best.p[0] = p[0]; best.p[1] = p[1]; best.p[2] = p[2];
    }
}

SF_FN void sf_visit(const SfFace* records, const int32_t* pairs, uint32_t begin, uint32_t end, const double* q, SfBest& best) {
    for (uint32_t k = begin; k < end; ++k) sf_test(records[pairs[k]], q, best);
}

// one query.  refused: the fill was refused (every result is the empty row).  *visited: the records tested; *ring: the last ring walked;
// *swept: 1 where the walk ended with the pass over all records
SF_FN void sf_query(const GmGrid& g, int64_t nf, bool refused, const uint32_t* start, const int32_t* pairs, const SfFace* records, const int32_t* wide, uint32_t nwide,
                    const float* qf, float* dist2, int32_t* face, int32_t* region, float* closest, float* bary, uint64_t* visited, int32_t* ring, int32_t* swept) {
    *visited = 0; *ring = 0; *swept = 0;
    *dist2 = INFINITY; *face = -1; *region = 0;
    closest[0] = closest[1] = closest[2] = NAN;
    bary[0] = bary[1] = 0.f;
    if (refused || !gm_usable(qf) || g.usable <= 0) return;
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    const int32_t cx = gm_cell(qf[0], g.lo[0], g.inv, g.dims[0]), cy = gm_cell(qf[1], g.lo[1], g.inv, g.dims[1]), cz = gm_cell(qf[2], g.lo[2], g.inv, g.dims[2]);
    const int32_t dx = g.dims[0], dy = g.dims[1], dz = g.dims[2];
    SfBest best;
    best.d = (double)INFINITY; best.face = 0x7FFFFFFF; best.region = 0; best.u1 = best.u2 = 0.0;
    best.p[0] = best.p[1] = best.p[2] = 0.0;
    uint64_t seen = nwide;
    int64_t looked = 0;
    for (uint32_t k = 0; k < nwide; ++k) sf_test(records[wide[k]], q, best);
    for (int32_t r = 0;; ++r) {
        const int32_t x0 = cx - r < 0 ? 0 : cx - r, x1 = cx + r > dx - 1 ? dx - 1 : cx + r;
        const int32_t y0 = cy - r < 0 ? 0 : cy - r, y1 = cy + r > dy - 1 ? dy - 1 : cy + r;
        const int32_t z0 = cz - r < 0 ? 0 : cz - r, z1 = cz + r > dz - 1 ? dz - 1 : cz + r;
        for (int32_t z = z0; z <= z1; ++z)
            for (int32_t y = y0; y <= y1; ++y) {
                const uint32_t row = ((uint32_t)z * (uint32_t)dy + (uint32_t)y) * (uint32_t)dx;
                if (z == cz - r || z == cz + r || y == cy - r || y == cy + r) {          // a row of a z face or a y face: one span
                    const uint32_t b = start[row + x0], e = start[row + x1 + 1];
                    sf_visit(records, pairs, b, e, q, best);
                    seen += e - b; ++looked;
                } else {                                                                  // (r >= 1 here) the two cells of the x faces
                    if (cx - r >= 0) {
                        const uint32_t b = start[row + cx - r], e = start[row + cx - r + 1];
                        sf_visit(records, pairs, b, e, q, best);
                        seen += e - b; ++looked;
                    }
                    if (cx + r <= dx - 1) {
                        const uint32_t b = start[row + cx + r], e = start[row + cx + r + 1];
                        sf_visit(records, pairs, b, e, q, best);
                        seen += e - b; ++looked;
                    }
                }
            }
        *ring = r;
        if (cx - r <= 0 && cx + r >= dx - 1 && cy - r <= 0 && cy + r >= dy - 1 && cz - r <= 0 && cz + r >= dz - 1) break;      // (a) the grid is covered
        const double s = (double)r * g.size * (1.0 - 0x1p-10);
        const double B = s * s;
        if (B >= 0x1p-100 && best.d <= B) break;                                                                              // (b)
        if (looked >= (int64_t)g.usable) {                                                                                    // (c)
            for (int64_t f = 0; f < nf; ++f) sf_test(records[f], q, best);
            seen += (uint64_t)nf;
            *swept = 1;
            break;
        }
    }
    *visited = seen;
    *dist2 = (float)best.d;
    *face = best.face;
    *region = best.region;
    for (int k = 0; k < 3; ++k) closest[k] = (float)best.p[k];
    bary[0] = (float)best.u1; bary[1] = (float)best.u2;
}

// ---- refusals and the scratch ----
inline const char* sf_refuse_grid(int64_t nf, float cell) {
    const char* why = gm_refuse_mesh(0, nf);
    if (!why && (!(cell >= 0.f) || !ms_finite(cell))) why = "cell must be finite and >= 0 (0: the automatic rule)";
    return why;
}
inline const char* sf_refuse_wide(int32_t wide_cells) {
    return (wide_cells < 1 || wide_cells > GP_SURFACE_MAX_WIDE_CELLS) ? "wide_cells must be 1 .. 64" : nullptr;
}

// the cells the scratch has room for: what sf_derive can choose with at most nf usable faces
inline int64_t sf_cell_capacity(int64_t nf, float cell) {
    if (cell > 0.f) return GP_GEOMETRY_MAX_CELLS;
    const int64_t r = sf_auto_cells(nf), c = r * r * r;
    return c > GP_GEOMETRY_MAX_CELLS ? GP_GEOMETRY_MAX_CELLS : c;
}
// [words: SF_WORDS uint32] [GmGrid] [start: cap + 1 uint32] [cursor: cap + 1 uint32] [tile sums] [records: nf] [wide: nf int32]
struct SfScratch { int64_t words, grid, start, cursor, sums, records, wide, cap, bytes; };
inline SfScratch sf_layout(int64_t nf, float cell) {
    SfScratch s;
    s.cap = sf_cell_capacity(nf, cell);
    s.words = 0;
    s.grid = 64;
    s.start = 256;
    s.cursor = s.start + gm_up(4 * (s.cap + 1));
    s.sums = s.cursor + gm_up(4 * (s.cap + 1));
    s.records = s.sums + gm_up(4 * (gm_tiles(s.cap + 1) + 1));
    s.wide = s.records + gm_up((int64_t)sizeof(SfFace) * nf);
    s.bytes = s.wide + gm_up(4 * nf);
    return s;
}
