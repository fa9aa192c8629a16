// geometry_core.h -- the per-face, per-sample, per-point, per-query and per-entry programs of the geometry metrics (csrc/gp_geometry.h),
// shared by the kernels of geometry_kernels.hip and by the stand-alone CPU build the tests run under the sanitizers
// (tests/geometry_emulate.cpp).  Every formula of the header stands here once.
//
//   gm_hash                            splitmix64's finaliser over (seed, i, k)
//   gm_face_area, gm_scale, gm_weight  a face's class and float64 area; the power of two of the largest; the integer weight
//   gm_sample_head, gm_sample          T, q and the refusal; one sample: its face by binary search, its barycentrics, its point
//   gm_interpolate                     attributes through a sample's weights
//   gm_usable, gm_auto_cells, gm_derive, gm_cell, gm_key       a usable point; the grid record; the cell function; the linear key
//   gm_query                           one query: the rings, the spans, the stopping rule, the sweep
//   gm_terms, gm_row                   one entry's twelve terms; the totals -> the table
//   gm_refuse_*, gm_*_layout           the refusals and the scratches
// The file must be compiled with -ffp-contract=off: every operation rounds once.
#pragma once
#include "gp_geometry.h"
#include "mesh_core.h"

#define GM_FN MS_FN
#define GM_BLOCK 256
#define GM_TILE 1024                          // elements per workgroup of the scans and of the metric tiles
#define GM_PER_LANE (GM_TILE / GM_BLOCK)
#define GM_TERMS 12                           // per direction: count, sum, sum2, max, within[8]
#define GM_MAX_BLOCKS 2048                    // the workgroups of a grid-stride launch at the most: 8 on each of 256 CUs

#define GM_FACE_OK 0                          // gm_face_area
#define GM_FACE_BAD_INDEX 1
#define GM_FACE_NON_FINITE 2

// ---- samples ----
GM_FN uint64_t gm_hash(uint64_t seed, uint64_t i, uint32_t k) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (3ull * i + k + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

GM_FN int gm_face_area(const float* vertices, const int32_t* faces, int64_t f, int64_t nv, double* area) {
    int32_t v[3];
    *area = 0.0;
    if (!ms_face(faces, f, nv, v, nullptr)) return GM_FACE_BAD_INDEX;
    const float* a = vertices + 3 * (int64_t)v[0];
    const float* b = vertices + 3 * (int64_t)v[1];
    const float* c = vertices + 3 * (int64_t)v[2];
    for (int k = 0; k < 3; ++k)
        if (!(ms_finite(a[k]) && ms_finite(b[k]) && ms_finite(c[k]))) return GM_FACE_NON_FINITE;
    const double ex = (double)b[0] - (double)a[0], ey = (double)b[1] - (double)a[1], ez = (double)b[2] - (double)a[2];
    const double gx = (double)c[0] - (double)a[0], gy = (double)c[1] - (double)a[1], gz = (double)c[2] - (double)a[2];
    const double nx = ey * gz - ez * gy, ny = ez * gx - ex * gz, nz = ex * gy - ey * gx;
    *area = sqrt((nx * nx + ny * ny) + nz * nz);
    return GM_FACE_OK;
}

GM_FN uint64_t gm_double_bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }      // (areas are >= 0: their bits order as they do)
GM_FN double gm_bits_double(uint64_t b) { double v; memcpy(&v, &b, 8); return v; }

// 2^(36 - E) for the largest area m = 1.xxx * 2^E, given as its bits; 0 where m == 0
GM_FN double gm_scale(uint64_t max_bits) {
    if (max_bits == 0) return 0.0;
    const int64_t e = (int64_t)((max_bits >> 52) & 0x7FF) - 1023;
    return gm_bits_double((uint64_t)(1023 + GP_GEOMETRY_WEIGHT_BITS - e) << 52);
}
GM_FN uint64_t gm_weight(double area, double scale) { return (uint64_t)(area * scale); }      // (below 2^37)

struct GmSampleHead { uint64_t total, q; int32_t status, pad; };

GM_FN GmSampleHead gm_sample_head(uint64_t total, int64_t n) {
    GmSampleHead h;
    h.total = total; h.pad = 0;
    h.status = total == 0 ? GP_GEOMETRY_REFUSED_EMPTY : (total < (uint64_t)n ? GP_GEOMETRY_REFUSED_TOO_MANY : 0);
    h.q = h.status ? 0 : total / (uint64_t)n;
    return h;
}

GM_FN float gm_mix3(float a, float b, float c, float u1, float u2) {
    float t1 = b - a;
    t1 = t1 * u1;
    t1 = t1 + a;
    float t2 = c - a;
    t2 = t2 * u2;
    return t1 + t2;
}

GM_FN void gm_sample(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const uint64_t* prefix, const GmSampleHead& h, uint64_t seed, int64_t i,
                     float* point, int32_t* face, float* bary) {
    int32_t v[3];
    int64_t lo = 0, hi = nf - 1;
    bool ok = h.status == 0 && nf > 0;
    if (ok) {
        const uint64_t t = (uint64_t)i * h.q + gm_hash(seed, (uint64_t)i, 0) % h.q;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (prefix[mid] > t) hi = mid; else lo = mid + 1;
        }
        ok = ms_face(faces, lo, nv, v, nullptr);          // (a face of weight > 0: its indices were in range)
    }
    if (!ok) {
        point[3 * i] = point[3 * i + 1] = point[3 * i + 2] = NAN;
        face[i] = -1;
        bary[2 * i] = bary[2 * i + 1] = 0.f;
        return;
    }
    uint32_t k1 = (uint32_t)(gm_hash(seed, (uint64_t)i, 1) >> 40), k2 = (uint32_t)(gm_hash(seed, (uint64_t)i, 2) >> 40);
    if (k1 + k2 > (1u << 24)) { k1 = (1u << 24) - k1; k2 = (1u << 24) - k2; }
    const float u1 = (float)k1 * 0x1p-24f, u2 = (float)k2 * 0x1p-24f;
    const float* a = vertices + 3 * (int64_t)v[0];
    const float* b = vertices + 3 * (int64_t)v[1];
    const float* c = vertices + 3 * (int64_t)v[2];
    for (int k = 0; k < 3; ++k) point[3 * i + k] = gm_mix3(a[k], b[k], c[k], u1, u2);
    face[i] = (int32_t)lo;
    bary[2 * i] = u1; bary[2 * i + 1] = u2;
}

GM_FN void gm_interpolate(const float* attributes, int32_t C, const int32_t* faces, int64_t nv, int64_t nf, const int32_t* face, const float* bary, int64_t i,
                          float* out) {
    int32_t v[3];
    const int32_t f = face[i];
    const bool ok = f >= 0 && f < nf && ms_face(faces, f, nv, v, nullptr);
    for (int32_t c = 0; c < C; ++c)
        out[i * C + c] = ok ? gm_mix3(attributes[(int64_t)v[0] * C + c], attributes[(int64_t)v[1] * C + c], attributes[(int64_t)v[2] * C + c], bary[2 * i], bary[2 * i + 1]) : 0.f;
}

// ---- the grid ----
struct alignas(16) GmRecord { float x, y, z; int32_t index; };
static_assert(sizeof(GmRecord) == 16, "a candidate is one 16-byte load");

struct GmGrid {
    double size;                              // of a cell, 1 / inv; +inf for one cell
    float lo[3], inv;
    int32_t dims[3], cells;
    int32_t usable, excluded, pad[2];
};

GM_FN bool gm_usable(const float* p) { return ms_finite(p[0]) && ms_finite(p[1]) && ms_finite(p[2]); }

// order-preserving bits of a float, for integer atomic minima and maxima of finite values
GM_FN uint32_t gm_ordered(float v) { uint32_t b; memcpy(&b, &v, 4); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
GM_FN float gm_unordered(uint32_t o) { const uint32_t b = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o; float v; memcpy(&v, &b, 4); return v; }

// round(1.5 * cbrt(usable)) in integers, clamped to 1 .. 1024: 1.5 is DESIGN section 30's measured choice
GM_FN int64_t gm_auto_cells(int64_t usable) {
    int64_t r = 1;
    while (8 * (r + 1) * (r + 1) * (r + 1) <= 27 * usable) ++r;          // (usable < 2^31: r <= 1935)
    if ((2 * r + 1) * (2 * r + 1) * (2 * r + 1) <= 27 * usable) ++r;
    return r > GP_GEOMETRY_MAX_AXIS ? GP_GEOMETRY_MAX_AXIS : r;
}

// bounds: the ordered bits of lo[3] then hi[3] (only read where usable > 0)
GM_FN void gm_derive(const uint32_t* bounds, int64_t usable, int64_t np, float cell, GmGrid* g) {
    double ext[3] = {0.0, 0.0, 0.0}, E = 0.0;
    for (int a = 0; a < 3; ++a) {
        g->lo[a] = usable > 0 ? gm_unordered(bounds[a]) : 0.f;
        if (usable > 0) ext[a] = (double)gm_unordered(bounds[3 + a]) - (double)g->lo[a];
        if (ext[a] > E) E = ext[a];
    }
    g->usable = (int32_t)usable; g->excluded = (int32_t)(np - usable); g->pad[0] = g->pad[1] = 0;
    g->dims[0] = g->dims[1] = g->dims[2] = 1; g->cells = 1; g->inv = 0.f; g->size = (double)INFINITY;
    if (!(E > 0.0)) return;
    int64_t R;
    if (cell > 0.f) {
        const double c = ceil(E / (double)cell);
        R = c < 1.0 ? 1 : (c > (double)GP_GEOMETRY_MAX_AXIS ? GP_GEOMETRY_MAX_AXIS : (int64_t)c);
    } else {
        R = gm_auto_cells(usable);
    }
    for (;;) {
        const float inv = (float)((double)R / E);
        if (!(inv >= 0x1p-96f && inv <= 0x1p96f)) return;          // (one cell)
        const double size = 1.0 / (double)inv;
        int64_t d[3], cells = 1;
        for (int a = 0; a < 3; ++a) {
            d[a] = (int64_t)floor(ext[a] / size) + 1;                 // (ext / size <= R * (1 + 2^-23))
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

GM_FN int32_t gm_cell(float x, float lo, float inv, int32_t dims) {
    const float t = floorf((x - lo) * inv);
    return t > 0.f ? (t < (float)(dims - 1) ? (int32_t)t : dims - 1) : 0;
}
GM_FN uint32_t gm_key(const GmGrid& g, const float* p) {
    const int32_t x = gm_cell(p[0], g.lo[0], g.inv, g.dims[0]), y = gm_cell(p[1], g.lo[1], g.inv, g.dims[1]), z = gm_cell(p[2], g.lo[2], g.inv, g.dims[2]);
    return ((uint32_t)z * (uint32_t)g.dims[1] + (uint32_t)y) * (uint32_t)g.dims[0] + (uint32_t)x;
}

struct GmBest { float d; int32_t j; };

GM_FN void gm_visit(const GmRecord* records, uint32_t begin, uint32_t end, float qx, float qy, float qz, GmBest& best) {
    for (uint32_t k = begin; k < end; ++k) {
        const GmRecord p = records[k];
        const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (d < best.d || (d == best.d && p.index < best.j)) { best.d = d; best.j = p.index; }
    }
}

// one query.  *visited: the candidates compared; *ring: the last ring walked; *swept: 1 where the walk ended with the pass over all records
GM_FN void gm_query(const GmGrid& g, const uint32_t* start, const GmRecord* records, const float* q, float* dist2, int32_t* index, uint64_t* visited, int32_t* ring,
                    int32_t* swept) {
    *visited = 0; *ring = 0; *swept = 0;
    *dist2 = INFINITY; *index = -1;
    if (!gm_usable(q) || g.usable <= 0) return;
    const float qx = q[0], qy = q[1], qz = q[2];
    const int32_t cx = gm_cell(qx, g.lo[0], g.inv, g.dims[0]), cy = gm_cell(qy, g.lo[1], g.inv, g.dims[1]), cz = gm_cell(qz, g.lo[2], g.inv, g.dims[2]);
    const int32_t dx = g.dims[0], dy = g.dims[1], dz = g.dims[2];
    GmBest best;
    best.d = INFINITY; best.j = 0x7FFFFFFF;
    uint64_t seen = 0;
    int64_t looked = 0;
    for (int32_t r = 0;; ++r) {
        const int32_t x0 = cx - r < 0 ? 0 : cx - r, x1 = cx + r > dx - 1 ? dx - 1 : cx + r;
        const int32_t y0 = cy - r < 0 ? 0 : cy - r, y1 = cy + r > dy - 1 ? dy - 1 : cy + r;
        const int32_t z0 = cz - r < 0 ? 0 : cz - r, z1 = cz + r > dz - 1 ? dz - 1 : cz + r;
        for (int32_t z = z0; z <= z1; ++z)
            for (int32_t y = y0; y <= y1; ++y) {
                const uint32_t row = ((uint32_t)z * (uint32_t)dy + (uint32_t)y) * (uint32_t)dx;
                if (z == cz - r || z == cz + r || y == cy - r || y == cy + r) {          // a row of a z face or a y face: one span
                    const uint32_t b = start[row + x0], e = start[row + x1 + 1];
                    gm_visit(records, b, e, qx, qy, qz, best);
                    seen += e - b; ++looked;
                } else {                                                                  // (r >= 1 here) the two cells of the x faces
                    if (cx - r >= 0) {
                        const uint32_t b = start[row + cx - r], e = start[row + cx - r + 1];
                        gm_visit(records, b, e, qx, qy, qz, best);
                        seen += e - b; ++looked;
                    }
                    if (cx + r <= dx - 1) {
                        const uint32_t b = start[row + cx + r], e = start[row + cx + r + 1];
                        gm_visit(records, b, e, qx, qy, qz, best);
                        seen += e - b; ++looked;
                    }
                }
            }
        *ring = r;
        if (cx - r <= 0 && cx + r >= dx - 1 && cy - r <= 0 && cy + r >= dy - 1 && cz - r <= 0 && cz + r >= dz - 1) break;      // (a) the grid is covered
        const double s = (double)r * g.size * (1.0 - 0x1p-10);
        const double B = s * s;
        if (B >= 0x1p-100 && (double)best.d <= B) break;                                                                      // (b)
        if (looked >= (int64_t)g.usable) {                                                                                    // (c)
            gm_visit(records, 0, (uint32_t)g.usable, qx, qy, qz, best);
            seen += (uint32_t)g.usable;
            *swept = 1;
            break;
        }
    }
    *visited = seen;
    *dist2 = best.d;
    *index = best.j == 0x7FFFFFFF ? -1 : best.j;
}

// ---- metrics ----
struct GmThresholds { float v[GP_GEOMETRY_MAX_THRESHOLDS]; int32_t nt; };

// the twelve terms of one entry (zeros where it does not count)
GM_FN void gm_terms(float d2, const GmThresholds& th, double* t) {
    const bool counts = ms_finite(d2);
    const double dist = counts ? sqrt((double)d2) : 0.0;
    t[0] = counts ? 1.0 : 0.0;
    t[1] = dist;
    t[2] = counts ? (double)d2 : 0.0;
    t[3] = dist;
    for (int k = 0; k < GP_GEOMETRY_MAX_THRESHOLDS; ++k) t[4 + k] = (counts && k < th.nt && dist <= (double)th.v[k]) ? 1.0 : 0.0;
}
GM_FN double gm_join(int term, double a, double b) { return term == 3 ? (a > b ? a : b) : a + b; }

// s: the totals of a -> b then b -> a, twelve each
GM_FN void gm_row(const double* s, int32_t nt, double* row) {
    const double* ab = s;
    const double* ba = s + GM_TERMS;
    for (int k = 0; k < 4; ++k) { row[GP_GEOMETRY_COUNT_AB + k] = ab[k]; row[GP_GEOMETRY_COUNT_BA + k] = ba[k]; }
    const double acc = ab[1] / ab[0], com = ba[1] / ba[0];
    row[GP_GEOMETRY_ACCURACY] = acc;
    row[GP_GEOMETRY_COMPLETENESS] = com;
    row[GP_GEOMETRY_CHAMFER_L1] = (acc + com) / 2.0;
    row[GP_GEOMETRY_CHAMFER_L2] = ab[2] / ab[0] + ba[2] / ba[0];
    row[GP_GEOMETRY_HAUSDORFF] = (ab[0] > 0.0 && ba[0] > 0.0) ? (ab[3] > ba[3] ? ab[3] : ba[3]) : (double)NAN;
    for (int k = 0; k < GP_GEOMETRY_MAX_THRESHOLDS; ++k) {
        const double p = k < nt ? ab[4 + k] / ab[0] : 0.0, r = k < nt ? ba[4 + k] / ba[0] : 0.0;
        row[GP_GEOMETRY_PRECISION + k] = p;
        row[GP_GEOMETRY_RECALL + k] = r;
        row[GP_GEOMETRY_FSCORE + k] = (p + r > 0.0) ? 2.0 * p * r / (p + r) : 0.0;
    }
}

// ---- refusals and the scratches ----
inline const char* gm_refuse_mesh(int64_t nv, int64_t nf) {
    if (nv < 0 || nf < 0) return "nv and nf must be >= 0";
    if (nv >= 0x80000000LL) return "nv must be below 2^31";
    if (nf >= GP_GEOMETRY_MAX_FACES) return "nf must be below 2^26";
    return nullptr;
}
inline const char* gm_refuse_count(int64_t n) { return (n < 0 || n >= 0x80000000LL) ? "the number of samples, queries or entries must be 0 .. 2^31 - 1" : nullptr; }
inline const char* gm_refuse_cloud(int64_t np, float cell) {
    if (np < 0 || np >= 0x7FFFFFFFLL) return "np must be 0 .. 2^31 - 2";
    if (!(cell >= 0.f) || !ms_finite(cell)) return "cell must be finite and >= 0 (0: the automatic rule)";
    return nullptr;
}

inline int64_t gm_up(int64_t bytes) { return (bytes + 255) / 256 * 256; }
inline int64_t gm_tiles(int64_t n) { return (n + GM_TILE - 1) / GM_TILE; }

// samples: [head: the bits of the largest area (8 bytes), GmSampleHead] [prefix: nf uint64] [tile sums: tiles + 1 uint64]
struct GmSampleScratch { int64_t head, prefix, sums, bytes; };
inline GmSampleScratch gm_sample_layout(int64_t nf) {
    GmSampleScratch s;
    s.head = 0;
    s.prefix = 256;
    s.sums = s.prefix + gm_up(8 * nf);
    s.bytes = s.sums + gm_up(8 * (gm_tiles(nf) + 1));
    return s;
}

// the cells the scratch has room for: what gm_derive can choose with at most np usable points
inline int64_t gm_cell_capacity(int64_t np, float cell) {
    if (cell > 0.f) return GP_GEOMETRY_MAX_CELLS;
    const int64_t r = gm_auto_cells(np), c = r * r * r;
    return c > GP_GEOMETRY_MAX_CELLS ? GP_GEOMETRY_MAX_CELLS : c;
}
// the grid: [bounds: 6 uint32, usable: 1 int32] [GmGrid] [start: cap + 1 uint32] [cursor: cap + 1 uint32] [tile sums] [records: np]
struct GmGridScratch { int64_t bounds, grid, start, cursor, sums, records, cap, bytes; };
inline GmGridScratch gm_grid_layout(int64_t np, float cell) {
    GmGridScratch s;
    s.cap = gm_cell_capacity(np, cell);
    s.bounds = 0;
    s.grid = 64;
    s.start = 256;
    s.cursor = s.start + gm_up(4 * (s.cap + 1));
    s.sums = s.cursor + gm_up(4 * (s.cap + 1));
    s.records = s.sums + gm_up(4 * (gm_tiles(s.cap + 1) + 1));
    s.bytes = s.records + gm_up(16 * np);
    return s;
}
static_assert(sizeof(GmGrid) <= 192, "the record fits between the bounds and the starts");

// metrics: the slots of a -> b, then of b -> a
inline int64_t gm_metrics_bytes(int64_t n_ab, int64_t n_ba) { return gm_up(8 * GM_TERMS * (gm_tiles(n_ab) + gm_tiles(n_ba)) + 256); }
