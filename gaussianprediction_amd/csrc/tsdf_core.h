// tsdf_core.h -- the per-voxel, per-edge and per-cell programs of TSDF fusion and mesh extraction (csrc/gp_tsdf.h), shared by the
// kernels of tsdf_kernels.hip and by the stand-alone CPU build the tests run under the sanitizers (tests/tsdf_emulate.cpp).
//
//   ts_integrate_view   one view into one grid point's registers (TsVoxel)
//   ts_cell_active      the active byte of the cell whose corner 000 a point is
//   ts_edge_marks       the seven crossing bits of a point's own edges;  ts_corners_inside: the eight INSIDE bits of a point's cell
//   ts_cell_triangles   how many triangles those bits give;  ts_cell_faces: the triangles themselves, as vertex numbers
//   ts_vertex           the vertex of one crossing edge
//   ts_tile_point       the point a lane of a tile's workgroup takes in its step u;  ts_chunk: that point's 64-point chunk in the tile
//   ts_refuse_grid      the size checks, as text (NULL: accepted);  ts_scratch_layout: where the arrays of the scratch begin
// The file must be compiled with -ffp-contract=off: every operation rounds once.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gp_tsdf.h"

#if defined(__HIPCC__)
#define TS_FN __host__ __device__ inline
#else
#define TS_FN inline
#endif

#define TS_BLOCK 256
#define TS_PER_LANE (GP_TSDF_TILE / TS_BLOCK)
#define TS_CHUNKS (GP_TSDF_TILE / 64)               // the 64-point chunks of a tile: one wave scan each

TS_FN bool ts_finite(float v) { return fabsf(v) < INFINITY; }            // (false for a NaN)

// the grid as the kernels take it, by value
struct TsGrid {
    int32_t nx, ny, nz;
    float ox, oy, oz, voxel;
};

TS_FN int64_t ts_points(const TsGrid& g) { return (int64_t)g.nx * g.ny * g.nz; }
TS_FN float ts_coord(int32_t i, float voxel, float origin) { return fmaf((float)i, voxel, origin); }
// the linear offset of the corner `bits` (x = 1, y = 2, z = 4) from a cell's corner 000
TS_FN int32_t ts_offset(const TsGrid& g, int bits) { return (bits & 1) + ((bits >> 1) & 1) * g.nx + ((bits >> 2) & 1) * g.nx * g.ny; }
// whether the corner `bits` of the cell at (i, j, k) is a grid point
TS_FN bool ts_exists(const TsGrid& g, int32_t i, int32_t j, int32_t k, int bits) {
    return i + (bits & 1) < g.nx && j + ((bits >> 1) & 1) < g.ny && k + ((bits >> 2) & 1) < g.nz;
}

// ---- integrate ----
struct TsVoxel { float tsdf, w, c[3]; };

// one axis of the projection: the pixel column (row) of P_a / P_z, or -1 where it is outside or not finite
TS_FN int32_t ts_pixel(float Pa, float Pz, float tanfov, int32_t size) {
    const float an = Pa / (Pz * tanfov);
    const float pa = ((an + 1.f) * (float)size - 1.f) * 0.5f;
    const float fa = floorf(pa + 0.5f);
    if (!(ts_finite(fa) && fa >= 0.f && fa < (float)size)) return -1;
    return (int32_t)fa;
}

// depth, valid, image: the view's own planes ([H][W], [H][W] or NULL, [3][H][W] or NULL: a volume without colour); m: its world_view
TS_FN void ts_integrate_view(TsVoxel& p, float x, float y, float z, const float* m, float tanfovx, float tanfovy, const float* depth,
                             const uint8_t* valid, const float* image, int32_t H, int32_t W, float trunc, float z_min, float view_weight,
                             float weight_max) {
    const float Px = fmaf(m[0], x, fmaf(m[4], y, fmaf(m[8], z, m[12])));
    const float Py = fmaf(m[1], x, fmaf(m[5], y, fmaf(m[9], z, m[13])));
    const float Pz = fmaf(m[2], x, fmaf(m[6], y, fmaf(m[10], z, m[14])));
    if (!(Pz > z_min)) return;
    const int32_t ix = ts_pixel(Px, Pz, tanfovx, W), iy = ts_pixel(Py, Pz, tanfovy, H);
    if (ix < 0 || iy < 0) return;
    const size_t plane = (size_t)H * W, at = (size_t)iy * W + ix;
    const float d = depth[at];
    if (!((!valid || valid[at] != 0) && ts_finite(d) && d > 0.f)) return;
    const float s = d - Pz;
    if (s < -trunc) return;
    const float t = fminf(1.f, s / trunc);
    const float wn = p.w + view_weight;
    p.tsdf = (p.tsdf * p.w + t * view_weight) / wn;
    if (image) {
        for (int c = 0; c < 3; ++c) p.c[c] = (p.c[c] * p.w + image[c * plane + at] * view_weight) / wn;
    }
    p.w = fminf(wn, weight_max);
}

// ---- extraction ----
TS_FN bool ts_usable(float tsdf, float weight, float min_weight) { return weight >= min_weight && ts_finite(tsdf); }

// the direction of edge e as corner bits, and the edge of a direction
TS_FN int ts_edge_bits(int e) { return (0x7653421 >> (4 * e)) & 7; }                    // 1, 2, 4, 3, 5, 6, 7
TS_FN int ts_edge_of_bits(int bits) { return (0x65423100 >> (4 * bits)) & 7; }          // 1 -> 0, 2 -> 1, 3 -> 3, 4 -> 2, 5 -> 4, 6 -> 5, 7 -> 6

TS_FN uint8_t ts_cell_active(const float* tsdf, const float* weight, const TsGrid& g, int64_t n, int32_t i, int32_t j, int32_t k, float min_weight) {
    if (!ts_exists(g, i, j, k, 7)) return 0;
    for (int b = 0; b < 8; ++b) {
        const int64_t q = n + ts_offset(g, b);
        if (!ts_usable(tsdf[q], weight[q], min_weight)) return 0;
    }
    return 1;
}

// bit b: corner b of the cell at n exists and is INSIDE
TS_FN int ts_corners_inside(const float* tsdf, const TsGrid& g, int64_t n, int32_t i, int32_t j, int32_t k, float iso) {
    int bits = 0;
    for (int b = 0; b < 8; ++b)
        if (ts_exists(g, i, j, k, b) && tsdf[n + ts_offset(g, b)] < iso) bits |= 1 << b;
    return bits;
}

// bit e: edge 7 n + e crosses.  corners: ts_corners_inside of the point's cell; active: every cell's byte
TS_FN uint8_t ts_edge_marks(const uint8_t* active, const TsGrid& g, int64_t n, int32_t i, int32_t j, int32_t k, int corners) {
    int marks = 0;
    for (int e = 0; e < GP_TSDF_EDGES; ++e) {
        const int d = ts_edge_bits(e);
        if (!ts_exists(g, i, j, k, d) || ((corners & 1) != 0) == (((corners >> d) & 1) != 0)) continue;
        bool in_cell = false;
        for (int s = 0; s < 8; ++s) {              // the cells of the edge: the owner's, stepped back along the axes it does not run along
            if ((s & d) != 0 || (s & 1) > i || ((s >> 1) & 1) > j || ((s >> 2) & 1) > k) continue;
            in_cell = in_cell || active[n - ts_offset(g, s)] != 0;
        }
        if (in_cell) marks |= 1 << e;
    }
    return (uint8_t)marks;
}

// the corners of tetrahedron q as bits, v0 .. v3 in the nibbles from the lowest: (0, 1<<a, (1<<a)|(1<<b), 7), (a, b, c) in lexicographic order
TS_FN int ts_tet_corner(int q, int v) {
    const uint32_t tets[6] = {0x7310, 0x7510, 0x7320, 0x7620, 0x7540, 0x7640};
    return (tets[q] >> (4 * v)) & 7;
}
TS_FN bool ts_tet_odd(int q) { return ((0x26 >> q) & 1) != 0; }                          // q = 1, 2, 5

// bit v: vertex v of tetrahedron q is inside
TS_FN int ts_tet_mask(int corners, int q) {
    int mask = 0;
    for (int v = 0; v < 4; ++v) mask |= ((corners >> ts_tet_corner(q, v)) & 1) << v;
    return mask;
}

TS_FN int ts_case_triangles(int mask) { return (0x16696994 >> (2 * mask)) & 3; }         // 0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0

TS_FN int ts_cell_triangles(int corners) {
    int n = 0;
    for (int q = 0; q < 6; ++q) n += ts_case_triangles(ts_tet_mask(corners, q));
    return n;
}

// The sixteen cases of a positively oriented tetrahedron by gp_tsdf.h's rule: per triangle three LOCAL edges, numbered 01, 02, 03, 12, 13, 23
// = 0 .. 5, in the nibbles from the lowest (triangle 0 first); 15: none.
TS_FN int ts_case_edge(int mask, int slot) {
    const uint32_t rows[16] = {0xffffff, 0xfff210, 0xfff340, 0x341421, 0xfff531, 0x532302, 0x150540, 0xfff542,
                               0xfff452, 0x450510, 0x523203, 0xfff351, 0x241431, 0xfff430, 0xfff120, 0xffffff};
    return (rows[mask] >> (4 * slot)) & 15;
}
// the two tetrahedron vertices of a local edge, the smaller first
TS_FN int ts_local_lo(int le) { return (0x211000 >> (4 * le)) & 3; }
TS_FN int ts_local_hi(int le) { return (0x332321 >> (4 * le)) & 3; }

// the vertex number of the edge from corner lo to corner hi (lo a subset of hi) of the cell at n
TS_FN int32_t ts_vertex_of(const uint8_t* marks, const uint32_t* first_vertex, const TsGrid& g, int64_t n, int lo, int hi) {
    const int64_t owner = n + ts_offset(g, lo);
    const int e = ts_edge_of_bits(hi ^ lo);
    uint32_t below = marks[owner] & ((1u << e) - 1u), k = 0;
    for (; below; below &= below - 1) ++k;
    return (int32_t)(first_vertex[owner] + k);
}

// faces: [3] per triangle of the active cell at n, in the order tetrahedron, triangle, `capacity` of them at the most; returns how many
TS_FN int ts_cell_faces(const uint8_t* marks, const uint32_t* first_vertex, const TsGrid& g, int64_t n, int corners, int capacity, int32_t* faces) {
    int count = 0;
    for (int q = 0; q < 6; ++q) {
        const int mask = ts_tet_mask(corners, q);
        const int tris = ts_case_triangles(mask);
        for (int s = 0; s < tris && count < capacity; ++s) {
            int32_t v[3];
            for (int r = 0; r < 3; ++r) {
                const int le = ts_case_edge(mask, 3 * s + r);
                v[r] = ts_vertex_of(marks, first_vertex, g, n, ts_tet_corner(q, ts_local_lo(le)), ts_tet_corner(q, ts_local_hi(le)));
            }
            const bool odd = ts_tet_odd(q);
            faces[3 * count] = v[0];
            faces[3 * count + 1] = odd ? v[2] : v[1];
            faces[3 * count + 2] = odd ? v[1] : v[2];
            ++count;
        }
    }
    return count;
}

// the vertex of the crossing edge e of the point n = (i, j, k); color: the volume's [3][points] or NULL, and then col is left alone
TS_FN void ts_vertex(const float* tsdf, const float* color, const TsGrid& g, int64_t n, int32_t i, int32_t j, int32_t k, int e, float iso,
                     float* pos, float* col) {
    const int d = ts_edge_bits(e);
    const int64_t n1 = n + ts_offset(g, d);
    const float t0 = tsdf[n], t1 = tsdf[n1];
    const float a = (iso - t0) / (t1 - t0);
    const float x0 = ts_coord(i, g.voxel, g.ox), x1 = ts_coord(i + (d & 1), g.voxel, g.ox);
    const float y0 = ts_coord(j, g.voxel, g.oy), y1 = ts_coord(j + ((d >> 1) & 1), g.voxel, g.oy);
    const float z0 = ts_coord(k, g.voxel, g.oz), z1 = ts_coord(k + ((d >> 2) & 1), g.voxel, g.oz);
    pos[0] = fmaf(a, x1 - x0, x0);
    pos[1] = fmaf(a, y1 - y0, y0);
    pos[2] = fmaf(a, z1 - z0, z0);
    if (color) {
        const int64_t points = ts_points(g);
        for (int c = 0; c < 3; ++c) {
            const float c0 = color[c * points + n], c1 = color[c * points + n1];
            col[c] = fmaf(a, c1 - c0, c0);
        }
    }
}

// ---- the tile order ----
// lane t of a tile's 256 takes the points t, t + 256, t + 512, t + 768 of the tile (u = 0 .. 3)
TS_FN int64_t ts_tile_point(int64_t tile, int u, int t) { return tile * GP_TSDF_TILE + (int64_t)u * TS_BLOCK + t; }
// its wave scan is that of wave t / 64 in step u: chunk u * 4 + t / 64 of the tile's 16, in ascending point order
TS_FN int ts_chunk(int u, int t) { return u * (TS_BLOCK / 64) + t / 64; }

// ---- refusals and the scratch ----
inline const char* ts_refuse_dims(int64_t nx, int64_t ny, int64_t nz) {
    if (nx < 1 || ny < 1 || nz < 1) return "nx, ny and nz must be >= 1";
    if (nx * ny >= 0x80000000LL || nx * ny * nz >= 0x80000000LL || GP_TSDF_EDGES * nx * ny * nz >= 0x80000000LL)      // (no step overflows)
        return "7*nx*ny*nz must be below 2^31";
    return nullptr;
}

inline const char* ts_refuse_volume(const gp_tsdf_volume* vol) {
    if (!vol) return "null argument";
    const char* why = ts_refuse_dims(vol->nx, vol->ny, vol->nz);
    if (why) return why;
    if (!(ts_finite(vol->origin_x) && ts_finite(vol->origin_y) && ts_finite(vol->origin_z) && ts_finite(vol->voxel) && ts_finite(vol->trunc)))
        return "origin, voxel and trunc must be finite";
    if (!(vol->voxel > 0.f) || !(vol->trunc > 0.f)) return "voxel and trunc must be > 0";
    if (!vol->tsdf || !vol->weight) return "null argument";
    return nullptr;
}

inline TsGrid ts_grid_of(const gp_tsdf_volume* vol) {
    TsGrid g;
    g.nx = vol->nx; g.ny = vol->ny; g.nz = vol->nz;
    g.ox = vol->origin_x; g.oy = vol->origin_y; g.oz = vol->origin_z; g.voxel = vol->voxel;
    return g;
}

inline int64_t ts_tiles(int64_t points) { return (points + GP_TSDF_TILE - 1) / GP_TSDF_TILE; }

// byte offsets of the scratch's arrays, each 256-byte aligned
struct TsScratch { int64_t active, marks, tris, first_vertex, first_tri, tile_vertices, tile_tris, bytes; };

inline TsScratch ts_scratch_layout(int64_t points) {
    const int64_t tiles = ts_tiles(points);
    const auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    TsScratch s;
    s.active = 0;
    s.marks = s.active + up(points);
    s.tris = s.marks + up(points);
    s.first_vertex = s.tris + up(points);
    s.first_tri = s.first_vertex + up(4 * points);
    s.tile_vertices = s.first_tri + up(4 * points);
    s.tile_tris = s.tile_vertices + up(4 * tiles);
    s.bytes = s.tile_tris + up(4 * tiles);
    return s;
}
