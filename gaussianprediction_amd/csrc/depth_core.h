// depth_core.h -- the per-element programs and the tile orders of the depth renders (csrc/gp_depth.h), shared by the kernels of
// depth_kernels.hip and by the stand-alone CPU build the tests run under the sanitizers (tests/depth_emulate.cpp).
//
//   dp_resolve_pixel   one pixel of the composite -> depth, valid
//   dp_value           the coloured quantity of one pixel (depth or disparity) and whether it is coloured;  dp_range_of: the pair
//                      used from the two words the integer minimum and maximum left;  dp_lut_row: the row of the table
//   dp_point           the camera-space point of a pixel;  dp_normal: one pixel's normal and nvalid;  dp_world: cam2world . (P, 1)
//   dp_metric_terms    one pixel's twelve terms;  dp_metric_row: the slots' totals -> a row of the table
//   dp_tile_pixel      the pixel a lane of a tile's workgroup takes in its step u (the order of every tiled kernel here)
//   dp_chunk           the place of that pixel's 64-pixel chunk in the tile's row-major order (the compaction's ranks)
//   dp_refuse_plane    the size checks, as text (NULL: accepted)
// The file must be compiled with -ffp-contract=off: every operation rounds once.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gp_depth.h"

#if defined(__HIPCC__)
#define DP_FN __host__ __device__ inline
#else
#define DP_FN inline
#endif

#define DP_BLOCK 256
#define DP_PER_LANE (GP_DEPTH_TILE / DP_BLOCK)
#define DP_CHUNKS (GP_DEPTH_TILE / 64)              // the 64-pixel chunks of a tile: one ballot each

DP_FN bool dp_finite(float v) { return fabsf(v) < INFINITY; }            // (false for a NaN)

DP_FN uint32_t dp_bits(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }
DP_FN float dp_float(uint32_t b) { float v; memcpy(&v, &b, 4); return v; }

// ---- resolve ----
struct DpResolved { float depth; uint8_t valid; };

DP_FN DpResolved dp_resolve_pixel(float accum, float alpha, float alpha_min) {
    const float d = accum / alpha;
    DpResolved r;
    r.valid = (alpha >= alpha_min && dp_finite(d) && d > 0.f) ? 1 : 0;
    r.depth = r.valid ? d : 0.f;
    return r;
}

// ---- colour ----
// v: the quantity mode colours; returns whether the pixel takes a colour (not the background)
DP_FN bool dp_value(float depth, const uint8_t* valid, int64_t p, int32_t mode, float* v) {
    *v = mode == 1 ? 1.f / depth : depth;
    return (!valid || valid[p] != 0) && dp_finite(*v) && *v > 0.f;
}

#define DP_RANGE_LO_INIT 0xFFFFFFFFu                // the words before any pixel entered them
#define DP_RANGE_HI_INIT 0u

// the pair used: the given one where lo < hi, else the floats whose bits the integer minimum and maximum left, (0, 1) where none did
DP_FN void dp_range_of(float lo, float hi, uint32_t lo_bits, uint32_t hi_bits, float* out) {
    if (lo < hi) { out[0] = lo; out[1] = hi; return; }
    if (hi_bits == DP_RANGE_HI_INIT) { out[0] = 0.f; out[1] = 1.f; return; }
    out[0] = dp_float(lo_bits);
    out[1] = dp_float(hi_bits);
}

DP_FN int dp_lut_row(float v, float lo, float hi) {
    const float t = hi == lo ? 0.f : (v - lo) / (hi - lo);
    if (t >= 1.f) return GP_DEPTH_LUT - 1;
    if (t >= 0.f) return (int)(t * 256.f);
    return 0;                                       // (t < 0, and a NaN from an infinite hi - lo)
}

// ---- points and normals ----
struct DpVec { float x, y, z; };

DP_FN DpVec dp_point(int32_t x, int32_t y, float z, float tanfovx, float tanfovy, int32_t W, int32_t H) {
    const float xn = (float)(2 * (int64_t)x + 1) / (float)W - 1.f;       // (64 bits: W may be close to 2^31 where H is 1)
    const float yn = (float)(2 * (int64_t)y + 1) / (float)H - 1.f;
    DpVec P;
    P.x = xn * tanfovx * z;
    P.y = yn * tanfovy * z;
    P.z = z;
    return P;
}

DP_FN bool dp_valid_at(const uint8_t* valid, int32_t x, int32_t y, int32_t W, int32_t H) {
    return x >= 0 && x < W && y >= 0 && y < H && (!valid || valid[(int64_t)y * W + x] != 0);
}

// n: the pixel's normal, or zeros; returns nvalid
DP_FN uint8_t dp_normal(const float* depth, const uint8_t* valid, int32_t x, int32_t y, float tanfovx, float tanfovy, int32_t W, int32_t H, float* n) {
    n[0] = n[1] = n[2] = 0.f;
    if (!(dp_valid_at(valid, x, y, W, H) && dp_valid_at(valid, x - 1, y, W, H) && dp_valid_at(valid, x + 1, y, W, H) &&
          dp_valid_at(valid, x, y - 1, W, H) && dp_valid_at(valid, x, y + 1, W, H)))
        return 0;
    const int64_t p = (int64_t)y * W + x;
    const DpVec P = dp_point(x, y, depth[p], tanfovx, tanfovy, W, H);
    const DpVec r = dp_point(x + 1, y, depth[p + 1], tanfovx, tanfovy, W, H), l = dp_point(x - 1, y, depth[p - 1], tanfovx, tanfovy, W, H);
    const DpVec d = dp_point(x, y + 1, depth[p + W], tanfovx, tanfovy, W, H), u = dp_point(x, y - 1, depth[p - W], tanfovx, tanfovy, W, H);
    const float ax = r.x - l.x, ay = r.y - l.y, az = r.z - l.z;
    const float bx = d.x - u.x, by = d.y - u.y, bz = d.z - u.z;
    float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    if (!(dp_finite(len) && len > 0.f)) return 0;
    nx = nx / len; ny = ny / len; nz = nz / len;
    const bool away = (nx * P.x + ny * P.y) + nz * P.z > 0.f;
    n[0] = away ? -nx : nx;
    n[1] = away ? -ny : ny;
    n[2] = away ? -nz : nz;
    return 1;
}

// m: cam2world, m[col*4 + row]
DP_FN DpVec dp_world(const float* m, DpVec P) {
    DpVec o;
    o.x = fmaf(m[0], P.x, fmaf(m[4], P.y, fmaf(m[8], P.z, m[12])));
    o.y = fmaf(m[1], P.x, fmaf(m[5], P.y, fmaf(m[9], P.z, m[13])));
    o.z = fmaf(m[2], P.x, fmaf(m[6], P.y, fmaf(m[10], P.z, m[14])));
    return o;
}

// ---- the tile order ----
// lane t of a tile's 256 takes the pixels t, t + 256, t + 512, t + 768 of the tile (u = 0 .. 3)
DP_FN int64_t dp_tile_pixel(int64_t tile, int u, int t) { return tile * GP_DEPTH_TILE + (int64_t)u * DP_BLOCK + t; }
// its ballot is that of wave t / 64 in step u: chunk u * 4 + t / 64 of the tile's 16, in row-major pixel order
DP_FN int dp_chunk(int u, int t) { return u * (DP_BLOCK / 64) + t / 64; }

// ---- metrics ----
// logf as gp_depth.h defines it: the double-precision logarithm rounded once to float32 -- the correctly rounded logf but for a double
// rounding at a near-tie.  (The device's own logf is within its 1 ulp and biased: it moved RMSE-log by 1e-8 at every image size,
// DESIGN section 25; two double logarithms a pixel cost nothing beside the pixel's 9 bytes.)
DP_FN float dp_logf(float x) { return (float)log((double)x); }

// t[0..12) += the pixel's terms
DP_FN void dp_metric_terms(float pred, float g, bool masked_in, const float* scale, float gt_min, float gt_max, float* t) {
    const float d = scale ? pred * scale[0] : pred;
    if (!(masked_in && dp_finite(d) && dp_finite(g) && d > 0.f && g > 0.f && gt_min <= g && g <= gt_max)) return;
    const float e = d - g;
    const float l = dp_logf(d) - dp_logf(g);
    const float r = fmaxf(d / g, g / d);
    t[0] += 1.f;
    t[1] += fabsf(e) / g;
    t[2] += e * e / g;
    t[3] += e * e;
    t[4] += l * l;
    t[5] += l;
    t[6] += r < 1.25f ? 1.f : 0.f;
    t[7] += r < 1.5625f ? 1.f : 0.f;
    t[8] += r < 1.953125f ? 1.f : 0.f;
    t[9] += d * g;
    t[10] += d * d;
    t[11] += g;
}

DP_FN void dp_metric_row(const double* s, double* row) {
    const double n = s[0];
    if (!(n > 0.0)) {
        for (int q = 0; q < GP_DEPTH_COLUMNS; ++q) row[q] = (double)NAN;
        return;
    }
    const double ml2 = s[4] / n, ml = s[5] / n;
    row[0] = n;
    row[1] = s[1] / n;
    row[2] = s[2] / n;
    row[3] = sqrt(s[3] / n);
    row[4] = sqrt(ml2);
    row[5] = s[6] / n;
    row[6] = s[7] / n;
    row[7] = s[8] / n;
    row[8] = ml2 - ml * ml;
    row[9] = s[9] / s[10];
    row[10] = s[11] / n;
    row[11] = 0.0;
}

// ---- refusals ----
inline const char* dp_refuse_plane(int64_t H, int64_t W) {
    if (H <= 0 || W <= 0) return "H and W must be > 0";
    if (H * W >= 0x80000000LL) return "H*W must be below 2^31";
    return nullptr;
}

inline int64_t dp_tiles(int64_t H, int64_t W) { return (H * W + GP_DEPTH_TILE - 1) / GP_DEPTH_TILE; }
