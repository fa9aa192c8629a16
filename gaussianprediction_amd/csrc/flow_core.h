// flow_core.h -- the per-element programs of the optical-flow renders (csrc/gp_flow.h), shared by the kernels of flow_kernels.hip and
// by the stand-alone CPU build the tests run under the sanitizers (tests/flow_emulate.cpp).
//
//   fl_pixel          one point in one view -> its pixel centre, and whether it passes the depth test
//   fl_project_row    one Gaussian at two times in two views -> its row (dx, dy, 1), or zeros
//   fl_resolve_pixel  one pixel of the composite -> flow, alpha, valid
//   fl_wheel          one entry of the colour wheel;  fl_magnitude, fl_color: the colour of one pixel
//   fl_metric_terms   one pixel's seven terms;  fl_metric_row: the slots' totals -> a row of the table
//   fl_warp_pixel     one channel of one warped pixel
//   fl_refuse_plane   the size checks, as text (NULL: accepted)
// The file must be compiled with -ffp-contract=off: every operation rounds once, fmaf where the projection kernel has one.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gp_flow.h"

#if defined(__HIPCC__)
#define FL_FN __host__ __device__ inline
#else
#define FL_FN inline
#endif

FL_FN bool fl_finite(float v) { return fabsf(v) < INFINITY; }            // (false for a NaN)

struct FlPixel { float x, y; bool front; };

// v, p: the view's two matrices, m[col*4 + row] (the expressions of the projection kernel, raster_kernels.hip)
FL_FN FlPixel fl_pixel(const float* v, const float* p, int32_t W, int32_t H, float x, float y, float z) {
    const float depth = fmaf(v[2], x, fmaf(v[6], y, fmaf(v[10], z, v[14])));
    const float hx = fmaf(p[0], x, fmaf(p[4], y, fmaf(p[8], z, p[12])));
    const float hy = fmaf(p[1], x, fmaf(p[5], y, fmaf(p[9], z, p[13])));
    const float hw = fmaf(p[3], x, fmaf(p[7], y, fmaf(p[11], z, p[15])));
    const float pw = 1.f / (hw + 0.0000001f);
    const float ndcx = hx * pw, ndcy = hy * pw;
    FlPixel o;
    o.x = ((ndcx + 1.f) * (float)W - 1.f) * 0.5f;
    o.y = ((ndcy + 1.f) * (float)H - 1.f) * 0.5f;
    o.front = depth > 0.2f;
    return o;
}

FL_FN void fl_project_row(const float* v0, const float* p0, int32_t W0, int32_t H0, const float* v1, const float* p1, int32_t W1, int32_t H1,
                          const float* a, const float* b, float* out) {
    const FlPixel q0 = fl_pixel(v0, p0, W0, H0, a[0], a[1], a[2]);
    const FlPixel q1 = fl_pixel(v1, p1, W1, H1, b[0], b[1], b[2]);
    const bool ok = q0.front && q1.front && fl_finite(q0.x) && fl_finite(q0.y) && fl_finite(q1.x) && fl_finite(q1.y);
    out[0] = ok ? q1.x - q0.x : 0.f;
    out[1] = ok ? q1.y - q0.y : 0.f;
    out[2] = ok ? 1.f : 0.f;
}

struct FlResolved { float u, v, alpha; uint8_t valid; };

FL_FN FlResolved fl_resolve_pixel(float c0, float c1, float c2, float alpha_min) {
    const float u = c0 / c2, v = c1 / c2;
    FlResolved r;
    r.valid = (c2 >= alpha_min && fl_finite(u) && fl_finite(v)) ? 1 : 0;
    r.u = r.valid ? u : 0.f;
    r.v = r.valid ? v : 0.f;
    r.alpha = c2;
    return r;
}

// ---- colour ----
FL_FN float fl_wheel(int k, int c) {
    int r, g, b;
    if (k < 15)      { r = 255; g = 255 * k / 15; b = 0; }
    else if (k < 21) { r = 255 - 255 * (k - 15) / 6; g = 255; b = 0; }
    else if (k < 25) { r = 0; g = 255; b = 255 * (k - 21) / 4; }
    else if (k < 36) { r = 0; g = 255 - 255 * (k - 25) / 11; b = 255; }
    else if (k < 49) { r = 255 * (k - 36) / 13; g = 0; b = 255; }
    else             { r = 255; g = 0; b = 255 - 255 * (k - 49) / 6; }
    return (float)(c == 0 ? r : c == 1 ? g : b) / 255.f;
}

// does the pixel take a colour (not the background)?
FL_FN bool fl_coloured(float fu, float fv, const uint8_t* valid, int64_t p) { return (!valid || valid[p] != 0) && fl_finite(fu) && fl_finite(fv); }

FL_FN float fl_magnitude(float fu, float fv) { return sqrtf(fu * fu + fv * fv); }

// the bits of a pixel's entry in the integer maximum: its magnitude where that is finite, else 0 (magnitudes are >= 0: their order is
// the order of their bits)
FL_FN uint32_t fl_magnitude_bits(float fu, float fv) {
    const float m = fl_magnitude(fu, fv);
    uint32_t bits;
    memcpy(&bits, &m, 4);
    return fl_finite(m) ? bits : 0u;
}

// found: the float whose bits the integer maximum left (0 where no pixel entered it)
FL_FN float fl_scale_of(float max_flow, float found) {
    if (max_flow > 0.f) return max_flow;
    return found > 0.f ? found : 1.f;
}

// wheel: [55][3] (fl_wheel); col: the three channels of a pixel that takes a colour
FL_FN void fl_color(float fu, float fv, float scale, const float* wheel, float* col) {
    const float u = fu / scale, v = fv / scale;
    const float rad = sqrtf(u * u + v * v);
    const float a = atan2f(-v, -u) / 3.14159265358979323846f;
    const float fk = ((a + 1.f) / 2.f) * 54.f;
    float k0f = floorf(fk);
    k0f = k0f >= 0.f ? k0f : 0.f;                  // (also a NaN)
    k0f = k0f <= 54.f ? k0f : 54.f;
    const int k0 = (int)k0f, k1 = (k0 + 1) % GP_FLOW_WHEEL;
    const float f = fk - k0f;
    for (int c = 0; c < 3; ++c) {
        float x = (1.f - f) * wheel[k0 * 3 + c] + f * wheel[k1 * 3 + c];
        x = rad <= 1.f ? 1.f - rad * (1.f - x) : x * 0.75f;
        col[c] = x;
    }
}

// ---- metrics ----
// t[0..7) += the pixel's terms
FL_FN void fl_metric_terms(float fu, float fv, float gu, float gv, bool masked_in, float* t) {
    if (!(masked_in && fl_finite(fu) && fl_finite(fv) && fl_finite(gu) && fl_finite(gv))) return;
    const float du = fu - gu, dv = fv - gv;
    const float epe = sqrtf(du * du + dv * dv), mag = sqrtf(gu * gu + gv * gv);
    t[0] += 1.f;
    t[1] += epe;
    t[2] += epe > 1.f ? 1.f : 0.f;
    t[3] += epe > 3.f ? 1.f : 0.f;
    t[4] += epe > 5.f ? 1.f : 0.f;
    t[5] += (epe > 3.f && epe > 0.05f * mag) ? 1.f : 0.f;
    t[6] += mag;
}

FL_FN void fl_metric_row(const double* s, double* row) {
    const double n = s[0];
    if (!(n > 0.0)) {
        for (int q = 0; q < GP_FLOW_COLUMNS; ++q) row[q] = (double)NAN;
        return;
    }
    row[0] = n;
    for (int q = 1; q < GP_FLOW_SUMS; ++q) row[q] = s[q] / n;
    row[7] = 0.0;
}

// ---- warp ----
FL_FN float fl_tap(const float* plane, int32_t H, int32_t W, int32_t y, int32_t x) {
    return (x >= 0 && x < W && y >= 0 && y < H) ? plane[(int64_t)y * W + x] : 0.f;
}

FL_FN float fl_warp_pixel(const float* plane, int32_t H, int32_t W, int32_t x, int32_t y, float fu, float fv) {
    const float sx = (float)x + fu, sy = (float)y + fv;
    if (!(fl_finite(sx) && fl_finite(sy))) return 0.f;
    const float x0f = floorf(sx), y0f = floorf(sy);
    // (all four taps outside: also keeps the conversions below in range)
    if (!(x0f >= -1.f && x0f < (float)W && y0f >= -1.f && y0f < (float)H)) return 0.f;
    const float ax = sx - x0f, ay = sy - y0f;
    const int32_t x0 = (int32_t)x0f, y0 = (int32_t)y0f;
    const float w00 = (1.f - ay) * (1.f - ax), w01 = (1.f - ay) * ax, w10 = ay * (1.f - ax), w11 = ay * ax;
    return ((w00 * fl_tap(plane, H, W, y0, x0) + w01 * fl_tap(plane, H, W, y0, x0 + 1)) + w10 * fl_tap(plane, H, W, y0 + 1, x0)) +
           w11 * fl_tap(plane, H, W, y0 + 1, x0 + 1);
}

// ---- refusals ----
inline const char* fl_refuse_plane(int64_t H, int64_t W) {
    if (H <= 0 || W <= 0) return "H and W must be > 0";
    if (H * W >= 0x80000000LL) return "H*W must be below 2^31";
    return nullptr;
}

inline int64_t fl_tiles(int64_t H, int64_t W) { return (H * W + GP_FLOW_TILE - 1) / GP_FLOW_TILE; }
