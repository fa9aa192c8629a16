// resize_core.h -- Pillow's 8-bit resampler (include/gp_resize.h) in this repository's own words: the coefficient builder, which
// runs on the host in double, and the integer pass of one output sample, which runs on the device and, for the host tests
// (tests/resize_emulate.cpp, under the sanitizers), on a CPU.  Nothing here is a tolerance: the tables and the bytes are Pillow's.
//
//   rs_ksize / rs_bounds / rs_coeffs   the tables of one axis: per output sample (xmin, n) and n 22-bit fixed-point weights
//   rs_tap_sum / rs_clip8              ss = 2^21 + sum pixel * k in int32; the byte is clamp(ss >> 22, 0, 255)
//   rs_premultiply / rs_unpremultiply  RGBA goes through premultiplied alpha, as Image.resize sends it
//   rs_window_rows / rs_fused_lds      the source rows a tile of the fused kernel needs, and the LDS bytes that decide the path
//   rs_*_sample / rs_fused_block       the kernels' programs, lane by lane
// The file must be compiled with -ffp-contract=off: a fused multiply-add changes the last bit of a weight.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/gp_resize.h"

#if defined(__HIPCC__)
#define RS_FN __host__ __device__ inline
#else
#define RS_FN inline
#endif

#define RS_PRECISION_BITS 22
#define RS_PI 3.14159265358979323846
#define RS_LDS_BUDGET 32768          // bytes of LDS a fused workgroup may ask for: beyond it the two-launch path runs

inline double rs_support(int filter) {
    switch (filter) {
        case GP_RESIZE_BOX: return 0.5;
        case GP_RESIZE_BILINEAR: case GP_RESIZE_HAMMING: return 1.0;
        case GP_RESIZE_BICUBIC: return 2.0;
        case GP_RESIZE_LANCZOS: return 3.0;
    }
    return -1.0;
}

inline double rs_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * RS_PI;
    return sin(x) / x;
}

inline double rs_weight(int filter, double x) {
    if (filter == GP_RESIZE_BOX) return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    if (filter == GP_RESIZE_LANCZOS) return (-3.0 <= x && x < 3.0) ? rs_sinc(x) * rs_sinc(x / 3) : 0.0;
    if (x < 0.0) x = -x;
    if (filter == GP_RESIZE_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
    if (filter == GP_RESIZE_HAMMING) {
        if (x == 0.0) return 1.0;
        if (x >= 1.0) return 0.0;
        x = x * RS_PI;
        return sin(x) / x * (0.54f + 0.46f * cos(x));          // (float constants widened to double: Pillow's bytes depend on it)
    }
    const double a = -0.5;                                     // bicubic
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct RsAxis {              // one axis of one resize, before any table exists
    int in, out, filter, ksize;
    double scale, fs, support;
};

inline int rs_axis(RsAxis& a, int in, int out, int filter) {
    if (in < 1 || out < 1 || rs_support(filter) < 0.0) return 1;
    a.in = in; a.out = out; a.filter = filter;
    a.scale = (double)in / out;
    a.fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = rs_support(filter) * a.fs;
    const double taps = ceil(a.support) * 2 + 1;
    if (taps > (double)(1 << 24)) return 1;
    a.ksize = (int)taps;
    return 0;
}

inline void rs_bounds(const RsAxis& a, int xx, int* xmin, int* n) {
    const double center = (xx + 0.5) * a.scale;
    int lo = (int)(center - a.support + 0.5), hi = (int)(center + a.support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > a.in) hi = a.in;
    *xmin = lo; *n = hi - lo;
}

// bounds [out][2], coeffs [out][ksize] (zero beyond n).  `w` is a caller's buffer of ksize doubles.
inline void rs_coeffs(const RsAxis& a, int32_t* bounds, int32_t* coeffs, double* w) {
    const double inv = 1.0 / a.fs;
    for (int xx = 0; xx < a.out; ++xx) {
        const double center = (xx + 0.5) * a.scale;
        int xmin, n;
        rs_bounds(a, xx, &xmin, &n);
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = rs_weight(a.filter, (x + xmin - center + 0.5) * inv);
            ww += w[x];
        }
        int32_t* k = coeffs + (size_t)xx * a.ksize;
        for (int x = 0; x < a.ksize; ++x) {
            if (x >= n) { k[x] = 0; continue; }
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int32_t)(v * (1 << RS_PRECISION_BITS) - 0.5) : (int32_t)(v * (1 << RS_PRECISION_BITS) + 0.5);
        }
        bounds[2 * xx] = xmin; bounds[2 * xx + 1] = n;
    }
}

// The most source rows a tile of `tile` consecutive output samples reads: what the fused kernel's LDS window must hold.
inline int rs_window_rows(const RsAxis& a, int tile) {
    int most = 0;
    for (int t0 = 0; t0 < a.out; t0 += tile) {
        const int t1 = (t0 + tile < a.out ? t0 + tile : a.out) - 1;
        int lo, n0, hi, n1;
        rs_bounds(a, t0, &lo, &n0);
        rs_bounds(a, t1, &hi, &n1);
        if (hi + n1 - lo > most) most = hi + n1 - lo;          // (xmin and xmin + n both grow with the sample)
    }
    return most;
}

// LDS bytes of a fused workgroup: both axes' coefficients of the tile, its bounds, the window of bytes between the passes, and the
// tile's resampled alpha.
inline int64_t rs_fused_lds(const RsAxis& ax, const RsAxis& ay, int* rows) {
    *rows = rs_window_rows(ay, GP_RESIZE_TILE_H);
    return 4 * ((int64_t)GP_RESIZE_TILE_W * (ax.ksize + 2) + (int64_t)GP_RESIZE_TILE_H * (ay.ksize + 2)) + ((int64_t)*rows + GP_RESIZE_TILE_H) * GP_RESIZE_TILE_W;
}

inline int rs_path(const RsAxis& ax, const RsAxis& ay, int* rows) {
    *rows = 0;
    if (ax.in == ax.out && ay.in == ay.out) return GP_RESIZE_PATH_COPY;
    if (ay.in == ay.out) return GP_RESIZE_PATH_HORIZONTAL;
    if (ax.in == ax.out) return GP_RESIZE_PATH_VERTICAL;
    return rs_fused_lds(ax, ay, rows) <= RS_LDS_BUDGET ? GP_RESIZE_PATH_FUSED : GP_RESIZE_PATH_TWO_LAUNCH;
}

// ---- the integer pass ------------------------------------------------------------------------------------------------------------------
RS_FN int rs_clip8(int32_t ss) {
    const int32_t v = ss >> RS_PRECISION_BITS;                 // (arithmetic)
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

RS_FN int rs_premultiply(int c, int alpha) {
    const int t = c * alpha + 128;
    return ((t >> 8) + t) >> 8;
}

RS_FN int rs_unpremultiply(int c, int alpha) {
    if (alpha == 0 || alpha == 255) return c;
    const int q = (255 * c) / alpha;
    return q > 255 ? 255 : q;
}

// n taps from px, `step` bytes apart; with `al` (the alpha plane at the same places) every pixel is premultiplied on load
RS_FN int rs_tap_sum(const uint8_t* px, const uint8_t* al, int64_t step, const int32_t* k, int n) {
    int32_t ss = 1 << (RS_PRECISION_BITS - 1);
    if (al) {
        for (int x = 0; x < n; ++x) ss += rs_premultiply(px[x * step], al[x * step]) * k[x];
    } else {
        for (int x = 0; x < n; ++x) ss += (int32_t)px[x * step] * k[x];
    }
    return rs_clip8(ss);
}

// (xmin, n) of a table entry, held inside [0, in) and the tap count whatever the table says: no read leaves the plane
RS_FN void rs_safe_bounds(const int32_t* bounds, int xx, int in, int taps, int* xmin, int* n) {
    int lo = bounds[2 * xx], cnt = bounds[2 * xx + 1];
    lo = lo < 0 ? 0 : lo > in ? in : lo;
    cnt = cnt < 0 ? 0 : cnt > taps ? taps : cnt;
    if (cnt > in - lo) cnt = in - lo;
    *xmin = lo; *n = cnt;
}

RS_FN float rs_unit(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn((float)v, 255.f);
#else
    return (float)v / 255.f;
#endif
}

// ---- the kernels' programs --------------------------------------------------------------------------------------------------------------
// In the phase style of png_core.h: inside RS_PHASE(t) ... RS_END every lane t of the workgroup runs the body and a barrier follows;
// nothing lives in a register across phases.  Under hipcc a phase is the lane's own code and __syncthreads(); without it
// (tests/resize_emulate.cpp) a phase is a loop over the lanes, so the same text, indices included, runs on a CPU under the sanitizers.
#define RS_BLOCK 256
#if defined(__HIPCC__)
#define RS_DEV __device__ inline
#define RS_PHASE(t) { const int t = (int)threadIdx.x;
#define RS_END } __syncthreads();
#else
#define RS_DEV inline
#define RS_PHASE(t) for (int t = 0; t < RS_BLOCK; ++t) {
#define RS_END }
#endif

struct RsPlan {
    int B, C, H, W, Ho, Wo;
    int xtaps, ytaps, alpha_mode, dst_kind, path;
    int rows;                // fused: the LDS window's rows
    const uint8_t* src;
    int64_t src_stride;
    const int32_t *xb, *xk, *yb, *yk;
    void* dst;
    int64_t dst_stride;      // bytes
    uint8_t* mid;            // two-launch: [B][C][H][Wo]
};

RS_FN int rs_min(int a, int b) { return a < b ? a : b; }
RS_FN int rs_max(int a, int b) { return a > b ? a : b; }

RS_DEV void rs_put(const RsPlan& p, int b, int c, int y, int x, int v) {
    const size_t at = ((size_t)c * p.Ho + y) * p.Wo + x;
    char* slot = (char*)p.dst + (size_t)b * (size_t)p.dst_stride;
    if (p.dst_kind == GP_RESIZE_DST_F32) ((float*)slot)[at] = rs_unit(v);
    else ((uint8_t*)slot)[at] = (uint8_t)v;
}

// one lane per sample; z = b * C + c
RS_DEV void rs_copy_sample(const RsPlan& p, int x, int y, int z) {
    const int b = z / p.C, c = z % p.C;
    if (x >= p.W) return;
    rs_put(p, b, c, y, x, p.src[(size_t)b * p.src_stride + ((size_t)c * p.H + y) * p.W + x]);
}

RS_DEV void rs_horizontal_sample(const RsPlan& p, int x, int y, int z) {
    const int b = z / p.C, c = z % p.C;
    if (x >= p.Wo) return;
    int xmin, n;
    rs_safe_bounds(p.xb, x, p.W, p.xtaps, &xmin, &n);
    const int32_t* k = p.xk + (size_t)x * p.xtaps;
    const uint8_t* img = p.src + (size_t)b * p.src_stride;
    const size_t row = (size_t)y * p.W + xmin, plane = (size_t)p.H * p.W;
    const bool colour = p.alpha_mode && c < 3;
    int v = rs_tap_sum(img + c * plane + row, colour ? img + 3 * plane + row : nullptr, 1, k, n);
    if (p.path == GP_RESIZE_PATH_HORIZONTAL) {
        if (colour) v = rs_unpremultiply(v, rs_tap_sum(img + 3 * plane + row, nullptr, 1, k, n));
        rs_put(p, b, c, y, x, v);
    } else {
        p.mid[(((size_t)b * p.C + c) * p.H + y) * p.Wo + x] = (uint8_t)v;
    }
}

RS_DEV void rs_vertical_sample(const RsPlan& p, int x, int y, int z) {
    const int b = z / p.C, c = z % p.C;
    if (x >= p.Wo) return;
    int ymin, n;
    rs_safe_bounds(p.yb, y, p.H, p.ytaps, &ymin, &n);
    const int32_t* k = p.yk + (size_t)y * p.ytaps;
    const bool from_src = p.path == GP_RESIZE_PATH_VERTICAL, colour = p.alpha_mode && c < 3;      // (from_src: W == Wo, nothing premultiplied yet)
    const uint8_t* img = from_src ? p.src + (size_t)b * p.src_stride : p.mid + (size_t)b * p.C * p.H * p.Wo;
    const size_t at = (size_t)ymin * p.Wo + x, plane = (size_t)p.H * p.Wo;
    int v = rs_tap_sum(img + c * plane + at, colour && from_src ? img + 3 * plane + at : nullptr, p.Wo, k, n);
    if (colour) v = rs_unpremultiply(v, rs_tap_sum(img + 3 * plane + at, nullptr, p.Wo, k, n));
    rs_put(p, b, c, y, x, v);
}

// The fused workgroup (bx, by, bz) of the grid (tiles along W, tiles along H, B with alpha_mode or else B * C): `lds` holds
// rs_fused_lds bytes -- kx [TW][xtaps], bounds [TW][2], ky [TH][ytaps], bounds [TH][2], the window [rows][TW], the tile's alpha [TH][TW].
RS_DEV void rs_fused_block(int32_t* lds, const RsPlan& p, int gx, int gy, int gz) {
    constexpr int TW = GP_RESIZE_TILE_W, TH = GP_RESIZE_TILE_H;
    int32_t* kx = lds;
    int32_t* bx = kx + TW * p.xtaps;
    int32_t* ky = bx + 2 * TW;
    int32_t* by = ky + TH * p.ytaps;
    uint8_t* win = (uint8_t*)(by + 2 * TH);
    uint8_t* alpha = win + (size_t)p.rows * TW;
    const int x0 = gx * TW, y0 = gy * TH;
    const int tw = rs_min(TW, p.Wo - x0), th = rs_min(TH, p.Ho - y0);
    RS_PHASE(t)
        for (int i = t; i < tw * p.xtaps; i += RS_BLOCK) kx[i] = p.xk[(size_t)x0 * p.xtaps + i];
        for (int i = t; i < th * p.ytaps; i += RS_BLOCK) ky[i] = p.yk[(size_t)y0 * p.ytaps + i];
        for (int i = t; i < tw; i += RS_BLOCK) rs_safe_bounds(p.xb, x0 + i, p.W, p.xtaps, &bx[2 * i], &bx[2 * i + 1]);
        for (int i = t; i < th; i += RS_BLOCK) rs_safe_bounds(p.yb, y0 + i, p.H, p.ytaps, &by[2 * i], &by[2 * i + 1]);
    RS_END
    const int b = p.alpha_mode ? gz : gz / p.C;
    const uint8_t* img = p.src + (size_t)b * p.src_stride;
    const size_t plane = (size_t)p.H * p.W;
    const int planes = p.alpha_mode ? 4 : 1;
    for (int q = 0; q < planes; ++q) {
        const int c = p.alpha_mode ? (q + 3) & 3 : gz % p.C;                        // alpha first: 3, 0, 1, 2
        const bool colour = p.alpha_mode && c < 3;
        RS_PHASE(t)                                                                 // the horizontal pass of the tile's source rows
            const int r0 = by[0], x = t % TW;                                       // (RS_BLOCK is a multiple of TW: a lane keeps its column)
            const int R = rs_max(0, rs_min(by[2 * (th - 1)] + by[2 * (th - 1) + 1] - r0, rs_min(p.rows, p.H - r0)));
            if (x < tw) {
                const int xmin = bx[2 * x], n = bx[2 * x + 1];
                for (int i = t; i < R * TW; i += RS_BLOCK) {
                    const size_t at = (size_t)(r0 + i / TW) * p.W + xmin;
                    win[i] = (uint8_t)rs_tap_sum(img + c * plane + at, colour ? img + 3 * plane + at : nullptr, 1, kx + x * p.xtaps, n);
                }
            }
        RS_END
        RS_PHASE(t)                                                                 // the vertical pass out of LDS, and the store
            const int r0 = by[0], x = t % TW;
            const int R = rs_max(0, rs_min(by[2 * (th - 1)] + by[2 * (th - 1) + 1] - r0, rs_min(p.rows, p.H - r0)));
            for (int y = t / TW; y < th && x < tw; y += RS_BLOCK / TW) {
                const int off = rs_min(rs_max(0, by[2 * y] - r0), R), n = rs_min(by[2 * y + 1], R - off);
                int v = rs_tap_sum(win + off * TW + x, nullptr, TW, ky + y * p.ytaps, n);
                if (p.alpha_mode && c == 3) alpha[y * TW + x] = (uint8_t)v;        // (its own lane reads it back, two barriers later)
                if (colour) v = rs_unpremultiply(v, alpha[y * TW + x]);
                rs_put(p, b, c, y0 + y, x0 + x, v);
            }
        RS_END
    }
}
