// trajectory_core.h -- the programs of the trajectory drawing (csrc/gp_trajectory.h), shared by the kernels of trajectory_kernels.hip
// and by the stand-alone CPU build the tests run under the sanitizers (tests/trajectory_emulate.cpp).
//
//   tj_project        one point -> its pixel, or TJ_NONE twice where it is not drawable
//   tj_segment        the pixels of one segment that lie inside the image, each handed to `claim(offset)`, offset = y*W + x
//   tj_point_step     one point of one step: project, draw from the previous pixel, return the new one
//   tj_resolve_pixel  one channel of one pixel of the result
//   tj_refusal        the argument checks of gp_traj_step, as text (NULL: accepted)
// The file must be compiled with -ffp-contract=off: every operation of tj_project rounds once.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gp_trajectory.h"

#if defined(__HIPCC__)
#define TJ_FN __host__ __device__ inline
#else
#define TJ_FN inline
#endif

#define TJ_NONE GP_TRAJ_NOT_DRAWABLE

struct TjPixel { int32_t x, y; };

TJ_FN TjPixel tj_project(const gp_traj_view& c, float x, float y, float z, float min_depth) {
    const float xc = ((c.R[0] * x + c.R[1] * y) + c.R[2] * z) + c.t[0];
    const float yc = ((c.R[3] * x + c.R[4] * y) + c.R[5] * z) + c.t[1];
    const float zc = ((c.R[6] * x + c.R[7] * y) + c.R[8] * z) + c.t[2];
    const float den = zc + 0.0001f;
    const float u = (c.f * xc) / den + c.cx;
    const float v = (c.f * yc) / den + c.cy;
    const float lim = (float)GP_TRAJ_COORD_LIMIT;
    // (a NaN or an infinity fails the comparisons; so does a NaN min_depth, which is "no depth test")
    const bool ok = fabsf(u) < lim && fabsf(v) < lim && !(zc <= min_depth);
    TjPixel p;
    p.x = ok ? (int32_t)u : TJ_NONE;
    p.y = ok ? (int32_t)v : TJ_NONE;
    return p;
}

TJ_FN bool tj_drawable(TjPixel p) { return p.x != TJ_NONE; }

// a, b: drawable pixels (|coordinate| < 2^20, so every product below stays under 2^44).  The closed form gives the minor offset and the
// remainder at the first k whose major coordinate is inside the image (one 64-bit division per segment); from there the remainder is
// carried: q(k) = floor((2*k*dn + dm - 1) / (2*dm)) grows by at most one per k because dn <= dm.
template <typename Claim>
TJ_FN void tj_segment(TjPixel a, TjPixel b, int32_t W, int32_t H, Claim claim) {
    const int32_t dx = b.x - a.x, dy = b.y - a.y;
    const int32_t adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const bool xmajor = adx >= ady;
    const int32_t dm = xmajor ? adx : ady, dn = xmajor ? ady : adx;
    const int32_t sm = xmajor ? (dx < 0 ? -1 : 1) : (dy < 0 ? -1 : 1), sn = xmajor ? (dy < 0 ? -1 : 1) : (dx < 0 ? -1 : 1);
    const int32_t am = xmajor ? a.x : a.y, an = xmajor ? a.y : a.x;
    const int32_t M = xmajor ? W : H, Nn = xmajor ? H : W;
    if (dm == 0) {
        if (a.x >= 0 && a.x < W && a.y >= 0 && a.y < H) claim((int64_t)a.y * W + a.x);
        return;
    }
    // the k in [0, dm] with 0 <= am + sm*k < M
    int64_t k_lo, k_hi;
    if (sm > 0) { k_lo = -(int64_t)am; k_hi = (int64_t)M - 1 - am; }
    else        { k_lo = (int64_t)am - (M - 1); k_hi = am; }
    if (k_lo < 0) k_lo = 0;
    if (k_hi > dm) k_hi = dm;
    if (k_lo > k_hi) return;
    const int64_t two_dm = 2 * (int64_t)dm, two_dn = 2 * (int64_t)dn;
    const int64_t num = k_lo * two_dn + dm - 1;
    int64_t q = num / two_dm, r = num - q * two_dm;          // (num >= 0: floor is truncation)
    int32_t major = am + sm * (int32_t)k_lo;
    for (int64_t k = k_lo; k <= k_hi; ++k) {
        const int64_t minor = an + sn * q;
        if (minor >= 0 && minor < Nn) claim(xmajor ? minor * W + major : (int64_t)major * W + minor);
        else if (sn > 0 ? minor >= Nn : minor < 0) return;   // (the minor coordinate moves one way: it has left the image for good)
        r += two_dn;
        if (r >= two_dm) { r -= two_dm; ++q; }
        major += sm;
    }
}

// xyz_row: the point's row of xyz, or NULL for a row outside the array.  prev: the pixel stored by step s - 1 (not read when s == 0).
template <typename Claim>
TJ_FN TjPixel tj_point_step(const gp_traj_view& c, const float* xyz_row, float min_depth, bool first, TjPixel prev, int32_t W, int32_t H,
                            Claim claim) {
    TjPixel now;
    now.x = now.y = TJ_NONE;
    if (xyz_row) now = tj_project(c, xyz_row[0], xyz_row[1], xyz_row[2], min_depth);
    if (!first && tj_drawable(prev) && tj_drawable(now)) tj_segment(prev, now, W, H, claim);
    return now;
}

TJ_FN float tj_resolve_pixel(uint32_t key, const float* colors, int64_t P, const float* base, int64_t offset, int64_t plane, int ch) {
    if (key != 0 && P > 0) return colors[(int64_t)((key - 1u) % (uint64_t)P) * 3 + ch];
    return base ? base[(int64_t)ch * plane + offset] : 0.0f;
}

inline const char* tj_refusal(int64_t N, int64_t P, int64_t s, int64_t H, int64_t W, bool has_idx) {
    if (N < 0 || P < 0 || s < 0) return "N, P and s must be >= 0";
    if (H <= 0 || W <= 0) return "H and W must be > 0";
    if (H * W >= 0x80000000LL) return "H*W must be below 2^31";
    if (P >= 0x80000000LL) return "P must be below 2^31";
    if (P > 0 && s >= 0xFFFFFFFELL / P) return "S*P must be below 2^32 - 1 (the keys are 32 bits wide)";      // (s + 1)*P >= 2^32 - 1
    if (!has_idx && N < P) return "without idx, xyz must hold at least P rows";
    if (has_idx && P > 0 && N == 0) return "idx given but xyz holds no row";
    return nullptr;
}
