// mesh_render_core.h -- the per-vertex, per-face, per-sample and per-pixel programs of the triangle rasterizer (csrc/gp_mesh_render.h),
// shared by the kernels of mesh_render_kernels.hip and by the stand-alone CPU build the tests run under the sanitizers
// (tests/mesh_render_emulate.cpp).  Every formula of the header stands here once.
//
//   mr_camera_point, mr_vertex        a vertex's camera point; its 16-byte record
//   mr_classify                       a face: dropped (and why) or drawn, with its corners, area, sign and clamped box
//   mr_sample                         one sample of one face: inside or not, the weights, the barycentrics, the depth
//   mr_key, mr_submit                 the visibility key; the atomic minimum (and the coverage count) of a counting sample
//   mr_draw_narrow, mr_draw_wide_lane the walks over a box: by one lane, and by lane `lane` of piece `piece` of a wide face
//   mr_resolve_pixel, mr_interpolate_pixel, mr_normal_pixel, mr_shade_pixel       the outputs
//   mr_refuse_view, mr_scratch_layout
// The file must be compiled with -ffp-contract=off: every operation rounds once.
#pragma once
#include "gp_mesh_render.h"
#include "depth_core.h"
#include "mesh_core.h"

#define MR_FN MS_FN
#define MR_BLOCK 256
#define MR_WIDE_BLOCKS 2048                  // the workgroups of the launch over the list of wide faces

#define MR_FLAG_NEAR 1u
#define MR_FLAG_RANGE 2u

#define MR_DRAW 0                            // mr_classify
#define MR_BAD_INDEX 1
#define MR_NEAR 2
#define MR_RANGE 3
#define MR_DEGENERATE 4
#define MR_CULLED 5
#define MR_CLASSES 6
#define MR_FACE_BLOCKS 2048                  // the workgroups of the launch over the faces at the most: 8 on each of 256 CUs

#define MR_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull

struct alignas(16) MrVertex { int32_t x, y; float r; uint32_t flags; };
static_assert(sizeof(MrVertex) == 16, "a corner is one 16-byte gather");

struct MrView { float tanfovx, tanfovy, z_near; int32_t W, H, cull; };

struct MrFace {
    MrVertex p[3];
    int64_t area;                            // |area2|
    int32_t sign;                            // +1: area2 > 0; -1: area2 < 0
    int32_t x0, y0, x1, y1;                  // the box in pixels, inclusive; x0 > x1 or y0 > y1: empty
};

struct MrSample { int64_t w[3]; float l[3], z; };

// ---- vertices ----
MR_FN void mr_camera_point(const float* m, const float* v, float* P) {
    for (int r = 0; r < 3; ++r) P[r] = fmaf(m[r], v[0], fmaf(m[4 + r], v[1], fmaf(m[8 + r], v[2], m[12 + r])));
}

MR_FN bool mr_snap(float p, int32_t* out) {
    const float s = floorf(fmaf(p, (float)GP_MESH_RENDER_SUBPIXEL, 0.5f));
    const bool ok = dp_finite(s) && fabsf(s) <= (float)GP_MESH_RENDER_GUARD;
    *out = ok ? (int32_t)s : 0;              // (a value that is not in range never reaches the conversion)
    return ok;
}

MR_FN MrVertex mr_vertex(const float* m, const float* v, const MrView& view) {
    float P[3];
    mr_camera_point(m, v, P);
    MrVertex o;
    o.flags = P[2] > view.z_near ? 0u : MR_FLAG_NEAR;
    const float xn = P[0] / (P[2] * view.tanfovx), yn = P[1] / (P[2] * view.tanfovy);
    const float px = ((xn + 1.f) * (float)view.W - 1.f) * 0.5f, py = ((yn + 1.f) * (float)view.H - 1.f) * 0.5f;
    const bool okx = mr_snap(px, &o.x), oky = mr_snap(py, &o.y);
    if (!(okx && oky)) o.flags |= MR_FLAG_RANGE;
    o.r = 1.f / P[2];
    return o;
}

// ---- faces ----
MR_FN int64_t mr_edge(const MrVertex& u, const MrVertex& v, int64_t px, int64_t py) {
    return ((int64_t)v.x - u.x) * (py - u.y) - ((int64_t)v.y - u.y) * (px - u.x);
}

MR_FN int32_t mr_min3(int32_t a, int32_t b, int32_t c) { const int32_t m = a < b ? a : b; return m < c ? m : c; }
MR_FN int32_t mr_max3(int32_t a, int32_t b, int32_t c) { const int32_t m = a > b ? a : b; return m > c ? m : c; }
MR_FN int32_t mr_floor_pixel(int32_t s) {         // floor(s / 256), also below zero
    return s >= 0 ? s / GP_MESH_RENDER_SUBPIXEL : -((GP_MESH_RENDER_SUBPIXEL - 1 - s) / GP_MESH_RENDER_SUBPIXEL);
}

MR_FN int64_t mr_box_pixels(const MrFace& t) {
    return (t.x0 > t.x1 || t.y0 > t.y1) ? 0 : ((int64_t)t.x1 - t.x0 + 1) * ((int64_t)t.y1 - t.y0 + 1);
}

// the class of face f; t is complete where the class is MR_DRAW
MR_FN int mr_classify(const int32_t* faces, int64_t f, int64_t nv, const MrVertex* records, const MrView& view, MrFace& t) {
    int32_t v[3];
    if (!ms_face(faces, f, nv, v, nullptr)) return MR_BAD_INDEX;
    for (int c = 0; c < 3; ++c) t.p[c] = records[v[c]];
    const uint32_t flags = t.p[0].flags | t.p[1].flags | t.p[2].flags;
    if (flags & MR_FLAG_NEAR) return MR_NEAR;
    if (flags & MR_FLAG_RANGE) return MR_RANGE;
    const int64_t area2 = mr_edge(t.p[0], t.p[1], t.p[2].x, t.p[2].y);
    if (area2 == 0) return MR_DEGENERATE;
    if ((view.cull == GP_MESH_RENDER_CULL_BACK && area2 > 0) || (view.cull == GP_MESH_RENDER_CULL_FRONT && area2 < 0)) return MR_CULLED;
    t.sign = area2 > 0 ? 1 : -1;
    t.area = area2 > 0 ? area2 : -area2;
    const int32_t lo_x = mr_min3(t.p[0].x, t.p[1].x, t.p[2].x), hi_x = mr_max3(t.p[0].x, t.p[1].x, t.p[2].x);
    const int32_t lo_y = mr_min3(t.p[0].y, t.p[1].y, t.p[2].y), hi_y = mr_max3(t.p[0].y, t.p[1].y, t.p[2].y);
    t.x0 = mr_floor_pixel(lo_x + (GP_MESH_RENDER_SUBPIXEL - 1)); t.x1 = mr_floor_pixel(hi_x);          // (|X| <= 2^23: no overflow)
    t.y0 = mr_floor_pixel(lo_y + (GP_MESH_RENDER_SUBPIXEL - 1)); t.y1 = mr_floor_pixel(hi_y);
    if (t.x0 < 0) t.x0 = 0;
    if (t.y0 < 0) t.y0 = 0;
    if (t.x1 > view.W - 1) t.x1 = view.W - 1;
    if (t.y1 > view.H - 1) t.y1 = view.H - 1;
    return MR_DRAW;
}

// the word of counts[] a class adds to
MR_FN int mr_count_word(int what) {
    return what == MR_DRAW ? GP_MESH_RENDER_DRAWN : what == MR_BAD_INDEX ? GP_MESH_RENDER_STATUS : what == MR_NEAR ? GP_MESH_RENDER_NEAR
         : what == MR_RANGE ? GP_MESH_RENDER_OUT_OF_RANGE : what == MR_DEGENERATE ? GP_MESH_RENDER_DEGENERATE : GP_MESH_RENDER_CULLED;
}

// ---- one sample ----
MR_FN bool mr_owns(int64_t dx, int64_t dy) { return dy > 0 || (dy == 0 && dx > 0); }

// whether pixel (ix, iy) counts for face t; s is complete where it does
MR_FN bool mr_sample(const MrFace& t, int32_t ix, int32_t iy, MrSample& s) {
    const int64_t px = (int64_t)ix * GP_MESH_RENDER_SUBPIXEL, py = (int64_t)iy * GP_MESH_RENDER_SUBPIXEL;
    for (int i = 0; i < 3; ++i) {
        const MrVertex& u = t.p[(i + 1) % 3];
        const MrVertex& v = t.p[(i + 2) % 3];
        const int64_t w = t.sign * mr_edge(u, v, px, py);
        if (w < 0) return false;
        if (w == 0 && !mr_owns(t.sign * ((int64_t)v.x - u.x), t.sign * ((int64_t)v.y - u.y))) return false;
        s.w[i] = w;
    }
    for (int i = 0; i < 3; ++i) s.l[i] = (float)((double)s.w[i] / (double)t.area);
    const float q = fmaf(s.l[0], t.p[0].r, fmaf(s.l[1], t.p[1].r, s.l[2] * t.p[2].r));
    s.z = 1.f / q;
    return dp_finite(s.z) && s.z > 0.f;
}

MR_FN uint64_t mr_key(float z, int64_t f) { return ((uint64_t)dp_bits(z) << 32) | (uint64_t)(uint32_t)f; }

// the buffer's word takes the minimum; the atomic is left out where a load already shows a key that is not larger (keys only decrease)
MR_FN void mr_submit(unsigned long long* vis, int32_t* coverage, int64_t pixel, uint64_t key) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (key < __hip_atomic_load(vis + pixel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(vis + pixel, (unsigned long long)key);
    if (coverage) atomicAdd(coverage + pixel, 1);
#else
    if (key < vis[pixel]) vis[pixel] = key;
    if (coverage) coverage[pixel] += 1;
#endif
}

MR_FN void mr_draw_pixel(const MrFace& t, int64_t f, int32_t ix, int32_t iy, int32_t W, unsigned long long* vis, int32_t* coverage) {
    MrSample s;
    if (mr_sample(t, ix, iy, s)) mr_submit(vis, coverage, (int64_t)iy * W + ix, mr_key(s.z, f));
}

// a box of at most GP_MESH_RENDER_NARROW_MAX pixels, by one lane
MR_FN void mr_draw_narrow(const MrFace& t, int64_t f, int32_t W, unsigned long long* vis, int32_t* coverage) {
    for (int32_t iy = t.y0; iy <= t.y1; ++iy)
        for (int32_t ix = t.x0; ix <= t.x1; ++ix) mr_draw_pixel(t, f, ix, iy, W, vis, coverage);
}

// lane `lane` of 64 of piece `piece` of GP_MESH_RENDER_SPLIT: the 8 x 8 blocks of the box in row-major order, block b to piece b % SPLIT,
// lane (lx, ly) = (lane & 7, lane >> 3) to the block's pixel (lx, ly)
MR_FN void mr_draw_wide_lane(const MrFace& t, int64_t f, int piece, int lane, int32_t W, unsigned long long* vis, int32_t* coverage) {
    const int64_t bx = ((int64_t)t.x1 - t.x0 + 8) / 8, by = ((int64_t)t.y1 - t.y0 + 8) / 8;
    for (int64_t b = piece; b < bx * by; b += GP_MESH_RENDER_SPLIT) {
        const int32_t ix = t.x0 + (int32_t)(b % bx) * 8 + (lane & 7), iy = t.y0 + (int32_t)(b / bx) * 8 + (lane >> 3);
        if (ix <= t.x1 && iy <= t.y1) mr_draw_pixel(t, f, ix, iy, W, vis, coverage);
    }
}

// ---- the outputs ----
MR_FN void mr_resolve_pixel(const unsigned long long* vis, const int32_t* faces, int64_t nv, int64_t nf, const MrVertex* records, const MrView& view, int32_t ix,
                            int32_t iy, int32_t* face, float* depth, uint8_t* valid, float* bary) {
    const int64_t p = (int64_t)iy * view.W + ix, plane = (int64_t)view.H * view.W;
    const uint64_t key = vis[p];
    const int64_t f = (int64_t)(key & 0xFFFFFFFFull);
    MrFace t;
    MrSample s;
    MrView all = view;
    all.cull = GP_MESH_RENDER_CULL_NONE;             // (the face that won was not culled)
    const bool ok = key != MR_EMPTY_KEY && f < nf && mr_classify(faces, f, nv, records, all, t) == MR_DRAW && mr_sample(t, ix, iy, s);
    face[p] = ok ? (int32_t)f : -1;
    depth[p] = ok ? s.z : 0.f;
    valid[p] = ok ? 1 : 0;
    for (int i = 0; i < 3; ++i) bary[i * plane + p] = ok ? s.l[i] : 0.f;
}

// out[c * plane + p], c < C
MR_FN void mr_interpolate_pixel(const float* attributes, int32_t C, const int32_t* faces, int64_t nv, int64_t nf, const MrVertex* records, const int32_t* face,
                                const uint8_t* valid, const float* bary, const float* background, int64_t p, int64_t plane, float* out) {
    int32_t v[3];
    const int64_t f = face[p];
    if (!valid[p] || f < 0 || f >= nf || !ms_face(faces, f, nv, v, nullptr)) {
        for (int c = 0; c < C; ++c) out[c * plane + p] = background[c];
        return;
    }
    float l[3], r[3], t[3];
    for (int i = 0; i < 3; ++i) { l[i] = bary[i * plane + p]; r[i] = records[v[i]].r; t[i] = l[i] * r[i]; }
    const float q = fmaf(l[0], r[0], fmaf(l[1], r[1], l[2] * r[2]));
    for (int c = 0; c < C; ++c) {
        const float a0 = attributes[(int64_t)v[0] * C + c], a1 = attributes[(int64_t)v[1] * C + c], a2 = attributes[(int64_t)v[2] * C + c];
        out[c * plane + p] = fmaf(t[0], a0, fmaf(t[1], a1, t[2] * a2)) / q;
    }
}

// n: the pixel's normal, or zeros; returns nvalid
MR_FN uint8_t mr_normal_pixel(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const float* m, const MrView& view, const int32_t* face,
                              const float* depth, const uint8_t* valid, int32_t ix, int32_t iy, float* n) {
    const int64_t p = (int64_t)iy * view.W + ix;
    int32_t v[3];
    n[0] = n[1] = n[2] = 0.f;
    const int64_t f = face[p];
    if (!valid[p] || f < 0 || f >= nf || !ms_face(faces, f, nv, v, nullptr)) return 0;
    float A[3], B[3], Cc[3];
    mr_camera_point(m, vertices + 3 * (int64_t)v[0], A);
    mr_camera_point(m, vertices + 3 * (int64_t)v[1], B);
    mr_camera_point(m, vertices + 3 * (int64_t)v[2], Cc);
    const float e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
    const float e2x = Cc[0] - A[0], e2y = Cc[1] - A[1], e2z = Cc[2] - A[2];
    float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    if (!(dp_finite(len) && len > 0.f)) return 0;
    nx = nx / len; ny = ny / len; nz = nz / len;
    const DpVec Q = dp_point(ix, iy, depth[p], view.tanfovx, view.tanfovy, view.W, view.H);
    const bool away = (nx * Q.x + ny * Q.y) + nz * Q.z > 0.f;
    n[0] = away ? -nx : nx;
    n[1] = away ? -ny : ny;
    n[2] = away ? -nz : nz;
    return 1;
}

MR_FN void mr_shade_pixel(const float* color, const float* normals, const uint8_t* nvalid, const float* depth, const MrView& view, float ambient, const float* bg,
                          int32_t ix, int32_t iy, float* out) {
    const int64_t p = (int64_t)iy * view.W + ix, plane = (int64_t)view.H * view.W;
    if (!nvalid[p]) {
        for (int c = 0; c < 3; ++c) out[c * plane + p] = bg[c];
        return;
    }
    const DpVec Q = dp_point(ix, iy, depth[p], view.tanfovx, view.tanfovy, view.W, view.H);
    const float nx = normals[p], ny = normals[plane + p], nz = normals[2 * plane + p];
    const float s = fabsf((nx * Q.x + ny * Q.y) + nz * Q.z) / sqrtf((Q.x * Q.x + Q.y * Q.y) + Q.z * Q.z);
    const float L = fmaf(1.f - ambient, s, ambient);
    for (int c = 0; c < 3; ++c) out[c * plane + p] = color[c * plane + p] * L;
}

// ---- refusals and the scratch ----
inline const char* mr_refuse_sizes(int64_t nv, int64_t nf, int64_t H, int64_t W) {
    const char* why = ms_refuse_sizes(nv, nf);
    if (why) return why;
    if (H <= 0 || W <= 0) return "H and W must be > 0";
    if (H > GP_MESH_RENDER_MAX_SIZE || W > GP_MESH_RENDER_MAX_SIZE) return "H and W must be <= 16384";
    return nullptr;
}

inline const char* mr_refuse_view(float tanfovx, float tanfovy) {
    return (dp_finite(tanfovx) && dp_finite(tanfovy)) ? nullptr : "tanfovx and tanfovy must be finite";
}

inline const char* mr_refuse_raster(float tanfovx, float tanfovy, float z_near, int32_t cull) {
    const char* why = mr_refuse_view(tanfovx, tanfovy);
    if (why) return why;
    if (!(dp_finite(z_near) && z_near > 0.f)) return "z_near must be finite and > 0";
    if (cull != GP_MESH_RENDER_CULL_NONE && cull != GP_MESH_RENDER_CULL_BACK && cull != GP_MESH_RENDER_CULL_FRONT)
        return "cull must be GP_MESH_RENDER_CULL_NONE, GP_MESH_RENDER_CULL_BACK or GP_MESH_RENDER_CULL_FRONT";
    return nullptr;
}

// byte offsets, each 256-byte aligned
struct MrScratch { int64_t words, records, vis, wide, bytes; };
#define MR_WORD_WIDE 0                       // words[]: the entries of the list of wide faces

inline MrScratch mr_scratch_layout(int64_t nv, int64_t nf, int64_t H, int64_t W) {
    const auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    MrScratch s;
    int64_t at = 0;
    const auto take = [&](int64_t bytes) { const int64_t here = at; at += up(bytes); return here; };
    s.words = take(4 * 8);
    s.records = take(16 * nv);
    s.vis = take(8 * H * W);
    s.wide = take(4 * nf);
    s.bytes = at;
    return s;
}
