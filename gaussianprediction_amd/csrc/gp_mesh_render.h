/* gp_mesh_render.h -- a triangle rasterizer on the device: a mesh and a camera become a face plane, a depth plane, barycentrics,
 * interpolated attributes, face normals and a headlight-shaded picture.  The C entry points of csrc/mesh_render_kernels.hip, a part
 * of libgp_hip.so with an ABI number of its own.  (The header lives beside the sources, not in include/: see DESIGN section 29.)
 *
 * What it adds: gp_tsdf.h, gp_mesh.h and gp_mesh_simplify.h end in a mesh that nothing here could draw.  With this the mesh is
 * rendered from any camera and compared, pixel by pixel, with the depth render it was fused from (gp_depth.h's metrics).
 *
 * Everything is float32, one correctly rounded operation at a time (the library is built without contraction; fmaf is one operation);
 * coverage is decided in 64-bit integers.  Every result is independent of the order in which the triangles are processed.
 *
 * A mesh: vertices [nv][3] float32, faces [nf][3] int32, on the device, gp_mesh.h's sizes (nv < 2^31, 3*nf < 2^31); nv = 0 and nf = 0
 * are accepted and give an empty picture.  A view: world_view [16] float32 on the device, the camera's world_view_transform as
 * stored, m[col*4 + row]; the tangents of its half angles; W and H, 1 .. GP_MESH_RENDER_MAX_SIZE each.  The camera looks along +z,
 * x to the right, y down.
 *
 * 1. Vertices, one record of 16 bytes each (X, Y int32; r float32; flags uint32), once per view.
 *      P_r = fmaf(m[r], x, fmaf(m[4 + r], y, fmaf(m[8 + r], z, m[12 + r])))     r = 0, 1, 2          (gp_tsdf.h's)
 *      NEAR unless P_z > z_near                                                                       (a NaN P_z is NEAR)
 *      xn = P_x / (P_z * tanfovx);  px = ((xn + 1.f) * (float)W - 1.f) * 0.5f;  the same with P_y, tanfovy, H for py
 *      sx = floorf(fmaf(px, 256.f, 0.5f)), sy likewise: 8 sub-pixel bits; pixel (ix, iy) is sampled at (256*ix, 256*iy)
 *      OUT OF RANGE unless sx and sy are finite and |sx|, |sy| <= 2^23 (compared as floats);  X = (int)sx, Y = (int)sy, 0 where not
 *      r = 1.f / P_z
 *    flags: bit 0 NEAR, bit 1 OUT OF RANGE (each on its own: a NEAR vertex's range bit is whatever the formulas above give).
 *
 * 2. Faces.  For a face (a, b, c), in the snapped integers, E_UV(P) = (Vx-Ux)*(Py-Uy) - (Vy-Uy)*(Px-Ux) in int64: with |X|, |Y| <=
 *    2^23 and W, H <= 2^14 every product stays below 2^51.  A face is tested in this order and DROPPED WHOLE at the first that holds:
 *      an index outside [0, nv)      counted in counts[STATUS] (so STATUS != 0 iff there was one); the rest is still drawn
 *      a NEAR corner                 counts[NEAR]
 *      an OUT OF RANGE corner        counts[OUT_OF_RANGE]
 *      area2 = E_AB(C) == 0          counts[DEGENERATE]
 *      culled                        counts[CULLED]
 *    and is otherwise DRAWN (counts[DRAWN], whether or not it covers a sample).  There is NO CLIPPING: a triangle that crosses the
 *    near plane or leaves the guard band of 2^23 sub-pixels (2^15 pixels) is dropped whole.  The triangles of a TSDF mesh are
 *    voxel-sized; this costs the geometry that touches the camera.
 *    Facing: area2 < 0 iff the geometric normal (b - a) x (c - a) faces the camera (x right, y down, z away).  cull BACK drops
 *    area2 > 0, cull FRONT drops area2 < 0.
 *    Coverage.  s = +1 where area2 > 0, -1 where area2 < 0 (that is: B and C swapped).  For the sample P of a pixel, in the face's
 *    STORED order
 *      w_0 = s * E_BC(P),  w_1 = s * E_CA(P),  w_2 = s * E_AB(P)         (w_0 + w_1 + w_2 = |area2|)
 *    and the edge of w_i runs along d_i = s * (C - B), s * (A - C), s * (B - A).  P is INSIDE iff for every i: w_i > 0, or w_i == 0
 *    and the edge OWNS it: d_y > 0 || (d_y == 0 && d_x > 0).  Exactly one of an edge and its reverse owns, so a sample on a shared
 *    edge or vertex of a consistently oriented surface belongs to exactly one triangle.  Candidates: the pixels with 256*ix in
 *    [min X, max X] and 256*iy in [min Y, max Y], clamped to the image (the face's BOX).
 *    Depth.  l_i = (float)((double)w_i / (double)|area2|) (exact conversions, one IEEE division, one rounding to float32; a zero is
 *    +0.0), the barycentrics in the stored order;
 *      q = fmaf(l_0, r_a, fmaf(l_1, r_b, l_2 * r_c));  z = 1.f / q;  the sample COUNTS iff it is inside, z is finite and z > 0.
 *    Visibility.  key = ((uint64)bits(z) << 32) | face.  The buffer [H][W] uint64 starts at all ones and takes the 64-bit unsigned
 *    atomic minimum of the keys of the counting samples: the nearest surface wins, at equal depth bits the smaller face number,
 *    whatever the order of arrival.  coverage (optional, [H][W] int32, zeroed here): += 1 per counting sample, integer atomic add.
 *    The launches: a lane per face draws a face whose box holds at most GP_MESH_RENDER_NARROW_MAX pixels itself (a plain load of the
 *    current key first: the atomic is left out where the key is not smaller -- keys only decrease); the others (counts[WIDE]) go,
 *    by a wave ballot and one atomic add per wave, into a list in the scratch, and a second launch of fixed size draws them,
 *    GP_MESH_RENDER_SPLIT waves per entry, each spreading 8 x 8 blocks of the box over its 64 lanes.  Nothing is read in between.
 *
 * 3. Resolve, a lane per pixel: for the winning face, w_i, l_i and z again through the same functions (equal bits).
 *      face [H][W] int32, -1 for none;  depth [H][W] float32, 0 for none;  valid [H][W] uint8;  bary [3][H][W] float32, 0 for none.
 *
 * 4. Interpolate.  attributes [nv][C] float32, 1 <= C <= GP_MESH_RENDER_MAX_CHANNELS, to out [C][H][W], perspective-correct:
 *      t_i = l_i * r_i;  q as above;  out_c = fmaf(t_0, a_0c, fmaf(t_1, a_1c, t_2 * a_2c)) / q;  background[c] where not valid.
 *
 * 5. Normals.  The face normal in camera space, from the un-snapped camera points of the corners (P as in 1.):
 *      e1 = P_b - P_a;  e2 = P_c - P_a;  n = (e1_y*e2_z - e1_z*e2_y,  e1_z*e2_x - e1_x*e2_z,  e1_x*e2_y - e1_y*e2_x)
 *      len = sqrtf((n_x*n_x + n_y*n_y) + n_z*n_z);  n = n / len
 *      negated where (n_x*Q_x + n_y*Q_y) + n_z*Q_z > 0, Q the pixel's point at the mesh depth by gp_depth.h's P(x, y): section 3's
 *      rule there, so that depth_ops.normals_image colours it unchanged.
 *    nvalid iff the pixel is valid and len is finite and > 0; otherwise (0, 0, 0) and 0.
 *
 * 6. Shade: a headlight at the camera.  Q as above;  s = fabsf((n_x*Q_x + n_y*Q_y) + n_z*Q_z) / sqrtf((Q_x*Q_x + Q_y*Q_y) + Q_z*Q_z)
 *      L = fmaf(1.f - ambient, s, ambient);  out_c = color_c * L  where nvalid, the background elsewhere.  color: [3][H][W].
 *
 * counts: [GP_MESH_RENDER_COUNT_WORDS] int32 on the device, zeroed by gp_mesh_render_rasterize (tallied by wave ballots; integer atomic adds, one per workgroup and word).
 * The scratch: gp_mesh_render_scratch_bytes(nv, nf, H, W) bytes, 256-byte aligned by the caller's allocator, refused unless 16-byte
 * aligned: one word block, the vertex records, the visibility buffer, the list.  gp_mesh_render_resolve and
 * gp_mesh_render_interpolate read what gp_mesh_render_rasterize left there (the same stream, sizes and scratch).
 *
 * Conventions are those of gp_hip.h and gp_mesh.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a gp_stream_t
 * last.  No entry synchronises or reads the device.  Refused everywhere, before any pointer is looked at: nv or nf < 0 or beyond
 * gp_mesh.h's sizes; H or W <= 0 or > GP_MESH_RENDER_MAX_SIZE; then a null or unaligned scratch, a null array that the sizes make
 * non-empty, non-finite tangents, a z_near that is not finite or not > 0, an unknown cull mode, C outside 1 ..
 * GP_MESH_RENDER_MAX_CHANNELS, an ambient that is not finite. */
#ifndef GP_MESH_RENDER_H
#define GP_MESH_RENDER_H

#include "../../include/gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_MESH_RENDER_ABI_VERSION 1

#define GP_MESH_RENDER_NARROW_MAX 64         /* the pixels of a box a single lane walks at the most */
#define GP_MESH_RENDER_SPLIT 16              /* the waves that share one entry of the list of wide faces */
#define GP_MESH_RENDER_MAX_SIZE 16384        /* W and H at the most */
#define GP_MESH_RENDER_MAX_CHANNELS 8
#define GP_MESH_RENDER_SUBPIXEL 256          /* snapped units per pixel */
#define GP_MESH_RENDER_GUARD 8388608         /* 2^23: |X|, |Y| at the most */

#define GP_MESH_RENDER_CULL_NONE 0
#define GP_MESH_RENDER_CULL_BACK 1
#define GP_MESH_RENDER_CULL_FRONT 2

#define GP_MESH_RENDER_STATUS 0              /* counts[]: faces with an index out of range */
#define GP_MESH_RENDER_DRAWN 1
#define GP_MESH_RENDER_NEAR 2
#define GP_MESH_RENDER_OUT_OF_RANGE 3
#define GP_MESH_RENDER_DEGENERATE 4
#define GP_MESH_RENDER_CULLED 5
#define GP_MESH_RENDER_WIDE 6                /*           drawn faces whose box holds more than GP_MESH_RENDER_NARROW_MAX pixels */
#define GP_MESH_RENDER_COUNT_WORDS 8

int gp_mesh_render_abi_version(void);

/* The bytes of the scratch.  -1 (and gp_last_error()) where the sizes are refused. */
int64_t gp_mesh_render_scratch_bytes(int64_t nv, int64_t nf, int32_t H, int32_t W);

/* coverage: [H][W] int32 or NULL; counts: [GP_MESH_RENDER_COUNT_WORDS] int32, on the device. */
int gp_mesh_render_rasterize(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const float* world_view, float tanfovx, float tanfovy,
                             int32_t H, int32_t W, float z_near, int32_t cull, void* scratch, int32_t* coverage, int32_t* counts, gp_stream_t stream);

/* After gp_mesh_render_rasterize.  face: [H][W] int32; depth: [H][W] float32; valid: [H][W] uint8; bary: [3][H][W] float32. */
int gp_mesh_render_resolve(const int32_t* faces, int64_t nv, int64_t nf, int32_t H, int32_t W, const void* scratch, int32_t* face, float* depth, uint8_t* valid,
                           float* bary, gp_stream_t stream);

/* After gp_mesh_render_rasterize.  attributes: [nv][C]; face, valid, bary: as resolve left them; background: [C] float32 on the HOST;
 * out: [C][H][W]. */
int gp_mesh_render_interpolate(const float* attributes, int32_t C, const int32_t* faces, int64_t nv, int64_t nf, int32_t H, int32_t W, const void* scratch,
                               const int32_t* face, const uint8_t* valid, const float* bary, const float* background, float* out, gp_stream_t stream);

/* face, depth, valid: as resolve left them; normals: [3][H][W] float32; nvalid: [H][W] uint8. */
int gp_mesh_render_normals(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const float* world_view, float tanfovx, float tanfovy, int32_t H,
                           int32_t W, const int32_t* face, const float* depth, const uint8_t* valid, float* normals, uint8_t* nvalid, gp_stream_t stream);

/* color, normals: [3][H][W]; nvalid: [H][W] uint8; depth: [H][W]; out: [3][H][W]. */
int gp_mesh_render_shade(const float* color, const float* normals, const uint8_t* nvalid, const float* depth, float tanfovx, float tanfovy, int32_t H, int32_t W,
                         float ambient, float bg_r, float bg_g, float bg_b, float* out, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
