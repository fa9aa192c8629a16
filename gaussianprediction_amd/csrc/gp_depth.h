/* gp_depth.h -- depth renders on the device: the C entry points of csrc/depth_kernels.hip, a part of libgp_hip.so with an ABI number of
 * its own.  (The header lives beside the sources, not in include/: see DESIGN section 25.)
 *
 * What it adds: render() returns "depth" = sum z_i alpha_i T_i (gp_raster_outputs.depth of include/gp_hip.h) and nothing uses it.  One
 * ordinary render with an override colour of ones over a zero background gives sum alpha_i T_i (alpha) in the same pass; everything
 * after that composite is here: the quotient, the range, the picture, normals, the visible surface as a point cloud, and the standard
 * depth errors against a ground truth.
 *
 * Everything is float32, one correctly rounded operation at a time (the library is built without contraction; fmaf is one operation).
 *
 * The view.  cam2world: [16] float32 on the device, indexed m[col*4 + row]: the inverse of the camera's world_view_transform.  The
 * camera-space point of pixel (x, y) at depth z:
 *      xn = (float)(2*x + 1) / (float)W - 1.f     (the inverse of the projection kernel's pix = ((ndc + 1) * W - 1) * 0.5)
 *      yn = (float)(2*y + 1) / (float)H - 1.f
 *      P  = (xn * tanfovx * z, yn * tanfovy * z, z)        each product left to right
 *
 * 1. Resolve.  d = accum / alpha (IEEE division).  A pixel is VALID iff alpha >= alpha_min, d is finite and d > 0.  depth is d where
 *    valid, else 0; valid is 1 or 0.
 *
 * 2. Colour.  mode 0: v = depth; mode 1 (disparity): v = 1.f / depth.  A pixel is COLOURED iff its valid byte is non-zero (a NULL
 *    array: every pixel), v is finite and v > 0; otherwise it takes the background.  lo and hi are used where lo < hi; otherwise lo and
 *    hi are the smallest and the largest v over the coloured pixels, found in the same call by 32-bit integer atomic minimum and
 *    maximum over the bits of the positive floats (their order is the order of their bits) -- independent of the order -- and (0, 1)
 *    where there are none.  range[0], range[1] receive the pair used.  t = (v - lo) / (hi - lo), and t = 0 where hi == lo.  The colour
 *    is row (int)(t * 256.f) of lut for 0 <= t < 1, row 255 for t >= 1, row 0 otherwise (feature_vis.colormap's rule).
 *
 * 3. Normals, in camera space.  With P(x, y) the point of pixel (x, y) at its own depth:
 *      a = P(x + 1, y) - P(x - 1, y);  b = P(x, y + 1) - P(x, y - 1)
 *      n = (a_y*b_z - a_z*b_y,  a_z*b_x - a_x*b_z,  a_x*b_y - a_y*b_x)            each a difference of two products, as written
 *      len = sqrtf((n_x*n_x + n_y*n_y) + n_z*n_z);  n = n / len
 *      n is negated where (n_x*P_x + n_y*P_y) + n_z*P_z > 0 (P the pixel's own point): it faces the camera.
 *    nvalid iff the pixel and its four neighbours are inside the image and valid (a NULL array: every pixel is) and len is finite and
 *    > 0; otherwise the normal is (0, 0, 0) and nvalid 0.  The picture of the normals: n * 0.5f + 0.5f where nvalid, else the background.
 *
 * 4. Unproject.  world = cam2world . (P, 1), as the fmaf chains of the rasterizer's xform4x3:
 *      X_r = fmaf(m[r], P_x, fmaf(m[4 + r], P_y, fmaf(m[8 + r], P_z, m[12 + r])))     r = 0, 1, 2
 *    The outputs hold the VALID pixels only (a NULL array: every pixel), in row-major pixel order: row k of points is the world point of
 *    the k-th valid pixel, row k of colors (image[0..3) at that pixel), index[k] its pixel number y*W + x; count[0] (int32) is how many.
 *    Rows at and beyond count are left untouched.  An ordered stream compaction, deterministic by construction: per-tile counts over
 *    GP_DEPTH_TILE consecutive pixels by wave ballots, an exclusive scan of the tile counts by one workgroup, and a placing launch
 *    that ranks the pixels inside its tile by ballot prefix and wave offsets through LDS.
 *
 * 5. Metrics of pred against gt, per image b of B.  d = pred * scale[b], or pred itself where scale is NULL.  A pixel COUNTS iff its
 *    mask byte is non-zero (a NULL mask: every pixel), d and g are finite, d > 0, g > 0 and gt_min <= g <= gt_max.  Its terms:
 *      e = d - g;  |e| / g;  e*e / g;  e*e;  l = logf(d) - logf(g);  l*l;  l;  r = fmaxf(d / g, g / d) and the three indicators
 *      r < 1.25f, r < 1.5625f, r < 1.953125f;  d*g;  d*d;  g
 *    -- twelve sums with the count, in that order.  Row b of table [B][12] float64: count; AbsRel = sum |e|/g / count; SqRel =
 *    sum e*e/g / count; RMSE = sqrt(sum e*e / count); RMSE-log = sqrt(sum l*l / count); delta_1, delta_2, delta_3 as shares of the
 *    count; SIlog = mean(l*l) - mean(l)*mean(l); the least-squares scale sum d*g / sum d*d; mean g; 0.  count == 0: a row of NaN.
 *    logf(x) here is (float)log((double)x): the double-precision logarithm rounded once to float32, the one step of this header that is
 *    not a float32 operation.  A double logarithm is correctly rounded on neither host nor device, so the two log columns are defined
 *    up to a double rounding at a near-tie (about 2^-29 of the arguments).
 *    The sums: the plane is cut into tiles of GP_DEPTH_TILE consecutive pixels; lane t of the tile's 256 adds its pixels
 *    t, t + 256, t + 512, t + 768 in that order in float32, the 64 lanes of a wave are added by xor butterflies (32, 16, 8, 4, 2, 1), the
 *    four waves as (w0 + w1) + (w2 + w3), and the tile's twelve sums leave as float64 with plain stores into a slot of their own.  One
 *    workgroup per image then adds the slots: lane t the slots t, t + 256, ... in ascending order in float64, the 256 lanes by a tree
 *    of strides 128, 64, ..., 1 (lane t += lane t + stride).  No float atomics: two calls give equal bytes, row b of a batch is the B = 1 row.
 *
 * Conventions are those of gp_hip.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a gp_stream_t last.  No entry
 * synchronises or reads the device.  Refused everywhere: H or W <= 0, H*W >= 2^31, a null pointer where one is required, a NaN
 * scalar; B <= 0 or B > 65535; a view whose W, H are not the call's. */
#ifndef GP_DEPTH_H
#define GP_DEPTH_H

#include "../../include/gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_DEPTH_ABI_VERSION 1

#define GP_DEPTH_TILE 1024           /* pixels per workgroup of gp_depth_metrics, of gp_depth_unproject and of the range search */
#define GP_DEPTH_SUMS 12             /* count, |e|/g, e*e/g, e*e, l*l, l, r < 1.25, r < 1.25^2, r < 1.25^3, d*g, d*d, g */
#define GP_DEPTH_COLUMNS 12
#define GP_DEPTH_LUT 256

typedef struct gp_depth_view {
    const float* cam2world;          /* [16] on the device: the inverse of the camera's world_view_transform */
    float tanfovx, tanfovy;
    int32_t W, H;
} gp_depth_view;

int gp_depth_abi_version(void);

/* accum, alpha, depth: [H][W] float32; valid: [H][W] uint8, all on the device. */
int gp_depth_resolve(const float* accum, const float* alpha, float alpha_min, float* depth, uint8_t* valid, int32_t H, int32_t W,
                     gp_stream_t stream);

/* depth: [H][W]; valid: [H][W] uint8 or NULL; lut: [GP_DEPTH_LUT][3] float32; range: [2] float32 (written); out: [3][H][W] float32, all
 * on the device.  Refused also: a mode other than 0 or 1. */
int gp_depth_colorize(const float* depth, const uint8_t* valid, int32_t mode, float lo, float hi, const float* lut, float bg_r, float bg_g,
                      float bg_b, float* range, float* out, int32_t H, int32_t W, gp_stream_t stream);

/* view: on the HOST.  depth: [H][W]; valid: [H][W] uint8 or NULL; normals: [3][H][W] float32; nvalid: [H][W] uint8, on the device. */
int gp_depth_normals(const float* depth, const uint8_t* valid, const gp_depth_view* view, float* normals, uint8_t* nvalid, int32_t H,
                     int32_t W, gp_stream_t stream);

/* normals: [3][H][W]; nvalid: [H][W] uint8; out: [3][H][W] float32, on the device. */
int gp_depth_normals_image(const float* normals, const uint8_t* nvalid, float bg_r, float bg_g, float bg_b, float* out, int32_t H,
                           int32_t W, gp_stream_t stream);

/* The bytes of gp_depth_unproject's scratch: ceil(H*W / GP_DEPTH_TILE) uint32.  -1 (and gp_last_error()) where the sizes are refused. */
int64_t gp_depth_unproject_scratch_bytes(int32_t H, int32_t W);

/* view: on the HOST.  depth: [H][W]; valid: [H][W] uint8 or NULL; image: [3][H][W] float32 or NULL; points: [H*W][3] float32; colors:
 * [H*W][3] float32 or NULL (required with an image, refused without one); index: [H*W] int32 or NULL; count: [1] int32; scratch: as
 * sized above, 4-byte aligned, all on the device. */
int gp_depth_unproject(const float* depth, const uint8_t* valid, const float* image, const gp_depth_view* view, float* points,
                       float* colors, int32_t* index, int32_t* count, void* scratch, int32_t H, int32_t W, gp_stream_t stream);

/* The bytes of gp_depth_metrics' scratch: B * ceil(H*W / GP_DEPTH_TILE) * GP_DEPTH_SUMS doubles.  -1 (and gp_last_error()) where B <= 0,
 * B > 65535 (the images are the second dimension of the launch) or the sizes are refused; gp_depth_metrics refuses the same. */
int64_t gp_depth_metrics_scratch_bytes(int32_t B, int32_t H, int32_t W);

/* pred, gt: [B][H][W] float32; mask: [B][H][W] uint8 or NULL; scale: [B] float32 or NULL; scratch: as sized above, 8-byte aligned;
 * table: [B][GP_DEPTH_COLUMNS] float64, all on the device.  Refused also: a NaN gt_min or gt_max. */
int gp_depth_metrics(const float* pred, const float* gt, const uint8_t* mask, const float* scale, float gt_min, float gt_max, int32_t B,
                     int32_t H, int32_t W, void* scratch, double* table, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
