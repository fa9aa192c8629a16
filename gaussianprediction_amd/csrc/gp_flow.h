/* gp_flow.h -- optical flow rendered on the device: the C entry points of csrc/flow_kernels.hip, a part of libgp_hip.so with an ABI
 * number of its own.  (The header lives beside the sources, not in include/: see DESIGN section 24.)
 *
 * What it adds: the reference's cameras carry fwd_flow / bwd_flow and its render loops unwrap "optical flow" view dicts, and nothing
 * there renders a flow.  Here the composite renders one: every Gaussian's screen displacement goes through the rasterizer as an
 * unclamped override colour with a third channel of ones, and the quotient of the composite is the flow.
 *
 * Everything is float32, one correctly rounded operation at a time (the library is built without contraction; fmaf is one operation).
 *
 * 1. Screen displacement.  A view is the rasterizer's: viewmatrix and projmatrix as [16] float32 on the device, indexed m[col*4 + row],
 *    plus W and H.  The pixel centre of a point (x, y, z) is the projection kernel's own, in its order:
 *      depth = fmaf(v[2], x, fmaf(v[6], y, fmaf(v[10], z, v[14])))                       (v = viewmatrix); the point passes iff depth > 0.2f
 *      h_r   = fmaf(p[r], x, fmaf(p[4 + r], y, fmaf(p[8 + r], z, p[12 + r])))  r = 0, 1, 3  (p = projmatrix)
 *      pw = 1.f / (h_3 + 0.0000001f);  ndc = h_r * pw;  pix.x = ((ndc_0 + 1.f) * (float)W - 1.f) * 0.5f,  pix.y likewise with H
 *    Row i of out is (pix1.x - pix0.x, pix1.y - pix0.y, 1) where point i of xyz0 passes in view0, point i of xyz1 passes in view1 and
 *    all four coordinates are finite, and (0, 0, 0) otherwise.
 *
 * 2. Resolve.  Per pixel of a composite [3][H][W] rendered from those rows over a ZERO background: alpha = composite[2] (as it is),
 *    u = composite[0] / alpha, v = composite[1] / alpha (IEEE divisions); the pixel is VALID iff alpha >= alpha_min and u and v are
 *    finite; flow = (u, v) where valid, else (0, 0); valid is 1 or 0.
 *
 * 3. Colour: the Middlebury colour wheel.  55 rows from the segments RY 15, YG 6, GC 4, CB 11, BM 13, MR 6, as integers
 *      RY i: (255, 255*i / 15, 0)   YG i: (255 - 255*i / 6, 255, 0)   GC i: (0, 255, 255*i / 4)
 *      CB i: (0, 255 - 255*i / 11, 255)   BM i: (255*i / 13, 0, 255)   MR i: (255, 0, 255 - 255*i / 6)        (integer divisions)
 *    each divided by 255.f.  Per pixel with scale s:  u = flow_u / s, v = flow_v / s;  rad = sqrtf(u*u + v*v);
 *      a = atan2f(-v, -u) / 3.14159265358979323846f;  fk = ((a + 1.f) / 2.f) * 54.f;  k0 = floorf(fk) (held in [0, 54]);
 *      f = fk - k0;  k1 = (k0 + 1) % 55;  col = (1.f - f) * wheel[k0][c] + f * wheel[k1][c];
 *      col = 1.f - rad * (1.f - col) where rad <= 1.f, else col * 0.75f.
 *    A pixel whose valid byte is 0 (with a valid array) or whose flow is not finite takes background[c].  The scale: max_flow where
 *    max_flow > 0; otherwise the largest FINITE sqrtf(fu*fu + fv*fv) over the pixels that do not take the background, found in the same
 *    call by an integer atomic maximum over the bits of the (non-negative) magnitudes -- independent of the order -- and 1 where
 *    there is none or it is 0.  scale[0] receives max_flow, or that largest magnitude (0 where there is none).  atan2f is not
 *    correctly rounded: the colours are defined up to its error.  Parity with flow_vis / cv2 is unpinned.
 *
 * 4. Metrics of flow against gt, per image b of B.  A pixel COUNTS iff mask[b][p] != 0 (a NULL mask: every pixel) and its four values
 *    are finite.  du = flow_u - gt_u, dv likewise; epe = sqrtf(du*du + dv*dv); mag = sqrtf(gt_u*gt_u + gt_v*gt_v).  Row b of table
 *    [B][8] float64: count; sum epe / count; the shares of the counted pixels with epe > 1.f, > 3.f, > 5.f; the share with
 *    epe > 3.f and epe > 0.05f * mag (KITTI's Fl); sum mag / count; 0.  count == 0: a row of NaN.
 *    The sums: the plane is cut into tiles of GP_FLOW_TILE consecutive pixels; lane t of the tile's 256 adds its pixels
 *    t, t + 256, t + 512, t + 768 in that order in float32, the 64 lanes of a wave are added by xor butterflies (32, 16, 8, 4, 2, 1), the
 *    four waves as (w0 + w1) + (w2 + w3), and the tile's seven sums leave as float64 with plain stores into a slot of their own.  One
 *    workgroup per image then adds the slots: lane t the slots t, t + 256, ... in ascending order in float64, the 256 lanes by a tree
 *    of strides 128, 64, ..., 1 (lane t += lane t + stride).  No float atomics: two calls give equal bytes, row b of a batch is the B = 1 row.
 *
 * 5. Warp.  out[c](x, y) = bilinear(image[c], x + flow_u(x, y), y + flow_v(x, y)):  sx = (float)x + flow_u, sy likewise; a sample
 *    position that is not finite gives 0.  x0 = floorf(sx), ax = sx - x0, y0 and ay likewise; the four taps (y0, x0), (y0, x0 + 1),
 *    (y0 + 1, x0), (y0 + 1, x0 + 1) have the weights (1.f - ay)*(1.f - ax), (1.f - ay)*ax, ay*(1.f - ax), ay*ax, each product formed
 *    first; a tap outside the image has the value 0; out = ((w00*v00 + w01*v01) + w10*v10) + w11*v11.
 *
 * Conventions are those of gp_hip.h: plain pointers and sizes, a return code != 0 plus gp_last_error(), a gp_stream_t last.  No entry
 * synchronises or reads the device. */
#ifndef GP_FLOW_H
#define GP_FLOW_H

#include "../../include/gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_FLOW_ABI_VERSION 1

#define GP_FLOW_TILE 1024            /* pixels per workgroup of gp_flow_metrics */
#define GP_FLOW_SUMS 7               /* count, epe, > 1, > 3, > 5, Fl, |gt| */
#define GP_FLOW_COLUMNS 8
#define GP_FLOW_WHEEL 55

typedef struct gp_flow_view {
    const float* viewmatrix;         /* [16] on the device: the camera's world_view_transform */
    const float* projmatrix;         /* [16] on the device: its full_proj_transform */
    int32_t W, H;
} gp_flow_view;

int gp_flow_abi_version(void);

/* view0, view1: on the HOST (view1 may be view0).  xyz0, xyz1: [N][3] float32; out: [N][3] float32, all on the device.  N == 0 launches
 * nothing.  Refused: N < 0 or N >= 2^31; W or H <= 0; a null pointer. */
int gp_flow_project(const gp_flow_view* view0, const gp_flow_view* view1, const float* xyz0, const float* xyz1, int64_t N, float* out,
                    gp_stream_t stream);

/* composite: [3][H][W]; flow: [2][H][W]; alpha: [H][W] float32; valid: [H][W] uint8, all on the device.  Refused: H or W <= 0,
 * H*W >= 2^31, a NaN alpha_min, a null pointer. */
int gp_flow_resolve(const float* composite, float alpha_min, float* flow, float* alpha, uint8_t* valid, int32_t H, int32_t W,
                    gp_stream_t stream);

/* flow: [2][H][W]; valid: [H][W] uint8 or NULL; scale: [1] float32 (written); out: [3][H][W] float32, all on the device.  Refused: the
 * sizes as above, a NaN max_flow, a null pointer. */
int gp_flow_colorize(const float* flow, const uint8_t* valid, float max_flow, float bg_r, float bg_g, float bg_b, float* scale, float* out,
                     int32_t H, int32_t W, gp_stream_t stream);

/* The bytes of gp_flow_metrics' scratch: B * ceil(H*W / GP_FLOW_TILE) * GP_FLOW_SUMS doubles.  -1 (and gp_last_error()) where B <= 0,
 * B > 65535 (the images are the second dimension of the launch) or the sizes are refused as above; gp_flow_metrics refuses the same. */
int64_t gp_flow_metrics_scratch_bytes(int32_t B, int32_t H, int32_t W);

/* flow, gt: [B][2][H][W] float32; mask: [B][H][W] uint8 or NULL; scratch: as sized above, 8-byte aligned; table: [B][GP_FLOW_COLUMNS]
 * float64, all on the device. */
int gp_flow_metrics(const float* flow, const float* gt, const uint8_t* mask, int32_t B, int32_t H, int32_t W, void* scratch, double* table,
                    gp_stream_t stream);

/* image, out: [C][H][W] float32; flow: [2][H][W] float32, all on the device; out must not overlap image.  Refused: C <= 0, the sizes as
 * above, C*H*W >= 2^31, a null pointer. */
int gp_flow_warp(const float* image, const float* flow, float* out, int32_t C, int32_t H, int32_t W, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
