/* gp_resize.h -- Pillow-exact image resizing on the device, for the metrics and the loaders that score or train at a reduced
 * resolution: the C entry points of csrc/resize_kernels.hip, a part of libgp_hip.so with an ABI number of its own.
 *
 * Conventions are those of gp_hip.h: plain device pointers and sizes, a return code != 0 (or -1 from a query) plus gp_last_error(),
 * no synchronisation and no host read inside any entry, a gp_stream_t last.  Nothing is atomic and nothing depends on an order: two
 * calls on equal inputs give equal bytes, and image b of a batch gives the bytes of the B = 1 call on that image.
 *
 * What they replace: Image.open(f).resize((int(w * ratio), int(h * ratio))) [REF metrics.py readImages] and PILtoTorch's resize
 * [REF utils/general_utils.py:21-27].  The result is Pillow's byte for byte, for its five convolution filters and the modes L, RGB
 * and RGBA.
 *
 * The algorithm, per axis (in -> out samples, a filter f of support s):
 *   scale = in / out, fs = max(scale, 1), support = s fs, ksize = (int)ceil(support) * 2 + 1 taps at most.  For output sample xx:
 *   center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0), n = min((int)(center + support + 0.5), in) - xmin,
 *   w[x] = f((x + xmin - center + 0.5) * (1 / fs)), normalised by their sum in index order, k[x] = (int)(w 2^22 -+ 0.5) truncating
 *   toward zero.  All of it in double without contraction (gp_resize_coeffs, on the host).
 *   One pass: ss = 2^21 + sum_{x < n} pixel[xmin + x] * k[x] in int32; the byte is clamp(ss >> 22, 0, 255), the shift arithmetic.
 * A resize is the horizontal pass over the source rows, then the vertical pass over its 8-bit result; a pass whose axis keeps its
 * size is skipped, and equal sizes are a copy.  With alpha_mode (C = 4) the colours are premultiplied on load, c' = ((t >> 8) + t) >> 8
 * with t = c alpha + 128, all four planes are resampled, and on the store a colour stays where alpha is 0 or 255 and is
 * min(255, (255 c') / alpha) elsewhere -- but never on a copy, which Image.resize returns untouched.
 *
 * Limits: 1 <= B, C in {1, 3, 4}, B * C <= 65535, every size in [1, 65535], at most 2^24 taps per sample. */
#ifndef GP_RESIZE_H
#define GP_RESIZE_H

#include "gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_RESIZE_ABI_VERSION 1

/* filters: Pillow's Image.Resampling values */
#define GP_RESIZE_LANCZOS 1
#define GP_RESIZE_BILINEAR 2
#define GP_RESIZE_BICUBIC 3
#define GP_RESIZE_BOX 4
#define GP_RESIZE_HAMMING 5

#define GP_RESIZE_DST_U8 0
#define GP_RESIZE_DST_F32 1          /* float32 = byte / 255, one correctly rounded division: torch's uint8.to(float32) / 255.0 */

/* what gp_resize_path answers */
#define GP_RESIZE_PATH_COPY 0        /* equal sizes */
#define GP_RESIZE_PATH_FUSED 1       /* both passes in one launch, the 8-bit intermediate in LDS */
#define GP_RESIZE_PATH_TWO_LAUNCH 2  /* the tile's window is beyond the LDS budget: the intermediate goes through `scratch` */
#define GP_RESIZE_PATH_HORIZONTAL 3  /* the height stays: one pass */
#define GP_RESIZE_PATH_VERTICAL 4    /* the width stays: one pass */

/* output pixels of one workgroup of the fused path */
#define GP_RESIZE_TILE_W 64
#define GP_RESIZE_TILE_H 32

int gp_resize_abi_version(void);

/* Taps per output sample of an axis in -> out; -1 for a size below 1, an unknown filter or more than 2^24 taps. */
int gp_resize_ksize(int32_t in, int32_t out, int32_t filter);

/* The tables of one axis, on the HOST: bounds [out][2] = (xmin, n), coeffs [out][ksize], zero beyond n.  No device is touched. */
int gp_resize_coeffs(int32_t in, int32_t out, int32_t filter, int32_t* bounds, int32_t* coeffs);

/* Bytes of `scratch` (256-byte aligned, uninitialised on entry) for gp_resize_u8: 0 on every path but the two-launch one; -1 outside
 * the limits. */
int64_t gp_resize_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t filter);

/* GP_RESIZE_PATH_* for these sizes: the boundary between the fused and the two-launch path is the byte count of the fused
 * workgroup's LDS (its coefficients and its window of source rows) against a budget of 32 KiB; -1 outside the limits. */
int gp_resize_path(int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t filter);

/* src: B images [C][H][W] planar uint8, src_stride bytes from one image to the next (>= C H W).  The tables are gp_resize_coeffs' of
 * (W, Wo, filter) and (H, Ho, filter), copied to the device; xtaps and ytaps are their ksize.  An axis that keeps its size takes no
 * table (its pointers may be NULL).  dst: [C][Ho][Wo] planar per image, dst_kind GP_RESIZE_DST_*, dst_stride BYTES from one image to
 * the next (>= C Ho Wo elements; a multiple of 4 for float32).  alpha_mode 1 needs C = 4 and uses plane 3.  scratch: NULL where
 * gp_resize_scratch_bytes is 0.  One launch, or two on the two-launch path. */
int gp_resize_u8(int32_t B, int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t filter, const uint8_t* src,
                 int64_t src_stride, const int32_t* xbounds, const int32_t* xcoeffs, int32_t xtaps, const int32_t* ybounds,
                 const int32_t* ycoeffs, int32_t ytaps, int32_t alpha_mode, int32_t dst_kind, void* dst, int64_t dst_stride,
                 void* scratch, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
