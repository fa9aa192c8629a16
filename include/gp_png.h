/* gp_png.h -- PNG encoding on the device, for the evaluation loops that write every rendered frame to disk: the C entry points of
 * csrc/png_kernels.hip, a part of libgp_hip.so with an ABI number of its own.
 *
 * Conventions are those of gp_hip.h: plain device pointers and sizes, a return code != 0 (or -1 from the int64_t queries) plus
 * gp_last_error(), no synchronisation and no host read inside any entry, a gp_stream_t last.  No atomic on global memory decides a
 * byte: two calls on equal inputs give equal files, and image b of a batch gives the file of the B = 1 call on that image.
 *
 * What they replace [REF eval.py:110,146,155,182,185,217,220]: torchvision.utils.save_image after every rendered frame.
 *
 * The file.  Signature, IHDR (8-bit RGB, no interlace), one IDAT chunk per band, IEND; every chunk CRC-32 and the zlib Adler-32 are
 * computed on the device.
 *   The filtered stream -- H rows of 1 + 3 W bytes, a filter type and the filtered RGB bytes -- is cut at every multiple of
 *   GP_PNG_BAND_BYTES (by byte position, not by row) into bands.
 *   A band is deflated with no reference before its first byte.  Its tokens are literals and distance-1 matches: inside a run of
 *   equal bytes the first byte is a literal, the bytes after it are cut into pieces of 258, and a piece of 3 or more bytes is one
 *   match, a shorter one literals.  A band is ONE dynamic-Huffman block (literal/length code lengths at most 15, a complete code; one
 *   distance code of length 1, the single-code case RFC 1951 allows; the code lengths sent with the repeat codes 16-18 under a
 *   complete code-length code of at most 7 bits) followed by an empty stored block, which ends the band on a byte boundary -- or one
 *   stored block when that is smaller.  The zlib header (78 01) opens the first chunk; a final empty stored block and the Adler-32
 *   close the last one.
 *   Without GP_PNG_FILTER_NONE every row takes, among the five filter types, the one with the smallest sum over its bytes of
 *   |filtered byte read as int8|; ties go to the lower type.
 *
 * Float input is quantised as GP_METRICS_QUANTIZE8 of gp_hip.h does it: floor(x * 255 + 0.5), one multiply and one add, clamped to
 * [0, 255]; a NaN gives 0.
 *
 * Limits: 1 <= B <= GP_PNG_MAX_BATCH, H >= 1, W >= 1, gp_png_bound(H, W) < 2^31 -- H * (3 W + 1) up to about 2.145e9 -- so that a file's
 * length fits a signed 32-bit word as well as the uint32 it is written as. */
#ifndef GP_PNG_H
#define GP_PNG_H

#include "gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_PNG_ABI_VERSION 1

#define GP_PNG_BAND_BYTES 16384   /* bytes of the filtered stream per band (one IDAT chunk, one workgroup); a multiple of 256 */
#define GP_PNG_MAX_BATCH 65535

#define GP_PNG_SRC_F32 0          /* src: float32 [B][3][H][W], as the rasterizer writes it */
#define GP_PNG_SRC_U8 1           /* src: uint8 [B][3][H][W], quant_out of gp_image_metrics */

#define GP_PNG_FILTER_NONE 1u     /* every row filter type 0 (tests; debugging a decoder mismatch) */

int gp_png_abi_version(void);

/* The largest file an H x W image can become, in bytes, a multiple of 8: every band stored (5 bytes of block header each), 12 bytes
 * of chunk framing per band, the zlib header and trailer, signature, IHDR and IEND.  -1 outside the limits. */
int64_t gp_png_bound(int32_t H, int32_t W);

/* Bytes of `scratch` (256-byte aligned, uninitialised on entry) for gp_png_encode; -1 outside the limits. */
int64_t gp_png_scratch_bytes(int32_t B, int32_t H, int32_t W);

/* out + b * out_stride receives the complete PNG file of image b, sizes[b] its length.  Bytes of the slot at and beyond sizes[b] are
 * not written.  out_stride >= gp_png_bound(H, W) is required (checked here), so no file can overflow its slot.  src_kind: GP_PNG_SRC_*;
 * flags: GP_PNG_FILTER_NONE or 0.  Four launches whatever B is. */
int gp_png_encode(int32_t B, int32_t H, int32_t W, const void* src, int32_t src_kind, uint32_t flags, uint8_t* out, int64_t out_stride,
                  uint32_t* sizes, void* scratch, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
