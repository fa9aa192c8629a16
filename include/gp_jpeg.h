/* gp_jpeg.h -- baseline JPEG encoding on the device, for the render loops that end in a video or a JPEG file: the C entry points of
 * csrc/jpeg_kernels.hip, a part of libgp_hip.so with an ABI number of its own.
 *
 * Conventions are those of gp_hip.h and gp_png.h: plain device pointers and sizes, a return code != 0 (or -1 from the int64_t queries)
 * plus gp_last_error(), no synchronisation and no host read inside any entry, a gp_stream_t last.  No atomic on global memory decides
 * a byte: two calls on equal inputs give equal files, and image b of a batch gives the file of the B = 1 call on that image.
 *
 * What they serve [REF eval.py:113-115, train_GCN.py:45-53,147, metrics.py:148]: the video of the rendered frames (Motion-JPEG, every
 * frame a complete JPEG file; the container is host bookkeeping, jpeg_ops.VideoWriter) and the error images deltas/%05d.jpg.
 *
 * The file.  Baseline sequential JPEG: SOI, APP0 (JFIF 1.01, no units, density 1:1), two DQT, SOF0 (8 bits, three components Y Cb Cr
 * full range, ids 1 2 3), four DHT (the Annex K.3 "typical" tables: DC 0, AC 0, DC 1, AC 1), DRI, SOS, the entropy-coded segments
 * with RST markers between them, EOI.  GP_JPEG_HEAD_BYTES bytes stand before the first entropy-coded byte.
 *
 *   Stage 1, colour.  R G B are 8-bit (float input is quantised exactly as gp_png_encode does it: floor(x * 255 + 0.5), one multiply
 *   and one add, clamped to [0, 255]; a NaN gives 0).  With 16 fractional bits, rounded to nearest and clamped to [0, 255]:
 *       Y  = ( 19595 R + 38470 G +  7471 B            + 32768) >> 16
 *       Cb = (-11058 R - 21710 G + 32768 B + (128<<16) + 32768) >> 16
 *       Cr = ( 32768 R - 27439 G -  5329 B + (128<<16) + 32768) >> 16
 *   (0.299, 0.587, 0.114; 0.168736, 0.331264, 0.5; 0.5, 0.418688, 0.081312 times 65536; each row of constants sums to 65536 or 0).
 *
 *   Stage 2, subsampling.  The three planes are extended to a whole number of MCUs -- 16 x 16 pixels with GP_JPEG_420, 8 x 8 with
 *   GP_JPEG_444 -- by replicating the last row and the last column.  GP_JPEG_420: a chroma sample is the mean of its 2 x 2 pixels,
 *   (a + b + c + d + 2) >> 2, and an MCU is four Y blocks (left to right, top to bottom), one Cb and one Cr.  GP_JPEG_444: one block each.
 *
 *   Stage 3, transform.  s = sample - 128; F = C s C^T with C[u][x] = a(u) cos((2 x + 1) u pi / 16), a(0) = sqrt(1/8), a(u) = 1/2: the
 *   orthonormal 8 x 8 DCT-II.  In integers throughout: K[u][x] = round(C[u][x] * 2^24);
 *       rows:     r[y][u] = (sum_x K[u][x] s[y][x] + 4) >> 3                  (64-bit sum, the result holds 21 fractional bits)
 *       columns:  F16[v][u] = (sum_y K[v][y] r[y][u] + 2^28) >> 29            (64-bit sum, the result holds 16 fractional bits)
 *       quantise: |coefficient| = (|F16| + (q << 15)) / (q << 16), the sign of F16: round-half-away(F / q); AC magnitudes are capped
 *                 at 1023 (the exact transform reaches 1020 at most).
 *   Error against the exact transform: |K / 2^24 - C| <= 2^-25 and |s| <= 128, so a row sum is off by at most 8 * 128 * 2^-25 = 2^-15
 *   and its rounding adds 2^-22; a column sum is then off by at most 2^-25 * 8 * 363 (|r| <= 128 * sum|C| < 363) + 2.83 * (2^-15 + 2^-22)
 *   < 1.74e-4, and the last rounding adds 2^-17: |F16 / 2^16 - F| < GP_JPEG_DCT_ERR = 2^-12 (2.44e-4).  A quantised coefficient can
 *   therefore differ from round-half-away(F / q) of the exact F only where F / q lies within GP_JPEG_DCT_ERR / q of a half-integer, and
 *   then by one.
 *
 *   Stage 4, entropy coding.  Zigzag order; the DC difference against the component's previous block (0 at the start of a restart
 *   interval); ZRL for every 16 zeros before a non-zero coefficient; EOB unless coefficient 63 is non-zero.  After every
 *   GP_JPEG_RESTART_MCUS MCUs (counted in raster order of the MCUs, across MCU rows) and after the last MCU the last byte is padded
 *   with one-bits; between intervals stands RST(m mod 8), m the number of the interval that ends.  A data byte 0xFF is followed by 0x00.
 *
 * The largest file (gp_jpeg_bound).  A block of 64 maximal coefficients costs the longest DC code (11 bits, chroma) + 11 bits, and
 * 63 * (16 + 10) bits: GP_JPEG_BLOCK_BITS = 1660.  An interval of n MCUs of k blocks (6 or 3) is at most ceil(1660 k n / 8) bytes, the
 * padding included, doubled by byte stuffing; every interval is followed by two bytes (RST or EOI); GP_JPEG_HEAD_BYTES in front.
 * One interval of 8 4:2:0 MCUs: 19920 bytes at most, which with the bits before stuffing (9968), the blocks (13824 + 6336), the
 * code tables (2144) and the prefix sums (2440) is 54632 bytes of the workgroup's LDS.
 *
 * Limits: 1 <= B <= GP_JPEG_MAX_BATCH, 1 <= H, W <= 65535 (SOF0 holds 16 bits), gp_jpeg_bound(H, W, s) < 2^31. */
#ifndef GP_JPEG_H
#define GP_JPEG_H

#include "gp_hip.h"
#include "gp_png.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_JPEG_ABI_VERSION 1

#define GP_JPEG_RESTART_MCUS 8     /* MCUs per restart interval: one workgroup, one independent entropy-coded segment */
#define GP_JPEG_BLOCK_BITS 1660    /* the most bits one 8 x 8 block can take before stuffing */
#define GP_JPEG_HEAD_BYTES 629     /* SOI .. SOS */
#define GP_JPEG_MAX_BATCH 65535
#define GP_JPEG_MAX_SIDE 65535

#define GP_JPEG_420 0              /* chroma halved in both directions (the default of jpeg_ops) */
#define GP_JPEG_444 1              /* no subsampling */

/* src_kind is GP_PNG_SRC_F32 or GP_PNG_SRC_U8 of gp_png.h. */

int gp_jpeg_abi_version(void);

/* Host only.  The two Annex K.1 tables scaled by the IJG rule: scale = 5000 / quality below 50, else 200 - 2 quality; an entry is
 * clamp((base * scale + 50) / 100, 1, 255).  lum and chr: 64 bytes each in natural (row-major) order.  1 <= quality <= 100. */
int gp_jpeg_quant_tables(int32_t quality, uint8_t* lum, uint8_t* chr);

/* The largest file an H x W image can become, in bytes, a multiple of 8 (derived above).  -1 outside the limits. */
int64_t gp_jpeg_bound(int32_t H, int32_t W, int32_t subsampling);

/* Bytes of `scratch` (256-byte aligned, uninitialised on entry) for gp_jpeg_encode; -1 outside the limits. */
int64_t gp_jpeg_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t subsampling);

/* out + b * out_stride receives the complete JPEG file of image b, sizes[b] its length.  Bytes of the slot at and beyond sizes[b] are
 * not written.  out_stride >= gp_jpeg_bound(H, W, subsampling) is required (checked here), so no file can overflow its slot.  src:
 * [B][3][H][W]; lum and chr: HOST pointers to 64 quantisation entries each in natural order, every entry >= 1, copied at the call.
 * Three launches whatever B is. */
int gp_jpeg_encode(int32_t B, int32_t H, int32_t W, const void* src, int32_t src_kind, const uint8_t* lum, const uint8_t* chr,
                   int32_t subsampling, uint8_t* out, int64_t out_stride, uint32_t* sizes, void* scratch, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
