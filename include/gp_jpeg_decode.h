/* gp_jpeg_decode.h -- baseline JPEG decoding on the device, for the loaders that read error images, Motion-JPEG frames and JPEG
 * ground truth back: the C entry points of csrc/jpeg_decode_kernels.hip, a part of libgp_hip.so with an ABI number of its own (the
 * encoder's is gp_jpeg.h).
 *
 * Conventions are those of gp_jpeg.h: plain device pointers and sizes, a return code != 0 (or -1 from the int64_t query) plus
 * gp_last_error(), no synchronisation and no host read inside any entry, a gp_stream_t last.  No atomic on global memory decides a
 * byte: two calls on equal inputs give equal pixels, and image b of a batch gives the pixels of the B = 1 call on that image.
 *
 * What they replace: np.array(Image.open(path)) per file [REF scene/dataset_readers.py:210-218, utils/general_utils.py:21-27,
 * metrics.py:148] and metrics._load_rgb of this package.
 *
 * The input.  B images of one shape H x W and one subsampling (GP_JPEG_420: Y 2 x 2, Cb and Cr 1 x 1, an MCU of 16 x 16 pixels and six
 * blocks; GP_JPEG_444: all 1 x 1, an MCU of 8 x 8 pixels and three blocks), baseline sequential, 8-bit samples, one interleaved scan.
 * The host has walked the markers and copied every image's entropy-coded data into `payload` (as the file holds it: the RST markers
 * may stay where they are, between the segments' ranges).
 *   A SEGMENT is one restart interval: a byte range of `payload`, still byte-stuffed, that one lane decodes on its own.  `segments`
 *   holds five int64 per segment: image, first payload byte, byte count, first MCU (raster order of the MCUs), MCU count.  The
 *   segments of image b are the entries image_seg[b] .. image_seg[b + 1] - 1, in MCU order, and their MCU ranges tile the image's
 *   ceil(H / mcu) * ceil(W / mcu) MCUs.  max_image_seg: the largest segment count of any image (it sizes the grid; an image with
 *   more has status TABLE).  A file without restart markers is one segment, and so one lane.
 *   `tables` holds GP_JPEG_DECODE_TABLE_BYTES per image: bytes 0-2 the quantisation table (0 / 1) of Y, Cb, Cr, bytes 3-5 their DC
 *   Huffman table, bytes 6-8 their AC Huffman table, bytes 9-15 zero; then two quantisation tables of 64 bytes in natural (row-major)
 *   order; then four Huffman tables DC 0, DC 1, AC 0, AC 1 of 16 + 256 bytes each: bits[16] (the number of codes of length 1 .. 16)
 *   and vals (the symbols in code order, the rest zero).
 *
 * The arithmetic, in full.  On every file an encoder wrote from pixels it gives libjpeg-turbo's bytes (ISLOW transform, fancy
 * upsampling), which is what Pillow's decoder returns.
 *
 *   Entropy decoding (T.81 F.2.2).  Codes are read most significant bit first; a data byte 0xFF is followed by 0x00, which is
 *   dropped.  Per block: the DC symbol is a category c <= 11, followed by c bits v; EXTEND(v, c) = v if v >= 2^(c-1), else
 *   v - 2^c + 1 (0 for c = 0); DC = (int16) (the previous DC of the component + EXTEND), the previous DC being 0 at the start of
 *   each segment.  AC symbols are (run << 4) | c at zigzag index k = 1 ..: c = 0 with run = 15 (ZRL) skips 16 coefficients; c = 0
 *   with any other run ends the block (EOB); otherwise k += run, coefficient k = EXTEND of the next c <= 10 bits, k += 1.  The block
 *   ends after index 63.  Coefficients are dezigzagged to natural order and stored as int16.
 *
 *   Dequantise.  x = coefficient * q, exact (|x| < 2^23).
 *
 *   IDCT.  The two-pass integer transform with 13-bit constants (CONST_BITS = 13, PASS1_BITS = 2), every intermediate in 64 bits --
 *   |coefficient * q| <= 2047 * 255 does not prove 32 bits enough: (in0 + in4) << 13 alone reaches 2^33.  One pass over eight inputs:
 *       even:  z1 = (in2 + in6) * 4433;  t2 = z1 - in6 * 15137;  t3 = z1 + in2 * 6270;  t0 = (in0 + in4) << 13;  t1 = (in0 - in4) << 13
 *              t10 = t0 + t3;  t13 = t0 - t3;  t11 = t1 + t2;  t12 = t1 - t2
 *       odd:   (t0, t1, t2, t3) = (in7, in5, in3, in1);  z1 = t0 + t3;  z2 = t1 + t2;  z3 = t0 + t2;  z4 = t1 + t3
 *              z5 = (z3 + z4) * 9633;  t0 *= 2446;  t1 *= 16819;  t2 *= 25172;  t3 *= 12299;  z1 *= -7373;  z2 *= -20995
 *              z3 = z3 * -16069 + z5;  z4 = z4 * -3196 + z5;  t0 += z1 + z3;  t1 += z2 + z4;  t2 += z2 + z3;  t3 += z1 + z4
 *       out 0 .. 7 = t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3
 *   The first pass runs over the columns of the dequantised block, each output (x + 2^10) >> 11; the second over the rows of its
 *   result, each output (x + 2^17) >> 18; then 128 is added and the sample clamped to [0, 255].  All shifts are arithmetic.
 *   (libjpeg limits the sample with a masked table, not a clamp; on coefficients that no encoder produces from pixels the two
 *   differ, and so may its 32-bit and SIMD transforms.  Equality with Pillow is claimed, and tested, for encoder-written files only.)
 *
 *   Chroma upsampling at GP_JPEG_420 works on the real chroma plane only, ch x cw = ceil(H / 2) x ceil(W / 2); the MCU padding is
 *   never read.  cw <= 2: output pixel (y, x) takes chroma sample (y >> 1, x >> 1).  Otherwise the triangle filter: for output row y,
 *   near = chroma row y >> 1, far = the row above it for even y and the row below for odd y (replicated at the top and bottom
 *   edges), s[i] = 3 near[i] + far[i]; out[2 i] = (3 s[i] + s[i - 1] + 8) >> 4, out[2 i + 1] = (3 s[i] + s[i + 1] + 7) >> 4, s
 *   replicated at the left and right edges.
 *
 *   Colour.  cb = Cb - 128, cr = Cr - 128; R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *   B = Y + ((116130 cb + 32768) >> 16), arithmetic shifts, each clamped to [0, 255].
 *
 * The output.  dst + b * dst_stride * (element size) receives [3][H][W] planar R G B as uint8, or as float32 = byte / 255 with one
 * correctly rounded division (bit-equal to torch's uint8.to(float32) / 255.0).
 *
 * status[b]: 0 or the GP_JPEG_DECODE_* code of the image's first failing segment.  The other images of the batch are untouched by
 * it; a failed image's pixels are unspecified but stay inside its slot.  The padding bits of a segment's last byte are not checked.
 * Whatever the payload and the tables hold, no kernel reads or writes outside its buffers and every loop ends: every read of the
 * payload is bounded by the segment's length (the bit reader gives zeros beyond it), every coefficient store by the segment's own
 * blocks, every pixel store by the image's planes, and the symbol loop runs under a budget of 65 steps per block.  No workgroup
 * waits for another.
 *
 * Limits: 1 <= B <= GP_JPEG_DECODE_MAX_BATCH, 1 <= H, W <= 65535, B <= nseg < 2^31, 1 <= max_image_seg <= nseg,
 * payload_bytes < 2^40, the MCU-padded planes of one image below 2^31 bytes. */
#ifndef GP_JPEG_DECODE_H
#define GP_JPEG_DECODE_H

#include "gp_hip.h"
#include "gp_jpeg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_JPEG_DECODE_ABI_VERSION 1

#define GP_JPEG_DECODE_MAX_BATCH 65535
#define GP_JPEG_DECODE_TABLE_BYTES 1232    /* 16 + 2 * 64 + 4 * (16 + 256) */

#define GP_JPEG_DECODE_DST_U8 0
#define GP_JPEG_DECODE_DST_F32 1

/* status words */
#define GP_JPEG_DECODE_OK 0
#define GP_JPEG_DECODE_TRUNCATED 1         /* the bits run out before the segment's MCUs are done */
#define GP_JPEG_DECODE_NO_CODE 2           /* no code of 16 bits or fewer matches */
#define GP_JPEG_DECODE_CATEGORY 3          /* a DC category above 11 or an AC category above 10 */
#define GP_JPEG_DECODE_RUN 4               /* a run takes the coefficient index past 63 */
#define GP_JPEG_DECODE_TRAILING 5          /* one or more whole bytes are left unread at the segment's end */
#define GP_JPEG_DECODE_MARKER 6            /* a 0xFF inside a segment followed by neither 0x00 nor the segment's end */
#define GP_JPEG_DECODE_HUFFMAN_TABLE 7     /* a Huffman table that is oversubscribed or holds more than 256 codes: refused before use */
#define GP_JPEG_DECODE_TABLE 8             /* a segment table that does not tile the image's MCUs or leaves the payload */
#define GP_JPEG_DECODE_BUDGET 9            /* the step budget ran out (cannot happen: every step moves on in its block) */

int gp_jpeg_decode_abi_version(void);

/* Bytes of `scratch` (256-byte aligned, uninitialised on entry) for gp_jpeg_decode; -1 outside the limits.  subsampling: GP_JPEG_420
 * or GP_JPEG_444 of gp_jpeg.h. */
int64_t gp_jpeg_decode_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t subsampling, int32_t nseg);

/* dst_kind: GP_JPEG_DECODE_DST_*; dst_stride: elements between two images' slots, >= 3 * H * W.  Four launches whatever B is. */
int gp_jpeg_decode(int32_t B, int32_t H, int32_t W, int32_t subsampling, int32_t dst_kind, const uint8_t* payload,
                   int64_t payload_bytes, const int64_t* segments, int32_t nseg, const int32_t* image_seg, int32_t max_image_seg,
                   const uint8_t* tables, void* dst, int64_t dst_stride, uint32_t* status, void* scratch, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
