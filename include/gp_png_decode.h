/* gp_png_decode.h -- PNG decoding on the device, for the loaders that read rendered frames and ground-truth images back: the C entry
 * points of csrc/png_decode_kernels.hip, a part of libgp_hip.so with an ABI number of its own (the encoder's is gp_png.h).
 *
 * Conventions are those of gp_hip.h: plain device pointers and sizes, a return code != 0 (or -1 from the int64_t query) plus
 * gp_last_error(), no synchronisation and no host read inside any entry, a gp_stream_t last.  No atomic on global memory decides a
 * byte: two calls on equal inputs give equal pixels, and image b of a batch gives the pixels of the B = 1 call on that image.
 *
 * What they replace: np.array(Image.open(path)) per file [REF scene/dataset_readers.py:210-218, utils/general_utils.py:21-27] and
 * metrics._load_rgb of this package.
 *
 * The input.  B images of one shape H x W x C (C = 1, 2, 3, 4 for the colour types 0, 4, 2, 6), 8 bits per sample, no interlace.
 * The host has walked the chunks (signature, lengths, CRC-32, IHDR) and copied every image's IDAT data, joined, into `payload`.
 *   A SEGMENT is a byte range of `payload` that is inflated by one workgroup on its own, into the bytes
 *   [out_first, out_first + out_len) of its image's filtered stream of S = H * (1 + C W) bytes.  `segments` holds five int64 per
 *   segment: image, first payload byte, the byte after its last, out_first, out_len.  The segments of image b are the entries
 *   image_seg[b] .. image_seg[b + 1] - 1, in stream order, and their output ranges tile [0, S).
 *   One segment: the whole zlib stream, decoded SERIALLY.  More than one: the image is decoded BANDED, which is speculative and
 *   exact -- a segment succeeds only if it starts at a block boundary at its first bit, consists of whole non-final deflate blocks
 *   (the last one: ends with the final block and the four Adler-32 bytes), ends at a block boundary on its last byte, produces
 *   exactly out_len bytes and never refers to a byte before out_first.  If all segments of an image hold, the joined stream parses
 *   the same way and the bytes are the stream's; if one does not, status[b] = GP_PNG_DECODE_NOT_BANDED, nothing is claimed about the
 *   pixels and the caller decodes the image again as one segment.  The first segment carries the zlib header (CM = 8, a window of at
 *   most 32 K, FCHECK, no FDICT); the Adler-32 is checked against the sums of the segments, combined.
 *
 * The output.  dst + b * dst_stride * (element size) receives [C_out][H][W] planar: the first C_out <= C channels, as uint8 or as
 * float32 = byte / 255 with one correctly rounded division (bit-equal to torch's uint8.to(float32) / 255.0).  With `background`
 * (three float32 on the device; needs C = 4, C_out = 3) the channels are composited over it as the D-NeRF reader does
 * [REF scene/dataset_readers.py:212-218], in float64 without contraction: n = v / 255.0, a = A / 255.0, arr = n * a + bg * (1 - a),
 * byte = the low eight bits of trunc(arr * 255.0).
 *
 * status[b]: 0 or one GP_PNG_DECODE_* code; mode[b]: GP_PNG_DECODE_MODE_*.  An image whose status is not 0 leaves its slot of dst
 * unwritten.  Whatever the payload and the tables hold, no kernel reads or writes outside its buffers and every loop ends: the bit
 * reader gives zeros beyond its segment, every store and every match source is checked against the segment's output range, and the
 * decoding loop runs under a budget of 8 * input bytes + output bytes + 64 steps, each of which consumes a bit or produces a byte.
 *
 * Limits: 1 <= B <= GP_PNG_DECODE_MAX_BATCH, 1 <= H <= 65535, W >= 1, S < 2^31, B <= nseg < 2^31, payload_bytes < 2^40. */
#ifndef GP_PNG_DECODE_H
#define GP_PNG_DECODE_H

#include "gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_PNG_DECODE_ABI_VERSION 1

#define GP_PNG_DECODE_MAX_BATCH 65535

#define GP_PNG_DECODE_DST_U8 0
#define GP_PNG_DECODE_DST_F32 1

#define GP_PNG_DECODE_MODE_SERIAL 1
#define GP_PNG_DECODE_MODE_BANDED 2

/* status words */
#define GP_PNG_DECODE_OK 0
#define GP_PNG_DECODE_TRUNCATED 1          /* the data ends inside the stream */
#define GP_PNG_DECODE_BLOCK_TYPE 2         /* block type 3 */
#define GP_PNG_DECODE_STORED_LEN 3         /* a stored block whose LEN is not ~NLEN */
#define GP_PNG_DECODE_TOO_MANY_CODES 4     /* HLIT above 286 or HDIST above 30 */
#define GP_PNG_DECODE_CLEN_CODE 5          /* the code-length code is oversubscribed or incomplete */
#define GP_PNG_DECODE_REPEAT_FIRST 6       /* code 16 with no length before it */
#define GP_PNG_DECODE_REPEAT_OVERRUN 7     /* a repeat that runs past HLIT + HDIST */
#define GP_PNG_DECODE_LIT_OVERSUBSCRIBED 8
#define GP_PNG_DECODE_LIT_INCOMPLETE 9
#define GP_PNG_DECODE_NO_END_OF_BLOCK 10   /* no code for symbol 256 */
#define GP_PNG_DECODE_LIT_SYMBOL 11        /* literal/length symbol 286 or 287 */
#define GP_PNG_DECODE_DIST_SYMBOL 12       /* distance symbol 30 or 31, or a distance where the block has no such code */
#define GP_PNG_DECODE_DIST_TOO_FAR 13      /* a distance before the start of the output */
#define GP_PNG_DECODE_OUTPUT_LONG 14       /* more bytes than H * (1 + C W) */
#define GP_PNG_DECODE_OUTPUT_SHORT 15      /* fewer */
#define GP_PNG_DECODE_ADLER 16
#define GP_PNG_DECODE_FILTER 17            /* a filter byte above 4 */
#define GP_PNG_DECODE_ZLIB_METHOD 18       /* CM is not 8 */
#define GP_PNG_DECODE_ZLIB_FDICT 19
#define GP_PNG_DECODE_ZLIB_FCHECK 20
#define GP_PNG_DECODE_ZLIB_WINDOW 21       /* CINFO above 7 */
#define GP_PNG_DECODE_DIST_CODE 22         /* the distance code is oversubscribed or incomplete */
#define GP_PNG_DECODE_NOT_BANDED 23        /* a segment of a banded image did not hold: decode the image as one segment */
#define GP_PNG_DECODE_TRAILING 24          /* bytes after the Adler-32 */
#define GP_PNG_DECODE_TABLE 25             /* a segment table that does not tile the image or leaves the payload */
#define GP_PNG_DECODE_BUDGET 26            /* the step budget ran out (cannot happen: every step consumes a bit or produces a byte) */
#define GP_PNG_DECODE_LIT_CODE 27          /* bits that no literal/length code of the block has */
#define GP_PNG_DECODE_FINAL_INSIDE 28      /* a segment's own reason: the final block before the last segment */

int gp_png_decode_abi_version(void);

/* Bytes of `scratch` (256-byte aligned, uninitialised on entry) for gp_png_decode; -1 outside the limits. */
int64_t gp_png_decode_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t nseg);

/* dst_kind: GP_PNG_DECODE_DST_*; dst_stride: elements between two images' slots, >= C_out * H * W; background: NULL or three float32.
 * Four launches whatever B is. */
int gp_png_decode(int32_t B, int32_t H, int32_t W, int32_t C, int32_t C_out, int32_t dst_kind, const uint8_t* payload,
                  int64_t payload_bytes, const int64_t* segments, int32_t nseg, const int32_t* image_seg, const float* background,
                  void* dst, int64_t dst_stride, uint32_t* status, uint32_t* mode, void* scratch, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
