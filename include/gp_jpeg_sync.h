/* gp_jpeg_sync.h -- a second entropy stage for gp_jpeg_decode.h: baseline JPEG files WITHOUT restart markers decoded on many lanes.  Such
 * a file is one segment, which gp_jpeg_decode gives to one lane.  Here the scan is cut into subsequences of GP_JPEG_SYNC_SUBSEQ_BYTES
 * bytes, a lane starts at every cut with a guessed state, and the lanes are corrected from their left neighbours until nothing changes
 * (the self-synchronising decode of Weissenberger and Schmidt, ICPP 2018).  The entry points of csrc/jpeg_sync_kernels.hip, a part of
 * libgp_hip.so with an ABI number of its own.  The transform and the pixel stage are gp_jpeg_decode's own, on the same coefficient layout.
 *
 * Conventions are those of gp_jpeg_decode.h: plain device pointers and sizes, a return code != 0 (or -1 from the int64_t query) plus
 * gp_last_error(), no synchronisation and no host read inside any entry, a gp_stream_t last.  No atomic on global memory decides a
 * byte: two calls on equal inputs give equal pixels, status and info words, and image b of a batch gives those of the B = 1 call.
 *
 * The input is gp_jpeg_decode's (payload, segments, image_seg, tables), with every image exactly one segment: nseg == B,
 * max_image_seg == 1, image_seg[b] == b, and row b of `segments` is {b, first payload byte, byte count n, 0, the image's MCU count}.
 * nseg != B or max_image_seg != 1 is refused before any launch; a row or an image_seg entry that says otherwise (they lie on the
 * device) makes the image GP_JPEG_SYNC_SERIAL.
 *
 * The rule, in full.  S = GP_JPEG_SYNC_SUBSEQ_BYTES, C = GP_JPEG_SYNC_CHUNK.  The scan is the image's n bytes, still stuffed; it has
 * ceil(n / S) subsequences, subsequence i being the bytes [i S, min((i + 1) S, n)), and ceil(subsequences / C) chunks of C consecutive
 * subsequences.
 *
 *   A POSITION is a bit index into the stuffed scan (bit 0 = the most significant bit of byte 0), normalised: the 0x00 behind a data
 *   byte 0xFF holds no position -- the position behind the last bit of the 0xFF is the first bit behind the 0x00.  Position 8 n is the end.
 *
 *   THE STATE a lane carries is (position, k, z): k = the index of the current block inside its MCU (0 .. 5 at GP_JPEG_420, 0 .. 2 at
 *   GP_JPEG_444; the component is Y for the first 4 resp. 1 of them, then Cb, then Cr), z = 0 where the block's DC code comes next,
 *   1 .. 63 = the zigzag index the next AC code starts from.  DC predictions are not part of it.  One further value, DEAD, says that no
 *   state can be given.  The true start of the scan is (0, 0, 0).
 *
 *   A STEP at (position, k, z) reads one symbol of gp_jpeg_decode.h's entropy decoding -- a Huffman code of the component's DC table
 *   (z = 0) or AC table (z > 0) in the next 16 bits, bits beyond the scan's end reading as zeros, and the extra bits its category asks
 *   for -- and moves on: behind a DC symbol z = 1; behind ZRL z += 16; behind a coefficient z += run + 1; behind EOB, or where z reaches
 *   64, the block is complete: k = (k + 1) mod (blocks per MCU), z = 0.
 *
 *   THE RULE ON AN IMPOSSIBLE SYMBOL.  Where no code of 16 bits or fewer matches, a DC category is above 11, an AC category above 10,
 *   a ZRL would take z past 47 (z + 16 > 63) or a run takes z + run past 63, nothing of the symbol is consumed: the position moves on
 *   by ONE bit and the state becomes (position + 1, 0, 0) -- block 0, DC.  Where the symbol is possible but its code and extra bits
 *   reach beyond the scan's last bit, the step is not taken and the decode ends at (8 n, k, z), k and z as they were.
 *
 *   exit(i), given an entry state: DEAD if the entry is DEAD; the entry itself if its position is at or beyond e = 8 min((i + 1) S, n);
 *   otherwise steps are taken from the entry until the position is at or beyond e, and the state then is the exit -- the first
 *   symbol boundary at or beyond the subsequence's end.  A lane whose bit reader loads a stray marker (0xFF followed by neither 0x00
 *   nor the scan's end; the reader fetches up to eight bytes ahead of the position) gives DEAD, and so does one that runs out of its
 *   budget of 8 S + 64 steps (it cannot: every step moves the position on by at least one bit).  The entry of subsequence 0 is the true
 *   start; the true entry of subsequence i > 0 is the true exit(i - 1).
 *
 *   THE SPECULATIVE START of subsequence i > 0 is (8 i S, 0, 0) -- the subsequence's first bit, block 0, DC -- or (8 (i S + 1), 0, 0)
 *   where the cut falls between a 0xFF and its 0x00.
 *
 *   Inside a chunk (one workgroup, a lane per subsequence): every lane computes its exit from its speculative start (subsequence 0
 *   from the true start).  Then rounds: every lane but the chunk's first looks at its left neighbour's stored exit; where that differs
 *   from the entry the lane decoded from last, it decodes again from there and stores the new exit.  A round in which no lane's entry
 *   differed ends the loop and is not counted; at most C rounds can change anything.  Lane 0's entry is given and every exit is a
 *   function of the exit before it, so at the fixpoint every stored exit follows from lane 0's entry.
 *   Across chunks (one workgroup per image, a lane per chunk): in a round, every chunk but the first looks at the last stored exit of
 *   the chunk before it; where that differs from the entry the chunk's first subsequence was decoded from last, the lane decodes the
 *   chunk's subsequences again in order, each from the new exit of the one before, and stops at the first whose new exit equals the
 *   stored one.  Rounds are counted as above; at most (chunks - 1) can change anything.  At that fixpoint every stored exit follows
 *   from the true start: the result is proved, not guessed, and a stream that never re-synchronises by itself (a constant image's
 *   scan is periodic) costs its rounds, not its correctness.
 *
 *   Then, from the true entries: every subsequence counts the DC symbols it reads (the blocks it begins) and sums their differences
 *   per component modulo 2^16 -- gp_jpeg_decode computes (int16)(prediction + difference), and wrap-around addition is associative;
 *   an exclusive scan gives every subsequence its first block and its three predictions; every subsequence decodes once more and
 *   stores its coefficients into the [nblk][64] int16 blocks of gp_jpeg_decode (zeroed by an earlier launch; a block that straddles a
 *   cut is written by two lanes, each its own coefficients).  Block j of the scan is block j mod (blocks per MCU) of MCU
 *   j / (blocks per MCU).  The lane that completes the image's last block applies gp_jpeg_decode's end rule (no stray marker loaded,
 *   fewer than 8 real bits left) and stops; lanes beyond it write nothing.
 *
 * status[b]: GP_JPEG_SYNC_OK -- the pixels are bit for bit those gp_jpeg_decode gives for the same single segment with status
 * GP_JPEG_DECODE_OK (Pillow's bytes on encoder-written files; the same uint8 / float32 outputs and dst_stride).
 * GP_JPEG_SYNC_SERIAL -- nothing is claimed about the pixels (they stay inside the image's slot); the caller runs the image through
 * gp_jpeg_decode, which gives the exact GP_JPEG_DECODE_* word.  SERIAL is the answer to a stream that is not well formed: a refused
 * Huffman table, an impossible symbol met from a true entry before the last block is complete, a DEAD state, a last block that no
 * lane completes, a failed end rule, a bad segment row.  It is never the answer to "the lanes did not synchronise".
 *
 * info[b] = {subsequences, chunks, the most counted rounds inside any chunk, the counted rounds across chunks}: a function of the
 * file, S and C alone (tests/jpeg_sync_ref.py restates it).  All zero for an image whose row or tables were refused.
 *
 * Whatever the payload holds, no kernel reads or writes outside its buffers, every loop bound is independent of the data (rounds <= C + 1
 * and <= chunks + 1, steps per subsequence <= 8 S + 64), and no workgroup waits for another inside a launch.
 *
 * Limits: those of gp_jpeg_decode.h, and payload_bytes < 2^37. */
#ifndef GP_JPEG_SYNC_H
#define GP_JPEG_SYNC_H

#include "gp_hip.h"
#include "gp_jpeg.h"
#include "gp_jpeg_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_JPEG_SYNC_ABI_VERSION 1

#define GP_JPEG_SYNC_SUBSEQ_BYTES 128      /* S: bytes of the stuffed scan per lane */
#define GP_JPEG_SYNC_CHUNK 256             /* C: subsequences, and lanes, per workgroup */

/* status words */
#define GP_JPEG_SYNC_OK 0
#define GP_JPEG_SYNC_SERIAL 1              /* not decoded here: run the image through gp_jpeg_decode */

int gp_jpeg_sync_abi_version(void);

/* Bytes of `scratch` (256-byte aligned, uninitialised on entry) for gp_jpeg_sync_decode; -1 outside the limits. */
int64_t gp_jpeg_sync_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t subsampling, int64_t payload_bytes);

/* gp_jpeg_decode's arguments (nseg == B, max_image_seg == 1) and info: uint32 [B][4].  Ten launches whatever B is. */
int gp_jpeg_sync_decode(int32_t B, int32_t H, int32_t W, int32_t subsampling, int32_t dst_kind, const uint8_t* payload,
                        int64_t payload_bytes, const int64_t* segments, int32_t nseg, const int32_t* image_seg, int32_t max_image_seg,
                        const uint8_t* tables, void* dst, int64_t dst_stride, uint32_t* status, uint32_t* info, void* scratch,
                        gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
