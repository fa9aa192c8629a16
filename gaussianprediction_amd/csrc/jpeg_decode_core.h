// jpeg_decode_core.h -- the workgroup programs of the JPEG decoder (include/gp_jpeg_decode.h), in the phase style of png_core.h: inside
// JPD_PHASE(t, n) ... JPD_END every lane t of the workgroup's n runs the body and a barrier follows; nothing lives in a register
// across phases.  Under hipcc a phase is the lane's own code and __syncthreads(); without it (tests/jpeg_decode_emulate.cpp) a phase
// is a loop over the lanes, so the same text decodes on a CPU, where the host tests run it under the sanitizers over every malformed
// stream first.
//
//   1. jpd_entropy_block  one workgroup of JPD_ENT_LANES lanes per JPD_ENT_LANES segments (restart intervals) of one image.  All lanes
//                         build the image's four decoding tables in LDS (a direct table over the next JPD_FAST bits, the canonical
//                         walk behind it); then lane t decodes segment t on its own through a 64-bit bit buffer that unstuffs at the
//                         refill, and writes whole blocks of int16 coefficients in natural order, zeros included.
//   2. jpd_status_block   one workgroup per image: the segment table checked, status[b] = the first failing segment's word.
//   3. jpd_idct_block     one workgroup per JPD_IDCT_BLOCKS blocks: dequantise, columns, rows, out of LDS rows of 9 words; eight
//                         lanes per block.  8-bit planes: Y over the MCU-padded frame, Cb and Cr at their own resolution.
//   4. jpd_pixel          one lane per output pixel: chroma upsampling, colour, the uint8 / float32 store.
// The workgroups of one launch never wait for one another; they communicate across launches only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/gp_jpeg_decode.h"

#define JPD_ENT_LANES 64                         // segments per workgroup of the entropy kernel: one wave
#define JPD_BLOCK 256                            // lanes of the other workgroups
#define JPD_FAST 9                               // bits of the direct decoding tables
#define JPD_SEG_WORDS 5
#define JPD_IDCT_BLOCKS (JPD_BLOCK / 8)          // blocks per workgroup of the transform
#define JPD_BSTRIDE 72                           // words of a block in LDS: rows of 9, so that neither a lane per row (stride 9) nor a
#define JPD_RSTRIDE 9                            //   lane per column (block stride 72 = 8 mod 32) meets a bank twice (as jpeg_core.h)
#define JPD_TAB_SEL 0                            // offsets into an image's GP_JPEG_DECODE_TABLE_BYTES
#define JPD_TAB_QT 16
#define JPD_TAB_HUFF 144
#define JPD_HUFF_BYTES 272                       // bits[16] + vals[256]

#if defined(__HIPCC__)
#define JPD_FN __device__ inline
#define JPD_HOST_FN __host__ __device__ inline
#define JPD_TABLE static __device__ const
#define JPD_PHASE(t, n) { const int t = (int)threadIdx.x;
#define JPD_END } __syncthreads();
#else
#define JPD_FN static inline
#define JPD_HOST_FN static inline
#define JPD_TABLE static const
#define JPD_PHASE(t, n) for (int t = 0; t < (n); ++t) {
#define JPD_END }
#endif

JPD_TABLE uint8_t jpd_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpdPlan {
    int B, H, W, sub, dst_kind, nseg, max_image_seg;
    int mw, mh, nmcu;        // MCUs across, down, per image
    int bpm;                 // blocks per MCU: 6 or 3
    int yw, yh, cw, ch;      // the MCU-padded planes: Y, and Cb / Cr
    int ybw, cbw;            // blocks across in them
    int ny, nc;              // blocks of the Y plane, of one chroma plane
    int nblk;                // ny + 2 nc
    int64_t plane_bytes;     // yw yh + 2 cw ch, padded to 16
    const uint8_t* payload;
    int64_t payload_bytes;
    const int64_t* seg;      // [nseg][5]
    const int32_t* image_seg;// [B + 1]
    const uint8_t* tables;   // [B][GP_JPEG_DECODE_TABLE_BYTES]
    void* dst;
    int64_t dst_stride;      // elements
    uint32_t* status;
    int16_t* coef;           // [B][nblk][64]: Y's blocks in raster order, then Cb's, then Cr's
    uint8_t* planes;         // [B][plane_bytes]: Y, Cb, Cr
    uint32_t* info;          // [nseg]: the segment's status
};

JPD_HOST_FN void jpd_plan_sizes(JpdPlan& p, int B, int H, int W, int sub, int nseg) {
    p.B = B; p.H = H; p.W = W; p.sub = sub; p.nseg = nseg;
    const int ms = sub == GP_JPEG_420 ? 16 : 8;
    p.mw = (W + ms - 1) / ms;
    p.mh = (H + ms - 1) / ms;
    p.nmcu = p.mw * p.mh;
    p.bpm = sub == GP_JPEG_420 ? 6 : 3;
    p.yw = p.mw * ms; p.yh = p.mh * ms;
    p.cw = p.mw * 8; p.ch = p.mh * 8;
    p.ybw = p.yw / 8; p.cbw = p.cw / 8;
    p.ny = p.ybw * (p.yh / 8);
    p.nc = p.cbw * (p.ch / 8);
    p.nblk = p.ny + 2 * p.nc;
    p.plane_bytes = ((int64_t)p.yw * p.yh + 2 * (int64_t)p.cw * p.ch + 15) / 16 * 16;
}

// ---- 1. the entropy-coded segments -------------------------------------------------------------------------------------------------------
// A canonical Huffman code: count[l] codes of length l = 1 .. 16, the first of them `first[l]`, their symbols from vals[offset[l]] on;
// and a direct table over the next JPD_FAST bits: (length << 8) | symbol, 0 where no code of at most JPD_FAST bits matches.
struct JpdHuff {
    uint16_t fast[1 << JPD_FAST];
    int32_t first[17];
    uint16_t count[17], offset[17];
    uint8_t vals[256];
};

struct JpdEntropyShared {
    JpdHuff h[4];            // DC 0, DC 1, AC 0, AC 1
    uint8_t sel[16], zigzag[64];
    uint32_t bad;            // written by lane 0 of the construction phase only
};

// the code of `h` from bits[16]; false where it is oversubscribed or holds more than 256 codes
JPD_FN bool jpd_construct(JpdHuff& h, const uint8_t* bits) {
    int left = 1, code = 0, off = 0;
    bool ok = true;
    h.count[0] = 0; h.first[0] = 0; h.offset[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        left = 2 * left - n;                     // (at most 2^16, at least -255 where it first goes negative)
        if (left < 0) { ok = false; left = 0; }
        h.count[l] = (uint16_t)n;
        h.first[l] = code;
        h.offset[l] = (uint16_t)off;
        off += n;
        code = (code + n) << 1;                  // (below 2^17 * 17 whatever bits[] holds)
    }
    return ok && off <= 256;
}

// lane t's share of the direct table of h (constructed, and not refused)
JPD_FN void jpd_fill_fast(JpdHuff& h, int t, int lanes) {
    for (int l = 1; l <= JPD_FAST; ++l)
        for (int i = t; i < h.count[l]; i += lanes) {
            const uint32_t c = (uint32_t)(h.first[l] + i), e = (uint32_t)(l << 8) | h.vals[h.offset[l] + i];
            for (uint32_t k = c << (JPD_FAST - l); k < ((c + 1) << (JPD_FAST - l)); ++k) h.fast[k] = (uint16_t)e;
        }
}

// the symbol of the code at the top of `code16`, its length in nb; -1 where no code of 16 bits or fewer matches
JPD_FN int jpd_symbol(const JpdHuff& h, uint32_t code16, int& nb) {
    const uint32_t e = h.fast[code16 >> (16 - JPD_FAST)];
    if (e) { nb = (int)(e >> 8); return (int)(e & 255); }
    for (int l = JPD_FAST + 1; l <= 16; ++l) {
        const int d = (int)(code16 >> (16 - l)) - h.first[l];
        if (d >= 0 && d < h.count[l]) { nb = l; return h.vals[h.offset[l] + d]; }      // offset + d < 256: the construction checked it
    }
    nb = 0;
    return -1;
}

struct JpdBits {             // a lane's own
    const uint8_t* in;
    int64_t len, pos;        // the segment's bytes; the next one to enter buf
    uint64_t buf;            // the next bits, from bit 63 down
    int cnt;                 // how many of them
    int pad;                 // how many of those (the last ones) are zeros fed beyond the segment's end
    int marker;              // a 0xFF followed by neither 0x00 nor the end was met: nothing is fed behind it
};

// (A reader that loaded eight bytes per access into a second register and fed the bit buffer from there was measured: 12 % slower.)
JPD_FN void jpd_refill(JpdBits& r) {
    if (r.cnt <= 32 && r.pos + 4 <= r.len) {     // four bytes in one go where none of them is 0xFF
        uint32_t w;
        memcpy(&w, r.in + r.pos, 4);
        const uint32_t n = ~w;
        if (!((n - 0x01010101u) & ~n & 0x80808080u)) {
            w = (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24);
            r.buf |= (uint64_t)w << (32 - r.cnt);
            r.cnt += 32;
            r.pos += 4;
        }
    }
    while (r.cnt <= 56) {
        uint32_t v = 0;
        if (r.pos < r.len) {
            v = r.in[r.pos++];
            if (v == 0xff && r.pos < r.len) {
                if (r.in[r.pos] == 0) ++r.pos;
                else { r.marker = 1; r.len = r.pos; }
            }
        } else
            r.pad += 8;
        r.buf |= (uint64_t)v << (56 - r.cnt);
        r.cnt += 8;
    }
}

JPD_FN int jpd_extend(uint32_t v, int c) { return c == 0 ? 0 : (v >> (c - 1)) ? (int)v : (int)v - (1 << c) + 1; }

// Lane's program: segment `g` of plan p = `count` MCUs from MCU `first` of image b, into the image's blocks.  Returns its status.
JPD_FN uint32_t jpd_decode_segment(const JpdEntropyShared& sh, const JpdPlan& p, int b, const uint8_t* in, int64_t len, int first, int count) {
    JpdBits r;
    r.in = in; r.len = len; r.pos = 0; r.buf = 0; r.cnt = 0; r.pad = 0; r.marker = 0;
    int pred0 = 0, pred1 = 0, pred2 = 0;                                       // (three names, not an array a lane would index at run time)
    int64_t steps = 0;
    const int64_t budget = (int64_t)count * p.bpm * 65;
    int16_t* coef = p.coef + (size_t)b * p.nblk * 64;
    const int v = p.sub == GP_JPEG_420 ? 2 : 1;
    // an error found in bits that lie beyond the data is the data's end; one found behind a stray marker is the marker's
#define JPD_FAIL_(code, peek) return r.marker ? (uint32_t)GP_JPEG_DECODE_MARKER : (r.cnt - (peek) < r.pad) ? (uint32_t)GP_JPEG_DECODE_TRUNCATED : (uint32_t)(code)
    for (int m = first; m < first + count; ++m) {
        const int my = m / p.mw, mx = m - my * p.mw;
        for (int k = 0; k < p.bpm; ++k) {
            const int c = k < v * v ? 0 : k - v * v + 1;
            int blk;                                                           // (my < mh and mx < mw: the block lies in its plane)
            if (c == 0) blk = (my * v + k / v) * p.ybw + mx * v + k % v;
            else blk = p.ny + (c - 1) * p.nc + my * p.cbw + mx;
            int16_t* z = coef + (size_t)blk * 64;
            for (int i = 0; i < 64; i += 8) { z[i] = 0; z[i + 1] = 0; z[i + 2] = 0; z[i + 3] = 0; z[i + 4] = 0; z[i + 5] = 0; z[i + 6] = 0; z[i + 7] = 0; }
            const JpdHuff& dc = sh.h[sh.sel[3 + c] & 1];
            const JpdHuff& ac = sh.h[2 + (sh.sel[6 + c] & 1)];
            jpd_refill(r);
            int nb;
            int s = jpd_symbol(dc, (uint32_t)(r.buf >> 48), nb);
            if (++steps > budget) JPD_FAIL_(GP_JPEG_DECODE_BUDGET, 0);
            if (s < 0) JPD_FAIL_(GP_JPEG_DECODE_NO_CODE, 16);
            r.buf <<= nb; r.cnt -= nb;
            if (r.cnt < r.pad) JPD_FAIL_(GP_JPEG_DECODE_TRUNCATED, 0);
            if (s > 11) JPD_FAIL_(GP_JPEG_DECODE_CATEGORY, 0);
            if (s) {
                const uint32_t bits = (uint32_t)(r.buf >> (64 - s));
                r.buf <<= s; r.cnt -= s;
                if (r.cnt < r.pad) JPD_FAIL_(GP_JPEG_DECODE_TRUNCATED, 0);
                const int d = jpd_extend(bits, s);
                if (c == 0) pred0 = (int16_t)(pred0 + d);
                else if (c == 1) pred1 = (int16_t)(pred1 + d);
                else pred2 = (int16_t)(pred2 + d);
            }
            z[0] = (int16_t)(c == 0 ? pred0 : c == 1 ? pred1 : pred2);
            int kk = 1;
            while (kk < 64) {
                jpd_refill(r);
                s = jpd_symbol(ac, (uint32_t)(r.buf >> 48), nb);
                if (++steps > budget) JPD_FAIL_(GP_JPEG_DECODE_BUDGET, 0);
                if (s < 0) JPD_FAIL_(GP_JPEG_DECODE_NO_CODE, 16);
                r.buf <<= nb; r.cnt -= nb;
                if (r.cnt < r.pad) JPD_FAIL_(GP_JPEG_DECODE_TRUNCATED, 0);
                const int run = s >> 4, cat = s & 15;
                if (cat == 0) {
                    if (run != 15) break;                                      // EOB
                    kk += 16;                                                  // ZRL: a coefficient must follow
                    if (kk > 63) JPD_FAIL_(GP_JPEG_DECODE_RUN, 0);
                    continue;
                }
                if (cat > 10) JPD_FAIL_(GP_JPEG_DECODE_CATEGORY, 0);
                kk += run;
                if (kk > 63) JPD_FAIL_(GP_JPEG_DECODE_RUN, 0);
                const uint32_t bits = (uint32_t)(r.buf >> (64 - cat));
                r.buf <<= cat; r.cnt -= cat;
                if (r.cnt < r.pad) JPD_FAIL_(GP_JPEG_DECODE_TRUNCATED, 0);
                z[sh.zigzag[kk]] = (int16_t)jpd_extend(bits, cat);
                ++kk;
            }
        }
    }
    jpd_refill(r);                                                             // (a stray marker right behind the last code is met here)
    if (r.marker) return GP_JPEG_DECODE_MARKER;
    if (r.cnt - r.pad >= 8) return GP_JPEG_DECODE_TRAILING;                    // (fewer than 8 real bits left: the zeros behind them say the bytes are used up)
#undef JPD_FAIL_
    return GP_JPEG_DECODE_OK;
}

// workgroup j of image b: the segments image_seg[b] + j * JPD_ENT_LANES + t
JPD_FN void jpd_entropy_block(JpdEntropyShared& sh, const JpdPlan& p, int b, int j) {
    const int64_t k0 = p.image_seg[b], k1 = p.image_seg[b + 1];
    if (!(k0 >= 0 && k0 <= k1 && k1 <= p.nseg) || k1 - k0 > p.max_image_seg) return;      // (the same answer in every lane; status: TABLE)
    if (k0 + (int64_t)j * JPD_ENT_LANES >= k1) return;
    const uint8_t* tab = p.tables + (size_t)b * GP_JPEG_DECODE_TABLE_BYTES;
    JPD_PHASE(t, JPD_ENT_LANES)
        for (int i = t; i < 4 * (1 << JPD_FAST); i += JPD_ENT_LANES) sh.h[i >> JPD_FAST].fast[i & ((1 << JPD_FAST) - 1)] = 0;
        for (int i = t; i < 4 * 256; i += JPD_ENT_LANES) sh.h[i >> 8].vals[i & 255] = tab[JPD_TAB_HUFF + (i >> 8) * JPD_HUFF_BYTES + 16 + (i & 255)];
        if (t < 16) sh.sel[t] = tab[JPD_TAB_SEL + t];
        if (t < 64) sh.zigzag[t] = jpd_zigzag[t];
        if (t == 0) {
            uint32_t bad = 0;
            for (int i = 0; i < 4; ++i) bad |= jpd_construct(sh.h[i], tab + JPD_TAB_HUFF + i * JPD_HUFF_BYTES) ? 0u : 1u;
            sh.bad = bad;
        }
    JPD_END
    if (!sh.bad) {
        JPD_PHASE(t, JPD_ENT_LANES)
            for (int i = 0; i < 4; ++i) jpd_fill_fast(sh.h[i], t, JPD_ENT_LANES);
        JPD_END
    }
    JPD_PHASE(t, JPD_ENT_LANES)
        const int64_t k = k0 + (int64_t)j * JPD_ENT_LANES + t;
        if (k < k1) {
            const int64_t* e = p.seg + (size_t)k * JPD_SEG_WORDS;
            const int64_t img = e[0], at = e[1], n = e[2], first = e[3], count = e[4];
            uint32_t st;
            if (!(img == b && at >= 0 && n >= 0 && at <= p.payload_bytes && n <= p.payload_bytes - at && first >= 0 && count >= 0 && first <= p.nmcu &&
                  count <= p.nmcu - first))
                st = GP_JPEG_DECODE_TABLE;
            else if (sh.bad)
                st = GP_JPEG_DECODE_HUFFMAN_TABLE;
            else
                st = jpd_decode_segment(sh, p, b, p.payload + at, n, (int)first, (int)count);
            p.info[k] = st;
        }
    JPD_END
}

// ---- 2. an image's word from its segments' ------------------------------------------------------------------------------------------------
struct JpdStatusShared {
    uint32_t bad[JPD_BLOCK];
    int64_t at[JPD_BLOCK];
};

JPD_FN void jpd_status_block(JpdStatusShared& sh, const JpdPlan& p, int b) {
    const int64_t k0 = p.image_seg[b], k1 = p.image_seg[b + 1];
    const bool sane = k0 >= 0 && k0 < k1 && k1 <= p.nseg && k1 - k0 <= p.max_image_seg;
    const int64_t n = sane ? k1 - k0 : 0;
    JPD_PHASE(t, JPD_BLOCK)
        uint32_t bad = 0;
        int64_t at = n;
        for (int64_t i = t; i < n && !bad; i += JPD_BLOCK) {                   // lane t's first failing segment
            const int64_t* e = p.seg + (size_t)(k0 + i) * JPD_SEG_WORDS;
            const int64_t want = i == 0 ? 0 : e[3 - JPD_SEG_WORDS] + e[4 - JPD_SEG_WORDS];        // where the segment before it ends
            if (e[0] != b || e[3] != want || (i == n - 1 && e[3] + e[4] != p.nmcu)) bad = GP_JPEG_DECODE_TABLE;
            else bad = p.info[k0 + i];
            if (bad) at = i;
        }
        sh.bad[t] = bad; sh.at[t] = at;
    JPD_END
    JPD_PHASE(t, JPD_BLOCK)
        if (t == 0) {
            uint32_t bad = sane ? 0u : (uint32_t)GP_JPEG_DECODE_TABLE;
            int64_t at = n;
            for (int u = 0; u < JPD_BLOCK; ++u)
                if (sh.bad[u] && sh.at[u] < at) { at = sh.at[u]; bad = sh.bad[u]; }
            p.status[b] = bad;
        }
    JPD_END
}

// ---- 3. dequantise and transform ------------------------------------------------------------------------------------------------------------
struct JpdIdctShared {
    int32_t ws[JPD_IDCT_BLOCKS * JPD_BSTRIDE];
};

// one pass of the header's transform over in[0 .. 7 * stride], in place; `shift` 11 or 18
JPD_FN void jpd_idct_1d(int32_t* d, int stride, int shift) {
    const int64_t in0 = d[0], in1 = d[stride], in2 = d[2 * stride], in3 = d[3 * stride], in4 = d[4 * stride], in5 = d[5 * stride], in6 = d[6 * stride],
                  in7 = d[7 * stride];
    int64_t z1 = (in2 + in6) * 4433;
    int64_t t2 = z1 - in6 * 15137, t3 = z1 + in2 * 6270;
    int64_t t0 = (in0 + in4) * 8192, t1 = (in0 - in4) * 8192;                  // (<< 13 of a value that may be negative)
    const int64_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = in7; t1 = in5; t2 = in3; t3 = in1;
    z1 = t0 + t3;
    int64_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int64_t z5 = (z3 + z4) * 9633;
    t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    const int64_t half = (int64_t)1 << (shift - 1);
    const int64_t o[8] = {t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int64_t x = (o[i] + half) >> shift;
        if (shift == 18) x = x + 128 < 0 ? 0 : x + 128 > 255 ? 255 : x + 128;  // the sample
        d[i * stride] = (int32_t)x;                                            // (first pass: |x| < 2^29 whatever the block holds -- inputs below
                                                                               //  2^23, eight of them, constants below 2^15, >> 11)
    }
}

// workgroup j of image b: blocks j * JPD_IDCT_BLOCKS ..; lane t: block t / 8, row or column t % 8
JPD_FN void jpd_idct_block(JpdIdctShared& sh, const JpdPlan& p, int b, int j) {
    const uint8_t* tab = p.tables + (size_t)b * GP_JPEG_DECODE_TABLE_BYTES;
    JPD_PHASE(t, JPD_BLOCK)                                                    // a row of coefficients per lane, times its table's row
        const int blk = j * JPD_IDCT_BLOCKS + (t >> 3), r = t & 7;
        if (blk < p.nblk) {
            const int c = blk < p.ny ? 0 : blk < p.ny + p.nc ? 1 : 2;
            const uint8_t* q = tab + JPD_TAB_QT + 64 * (tab[JPD_TAB_SEL + c] & 1) + 8 * r;
            const int16_t* z = p.coef + ((size_t)b * p.nblk + blk) * 64 + 8 * r;
            int32_t* w = sh.ws + (t >> 3) * JPD_BSTRIDE + r * JPD_RSTRIDE;
            int16_t row[8];
            memcpy(row, z, 16);                                                // (16-byte aligned: one load)
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = (int32_t)row[i] * (int32_t)q[i];
        }
    JPD_END
    JPD_PHASE(t, JPD_BLOCK)                                                    // a column per lane
        if (j * JPD_IDCT_BLOCKS + (t >> 3) < p.nblk) jpd_idct_1d(sh.ws + (t >> 3) * JPD_BSTRIDE + (t & 7), JPD_RSTRIDE, 11);
    JPD_END
    JPD_PHASE(t, JPD_BLOCK)                                                    // a row per lane, and its eight samples
        const int blk = j * JPD_IDCT_BLOCKS + (t >> 3), r = t & 7;
        if (blk < p.nblk) {
            int32_t* w = sh.ws + (t >> 3) * JPD_BSTRIDE + r * JPD_RSTRIDE;
            jpd_idct_1d(w, 1, 18);
            uint8_t* plane = p.planes + (size_t)b * p.plane_bytes;
            int at, width;
            if (blk < p.ny) { at = blk; width = p.yw; }
            else {
                const int c = blk < p.ny + p.nc ? 0 : 1;
                at = blk - p.ny - c * p.nc;
                width = p.cw;
                plane += (size_t)p.yw * p.yh + (size_t)c * p.cw * p.ch;
            }
            const int bw = width / 8, by = at / bw, bx = at - by * bw;          // (by * 8 + r < the plane's rows: at < its blocks)
            uint8_t* o = plane + (size_t)(by * 8 + r) * width + bx * 8;
            uint64_t eight = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) eight |= (uint64_t)(uint8_t)w[i] << (8 * i);
            memcpy(o, &eight, 8);                                              // (8-byte aligned: one store)
        }
    JPD_END
}

// ---- 4. upsampling, colour, the planar output ---------------------------------------------------------------------------------------------
JPD_FN float jpd_unit(int v) {
#if defined(__HIPCC__)
    return __fdiv_rn((float)v, 255.f);
#else
    return (float)v / 255.f;
#endif
}

JPD_FN int jpd_clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// chroma sample of output pixel (y, x) at 4:2:0, from the real ch x cw part of plane `c` (row stride `stride`)
JPD_FN int jpd_upsample(const uint8_t* c, int stride, int ch, int cw, int y, int x) {
    const int cy = y >> 1, cx = x >> 1;
    if (cw <= 2) return c[(size_t)cy * stride + cx];
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : fy > ch - 1 ? ch - 1 : fy;
    int ox = (x & 1) ? cx + 1 : cx - 1;
    ox = ox < 0 ? 0 : ox > cw - 1 ? cw - 1 : ox;
    const uint8_t* near = c + (size_t)cy * stride;
    const uint8_t* far = c + (size_t)fy * stride;
    const int s = 3 * near[cx] + far[cx], so = 3 * near[ox] + far[ox];
    return (3 * s + so + ((x & 1) ? 7 : 8)) >> 4;
}

JPD_FN void jpd_pixel(const JpdPlan& p, int b, int y, int x) {
    const uint8_t* Y = p.planes + (size_t)b * p.plane_bytes;
    const uint8_t* Cb = Y + (size_t)p.yw * p.yh;
    const uint8_t* Cr = Cb + (size_t)p.cw * p.ch;
    const int yy = Y[(size_t)y * p.yw + x];
    int cb, cr;
    if (p.sub == GP_JPEG_420) {
        const int ch = (p.H + 1) >> 1, cw = (p.W + 1) >> 1;
        cb = jpd_upsample(Cb, p.cw, ch, cw, y, x);
        cr = jpd_upsample(Cr, p.cw, ch, cw, y, x);
    } else {
        cb = Cb[(size_t)y * p.cw + x];
        cr = Cr[(size_t)y * p.cw + x];
    }
    cb -= 128; cr -= 128;
    const int rgb[3] = {jpd_clamp8(yy + ((91881 * cr + 32768) >> 16)), jpd_clamp8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16)),
                        jpd_clamp8(yy + ((116130 * cb + 32768) >> 16))};
    const size_t plane = (size_t)p.H * p.W, at = (size_t)b * (size_t)p.dst_stride + (size_t)y * p.W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (p.dst_kind == GP_JPEG_DECODE_DST_F32) ((float*)p.dst)[at + c * plane] = jpd_unit(rgb[c]);
        else ((uint8_t*)p.dst)[at + c * plane] = (uint8_t)rgb[c];
    }
}
