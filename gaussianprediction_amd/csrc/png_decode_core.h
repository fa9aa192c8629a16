// png_decode_core.h -- the workgroup programs of the PNG decoder (include/gp_png_decode.h), in the phase style of png_core.h: inside
// PNG_PHASE(t) ... PNG_END every lane t runs the body and a barrier follows; nothing lives in a register across phases.  Under hipcc
// a phase is the lane's own code and __syncthreads(); without it (tests/png_decode_emulate.cpp) a phase is a loop over the lanes, so
// the same text decodes on a CPU, where the host tests run it under the sanitizers over every malformed stream first.
//
//   1. pngd_inflate_block   one workgroup per segment.  Lane 0 reads the bits and turns them into a batch of at most PNGD_BATCH output
//                           bytes: literals go straight into the batch as values, matches and stored runs as tokens.  All lanes then
//                           expand the tokens into one source position per byte, follow those positions back to a literal of the
//                           batch or to the 32 K window in LDS, and flush the batch to the window and to memory, with its Adler sums.
//   2. pngd_status_block    one workgroup per image: the segments' words and Adler sums combined into status[b] and mode[b].
//   3. pngd_unfilter_block  one workgroup per image: lane r takes row r of a group of 256 rows one chunk of PNGD_CHUNK pixels behind
//                           lane r - 1, in place, so Avg and Paeth find the row above already done.
//   4. pngd_convert_pixel   one lane per pixel: planar uint8 / float32, the division, the composite.
// The workgroups of one launch never wait for one another; they communicate across launches only.
#pragma once
#include "png_core.h"

#include "../../include/gp_png_decode.h"

#define PNGD_WINDOW 32768
#define PNGD_BATCH 2048                          // output bytes per round of the inflate loop
#define PNGD_MAXTOK 384                          // matches of a batch
#define PNGD_MAXSTORED 8                         // stored runs of a batch
#define PNGD_INBUF 1024                          // input bytes staged in LDS per round (bytes beyond it are read from memory)
#define PNGD_FAST 10                             // bits of the direct decoding tables
#define PNGD_CHUNK 16                            // pixels a lane of the unfilter takes per step
#define PNGD_SEG_WORDS 5
#define PNGD_INFO_WORDS 4                        // per segment: status, Adler sums (a, b) of its bytes, the stream's Adler-32 (last segment)

struct PngdPlan {
    int B, H, W, C, C_out;
    int dst_kind, nseg;
    int row;                 // 1 + C W
    int64_t S, S_pad;        // H * row; its stride in scratch (a multiple of 16)
    const uint8_t* payload;
    int64_t payload_bytes;
    const int64_t* seg;      // [nseg][5]
    const int32_t* image_seg;// [B + 1]
    const float* bg;         // null or three floats
    void* dst;
    int64_t dst_stride;      // elements
    uint32_t* status;
    uint32_t* mode;
    uint8_t* filt;           // [B][S_pad]: the filtered stream, unfiltered in place
    uint32_t* info;          // [nseg][4]
};

// ---- 1. inflate one segment -----------------------------------------------------------------------------------------------------------
// A canonical Huffman code as puff.c keeps it -- count[l] codes of length l, the symbols in order of (length, symbol) -- and a direct
// table over the next PNGD_FAST bits: (symbol << 4) | length, 0 where no code of at most PNGD_FAST bits matches.
struct PngdHuff {
    uint16_t count[16];
    uint16_t start[16];      // where length l begins in symbol[]
    uint16_t base[16];       // the first code of length l
    uint16_t symbol[PNG_NSYM];
    uint16_t fast[1 << PNGD_FAST];
    int n;                   // symbols with a code
};

enum { PNGD_ST_ZLIB = 0, PNGD_ST_HEADER, PNGD_ST_STORED, PNGD_ST_CODES, PNGD_ST_TRAILER, PNGD_ST_DONE };

struct PngdReader {          // lane 0's own, kept here between the rounds
    uint64_t bitbuf;
    int bitcnt;
    int64_t next;            // the next input byte to enter bitbuf
    int64_t steps;
    int state, final_block, stored_left, tables_fixed;
    uint32_t sum_a, sum_b;   // Adler sums of the segment's bytes so far (from 0, 0)
};

struct PngdInflateShared {
    uint8_t window[PNGD_WINDOW];
    int32_t src[PNGD_BATCH];             // per byte of the batch: -(value + 1), or the position (in the segment's output) it copies
    uint8_t val[PNGD_BATCH];
    uint8_t in[PNGD_INBUF];
    int32_t tok_start[PNGD_MAXTOK];
    uint16_t tok_len[PNGD_MAXTOK], tok_dist[PNGD_MAXTOK];
    int32_t st_start[PNGD_MAXSTORED], st_len[PNGD_MAXSTORED];
    int64_t st_from[PNGD_MAXSTORED];
    PngdHuff lit, dist;
    uint8_t len[PNG_NSYM + 32];          // code lengths of the block: literal/length, then distance from hlit on
    int hlit;
    PngdReader rd;
    int64_t in_base;
    int in_have;
    int32_t p0, p1;                      // the batch: output positions [p0, p1) of the segment
    int ntok, nstored;
    int need_fill;                       // written by the decoding phase only
    int stop;                            // written by the closing phase only
    uint32_t status, adler_want;
    unsigned long long batch_a, batch_b;
};

PNG_FN int pngd_construct(PngdHuff& h, const uint8_t* len, int n, int& maxlen) {      // > 0: incomplete, < 0: oversubscribed
    for (int l = 0; l < 16; ++l) h.count[l] = 0;
    for (int s = 0; s < n; ++s) h.count[len[s]]++;           // (len[] < 16 by construction)
    h.count[0] = 0;
    int left = 1;
    maxlen = 0;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) return left;
        if (h.count[l]) maxlen = l;
    }
    int off = 0, code = 0;
    uint16_t at[16];
    for (int l = 1; l < 16; ++l) {
        code = (code + (l > 1 ? h.count[l - 1] : 0)) << 1;
        h.base[l] = (uint16_t)code;
        h.start[l] = at[l] = (uint16_t)off;
        off += h.count[l];
    }
    h.n = off;
    for (int s = 0; s < n; ++s)
        if (len[s]) h.symbol[at[len[s]]++] = (uint16_t)s;
    return left;
}

// the symbol of the code at the low end of `bits` (at least 15 valid bits), its length in nb; -1 where no code matches
PNG_FN int pngd_decode(const PngdHuff& h, uint32_t bits, bool use_fast, int& nb) {
    if (use_fast) {
        const uint32_t e = h.fast[bits & ((1u << PNGD_FAST) - 1)];
        if (e) { nb = (int)(e & 15); return (int)(e >> 4); }
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)(bits & 1);
        bits >>= 1;
        const int count = h.count[l];
        if (code - count < first) { nb = l; return h.symbol[index + (code - first)]; }       // index + (code - first) < h.n <= PNG_NSYM
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    nb = 0;
    return -1;
}

// lane t's share of the direct table of h; len: the lengths its symbols were constructed from
PNG_FN void pngd_fill_fast(PngdHuff& h, const uint8_t* len, int t) {
    for (int i = t; i < h.n; i += PNG_BLOCK) {
        const int s = h.symbol[i], l = len[s];
        if (l < 1 || l > PNGD_FAST) continue;
        uint32_t v = (uint32_t)h.base[l] + (uint32_t)(i - h.start[l]), r = 0;
        for (int k = 0; k < l; ++k) { r = (r << 1) | (v & 1); v >>= 1; }
        for (uint32_t k = r; k < (1u << PNGD_FAST); k += 1u << l) h.fast[k] = (uint16_t)((s << 4) | l);
    }
}

struct PngdSegment {
    const uint8_t* in;       // its first payload byte
    int64_t in_len;
    int32_t out_len;
    int first, last;         // of its image
};

PNG_FN uint32_t pngd_in_byte(const PngdInflateShared& sh, const PngdSegment& g, int64_t i) {     // zeros beyond the segment's last byte
    if (i >= g.in_len) return 0;
    const int64_t o = i - sh.in_base;
    return (o >= 0 && o < sh.in_have) ? sh.in[o] : g.in[i];
}

#define PNGD_NEED_() do {                                                                                                   \
        if (r.bitcnt < 32) {                                                                                                \
            const int64_t o_ = r.next - in_base;                                                                         \
            if (o_ >= 0 && o_ + 4 <= in_have) {           /* the bytes that take bitcnt past 31, from LDS in one go */   \
                const int k_ = (39 - r.bitcnt) >> 3;                                                                        \
                uint32_t w_ = (uint32_t)sh.in[o_] | ((uint32_t)sh.in[o_ + 1] << 8) | ((uint32_t)sh.in[o_ + 2] << 16) | ((uint32_t)sh.in[o_ + 3] << 24); \
                if (k_ < 4) w_ &= (1u << (8 * k_)) - 1;                                                                     \
                r.bitbuf |= (uint64_t)w_ << r.bitcnt;                                                                       \
                r.next += k_;                                                                                               \
                r.bitcnt += 8 * k_;                                                                                         \
            } else                                                                                                          \
                while (r.bitcnt < 32) { r.bitbuf |= (uint64_t)pngd_in_byte(sh, g, r.next) << r.bitcnt; ++r.next; r.bitcnt += 8; } \
        }                                                                                                                   \
    } while (0)
#define PNGD_BITS_(n) ((uint32_t)r.bitbuf & ((1u << (n)) - 1))
#define PNGD_DROP_(n) do { r.bitbuf >>= (n); r.bitcnt -= (n); } while (0)
#define PNGD_USED_() (8 * r.next - r.bitcnt)                                  // bits consumed so far
// an error found in bits that lie beyond the data is the data's end
#define PNGD_FAIL_(code, peek) do { sh.status = (PNGD_USED_() + (peek) > total_bits) ? GP_PNG_DECODE_TRUNCATED : (uint32_t)(code); goto out; } while (0)

// The decoding round of lane 0: bits into literals and tokens until the batch is full, the tables of a new block want filling by all
// lanes, or the segment ends.  Every pass of the loop consumes at least one bit or produces at least one byte.
PNG_FN void pngd_decode_round(PngdInflateShared& sh, const PngdSegment& g) {
    PngdReader r = sh.rd;
    const int64_t in_base = sh.in_base;                                        // (constants of the round, read once: the stores to sh.src
    const int in_have = sh.in_have;                                            //  below would make the compiler read them again per symbol)
    const int32_t p0 = sh.p0;
    const int64_t total_bits = 8 * g.in_len, budget = total_bits + g.out_len + 64;
    int32_t p1 = p0;
    int ntok = 0, nstored = 0;
    sh.need_fill = 0;
    while (r.state != PNGD_ST_DONE && p1 - p0 + 258 <= PNGD_BATCH && ntok < PNGD_MAXTOK && nstored < PNGD_MAXSTORED &&
           (r.next < in_base + PNGD_INBUF || p1 == p0)) {
        if (++r.steps > budget) PNGD_FAIL_(GP_PNG_DECODE_BUDGET, 0);
        if (PNGD_USED_() > total_bits) PNGD_FAIL_(GP_PNG_DECODE_TRUNCATED, 0);
        if (r.state == PNGD_ST_ZLIB) {
            PNGD_NEED_();
            const uint32_t cmf = PNGD_BITS_(8), flg = PNGD_BITS_(16) >> 8;
            PNGD_DROP_(16);
            if ((cmf & 15) != 8) PNGD_FAIL_(GP_PNG_DECODE_ZLIB_METHOD, 0);
            if ((cmf >> 4) > 7) PNGD_FAIL_(GP_PNG_DECODE_ZLIB_WINDOW, 0);
            if ((cmf * 256 + flg) % 31) PNGD_FAIL_(GP_PNG_DECODE_ZLIB_FCHECK, 0);
            if (flg & 32) PNGD_FAIL_(GP_PNG_DECODE_ZLIB_FDICT, 0);
            r.state = PNGD_ST_HEADER;
        } else if (r.state == PNGD_ST_HEADER) {
            if (r.final_block) {
                if (!g.last) PNGD_FAIL_(GP_PNG_DECODE_FINAL_INSIDE, 0);
                r.state = PNGD_ST_TRAILER;
                continue;                                                      // (the trailer's pass consumes bits)
            }
            if (!g.last && PNGD_USED_() == total_bits) {                       // a band's end: a block boundary on its last byte
                if (p1 != g.out_len) PNGD_FAIL_(GP_PNG_DECODE_OUTPUT_SHORT, 0);
                r.state = PNGD_ST_DONE;
                continue;
            }
            PNGD_NEED_();
            r.final_block = (int)PNGD_BITS_(1);
            const uint32_t type = PNGD_BITS_(3) >> 1;
            PNGD_DROP_(3);
            if (type == 3) PNGD_FAIL_(GP_PNG_DECODE_BLOCK_TYPE, 0);
            if (type == 0) {
                PNGD_DROP_(r.bitcnt & 7);
                PNGD_NEED_();
                const uint32_t v = (uint32_t)r.bitbuf;
                PNGD_DROP_(32);
                if ((v & 0xffffu) != ((~v >> 16) & 0xffffu)) PNGD_FAIL_(GP_PNG_DECODE_STORED_LEN, 0);
                if (PNGD_USED_() > total_bits) PNGD_FAIL_(GP_PNG_DECODE_TRUNCATED, 0);
                r.next -= r.bitcnt / 8;                                        // back to bytes (bitcnt is a multiple of 8 here)
                r.bitcnt = 0;
                r.bitbuf = 0;
                r.stored_left = (int)(v & 0xffffu);
                r.state = r.stored_left ? PNGD_ST_STORED : PNGD_ST_HEADER;
            } else if (type == 1) {
                if (!r.tables_fixed) {
                    for (int s = 0; s < PNG_NSYM; ++s) sh.len[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                    for (int s = 0; s < 32; ++s) sh.len[PNG_NSYM + s] = 5;     // (30 and 31 have codes; using one is an error)
                    sh.hlit = PNG_NSYM;
                    int m;
                    pngd_construct(sh.lit, sh.len, PNG_NSYM, m);
                    pngd_construct(sh.dist, sh.len + PNG_NSYM, 32, m);
                    r.tables_fixed = 1;
                    sh.need_fill = 1;
                }
                r.state = PNGD_ST_CODES;
                if (sh.need_fill) break;
            } else {
                PNGD_NEED_();
                const int hlit = (int)PNGD_BITS_(5) + 257, hdist = (int)(PNGD_BITS_(10) >> 5) + 1, hclen = (int)(PNGD_BITS_(14) >> 10) + 4;
                PNGD_DROP_(14);
                if (hlit > 286 || hdist > 30) PNGD_FAIL_(GP_PNG_DECODE_TOO_MANY_CODES, 0);
                const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                uint8_t cl[19];
                for (int i = 0; i < 19; ++i) cl[i] = 0;
                for (int i = 0; i < hclen; ++i) {
                    PNGD_NEED_();
                    cl[order[i]] = (uint8_t)PNGD_BITS_(3);
                    PNGD_DROP_(3);
                }
                int m;
                r.tables_fixed = 0;
                if (pngd_construct(sh.lit, cl, 19, m) != 0) PNGD_FAIL_(GP_PNG_DECODE_CLEN_CODE, 0);     // (the literal table's arrays serve the code-length code first)
                int idx = 0;
                while (idx < hlit + hdist) {
                    PNGD_NEED_();
                    int nb;
                    const int s = pngd_decode(sh.lit, (uint32_t)r.bitbuf, false, nb);
                    if (s < 0) PNGD_FAIL_(GP_PNG_DECODE_CLEN_CODE, 15);
                    PNGD_DROP_(nb);
                    if (s < 16) { sh.len[idx++] = (uint8_t)s; continue; }
                    int prev = 0, rep;
                    if (s == 16) {
                        if (idx == 0) PNGD_FAIL_(GP_PNG_DECODE_REPEAT_FIRST, 0);
                        prev = sh.len[idx - 1];
                        rep = 3 + (int)PNGD_BITS_(2);
                        PNGD_DROP_(2);
                    } else if (s == 17) {
                        rep = 3 + (int)PNGD_BITS_(3);
                        PNGD_DROP_(3);
                    } else {
                        rep = 11 + (int)PNGD_BITS_(7);
                        PNGD_DROP_(7);
                    }
                    if (idx + rep > hlit + hdist) PNGD_FAIL_(GP_PNG_DECODE_REPEAT_OVERRUN, 0);
                    while (rep--) sh.len[idx++] = (uint8_t)prev;
                    if (PNGD_USED_() > total_bits) PNGD_FAIL_(GP_PNG_DECODE_TRUNCATED, 0);
                }
                if (PNGD_USED_() > total_bits) PNGD_FAIL_(GP_PNG_DECODE_TRUNCATED, 0);
                if (sh.len[256] == 0) PNGD_FAIL_(GP_PNG_DECODE_NO_END_OF_BLOCK, 0);
                sh.hlit = hlit;
                int left = pngd_construct(sh.lit, sh.len, hlit, m);            // incomplete: only as one code of length 1 (zlib's rule)
                if (left < 0) PNGD_FAIL_(GP_PNG_DECODE_LIT_OVERSUBSCRIBED, 0);
                if (left > 0 && m != 1) PNGD_FAIL_(GP_PNG_DECODE_LIT_INCOMPLETE, 0);
                left = pngd_construct(sh.dist, sh.len + hlit, hdist, m);       // (no distance code at all: m = 0, every distance an error)
                if (left < 0 || (left > 0 && m > 1)) PNGD_FAIL_(GP_PNG_DECODE_DIST_CODE, 0);
                r.state = PNGD_ST_CODES;
                sh.need_fill = 1;
                break;
            }
        } else if (r.state == PNGD_ST_STORED) {
            int n = r.stored_left;
            if (n > PNGD_BATCH - (p1 - p0)) n = PNGD_BATCH - (p1 - p0);
            if (n > g.out_len - p1) PNGD_FAIL_(GP_PNG_DECODE_OUTPUT_LONG, 0);
            if (n > g.in_len - r.next) { r.next += n; PNGD_FAIL_(GP_PNG_DECODE_TRUNCATED, 0); }
            sh.st_start[nstored] = p1;
            sh.st_len[nstored] = n;
            sh.st_from[nstored] = r.next;
            ++nstored;
            r.next += n;
            p1 += n;
            r.stored_left -= n;
            if (!r.stored_left) r.state = PNGD_ST_HEADER;
        } else if (r.state == PNGD_ST_CODES) {
            PNGD_NEED_();
            int nb;
            const int s = pngd_decode(sh.lit, (uint32_t)r.bitbuf, true, nb);
            if (s < 0) PNGD_FAIL_(GP_PNG_DECODE_LIT_CODE, 15);
            PNGD_DROP_(nb);
            if (PNGD_USED_() > total_bits) PNGD_FAIL_(GP_PNG_DECODE_TRUNCATED, 0);
            if (s < 256) {
                if (p1 >= g.out_len) PNGD_FAIL_(GP_PNG_DECODE_OUTPUT_LONG, 0);
                sh.src[p1 - p0] = -(s + 1);
                ++p1;
                // the literals that follow at once, while the direct table knows them and the round's bounds hold (each is a step)
                while (p1 - p0 + 258 <= PNGD_BATCH && p1 < g.out_len && r.steps < budget) {
                    PNGD_NEED_();
                    const uint32_t e = sh.lit.fast[(uint32_t)r.bitbuf & ((1u << PNGD_FAST) - 1)];
                    if (!e || (e >> 4) >= 256 || PNGD_USED_() + (int)(e & 15) > total_bits || r.next >= in_base + PNGD_INBUF) break;
                    PNGD_DROP_((int)(e & 15));
                    sh.src[p1 - p0] = -((int32_t)(e >> 4) + 1);
                    ++p1;
                    ++r.steps;
                }
                continue;
            }
            if (s == 256) { r.state = PNGD_ST_HEADER; continue; }
            if (s >= 286) PNGD_FAIL_(GP_PNG_DECODE_LIT_SYMBOL, 0);
            int length;
            if (s < 265) length = s - 254;
            else if (s == 285) length = 258;
            else {
                const int e = (s - 261) >> 2;
                length = 3 + ((4 + ((s - 261) & 3)) << e) + (int)PNGD_BITS_(e);
                PNGD_DROP_(e);
            }
            PNGD_NEED_();
            const int d = pngd_decode(sh.dist, (uint32_t)r.bitbuf, true, nb);
            if (d < 0) PNGD_FAIL_(GP_PNG_DECODE_DIST_SYMBOL, 15);
            PNGD_DROP_(nb);
            if (d >= 30) PNGD_FAIL_(GP_PNG_DECODE_DIST_SYMBOL, 0);
            int distance;
            if (d < 4) distance = d + 1;
            else {
                const int e = (d >> 1) - 1;
                distance = 1 + ((2 + (d & 1)) << e) + (int)PNGD_BITS_(e);
                PNGD_DROP_(e);
            }
            if (PNGD_USED_() > total_bits) PNGD_FAIL_(GP_PNG_DECODE_TRUNCATED, 0);
            if (distance > p1) PNGD_FAIL_(GP_PNG_DECODE_DIST_TOO_FAR, 0);
            if (length > g.out_len - p1) PNGD_FAIL_(GP_PNG_DECODE_OUTPUT_LONG, 0);
            sh.tok_start[ntok] = p1;
            sh.tok_len[ntok] = (uint16_t)length;
            sh.tok_dist[ntok] = (uint16_t)(distance - 1);
            ++ntok;
            p1 += length;
        } else {                                                               // PNGD_ST_TRAILER
            PNGD_DROP_(r.bitcnt & 7);
            PNGD_NEED_();
            const uint32_t v = (uint32_t)r.bitbuf;
            PNGD_DROP_(32);
            if (PNGD_USED_() > total_bits) PNGD_FAIL_(GP_PNG_DECODE_TRUNCATED, 0);
            sh.adler_want = (v << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24);
            if (p1 != g.out_len) PNGD_FAIL_(GP_PNG_DECODE_OUTPUT_SHORT, 0);
            if (PNGD_USED_() != total_bits) PNGD_FAIL_(GP_PNG_DECODE_TRAILING, 0);
            r.state = PNGD_ST_DONE;
        }
    }
out:
    if (sh.status) {                                                           // nothing of a failed round is written
        p1 = p0;
        ntok = nstored = 0;
        sh.need_fill = 0;
        r.state = PNGD_ST_DONE;
    }
    sh.p1 = p1;
    sh.ntok = ntok;
    sh.nstored = nstored;
    sh.rd = r;
}
#undef PNGD_NEED_
#undef PNGD_BITS_
#undef PNGD_DROP_
#undef PNGD_USED_
#undef PNGD_FAIL_

PNG_FN void pngd_inflate_block(PngdInflateShared& sh, const PngdPlan& p, int k) {
    const int64_t* e = p.seg + (size_t)k * PNGD_SEG_WORDS;
    const int64_t img = e[0], ib = e[1], ie = e[2], of = e[3], ol = e[4];
    uint32_t* info = p.info + (size_t)k * PNGD_INFO_WORDS;
    const bool sane = img >= 0 && img < p.B && ib >= 0 && ib <= ie && ie <= p.payload_bytes && of >= 0 && of <= p.S && ol >= 0 && ol <= p.S - of;
    if (!sane) {                                                               // (the same answer in every lane)
        PNG_PHASE(t)
            if (t == 0) { info[0] = GP_PNG_DECODE_TABLE; info[1] = info[2] = info[3] = 0; }
        PNG_END
        return;
    }
    PngdSegment g;
    g.in = p.payload + ib;
    g.in_len = ie - ib;
    g.out_len = (int32_t)ol;
    g.first = of == 0;
    g.last = of + ol == p.S;
    uint8_t* out = p.filt + (size_t)img * p.S_pad + of;
    PNG_PHASE(t)
        if (t == 0) {
            PngdReader r{};
            r.state = g.first ? PNGD_ST_ZLIB : PNGD_ST_HEADER;
            sh.rd = r;
            sh.in_base = 0;
            sh.p0 = sh.p1 = 0;
            sh.status = 0;
            sh.adler_want = 0;
            sh.stop = 0;
            sh.need_fill = 0;
            sh.batch_a = sh.batch_b = 0;
            sh.lit.n = sh.dist.n = 0;
        }
    PNG_END
    for (;;) {
        PNG_PHASE(t)                                                           // the next input bytes into LDS
            const int64_t left = g.in_len - sh.in_base;
            const int have = (int)(left < PNGD_INBUF ? (left > 0 ? left : 0) : PNGD_INBUF);
            for (int i = t; i < have; i += PNG_BLOCK) sh.in[i] = g.in[sh.in_base + i];
            if (t == 0) sh.in_have = have;
        PNG_END
        PNG_PHASE(t)
            if (t == 0) pngd_decode_round(sh, g);
        PNG_END
        if (sh.need_fill) {
            PNG_PHASE(t)
                for (int i = t; i < (1 << PNGD_FAST); i += PNG_BLOCK) sh.lit.fast[i] = sh.dist.fast[i] = 0;
            PNG_END
            PNG_PHASE(t)
                pngd_fill_fast(sh.lit, sh.len, t);
                pngd_fill_fast(sh.dist, sh.len + sh.hlit, t);
            PNG_END
        }
        PNG_PHASE(t)                                                           // tokens -> one source per byte
            for (int i = t; i < sh.ntok; i += PNG_BLOCK) {
                const int32_t s = sh.tok_start[i];
                const int n = sh.tok_len[i], d = (int)sh.tok_dist[i] + 1;
                int32_t* dst = sh.src + (s - sh.p0);
                for (int j = 0, m = 0; j < n; ++j) {                           // byte j copies s - d + j % d: a position before the token
                    dst[j] = s - d + m;
                    if (++m == d) m = 0;
                }
            }
            for (int i = 0; i < sh.nstored; ++i) {
                const uint8_t* from = g.in + sh.st_from[i];
                int32_t* dst = sh.src + (sh.st_start[i] - sh.p0);
                for (int j = t; j < sh.st_len[i]; j += PNG_BLOCK) dst[j] = -((int32_t)from[j] + 1);
            }
        PNG_END
        PNG_PHASE(t)                                                           // follow the sources: every hop goes to a lower position
            const int n = sh.p1 - sh.p0;
            for (int j = t; j < n; j += PNG_BLOCK) {
                int32_t q = sh.src[j];
                while (q >= sh.p0) q = sh.src[q - sh.p0];
                sh.val[j] = q < 0 ? (uint8_t)(-q - 1) : sh.window[q & (PNGD_WINDOW - 1)];
            }
        PNG_END
        PNG_PHASE(t)
            const int n = sh.p1 - sh.p0;
            uint32_t a = 0, b = 0;
            for (int j = t; j < n; j += PNG_BLOCK) {
                const uint8_t v = sh.val[j];
                sh.window[(sh.p0 + j) & (PNGD_WINDOW - 1)] = v;
                out[sh.p0 + j] = v;                                            // sh.p0 + j < sh.p1 <= out_len
                a += v;
                b += (uint32_t)(n - j) * v;
            }
            if (a) { PNG_ADD(&sh.batch_a, (unsigned long long)a); PNG_ADD(&sh.batch_b, (unsigned long long)b); }
        PNG_END
        PNG_PHASE(t)
            if (t == 0) {
                const uint32_t n = (uint32_t)(sh.p1 - sh.p0);
                sh.rd.sum_b = (uint32_t)((sh.rd.sum_b + (uint64_t)n * sh.rd.sum_a + sh.batch_b) % PNG_ADLER);
                sh.rd.sum_a = (uint32_t)((sh.rd.sum_a + sh.batch_a) % PNG_ADLER);
                sh.batch_a = sh.batch_b = 0;
                sh.p0 = sh.p1;
                sh.in_base = sh.rd.next - sh.rd.bitcnt / 8;                    // the first byte with unread bits
                sh.stop = sh.rd.state == PNGD_ST_DONE;
                if (sh.stop) {
                    info[0] = sh.status;
                    info[1] = sh.rd.sum_a;
                    info[2] = sh.rd.sum_b;
                    info[3] = sh.adler_want;
                }
            }
        PNG_END
        if (sh.stop) break;
    }
}

// ---- 2. an image's words from its segments' ----------------------------------------------------------------------------------------------
struct PngdStatusShared {
    uint32_t a[PNG_BLOCK], b[PNG_BLOCK], m[PNG_BLOCK], bad[PNG_BLOCK];
};

PNG_FN void pngd_status_block(PngdStatusShared& sh, const PngdPlan& p, int b) {
    const int64_t k0 = p.image_seg[b], k1 = p.image_seg[b + 1];
    const bool sane = k0 >= 0 && k0 < k1 && k1 <= p.nseg;
    const int n = sane ? (int)(k1 - k0) : 0, per = (n + PNG_BLOCK - 1) / PNG_BLOCK;
    PNG_PHASE(t)
        const int i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
        uint32_t A = 0, Bv = 0, M = 0, bad = 0;
        for (int i = i0; i < i1; ++i) {
            const int64_t* e = p.seg + (size_t)(k0 + i) * PNGD_SEG_WORDS;
            const uint32_t* info = p.info + (size_t)(k0 + i) * PNGD_INFO_WORDS;
            const int64_t want = i == 0 ? 0 : e[3 - PNGD_SEG_WORDS] + e[4 - PNGD_SEG_WORDS];      // where the segment before it ends
            if (e[0] != b || e[3] != want || (i == n - 1 && e[3] + e[4] != p.S)) bad = GP_PNG_DECODE_TABLE;
            else if (info[0] && !bad) bad = info[0];
            const uint32_t m = (uint32_t)((uint64_t)e[4] % PNG_ADLER);
            Bv = (uint32_t)((Bv + (uint64_t)m * A + info[2]) % PNG_ADLER);
            A = (A + info[1]) % PNG_ADLER;
            M = (M + m) % PNG_ADLER;
        }
        sh.a[t] = A; sh.b[t] = Bv; sh.m[t] = M; sh.bad[t] = bad;
    PNG_END
    PNG_PHASE(t)
        if (t == 0) {
            uint32_t A = 1, Bv = 0, bad = sane ? 0u : (uint32_t)GP_PNG_DECODE_TABLE;
            for (int u = 0; u < PNG_BLOCK; ++u) {
                Bv = (uint32_t)((Bv + (uint64_t)sh.m[u] * A + sh.b[u]) % PNG_ADLER);
                A = (A + sh.a[u]) % PNG_ADLER;
                if (!bad) bad = sh.bad[u];
            }
            if (!bad && ((Bv << 16) | A) != p.info[(size_t)(k1 - 1) * PNGD_INFO_WORDS + 3]) bad = GP_PNG_DECODE_ADLER;
            if (bad && bad != GP_PNG_DECODE_TABLE && n > 1) bad = GP_PNG_DECODE_NOT_BANDED;
            p.status[b] = bad;
            p.mode[b] = n > 1 ? GP_PNG_DECODE_MODE_BANDED : GP_PNG_DECODE_MODE_SERIAL;
        }
    PNG_END
}

// ---- 3. the row filters undone in place ----------------------------------------------------------------------------------------------------
struct PngdUnfilterShared {
    uint32_t bad;
};

PNG_FN void pngd_unfilter_chunk(uint8_t* cur, const uint8_t* up, int ftype, int C, int x0, int x1) {
    if (ftype == 0) return;
    // the chunk's bytes and the row above's come in first, all loads in flight together; the chain then runs in registers
    uint8_t line[PNGD_CHUNK * 4], above[PNGD_CHUNK * 4];
    const int n = (x1 - x0) * C, at = x0 * C;
#pragma unroll
    for (int i = 0; i < PNGD_CHUNK * 4; ++i) {
        line[i] = i < n ? cur[at + i] : 0;
        above[i] = (up && i < n) ? up[at + i] : 0;
    }
    int a[4] = {0, 0, 0, 0}, c[4] = {0, 0, 0, 0};
    if (x0 > 0)
        for (int ch = 0; ch < C; ++ch) { a[ch] = cur[at - C + ch]; c[ch] = up ? up[at - C + ch] : 0; }
    if (C == 3) {
#pragma unroll
        for (int i = 0; i < PNGD_CHUNK * 3; ++i) {
            const int ch = i % 3, b = above[i];
            const int pred = ftype == 1 ? a[ch] : ftype == 2 ? b : ftype == 3 ? (a[ch] + b) >> 1 : png_paeth(a[ch], b, c[ch]);
            line[i] = (uint8_t)(line[i] + pred);
            a[ch] = line[i];
            c[ch] = b;
        }
    } else {
        for (int i = 0, ch = 0; i < n; ++i) {
            const int b = above[i];
            const int pred = ftype == 1 ? a[ch] : ftype == 2 ? b : ftype == 3 ? (a[ch] + b) >> 1 : png_paeth(a[ch], b, c[ch]);
            line[i] = (uint8_t)(line[i] + pred);
            a[ch] = line[i];
            c[ch] = b;
            if (++ch == C) ch = 0;
        }
    }
#pragma unroll
    for (int i = 0; i < PNGD_CHUNK * 4; ++i)
        if (i < n) cur[at + i] = line[i];
}

PNG_FN void pngd_unfilter_block(PngdUnfilterShared& sh, const PngdPlan& p, int b) {
    if (p.status[b]) return;                                                   // (written by the launch before: the same in every lane)
    uint8_t* f = p.filt + (size_t)b * p.S_pad;
    PNG_PHASE(t)
        if (t == 0) sh.bad = 0;
    PNG_END
    PNG_PHASE(t)
        uint32_t bad = 0;
        for (int y = t; y < p.H; y += PNG_BLOCK) bad |= f[(size_t)y * p.row] > 4;
        if (bad) PNG_OR(&sh.bad, 1u);
    PNG_END
    if (sh.bad) {
        PNG_PHASE(t)
            if (t == 0) p.status[b] = GP_PNG_DECODE_FILTER;
        PNG_END
        return;
    }
    const int nch = (p.W + PNGD_CHUNK - 1) / PNGD_CHUNK;
    for (int y0 = 0; y0 < p.H; y0 += PNG_BLOCK) {
        const int rows = p.H - y0 < PNG_BLOCK ? p.H - y0 : PNG_BLOCK;
        for (int s = 0; s < nch + rows - 1; ++s) {                             // lane t: chunk s - t of row y0 + t, the row above one chunk ahead
            PNG_PHASE(t)
                const int k = s - t;
                if (t < rows && k >= 0 && k < nch) {
                    uint8_t* cur = f + (size_t)(y0 + t) * p.row;
                    const int x1 = (k + 1) * PNGD_CHUNK < p.W ? (k + 1) * PNGD_CHUNK : p.W;
                    pngd_unfilter_chunk(cur + 1, y0 + t > 0 ? cur + 1 - p.row : nullptr, cur[0], p.C, k * PNGD_CHUNK, x1);
                }
            PNG_END
        }
    }
}

// ---- 4. planar output ------------------------------------------------------------------------------------------------------------------------
PNG_FN float pngd_unit(int v) {
#if defined(__HIPCC__)
    return __fdiv_rn((float)v, 255.f);
#else
    return (float)v / 255.f;
#endif
}

PNG_FN int pngd_composite(int v, int alpha, float bg) {                        // [REF scene/dataset_readers.py:216-218] in float64
#if defined(__HIPCC__)
    const double n = __ddiv_rn((double)v, 255.0), a = __ddiv_rn((double)alpha, 255.0);
    const double arr = __dadd_rn(__dmul_rn(n, a), __dmul_rn((double)bg, __dsub_rn(1.0, a)));
    const double s = __dmul_rn(arr, 255.0);
#else
    const double n = (double)v / 255.0, a = (double)alpha / 255.0;
    const double arr = n * a + (double)bg * (1.0 - a);
    const double s = arr * 255.0;
#endif
    if (!(s > -2147483648.0 && s < 2147483648.0)) return 0;
    return (int)s & 255;
}

PNG_FN void pngd_convert_pixel(const PngdPlan& p, int b, int y, int x) {
    if (p.status[b]) return;
    const uint8_t* px = p.filt + (size_t)b * p.S_pad + (size_t)y * p.row + 1 + (size_t)x * p.C;
    const size_t plane = (size_t)p.H * p.W, at = (size_t)b * (size_t)p.dst_stride + (size_t)y * p.W + x;
    for (int ch = 0; ch < p.C_out; ++ch) {
        const int v = p.bg ? pngd_composite(px[ch], px[3], p.bg[ch]) : px[ch];
        if (p.dst_kind == GP_PNG_DECODE_DST_F32) ((float*)p.dst)[at + ch * plane] = pngd_unit(v);
        else ((uint8_t*)p.dst)[at + ch * plane] = (uint8_t)v;
    }
}
