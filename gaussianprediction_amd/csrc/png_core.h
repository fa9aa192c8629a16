// png_core.h -- the four workgroup programs of the PNG encoder (include/gp_png.h), written as phases: inside PNG_PHASE(t) ... PNG_END
// every lane t of the workgroup runs the body, and a barrier follows.  Nothing lives in a register across phases: what a lane carries
// from one phase to the next sits in a per-lane array of the shared block.  Under hipcc a phase is the lane's own code and
// __syncthreads(); without it (tests/png_emulate.cpp) a phase is a loop over the lanes, so the same text encodes on a CPU and the
// host tests hold its files against zlib's decoder.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gp_png.h"

#define PNG_BLOCK 256
#define PNG_BAND GP_PNG_BAND_BYTES
#define PNG_SLICE (PNG_BAND / PNG_BLOCK)        // bytes of a band per lane
#define PNG_OUT_WORDS (PNG_BAND / 4 + 4)        // a band's bits: never more than its stored form, PNG_BAND + 5 bytes (+ the word a put may touch)
#define PNG_COMP_STRIDE (PNG_BAND + 8)          // a band's slot in scratch
#define PNG_NLIT 286
#define PNG_NSYM 288
#define PNG_MAX_HTOK 320                        // code-length tokens of a block header (at most 286 + 1)
#define PNG_ADLER 65521u
#define PNG_HEAD_BYTES 33                       // signature + IHDR

#if defined(__HIPCC__)
#define PNG_FN __device__ inline
#define PNG_MEMBER __device__
#define PNG_PHASE(t) { const int t = (int)threadIdx.x;
#define PNG_END } __syncthreads();
#define PNG_ADD(p, v) atomicAdd((p), (v))       // LDS atomics on integers: the result does not depend on the order
#define PNG_OR(p, v) atomicOr((p), (v))
#define PNG_XOR(p, v) atomicXor((p), (v))
#else
#define PNG_FN static inline
#define PNG_MEMBER
#define PNG_PHASE(t) for (int t = 0; t < PNG_BLOCK; ++t) {
#define PNG_END }
#define PNG_ADD(p, v) (*(p) += (v))
#define PNG_OR(p, v) (*(p) |= (v))
#define PNG_XOR(p, v) (*(p) ^= (v))
#endif

struct PngPlan {
    int B, H, W;
    int row;                 // 1 + 3 W
    int64_t S;               // H * row, the filtered stream
    int64_t S_pad;           // its stride in scratch (a multiple of 16)
    int NB;                  // bands
    uint32_t flags;
    int src_kind;
    const void* src;
    uint8_t* filt;           // [B][S_pad]
    uint8_t* comp;           // [B][NB][PNG_COMP_STRIDE]
    uint32_t* info;          // [B][NB][4]: deflate bytes, Adler sums (a, b) of the band's bytes, the band's length
    uint32_t* chunk_off;     // [B][NB]: where the band's chunk starts in the file
    uint32_t* adler;         // [B]
    uint8_t* out;
    int64_t out_stride;
    uint32_t* sizes;
};

// ---- 1. quantise and filter: one workgroup per row --------------------------------------------------------------------------------
struct PngFilterShared {
    unsigned long long sum[5];
    int ftype;
};

// element i of `src` as 8 bits (the JPEG encoder's jpeg_core.h reads its pixels through this too)
PNG_FN int png_q8_at(const void* src, int src_kind, size_t i) {
    if (src_kind == GP_PNG_SRC_U8) return ((const uint8_t*)src)[i];
    const float v = ((const float*)src)[i];
#if defined(__HIPCC__)
    const float s = __fadd_rn(__fmul_rn(v, 255.f), 0.5f);
#else
    const float s = v * 255.f + 0.5f;
#endif
    return (int)fminf(fmaxf(floorf(s), 0.f), 255.f);      // (fmaxf(NaN, 0) = 0)
}

PNG_FN int png_q8(const PngPlan& p, int b, int c, int y, int x) {
    return png_q8_at(p.src, p.src_kind, (((size_t)b * 3 + c) * p.H + y) * p.W + x);
}

PNG_FN int png_paeth(int a, int b, int c) {
    const int pp = a + b - c;
    const int pa = pp > a ? pp - a : a - pp, pb = pp > b ? pp - b : b - pp, pc = pp > c ? pp - c : c - pp;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the five filtered values of byte j of row y
PNG_FN void png_residuals(const PngPlan& p, int b, int y, int j, int r[5]) {
    const int x = j / 3, c = j - 3 * x;
    const int raw = png_q8(p, b, c, y, x);
    const int a = x > 0 ? png_q8(p, b, c, y, x - 1) : 0;
    const int up = y > 0 ? png_q8(p, b, c, y - 1, x) : 0;
    const int ul = (x > 0 && y > 0) ? png_q8(p, b, c, y - 1, x - 1) : 0;
    r[0] = raw;
    r[1] = (raw - a) & 255;
    r[2] = (raw - up) & 255;
    r[3] = (raw - ((a + up) >> 1)) & 255;
    r[4] = (raw - png_paeth(a, up, ul)) & 255;
}

PNG_FN void png_filter_block(PngFilterShared& sh, const PngPlan& p, int b, int y) {
    const int n = 3 * p.W;
    const bool choose = !(p.flags & GP_PNG_FILTER_NONE);
    PNG_PHASE(t)
        if (t < 5) sh.sum[t] = 0;
        if (t == 0) sh.ftype = 0;
    PNG_END
    if (choose) {
        PNG_PHASE(t)
            unsigned long long s[5] = {0, 0, 0, 0, 0};
            for (int j = t; j < n; j += PNG_BLOCK) {
                int r[5];
                png_residuals(p, b, y, j, r);
                for (int f = 0; f < 5; ++f) s[f] += (unsigned)(r[f] < 128 ? r[f] : 256 - r[f]);
            }
            for (int f = 0; f < 5; ++f)
                if (s[f]) PNG_ADD(&sh.sum[f], s[f]);
        PNG_END
        PNG_PHASE(t)
            if (t == 0) {
                int best = 0;
                for (int f = 1; f < 5; ++f)
                    if (sh.sum[f] < sh.sum[best]) best = f;
                sh.ftype = best;
            }
        PNG_END
    }
    PNG_PHASE(t)
        uint8_t* dst = p.filt + (size_t)b * p.S_pad + (size_t)y * p.row;
        const int f = sh.ftype;
        if (t == 0) dst[0] = (uint8_t)f;
        for (int j = t; j < n; j += PNG_BLOCK) {
            int r[5];
            png_residuals(p, b, y, j, r);
            dst[1 + j] = (uint8_t)r[f];
        }
    PNG_END
}

// ---- 2. deflate one band: one workgroup per band -------------------------------------------------------------------------------
struct PngBandShared {
    uint32_t out[PNG_OUT_WORDS];
    uint8_t in[PNG_BAND];
    uint32_t hist[PNG_NSYM];
    uint32_t key[PNG_NSYM];          // the used symbols' counts in ascending order, then their code lengths
    uint16_t sym[PNG_NSYM];          // the symbols in that order
    uint16_t code[PNG_NSYM];         // bit-reversed codes
    uint8_t len[PNG_NSYM];
    int32_t lane_head[PNG_BLOCK];    // the last run start inside the lane's slice, -1 for none
    int32_t lane_first[PNG_BLOCK];   // the first one, -1 for none
    int32_t lane_start[PNG_BLOCK];   // the run start that reaches into the slice
    uint32_t lane_bits[PNG_BLOCK];
    uint32_t lane_off[PNG_BLOCK];
    uint32_t adl_a[PNG_BLOCK], adl_b[PNG_BLOCK];
    uint16_t htok[PNG_MAX_HTOK];     // header tokens: code-length symbol | extra << 5
    uint32_t clfreq[19], clkey[19];
    uint16_t clsym[19], clcode[19];
    uint8_t cllen[19];
    uint32_t nused;
    int nhtok, hlit, hclen;
    uint32_t hdr_bits, data_end, comp_len, adler_a, adler_b;
    int use_huff;
};

// length 3 .. 258 -> length code 0 .. 28 (symbol 257 + code), its extra bits and their value
PNG_FN int png_length_code(int m, int& ebits, int& evalue) {
    if (m == 258) { ebits = 0; evalue = 0; return 28; }
    const int l = m - 3;
    if (l < 8) { ebits = 0; evalue = 0; return l; }
    const int e = (31 - __builtin_clz((unsigned)l)) - 2;
    ebits = e;
    evalue = l & ((1 << e) - 1);
    return 4 * e + 4 + ((l >> e) & 3);
}

// Where the run of equal bytes that holds position i (and i + 1, i + 2) ends, looked for no further than 258 bytes from i: byte by
// byte to the end of i's slice, then a slice at a time -- first[u] is the first run start inside lane u's slice, -1 for none, so a
// slice without one continues the run whole.
PNG_FN int png_match_end(const uint8_t* x, int n, int i, const int32_t* first) {
    const int lim = i + 258 < n ? i + 258 : n;
    int p = i + 3;
    while (p < lim && p % PNG_SLICE != 0 && x[p] == x[i]) ++p;
    if (p < lim && p % PNG_SLICE != 0) return p;
    while (p < lim) {
        const int f = first[p / PNG_SLICE];
        if (f >= 0) { p = f; break; }
        p += PNG_SLICE;
    }
    return p < lim ? p : lim;
}

// the tokens of positions [a, b) of a band of n bytes; `s`: the start of the run position a - 1 belongs to
template <class F>
PNG_FN void png_walk(const uint8_t* x, int n, int a, int b, int s, const int32_t* first, F& f) {
    for (int i = a; i < b; ++i) {
        if (i == 0 || x[i] != x[i - 1]) { s = i; f.literal(x[i]); continue; }
        const int j = (i - s - 1) % 258;         // position inside its piece of 258; the piece starts at i - j
        if (j >= 2) continue;                    // a piece that reaches here has 3 bytes: a match, emitted at its start
        if (j == 1) {
            if (!(i + 1 < n && x[i + 1] == x[i])) f.literal(x[i]);
            continue;
        }
        if (i + 2 < n && x[i + 1] == x[i] && x[i + 2] == x[i]) f.match(png_match_end(x, n, i, first) - i);
        else f.literal(x[i]);
    }
}

struct PngCount {
    uint32_t* hist;
    PNG_MEMBER void literal(int v) { PNG_ADD(&hist[v], 1u); }
    PNG_MEMBER void match(int m) { int eb, ev; PNG_ADD(&hist[257 + png_length_code(m, eb, ev)], 1u); }
};
struct PngMeasure {
    const uint8_t* len;
    uint32_t bits;
    PNG_MEMBER void literal(int v) { bits += len[v]; }
    PNG_MEMBER void match(int m) { int eb, ev; bits += len[257 + png_length_code(m, eb, ev)] + eb + 1; }
};

PNG_FN void png_put(uint32_t* out, uint32_t pos, uint32_t value, int nbits) {      // nbits <= 32, value < 2^nbits
    if (nbits <= 0) return;
    const uint32_t w = pos >> 5, s = pos & 31;
    PNG_OR(&out[w], value << s);
    if (s + nbits > 32) PNG_OR(&out[w + 1], value >> (32 - s));
}

struct PngEmit {
    const uint8_t* len;
    const uint16_t* code;
    uint32_t* out;
    uint32_t pos;
    PNG_MEMBER void literal(int v) { png_put(out, pos, code[v], len[v]); pos += len[v]; }
    PNG_MEMBER void match(int m) {
        int eb, ev;
        const int s = 257 + png_length_code(m, eb, ev);
        const int nb = len[s] + eb + 1;                   // (the distance code: the one code of length 1, bit 0)
        png_put(out, pos, (uint32_t)code[s] | ((uint32_t)ev << len[s]), nb);
        pos += nb;
    }
};

// Code lengths of at most maxb bits for n >= 2 symbols whose counts stand in key[0 .. n) in ascending order (sym[i]: the symbol),
// then the canonical codes, bit-reversed.  The lengths: Moffat and Katajainen's in-place minimum-redundancy computation; the limit:
// lengths above maxb are cut to it and the Kraft sum is brought back to one by moving the rarest codes down (the rule of miniz's
// tdefl_huffman_enforce_max_code_size), which leaves a complete code.  len[] / code[] of the nsym symbols are overwritten.
PNG_FN void png_build_code(uint32_t* key, const uint16_t* sym, int n, int maxb, int nsym, uint8_t* len, uint16_t* code) {
    int num[16], next[17];
    for (int i = 0; i < 16; ++i) num[i] = 0;
    for (int s = 0; s < nsym; ++s) { len[s] = 0; code[s] = 0; }
    if (n == 1) {
        key[0] = 1;
    } else {
        key[0] += key[1];
        int root = 0, leaf = 2, nx;
        for (nx = 1; nx < n - 1; ++nx) {
            if (leaf >= n || key[root] < key[leaf]) { key[nx] = key[root]; key[root++] = (uint32_t)nx; } else key[nx] = key[leaf++];
            if (leaf >= n || (root < nx && key[root] < key[leaf])) { key[nx] += key[root]; key[root++] = (uint32_t)nx; } else key[nx] += key[leaf++];
        }
        key[n - 2] = 0;
        for (nx = n - 3; nx >= 0; --nx) key[nx] = key[key[nx]] + 1;
        int avbl = 1, used = 0, dpth = 0;
        root = n - 2;
        nx = n - 1;
        while (avbl > 0) {
            while (root >= 0 && (int)key[root] == dpth) { ++used; --root; }
            while (avbl > used) { key[nx--] = (uint32_t)dpth; --avbl; }
            avbl = 2 * used;
            ++dpth;
            used = 0;
        }
    }
    for (int i = 0; i < n; ++i) num[(int)key[i] < maxb ? (int)key[i] : maxb]++;
    if (n > 1) {
        uint32_t total = 0;
        for (int i = maxb; i > 0; --i) total += (uint32_t)num[i] << (maxb - i);
        while (total > (1u << maxb)) {
            num[maxb]--;
            for (int i = maxb - 1; i > 0; --i)
                if (num[i]) { num[i]--; num[i + 1] += 2; break; }
            --total;
        }
    }
    int j = n;
    for (int i = 1; i <= maxb; ++i)
        for (int l = num[i]; l > 0; --l) len[sym[--j]] = (uint8_t)i;      // the most frequent symbols take the shortest codes
    uint32_t c = 0;
    next[0] = 0;
    for (int bits = 1; bits <= maxb; ++bits) { c = (c + (bits > 1 ? num[bits - 1] : 0)) << 1; next[bits] = (int)c; }
    for (int s = 0; s < nsym; ++s) {
        const int l = len[s];
        if (!l) continue;
        uint32_t v = (uint32_t)next[l]++, r = 0;
        for (int k = 0; k < l; ++k) { r = (r << 1) | (v & 1); v >>= 1; }
        code[s] = (uint16_t)r;
    }
}

// The block header of lane 0: the code-length tokens of len[0 .. hlit) and of the one distance length (the run rules of zlib's
// scan_tree), the code-length code, and the header's bits in sh.out.
PNG_FN void png_block_header(PngBandShared& sh) {
    int hlit = PNG_NLIT;
    while (hlit > 257 && sh.len[hlit - 1] == 0) --hlit;
    sh.hlit = hlit;
    for (int i = 0; i < 19; ++i) sh.clfreq[i] = 0;
    int nt = 0;
#define PNG_TOK_(s, extra) do { sh.htok[nt++] = (uint16_t)((s) | ((extra) << 5)); sh.clfreq[s]++; } while (0)
    int prevlen = -1, nextlen = sh.len[0], count = 0, maxc = 7, minc = 4;
    if (nextlen == 0) { maxc = 138; minc = 3; }
    for (int n = 0; n < hlit; ++n) {
        const int curlen = nextlen;
        nextlen = n + 1 < hlit ? sh.len[n + 1] : 0xffff;
        if (++count < maxc && curlen == nextlen) continue;
        if (count < minc) {
            for (; count > 0; --count) PNG_TOK_(curlen, 0);
        } else if (curlen != 0) {
            if (curlen != prevlen) { PNG_TOK_(curlen, 0); --count; }
            PNG_TOK_(16, count - 3);
        } else if (count <= 10) {
            PNG_TOK_(17, count - 3);
        } else {
            PNG_TOK_(18, count - 11);
        }
        count = 0;
        prevlen = curlen;
        if (nextlen == 0) { maxc = 138; minc = 3; }
        else if (curlen == nextlen) { maxc = 6; minc = 3; }
        else { maxc = 7; minc = 4; }
    }
    PNG_TOK_(1, 0);                                  // the distance code: one symbol, length 1
#undef PNG_TOK_
    sh.nhtok = nt;
    // the code-length code: complete, so at least two symbols
    int used = 0;
    for (int i = 0; i < 19; ++i) used += sh.clfreq[i] != 0;
    if (used < 2) sh.clfreq[sh.clfreq[0] ? 1 : 0] = 1;
    int n = 0;
    for (int s = 0; s < 19; ++s) {                   // insertion sort by (count, symbol)
        const uint32_t f = sh.clfreq[s];
        if (!f) continue;
        int k = n++;
        while (k > 0 && sh.clkey[k - 1] > f) { sh.clkey[k] = sh.clkey[k - 1]; sh.clsym[k] = sh.clsym[k - 1]; --k; }
        sh.clkey[k] = f;
        sh.clsym[k] = (uint16_t)s;
    }
    png_build_code(sh.clkey, sh.clsym, n, 7, 19, sh.cllen, sh.clcode);
    const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = 19;
    while (hclen > 4 && sh.cllen[order[hclen - 1]] == 0) --hclen;
    sh.hclen = hclen;
    uint32_t pos = 0;
    png_put(sh.out, pos, 4u, 3); pos += 3;           // BFINAL = 0, BTYPE = 10
    png_put(sh.out, pos, (uint32_t)(hlit - 257), 5); pos += 5;
    png_put(sh.out, pos, 0u, 5); pos += 5;           // HDIST: one distance code
    png_put(sh.out, pos, (uint32_t)(hclen - 4), 4); pos += 4;
    for (int i = 0; i < hclen; ++i) { png_put(sh.out, pos, sh.cllen[order[i]], 3); pos += 3; }
    for (int i = 0; i < nt; ++i) {
        const int s = sh.htok[i] & 31, extra = sh.htok[i] >> 5;
        png_put(sh.out, pos, sh.clcode[s], sh.cllen[s]); pos += sh.cllen[s];
        const int eb = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
        png_put(sh.out, pos, (uint32_t)extra, eb); pos += eb;
    }
    sh.hdr_bits = pos;
}

PNG_FN void png_band_block(PngBandShared& sh, const PngPlan& p, int b, int k) {
    const int64_t first = (int64_t)k * PNG_BAND;
    const int n = (int)(p.S - first < PNG_BAND ? p.S - first : PNG_BAND);
    const uint8_t* src = p.filt + (size_t)b * p.S_pad + first;
    uint8_t* dst = p.comp + ((size_t)b * p.NB + k) * PNG_COMP_STRIDE;
    PNG_PHASE(t)
        const uint32_t* src32 = (const uint32_t*)src;                 // (S_pad and PNG_BAND are multiples of 16)
        uint32_t* in32 = (uint32_t*)sh.in;
        for (int w = t; w < (n + 3) / 4; w += PNG_BLOCK) in32[w] = src32[w];
        for (int w = t; w < PNG_OUT_WORDS; w += PNG_BLOCK) sh.out[w] = 0;
        for (int s = t; s < PNG_NSYM; s += PNG_BLOCK) sh.hist[s] = 0;
        if (t == 0) sh.nused = 0;
    PNG_END
    PNG_PHASE(t)
        const int a = t * PNG_SLICE < n ? t * PNG_SLICE : n, e = a + PNG_SLICE < n ? a + PNG_SLICE : n;
        int head = -1, first = -1;
        uint32_t sa = 0, sb = 0;
        for (int i = a; i < e; ++i) {
            if (i == 0 || sh.in[i] != sh.in[i - 1]) {
                head = i;
                if (first < 0) first = i;
            }
            sa += sh.in[i];
            sb += (uint32_t)(e - i) * sh.in[i];
        }
        sh.lane_head[t] = head;
        sh.lane_first[t] = first;
        sh.adl_a[t] = sa;
        sh.adl_b[t] = sb;
    PNG_END
    PNG_PHASE(t)
        const int a = t * PNG_SLICE < n ? t * PNG_SLICE : n, e = a + PNG_SLICE < n ? a + PNG_SLICE : n;
        int s = 0;
        for (int u = 0; u < t; ++u) s = sh.lane_head[u] > s ? sh.lane_head[u] : s;
        sh.lane_start[t] = s;
        PngCount f{sh.hist};
        png_walk(sh.in, n, a, e, s, sh.lane_first, f);
        if (t == 0) PNG_ADD(&sh.hist[256], 1u);
    PNG_END
    PNG_PHASE(t)                                                      // the used symbols by ascending (count, symbol): a rank sort
        for (int s = t; s < PNG_NLIT; s += PNG_BLOCK) {
            const uint32_t f = sh.hist[s];
            if (!f) continue;
            int rank = 0;
            for (int o = 0; o < PNG_NLIT; ++o) {
                const uint32_t g = sh.hist[o];
                rank += g != 0 && (g < f || (g == f && o < s));
            }
            sh.key[rank] = f;
            sh.sym[rank] = (uint16_t)s;
            PNG_ADD(&sh.nused, 1u);
        }
    PNG_END
    PNG_PHASE(t)
        if (t == 0) {
            png_build_code(sh.key, sh.sym, (int)sh.nused, 15, PNG_NSYM, sh.len, sh.code);
            png_block_header(sh);
            uint32_t A = 0, Bv = 0;                                    // the band's Adler sums from the lanes', in lane order
            for (int u = 0; u < PNG_BLOCK; ++u) {
                const int a = u * PNG_SLICE < n ? u * PNG_SLICE : n, e = a + PNG_SLICE < n ? a + PNG_SLICE : n;
                Bv = (Bv + (uint32_t)(e - a) * A + sh.adl_b[u]) % PNG_ADLER;
                A = (A + sh.adl_a[u]) % PNG_ADLER;
            }
            sh.adler_a = A;
            sh.adler_b = Bv;
        }
    PNG_END
    PNG_PHASE(t)
        const int a = t * PNG_SLICE < n ? t * PNG_SLICE : n, e = a + PNG_SLICE < n ? a + PNG_SLICE : n;
        PngMeasure f{sh.len, 0};
        png_walk(sh.in, n, a, e, sh.lane_start[t], sh.lane_first, f);
        sh.lane_bits[t] = f.bits;
    PNG_END
    PNG_PHASE(t)
        uint32_t off = sh.hdr_bits;
        for (int u = 0; u < t; ++u) off += sh.lane_bits[u];
        sh.lane_off[t] = off;
        if (t == PNG_BLOCK - 1) {
            sh.data_end = off + sh.lane_bits[t];
            // the end-of-block code, the three header bits of the empty stored block, padding, LEN and NLEN
            const uint32_t huff = (sh.data_end + sh.len[256] + 3 + 7) / 8 + 4, stored = (uint32_t)n + 5;
            sh.use_huff = huff <= stored;
            sh.comp_len = huff <= stored ? huff : stored;
        }
    PNG_END
    if (sh.use_huff) {
        PNG_PHASE(t)
            const int a = t * PNG_SLICE < n ? t * PNG_SLICE : n, e = a + PNG_SLICE < n ? a + PNG_SLICE : n;
            PngEmit f{sh.len, sh.code, sh.out, sh.lane_off[t]};
            png_walk(sh.in, n, a, e, sh.lane_start[t], sh.lane_first, f);
            if (t == PNG_BLOCK - 1) {
                png_put(sh.out, sh.data_end, sh.code[256], sh.len[256]);
                png_put(sh.out, (sh.comp_len - 2) * 8, 0xffffu, 16);  // (the zero bits between are there already)
            }
        PNG_END
    }
    PNG_PHASE(t)
        if (sh.use_huff) {
            uint32_t* dst32 = (uint32_t*)dst;
            for (uint32_t w = t; w < (sh.comp_len + 3) / 4; w += PNG_BLOCK) dst32[w] = sh.out[w];
        } else {
            if (t == 0) {
                dst[0] = 0;                                            // BFINAL = 0, BTYPE = 00
                dst[1] = (uint8_t)(n & 255);
                dst[2] = (uint8_t)(n >> 8);
                dst[3] = (uint8_t)(~n & 255);
                dst[4] = (uint8_t)((~n >> 8) & 255);
            }
            for (int i = t; i < n; i += PNG_BLOCK) dst[5 + i] = sh.in[i];
        }
        if (t == 0) {
            uint32_t* info = p.info + ((size_t)b * p.NB + k) * 4;
            info[0] = sh.comp_len;
            info[1] = sh.adler_a;
            info[2] = sh.adler_b;
            info[3] = (uint32_t)n;
        }
    PNG_END
}

// ---- 3. where every chunk goes, the Adler-32 and the file's length: one workgroup per image --------------------------------------
struct PngLayoutShared {
    uint32_t bytes[PNG_BLOCK], a[PNG_BLOCK], b[PNG_BLOCK], m[PNG_BLOCK], start[PNG_BLOCK];
};

PNG_FN uint32_t png_chunk_data_len(const PngPlan& p, const uint32_t* info, int k) {
    return info[(size_t)k * 4] + (k == 0 ? 2u : 0u) + (k == p.NB - 1 ? 9u : 0u);
}

PNG_FN void png_layout_block(PngLayoutShared& sh, const PngPlan& p, int b) {
    const uint32_t* info = p.info + (size_t)b * p.NB * 4;
    const int per = (p.NB + PNG_BLOCK - 1) / PNG_BLOCK;
    PNG_PHASE(t)
        const int k0 = t * per < p.NB ? t * per : p.NB, k1 = k0 + per < p.NB ? k0 + per : p.NB;
        uint32_t bytes = 0, A = 0, Bv = 0, M = 0;
        for (int k = k0; k < k1; ++k) {
            bytes += 12 + png_chunk_data_len(p, info, k);
            const uint32_t m = info[(size_t)k * 4 + 3];
            Bv = (uint32_t)((Bv + (uint64_t)m * A + info[(size_t)k * 4 + 2]) % PNG_ADLER);
            A = (A + info[(size_t)k * 4 + 1]) % PNG_ADLER;
            M = (M + m) % PNG_ADLER;
        }
        sh.bytes[t] = bytes; sh.a[t] = A; sh.b[t] = Bv; sh.m[t] = M;
    PNG_END
    PNG_PHASE(t)
        if (t == 0) {
            uint32_t off = PNG_HEAD_BYTES, A = 1, Bv = 0;
            for (int u = 0; u < PNG_BLOCK; ++u) {
                sh.start[u] = off;
                off += sh.bytes[u];
                Bv = (uint32_t)((Bv + (uint64_t)sh.m[u] * A + sh.b[u]) % PNG_ADLER);
                A = (A + sh.a[u]) % PNG_ADLER;
            }
            p.adler[b] = (Bv << 16) | A;
            p.sizes[b] = off + 12;                                     // IEND
        }
    PNG_END
    PNG_PHASE(t)
        const int k0 = t * per < p.NB ? t * per : p.NB, k1 = k0 + per < p.NB ? k0 + per : p.NB;
        uint32_t off = sh.start[t];
        for (int k = k0; k < k1; ++k) {
            p.chunk_off[(size_t)b * p.NB + k] = off;
            off += 12 + png_chunk_data_len(p, info, k);
        }
    PNG_END
}

// ---- 4. the chunks in place, with their CRC-32: one workgroup per band ------------------------------------------------------------
struct PngChunkShared {
    uint32_t table[256];
    uint32_t crc;
};

#define PNG_POLY 0xedb88320u
// a(x) b(x) mod P in the reflected representation (bit 31 is x^0): the multiplication behind zlib's crc32_combine, as 32 steps
// whatever the operands are -- zlib's loop ends at the lowest set bit of `a` and does not end for a = 0, which a CRC can be
PNG_FN uint32_t png_mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) r ^= b;
        b = (b & 1) ? (b >> 1) ^ PNG_POLY : b >> 1;
    }
    return r;
}
PNG_FN uint32_t png_xpow8(uint32_t n) {                                // x^(8 n) mod P
    uint32_t r = 1u << 31, sq = 1u << 23;
    for (; n; n >>= 1) {
        if (n & 1) r = png_mulmod(r, sq);
        sq = png_mulmod(sq, sq);
    }
    return r;
}
PNG_FN uint32_t png_crc_bytes(const uint32_t* table, const uint8_t* s, int n) {
    uint32_t c = ~0u;
    for (int i = 0; i < n; ++i) c = table[(c ^ s[i]) & 255] ^ (c >> 8);
    return ~c;
}
PNG_FN void png_be32(uint8_t* d, uint32_t v) { d[0] = (uint8_t)(v >> 24); d[1] = (uint8_t)(v >> 16); d[2] = (uint8_t)(v >> 8); d[3] = (uint8_t)v; }

PNG_FN void png_chunk_block(PngChunkShared& sh, const PngPlan& p, int b, int k) {
    const uint32_t* info = p.info + (size_t)b * p.NB * 4;
    const uint32_t comp_len = info[(size_t)k * 4], data_len = png_chunk_data_len(p, info, k);
    const uint32_t T = 4 + data_len;                                   // the bytes under the CRC: type and data
    const uint32_t lead = k == 0 ? 2u : 0u;
    const uint8_t* comp = p.comp + ((size_t)b * p.NB + k) * PNG_COMP_STRIDE;
    uint8_t* file = p.out + (size_t)b * p.out_stride;
    uint8_t* chunk = file + p.chunk_off[(size_t)b * p.NB + k];
    const uint32_t adler = p.adler[b];
    PNG_PHASE(t)
        uint32_t c = (uint32_t)t;
        for (int i = 0; i < 8; ++i) c = (c & 1) ? (c >> 1) ^ PNG_POLY : c >> 1;
        sh.table[t] = c;
        if (t == 0) sh.crc = 0;
    PNG_END
    PNG_PHASE(t)
        // CRC(A || B) = CRC(A) x^(8 |B|) + CRC(B): every lane's slice contributes its CRC times x^(8 * the bytes after it)
        const uint32_t per = (T + PNG_BLOCK - 1) / PNG_BLOCK;
        const uint32_t i0 = (uint32_t)t * per < T ? (uint32_t)t * per : T, i1 = i0 + per < T ? i0 + per : T;
        if (i0 < i1) {
            uint32_t c = ~0u;
            for (uint32_t i = i0; i < i1; ++i) {
                uint8_t v;
                if (i < 4) v = (uint8_t)("IDAT"[i]);
                else if (i - 4 < lead) v = i == 4 ? 0x78 : 0x01;                       // the zlib header: deflate, 32 K window, level 0
                else if (i - 4 - lead < comp_len) v = comp[i - 4 - lead];
                else {                                                                 // the final empty stored block and the Adler-32
                    const uint32_t q = i - 4 - lead - comp_len;
                    v = q == 0 ? 0x01 : q < 3 ? 0x00 : q < 5 ? 0xff : (uint8_t)(adler >> (8 * (8 - q)));
                }
                chunk[4 + i] = v;
                c = sh.table[(c ^ v) & 255] ^ (c >> 8);
            }
            PNG_XOR(&sh.crc, png_mulmod(png_xpow8(T - i1), ~c));
        }
    PNG_END
    PNG_PHASE(t)
        if (t == 0) {
            png_be32(chunk, data_len);
            png_be32(chunk + 4 + T, sh.crc);
            if (k == 0) {
                const uint8_t sig[16] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
                for (int i = 0; i < 16; ++i) file[i] = sig[i];
                png_be32(file + 16, (uint32_t)p.W);
                png_be32(file + 20, (uint32_t)p.H);
                file[24] = 8; file[25] = 2; file[26] = 0; file[27] = 0; file[28] = 0;      // 8 bits, RGB, deflate, adaptive filters, no interlace
                png_be32(file + 29, png_crc_bytes(sh.table, file + 12, 17));
            }
            if (k == p.NB - 1) {
                uint8_t* e = chunk + 8 + T;
                png_be32(e, 0);
                e[4] = 'I'; e[5] = 'E'; e[6] = 'N'; e[7] = 'D';
                png_be32(e + 8, png_crc_bytes(sh.table, e + 4, 4));
            }
        }
    PNG_END
}
