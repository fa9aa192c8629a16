// jpeg_sync_core.h -- the workgroup programs of the self-synchronising entropy stage (include/gp_jpeg_sync.h), in the phase style of
// jpeg_decode_core.h, whose tables (JpdHuff, jpd_construct, jpd_fill_fast, jpd_symbol), transform and pixel stage it reuses: the same
// text runs on a CPU (tests/jpeg_sync_emulate.cpp).
//
//   0. jps_plan_block    one workgroup: every image's segment row checked, its subsequences counted, its first slot in the batch's arrays
//   1. jps_chunk_block   one workgroup per chunk of JPS_C subsequences of one image, a lane each: the speculative pass, then rounds
//                        until no lane's entry changed -- the exits of the chunk follow from its first lane's entry
//   2. jps_cross_block   one workgroup per image, a lane per chunk: chunks repaired from the chunk before, to a fixpoint
//   3. jps_count_block   a lane per subsequence, from its true entry: the blocks it begins, its sums of DC differences
//   4. jps_scan_block    one workgroup per image: the exclusive scan of those
//   5. jps_write_block   a lane per subsequence: the coefficients, into blocks zeroed by an earlier launch
//   6. jps_status_block  one workgroup per image: status[b], info[b]
// then jpd_idct_block and jpd_pixel.  The workgroups of one launch never wait for one another.
#pragma once
#include "jpeg_decode_core.h"

#include "../../include/gp_jpeg_sync.h"

#define JPS_S GP_JPEG_SYNC_SUBSEQ_BYTES
#define JPS_C GP_JPEG_SYNC_CHUNK
#define JPS_DEAD (~(uint64_t)0)
#define JPS_BUDGET (8 * JPS_S + 64)
#define JPS_ERR 1u                                // flag[]: an impossible symbol, a DEAD state
#define JPS_DONE 2u                               //         the image's last block completed and the end rule held
#define JPS_END 4u                                //         ... and the end rule failed

static_assert(JPS_C == JPD_BLOCK, "one lane count for every workgroup of this stage");

struct JpsPlan {
    JpdPlan d;               // sizes, payload, seg, image_seg, tables, dst, status, coef, planes (d.info unused)
    int64_t slots;           // subsequence slots of the batch: payload_bytes / S + B
    uint32_t* img;           // [B][4]: first slot, subsequences, counted rounds across chunks, 1 where the row is sane
    uint64_t* ex;            // [slots] the stored exit of every subsequence
    uint64_t* used;          // [slots] at a chunk's first subsequence: the entry it was decoded from last
    uint32_t* nb;            // [slots] blocks begun; after the scan, the first block
    uint64_t* dc;            // [slots] three 16-bit sums of DC differences; after the scan, the three predictions
    uint32_t* flag;          // [slots] JPS_ERR | JPS_DONE | JPS_END of the writing pass (before it: a chunk waiting for its repair)
    uint32_t* rnd;           // [slots] at a chunk's first subsequence: its counted rounds
    uint32_t* info;          // [B][4]
};

JPD_HOST_FN int64_t jps_slots(int B, int64_t payload_bytes) { return payload_bytes / JPS_S + B; }

struct JpsBits {             // JpdBits, and where its first bit lies
    const uint8_t* in;
    int64_t len, pos;
    uint64_t buf;
    uint64_t ffm;            // a bit at the last bit of every 0xFF in buf whose 0x00 was dropped
    int cnt, pad, marker;
};

JPD_FN void jps_refill(JpsBits& r) {
    if (r.cnt <= 32 && r.pos + 4 <= r.len) {
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
                if (r.in[r.pos] == 0) { ++r.pos; r.ffm |= (uint64_t)1 << (56 - r.cnt); }
                else { r.marker = 1; r.len = r.pos; }
            }
        } else
            r.pad += 8;
        r.buf |= (uint64_t)v << (56 - r.cnt);
        r.cnt += 8;
    }
}

JPD_FN void jps_skip(JpsBits& r, int n) { r.buf <<= n; r.ffm <<= n; r.cnt -= n; }          // (n < 64)

// the normalised position of the reader's first bit: the bytes taken, less the real bits still held, less the dropped 0x00 of every
// 0xFF whose last bit is still held
JPD_FN int64_t jps_at(const JpsBits& r) { return 8 * r.pos - (r.cnt - r.pad) - 8 * (int64_t)__builtin_popcountll(r.ffm); }

JPD_FN uint64_t jps_pack(int64_t at, int k, int z) { return ((uint64_t)at << 16) | ((uint64_t)k << 8) | (uint64_t)z; }

// the speculative start of subsequence s > 0 of the scan in[0 .. n)  (s S < n)
JPD_FN uint64_t jps_start(const uint8_t* in, int64_t s) {
    const int64_t q = s * JPS_S;
    return jps_pack(8 * (q + (in[q - 1] == 0xff && in[q] == 0 ? 1 : 0)), 0, 0);
}

JPD_FN int16_t* jps_block(const JpdPlan& p, int b, int64_t j) {                // block j of image b's scan  (j < nmcu bpm)
    const int m = (int)(j / p.bpm), k = (int)(j - (int64_t)m * p.bpm), v = p.sub == GP_JPEG_420 ? 2 : 1;
    const int my = m / p.mw, mx = m - my * p.mw, c = k < v * v ? 0 : k - v * v + 1;
    const int blk = c == 0 ? (my * v + k / v) * p.ybw + mx * v + k % v : p.ny + (c - 1) * p.nc + my * p.cbw + mx;
    return p.coef + ((size_t)b * p.nblk + blk) * 64;
}

struct JpsTake {             // mode 1, out: nb blocks begun, d0 .. d2 the sums; mode 2, in: the first block, the predictions; out: flag
    uint32_t nb;
    int32_t d0, d1, d2;
    uint32_t flag;
};

// exit(i) of the header for the subsequence that ends at bit end8 of the scan in[0 .. n), from `entry`.  mode 0: nothing else; 1: the
// counts of `o`; 2: the coefficients (every store into a block j < nmcu bpm of image b).
JPD_FN uint64_t jps_decode(const JpdEntropyShared& sh, const JpdPlan& p, int b, const uint8_t* in, int64_t n, int64_t end8, uint64_t entry, int mode,
                           JpsTake& o) {
    if (entry == JPS_DEAD) { o.flag |= JPS_ERR; return JPS_DEAD; }
    int64_t at = (int64_t)(entry >> 16);
    int k = (int)(entry >> 8) & 255, z = (int)entry & 255;
    if (at >= end8) return entry;
    const int ny = p.sub == GP_JPEG_420 ? 4 : 1;
    const int64_t total = (int64_t)p.nmcu * p.bpm;
    int64_t next = o.nb, cur = next - 1;                                       // mode 2: the next block to begin, the one being decoded
    int pred0 = (int16_t)o.d0, pred1 = (int16_t)o.d1, pred2 = (int16_t)o.d2;
    int16_t* zb = nullptr;
    if (mode == 2) {
        if (z ? cur >= total : next >= total) return entry;                    // beyond the image's last block: nothing is written
        if (z && cur < 0) { o.flag |= JPS_ERR; return entry; }
        if (z) zb = jps_block(p, b, cur);
    }
    JpsBits r;
    r.in = in; r.len = n; r.pos = at >> 3; r.buf = 0; r.ffm = 0; r.cnt = 0; r.pad = 0; r.marker = 0;
    jps_refill(r);
    jps_skip(r, (int)(at & 7));
    for (int steps = 0;; ++steps) {
        if (steps > JPS_BUDGET) { o.flag |= JPS_ERR; return JPS_DEAD; }
        if (8 * r.pos - (r.cnt - r.pad) >= end8) {                             // (an upper bound of the position; the exact one where it matters)
            at = jps_at(r);
            if (at >= end8) break;
        }
        jps_refill(r);
        if (r.marker) { o.flag |= JPS_ERR; return JPS_DEAD; }
        const int c = k < ny ? 0 : k - ny + 1;
        const uint32_t look = (uint32_t)(r.buf >> 48);
        int nbits, s, run = 0, cat;
        bool bad;
        if (z == 0) {
            s = jpd_symbol(sh.h[sh.sel[3 + c] & 1], look, nbits);
            cat = s;
            bad = s < 0 || s > 11;
        } else {
            s = jpd_symbol(sh.h[2 + (sh.sel[6 + c] & 1)], look, nbits);
            run = s >> 4; cat = s & 15;
            bad = s < 0 || cat > 10 || (cat == 0 ? (run == 15 && z + 16 > 63) : z + run > 63);
        }
        if (bad) {                                                             // the rule on an impossible symbol: one bit on, block 0, DC
            if (mode) o.flag |= JPS_ERR;
            if (mode == 2) return entry;
            jps_skip(r, 1);
            k = 0; z = 0;
            continue;
        }
        if (r.cnt - r.pad < nbits + cat) return jps_pack(8 * n, k, z);         // the symbol reaches beyond the scan: not taken
        jps_skip(r, nbits);
        int val = 0;
        if (cat) {
            const uint32_t bits = (uint32_t)(r.buf >> (64 - cat));
            jps_skip(r, cat);
            val = jpd_extend(bits, cat);
        }
        bool complete = false;
        if (z == 0) {
            if (mode == 1) {
                ++o.nb;
                if (c == 0) o.d0 += val; else if (c == 1) o.d1 += val; else o.d2 += val;
            }
            if (mode == 2) {
                cur = next++;
                if (cur >= total) return entry;
                zb = jps_block(p, b, cur);
                if (c == 0) zb[0] = (int16_t)(pred0 = (int16_t)(pred0 + val));
                else if (c == 1) zb[0] = (int16_t)(pred1 = (int16_t)(pred1 + val));
                else zb[0] = (int16_t)(pred2 = (int16_t)(pred2 + val));
            }
            z = 1;
        } else if (cat == 0) {
            if (run == 15) z += 16;
            else complete = true;
        } else {
            z += run;
            if (mode == 2) zb[sh.zigzag[z]] = (int16_t)val;
            complete = ++z == 64;
        }
        if (complete) {
            k = k + 1 == p.bpm ? 0 : k + 1;
            z = 0;
            if (mode == 2 && cur == total - 1) {                               // the end rule of jpd_decode_segment
                jps_refill(r);
                o.flag |= (r.marker || r.cnt - r.pad >= 8) ? JPS_END : JPS_DONE;
                return entry;
            }
        }
    }
    return jps_pack(at, k, z);
}

// the image's decoding tables into sh, by `JPS_C` lanes (as jpd_entropy_block builds them); sh.bad where one is refused
JPD_FN void jps_tables(JpdEntropyShared& sh, const uint8_t* tab) {
    JPD_PHASE(t, JPS_C)
        for (int i = t; i < 4 * (1 << JPD_FAST); i += JPS_C) sh.h[i >> JPD_FAST].fast[i & ((1 << JPD_FAST) - 1)] = 0;
        for (int i = t; i < 4 * 256; i += JPS_C) sh.h[i >> 8].vals[i & 255] = tab[JPD_TAB_HUFF + (i >> 8) * JPD_HUFF_BYTES + 16 + (i & 255)];
        if (t < 16) sh.sel[t] = tab[JPD_TAB_SEL + t];
        if (t < 64) sh.zigzag[t] = jpd_zigzag[t];
        if (t == 0) {
            uint32_t bad = 0;
            for (int i = 0; i < 4; ++i) bad |= jpd_construct(sh.h[i], tab + JPD_TAB_HUFF + i * JPD_HUFF_BYTES) ? 0u : 1u;
            sh.bad = bad;
        }
    JPD_END
    if (!sh.bad) {
        JPD_PHASE(t, JPS_C)
            for (int i = 0; i < 4; ++i) jpd_fill_fast(sh.h[i], t, JPS_C);
        JPD_END
    }
}

// ---- 0. the images' rows ------------------------------------------------------------------------------------------------------------------
struct JpsPlanShared {
    int64_t sum[JPS_C];
};

JPD_FN int64_t jps_row_subseqs(const JpsPlan& p, int b) {                      // the subsequences of image b; -1 where its row is refused
    const int64_t* e = p.d.seg + (size_t)b * JPD_SEG_WORDS;
    const int64_t at = e[1], n = e[2];
    if (!(p.d.image_seg[b] == b && p.d.image_seg[b + 1] == b + 1 && e[0] == b && at >= 0 && n >= 0 && at <= p.d.payload_bytes && n <= p.d.payload_bytes - at &&
          n < ((int64_t)1 << 31) && e[3] == 0 && e[4] == p.d.nmcu))
        return -1;
    return (n + JPS_S - 1) / JPS_S;
}

JPD_FN void jps_plan_block(JpsPlanShared& sh, const JpsPlan& p) {
    const int span = (p.d.B + JPS_C - 1) / JPS_C;
    JPD_PHASE(t, JPS_C)
        int64_t sum = 0;
        for (int b = t * span; b < p.d.B && b < (t + 1) * span; ++b) {
            const int64_t m = jps_row_subseqs(p, b);
            sum += m > 0 ? m : 0;
        }
        sh.sum[t] = sum;
    JPD_END
    JPD_PHASE(t, JPS_C)
        if (t == 0) {
            int64_t run = 0;
            for (int u = 0; u < JPS_C; ++u) { const int64_t v = sh.sum[u]; sh.sum[u] = run; run += v; }
        }
    JPD_END
    JPD_PHASE(t, JPS_C)
        int64_t run = sh.sum[t];
        for (int b = t * span; b < p.d.B && b < (t + 1) * span; ++b) {
            const int64_t m = jps_row_subseqs(p, b);
            const bool sane = m >= 0 && run + m <= p.slots;                    // (rows that overlap may ask for more slots than the payload has)
            uint32_t* g = p.img + (size_t)b * 4;
            g[0] = sane ? (uint32_t)run : 0u; g[1] = sane ? (uint32_t)m : 0u; g[2] = 0; g[3] = sane ? 1u : 0u;
            run += m > 0 ? m : 0;
        }
    JPD_END
}

// ---- 1. inside a chunk --------------------------------------------------------------------------------------------------------------------
struct JpsChunkShared {
    JpdEntropyShared e;
    uint64_t ent[JPS_C], ex[JPS_C];
    uint8_t pend[JPS_C];
    uint32_t changed;        // the last round (from 1) in which a lane's entry differed
};

JPD_FN void jps_chunk_block(JpsChunkShared& sh, const JpsPlan& p, int b, int j) {
    const uint32_t* g = p.img + (size_t)b * 4;
    const int64_t off = g[0], nsub = g[1], s0 = (int64_t)j * JPS_C;
    if (s0 >= nsub) return;                                                    // (the same answer in every lane)
    const int64_t* e = p.d.seg + (size_t)b * JPD_SEG_WORDS;
    const uint8_t* in = p.d.payload + e[1];
    const int64_t n = e[2];
    jps_tables(sh.e, p.d.tables + (size_t)b * GP_JPEG_DECODE_TABLE_BYTES);
    if (sh.e.bad) return;
    JPD_PHASE(t, JPS_C)
        const int64_t s = s0 + t;
        if (t == 0) sh.changed = 0;
        sh.pend[t] = 0;
        if (s < nsub) {
            JpsTake o{};
            const uint64_t entry = s == 0 ? 0 : jps_start(in, s);
            sh.ent[t] = entry;
            const int64_t end = (s + 1) * JPS_S < n ? (s + 1) * JPS_S : n;
            sh.ex[t] = jps_decode(sh.e, p.d, b, in, n, 8 * end, entry, 0, o);
        }
    JPD_END
    uint32_t rounds = 0;
    for (uint32_t r = 1; r <= JPS_C + 1; ++r) {                                // (lanes + 1: the bound does not depend on the data)
        JPD_PHASE(t, JPS_C)
            if (t > 0 && s0 + t < nsub && sh.ex[t - 1] != sh.ent[t]) { sh.ent[t] = sh.ex[t - 1]; sh.pend[t] = 1; sh.changed = r; }      // (ex is only read here)
        JPD_END
        if (sh.changed != r) break;                                            // (read behind the barrier, written again only behind the next)
        rounds = r;
        JPD_PHASE(t, JPS_C)
            if (sh.pend[t]) {
                const int64_t s = s0 + t;
                JpsTake o{};
                sh.pend[t] = 0;
                const int64_t end = (s + 1) * JPS_S < n ? (s + 1) * JPS_S : n;
                sh.ex[t] = jps_decode(sh.e, p.d, b, in, n, 8 * end, sh.ent[t], 0, o);
            }
        JPD_END
    }
    JPD_PHASE(t, JPS_C)
        if (s0 + t < nsub) p.ex[off + s0 + t] = sh.ex[t];
        if (t == 0) { p.used[off + s0] = sh.ent[0]; p.rnd[off + s0] = rounds; p.flag[off + s0] = 0; }
    JPD_END
}

// ---- 2. across chunks ---------------------------------------------------------------------------------------------------------------------
JPD_FN void jps_cross_block(JpsChunkShared& sh, const JpsPlan& p, int b) {
    uint32_t* g = p.img + (size_t)b * 4;
    const int64_t off = g[0], nsub = g[1], nch = (nsub + JPS_C - 1) / JPS_C;
    if (nch < 2) return;
    const int64_t* e = p.d.seg + (size_t)b * JPD_SEG_WORDS;
    const uint8_t* in = p.d.payload + e[1];
    const int64_t n = e[2];
    jps_tables(sh.e, p.d.tables + (size_t)b * GP_JPEG_DECODE_TABLE_BYTES);
    if (sh.e.bad) return;
    JPD_PHASE(t, JPS_C)
        if (t == 0) sh.changed = 0;
    JPD_END
    uint32_t rounds = 0;
    for (int64_t r = 1; r <= nch + 1; ++r) {                                   // (chunks + 1)
        JPD_PHASE(t, JPS_C)
            for (int64_t c = t; c < nch; c += JPS_C) {
                const int64_t s = off + c * JPS_C;
                if (c > 0 && p.ex[s - 1] != p.used[s]) { p.used[s] = p.ex[s - 1]; p.flag[s] = 1; sh.changed = (uint32_t)r; }      // (ex is only read here)
            }
        JPD_END
        if (sh.changed != (uint32_t)r) break;
        rounds = (uint32_t)r;
        JPD_PHASE(t, JPS_C)
            for (int64_t c = t; c < nch; c += JPS_C) {
                const int64_t s0 = c * JPS_C;
                if (!p.flag[off + s0]) continue;
                p.flag[off + s0] = 0;
                uint64_t entry = p.used[off + s0];
                for (int64_t s = s0; s < s0 + JPS_C && s < nsub; ++s) {         // until a new exit equals the stored one: the rest follows from it
                    JpsTake o{};
                    const int64_t end = (s + 1) * JPS_S < n ? (s + 1) * JPS_S : n;
                    const uint64_t x = jps_decode(sh.e, p.d, b, in, n, 8 * end, entry, 0, o);
                    if (x == p.ex[off + s]) break;
                    p.ex[off + s] = x;
                    entry = x;
                }
            }
        JPD_END
    }
    JPD_PHASE(t, JPS_C)
        if (t == 0) g[2] = rounds;
    JPD_END
}

// ---- 3. the blocks a subsequence begins, its DC sums; 5. its coefficients -------------------------------------------------------------------
JPD_FN void jps_pass_block(JpdEntropyShared& sh, const JpsPlan& p, int b, int j, int mode) {
    const uint32_t* g = p.img + (size_t)b * 4;
    const int64_t off = g[0], nsub = g[1], s0 = (int64_t)j * JPS_C;
    if (s0 >= nsub) return;
    const int64_t* e = p.d.seg + (size_t)b * JPD_SEG_WORDS;
    const uint8_t* in = p.d.payload + e[1];
    const int64_t n = e[2];
    jps_tables(sh, p.d.tables + (size_t)b * GP_JPEG_DECODE_TABLE_BYTES);
    if (sh.bad) return;
    JPD_PHASE(t, JPS_C)
        const int64_t s = s0 + t;
        if (s < nsub) {
            JpsTake o{};
            if (mode == 2) {
                const uint64_t d = p.dc[off + s];
                o.nb = p.nb[off + s]; o.d0 = (int)(d & 0xffff); o.d1 = (int)((d >> 16) & 0xffff); o.d2 = (int)((d >> 32) & 0xffff);
            }
            const int64_t end = (s + 1) * JPS_S < n ? (s + 1) * JPS_S : n;
            jps_decode(sh, p.d, b, in, n, 8 * end, s == 0 ? 0 : p.ex[off + s - 1], mode, o);
            if (mode == 1) {
                p.nb[off + s] = o.nb;
                p.dc[off + s] = (uint64_t)(uint16_t)o.d0 | ((uint64_t)(uint16_t)o.d1 << 16) | ((uint64_t)(uint16_t)o.d2 << 32);
            } else
                p.flag[off + s] = o.flag;
        }
    JPD_END
}

// ---- 4. every subsequence's first block and predictions ---------------------------------------------------------------------------------------
struct JpsScanShared {
    uint32_t nb[JPS_C];
    uint64_t dc[JPS_C];
};

JPD_FN uint64_t jps_add3(uint64_t a, uint64_t b) {                             // three 16-bit sums, each wrapping on its own
    return (((a & 0xffffull) + (b & 0xffffull)) & 0xffffull) | (((a & 0xffff0000ull) + (b & 0xffff0000ull)) & 0xffff0000ull) |
           (((a & 0xffff00000000ull) + (b & 0xffff00000000ull)) & 0xffff00000000ull);
}

JPD_FN void jps_scan_block(JpsScanShared& sh, const JpsPlan& p, int b) {
    const uint32_t* g = p.img + (size_t)b * 4;
    const int64_t off = g[0], nsub = g[1], span = (nsub + JPS_C - 1) / JPS_C;
    JPD_PHASE(t, JPS_C)
        uint32_t nb = 0;
        uint64_t dc = 0;
        for (int64_t s = t * span; s < nsub && s < (t + 1) * span; ++s) { nb += p.nb[off + s]; dc = jps_add3(dc, p.dc[off + s]); }
        sh.nb[t] = nb; sh.dc[t] = dc;
    JPD_END
    JPD_PHASE(t, JPS_C)
        if (t == 0) {
            uint32_t nb = 0;
            uint64_t dc = 0;
            for (int u = 0; u < JPS_C; ++u) {
                const uint32_t a = sh.nb[u];
                const uint64_t d = sh.dc[u];
                sh.nb[u] = nb; sh.dc[u] = dc;
                nb += a; dc = jps_add3(dc, d);
            }
        }
    JPD_END
    JPD_PHASE(t, JPS_C)
        uint32_t nb = sh.nb[t];
        uint64_t dc = sh.dc[t];
        for (int64_t s = t * span; s < nsub && s < (t + 1) * span; ++s) {
            const uint32_t a = p.nb[off + s];
            const uint64_t d = p.dc[off + s];
            p.nb[off + s] = nb; p.dc[off + s] = dc;
            nb += a; dc = jps_add3(dc, d);
        }
    JPD_END
}

// ---- 6. the image's word ----------------------------------------------------------------------------------------------------------------------
struct JpsStatusShared {
    uint32_t flags[JPS_C], done[JPS_C], rnd[JPS_C];
    JpdHuff h;               // lane 0's, to check the tables with (its direct table is not touched)
};

JPD_FN void jps_status_block(JpsStatusShared& sh, const JpsPlan& p, int b) {
    const uint32_t* g = p.img + (size_t)b * 4;
    const int64_t off = g[0], nsub = g[1], nch = (nsub + JPS_C - 1) / JPS_C;
    const uint8_t* tab = p.d.tables + (size_t)b * GP_JPEG_DECODE_TABLE_BYTES;
    JPD_PHASE(t, JPS_C)
        uint32_t flags = 0, done = 0, rnd = 0;
        for (int64_t s = t; s < nsub; s += JPS_C) {
            const uint32_t f = p.flag[off + s];
            flags |= f;
            done += (f & JPS_DONE) ? 1u : 0u;
        }
        for (int64_t c = t; c < nch; c += JPS_C) rnd = p.rnd[off + c * JPS_C] > rnd ? p.rnd[off + c * JPS_C] : rnd;
        sh.flags[t] = flags; sh.done[t] = done; sh.rnd[t] = rnd;
    JPD_END
    JPD_PHASE(t, JPS_C)
        if (t == 0) {
            uint32_t flags = 0, done = 0, rnd = 0;
            for (int u = 0; u < JPS_C; ++u) { flags |= sh.flags[u]; done += sh.done[u]; rnd = sh.rnd[u] > rnd ? sh.rnd[u] : rnd; }
            bool tables = true;
            for (int i = 0; i < 4; ++i) tables = jpd_construct(sh.h, tab + JPD_TAB_HUFF + i * JPD_HUFF_BYTES) && tables;
            const bool ran = g[3] && tables;
            p.d.status[b] = ran && nsub > 0 && done == 1 && !(flags & (JPS_ERR | JPS_END)) ? (uint32_t)GP_JPEG_SYNC_OK : (uint32_t)GP_JPEG_SYNC_SERIAL;
            uint32_t* o = p.info + (size_t)b * 4;
            o[0] = ran ? (uint32_t)nsub : 0u; o[1] = ran ? (uint32_t)nch : 0u; o[2] = ran ? rnd : 0u; o[3] = ran ? g[2] : 0u;
        }
    JPD_END
}
