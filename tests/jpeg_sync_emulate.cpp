// The self-synchronising entropy stage's workgroup programs (csrc/jpeg_sync_core.h) and the transform and pixel stage behind them
// (csrc/jpeg_decode_core.h) run on the CPU, every phase as a loop over the lanes, every launch as a loop over its workgroups:
//   jpeg_sync_emulate job.bin out.bin
// job.bin: int32 B, H, W, subsampling, dst_kind, nseg, max_image_seg, guard; int64 payload_bytes; int64 segments[nseg][5];
//          int32 image_seg[B + 1]; uint8 tables[B][GP_JPEG_DECODE_TABLE_BYTES]; the payload  (the job of tests/jpeg_decode_emulate.cpp).
// out.bin: uint32 status[B]; uint32 info[B][4]; then B slots of 3 * H * W + guard elements (filled with 0xa5 before the run).
// Exit code 4 where the C entry would refuse the call (nseg != B, max_image_seg != 1).  Every buffer is its own heap block of exactly
// the size the C entry carves, so that -fsanitize=address,undefined (how tests/test_jpeg_sync_host.py builds this where the host
// compiler can) sees any access outside them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../gaussianprediction_amd/csrc/jpeg_sync_core.h"

template <class T>
static T* block(size_t n, int fill) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (!p) exit(7);
    memset(p, fill, n * sizeof(T));
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t h[8];
    int64_t payload_bytes;
    if (fread(h, 4, 8, f) != 8 || fread(&payload_bytes, 8, 1, f) != 1) return 3;
    if (h[5] != h[0] || h[6] != 1) return 4;
    JpsPlan q{};
    JpdPlan& p = q.d;
    jpd_plan_sizes(p, h[0], h[1], h[2], h[3], h[5]);
    p.dst_kind = h[4]; p.max_image_seg = h[6];
    const int guard = h[7];
    int64_t* seg = block<int64_t>((size_t)p.nseg * JPD_SEG_WORDS, 0);
    int32_t* image_seg = block<int32_t>((size_t)p.B + 1, 0);
    uint8_t* tables = block<uint8_t>((size_t)p.B * GP_JPEG_DECODE_TABLE_BYTES, 0);
    uint8_t* payload = block<uint8_t>((size_t)payload_bytes, 0);
    if (fread(seg, 8, (size_t)p.nseg * JPD_SEG_WORDS, f) != (size_t)p.nseg * JPD_SEG_WORDS || fread(image_seg, 4, (size_t)p.B + 1, f) != (size_t)p.B + 1 ||
        fread(tables, GP_JPEG_DECODE_TABLE_BYTES, (size_t)p.B, f) != (size_t)p.B || fread(payload, 1, (size_t)payload_bytes, f) != (size_t)payload_bytes)
        return 3;
    fclose(f);
    const size_t esz = p.dst_kind == GP_JPEG_DECODE_DST_F32 ? 4 : 1;
    p.dst_stride = (int64_t)3 * p.H * p.W + guard;
    uint8_t* dst = block<uint8_t>((size_t)p.B * p.dst_stride * esz, 0xa5);
    p.payload = payload; p.payload_bytes = payload_bytes; p.seg = seg; p.image_seg = image_seg; p.tables = tables;
    p.dst = dst;
    p.status = block<uint32_t>((size_t)p.B, 0xee);
    p.coef = block<int16_t>((size_t)p.B * p.nblk * 64, 0xee);          // (scratch is uninitialised on the device)
    p.planes = block<uint8_t>((size_t)p.B * p.plane_bytes, 0xee);
    q.slots = jps_slots(p.B, payload_bytes);
    q.img = block<uint32_t>((size_t)p.B * 4, 0xee);
    q.ex = block<uint64_t>((size_t)q.slots, 0xee);
    q.used = block<uint64_t>((size_t)q.slots, 0xee);
    q.dc = block<uint64_t>((size_t)q.slots, 0xee);
    q.nb = block<uint32_t>((size_t)q.slots, 0xee);
    q.flag = block<uint32_t>((size_t)q.slots, 0xee);
    q.rnd = block<uint32_t>((size_t)q.slots, 0xee);
    q.info = block<uint32_t>((size_t)p.B * 4, 0xee);
    static JpsPlanShared ps;
    static JpsChunkShared cs;
    static JpdEntropyShared es;
    static JpsScanShared ns;
    static JpsStatusShared ss;
    static JpdIdctShared is;
    const int chunks = (int)((payload_bytes / JPS_S + 1 + JPS_C - 1) / JPS_C);
    memset(p.coef, 0, (size_t)p.B * p.nblk * 64 * sizeof(int16_t));   // launch 0
    memset(&ps, 0xee, sizeof ps);                                      // (LDS is uninitialised too)
    jps_plan_block(ps, q);
    for (int b = 0; b < p.B; ++b)
        for (int j = 0; j < chunks; ++j) { memset(&cs, 0xee, sizeof cs); jps_chunk_block(cs, q, b, j); }
    for (int b = 0; b < p.B; ++b) { memset(&cs, 0xee, sizeof cs); jps_cross_block(cs, q, b); }
    for (int b = 0; b < p.B; ++b)
        for (int j = 0; j < chunks; ++j) { memset(&es, 0xee, sizeof es); jps_pass_block(es, q, b, j, 1); }
    for (int b = 0; b < p.B; ++b) { memset(&ns, 0xee, sizeof ns); jps_scan_block(ns, q, b); }
    for (int b = 0; b < p.B; ++b)
        for (int j = 0; j < chunks; ++j) { memset(&es, 0xee, sizeof es); jps_pass_block(es, q, b, j, 2); }
    for (int b = 0; b < p.B; ++b) { memset(&ss, 0xee, sizeof ss); jps_status_block(ss, q, b); }
    for (int b = 0; b < p.B; ++b)
        for (int j = 0; j < (p.nblk + JPD_IDCT_BLOCKS - 1) / JPD_IDCT_BLOCKS; ++j) { memset(&is, 0xee, sizeof is); jpd_idct_block(is, p, b, j); }
    for (int b = 0; b < p.B; ++b)
        for (int y = 0; y < p.H; ++y)
            for (int x = 0; x < p.W; ++x) jpd_pixel(p, b, y, x);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(p.status, 4, (size_t)p.B, f) != (size_t)p.B || fwrite(q.info, 16, (size_t)p.B, f) != (size_t)p.B ||
        fwrite(dst, esz, (size_t)p.B * p.dst_stride, f) != (size_t)p.B * p.dst_stride)
        return 6;
    fclose(f);
    free(seg); free(image_seg); free(tables); free(payload); free(dst); free(p.status); free(p.coef); free(p.planes);
    free(q.img); free(q.ex); free(q.used); free(q.dc); free(q.nb); free(q.flag); free(q.rnd); free(q.info);
    return 0;
}
