// The JPEG decoder's workgroup programs (csrc/jpeg_decode_core.h) run on the CPU, every phase as a loop over the lanes:
//   jpeg_decode_emulate job.bin out.bin
// job.bin: int32 B, H, W, subsampling, dst_kind, nseg, max_image_seg, guard; int64 payload_bytes; int64 segments[nseg][5];
//          int32 image_seg[B + 1]; uint8 tables[B][GP_JPEG_DECODE_TABLE_BYTES]; the payload.
// out.bin: uint32 status[B]; then B slots of 3 * H * W + guard elements (filled with 0xa5 before the run).
// Every buffer is its own heap block of exactly the size the C entry asks for, so that -fsanitize=address,undefined (how
// tests/test_jpeg_decode_host.py builds this where the host compiler can) sees any access outside them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../gaussianprediction_amd/csrc/jpeg_decode_core.h"

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
    JpdPlan p{};
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
    p.info = block<uint32_t>((size_t)p.nseg, 0xee);
    static JpdEntropyShared es;
    static JpdStatusShared ss;
    static JpdIdctShared is;
    for (int b = 0; b < p.B; ++b)
        for (int j = 0; j < (p.max_image_seg + JPD_ENT_LANES - 1) / JPD_ENT_LANES; ++j) {
            memset(&es, 0xee, sizeof es);                               // (so is LDS)
            jpd_entropy_block(es, p, b, j);
        }
    for (int b = 0; b < p.B; ++b) jpd_status_block(ss, p, b);
    for (int b = 0; b < p.B; ++b)
        for (int j = 0; j < (p.nblk + JPD_IDCT_BLOCKS - 1) / JPD_IDCT_BLOCKS; ++j) {
            memset(&is, 0xee, sizeof is);
            jpd_idct_block(is, p, b, j);
        }
    for (int b = 0; b < p.B; ++b)
        for (int y = 0; y < p.H; ++y)
            for (int x = 0; x < p.W; ++x) jpd_pixel(p, b, y, x);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(p.status, 4, (size_t)p.B, f) != (size_t)p.B || fwrite(dst, esz, (size_t)p.B * p.dst_stride, f) != (size_t)p.B * p.dst_stride) return 6;
    fclose(f);
    free(seg); free(image_seg); free(tables); free(payload); free(dst); free(p.status); free(p.coef); free(p.planes); free(p.info);
    return 0;
}
