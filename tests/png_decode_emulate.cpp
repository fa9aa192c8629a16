// The PNG decoder's workgroup programs (csrc/png_decode_core.h) run on the CPU, every phase as a loop over the lanes:
//   png_decode_emulate job.bin out.bin
// job.bin: int32 B, H, W, C, C_out, dst_kind, has_bg, nseg, guard; float bg[3]; int64 payload_bytes; int64 segments[nseg][5];
//          int32 image_seg[B + 1]; the payload.
// out.bin: uint32 status[B], mode[B]; then B slots of C_out * H * W + guard elements (filled with 0xa5 before the run).
// Every buffer is its own heap block of exactly the size the C entry asks for, so that -fsanitize=address,undefined (how
// tests/test_png_decode_host.py builds this where the host compiler can) sees any access outside them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../gaussianprediction_amd/csrc/png_decode_core.h"

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
    int32_t h[9];
    float bg[3];
    int64_t payload_bytes;
    if (fread(h, 4, 9, f) != 9 || fread(bg, 4, 3, f) != 3 || fread(&payload_bytes, 8, 1, f) != 1) return 3;
    PngdPlan p{};
    p.B = h[0]; p.H = h[1]; p.W = h[2]; p.C = h[3]; p.C_out = h[4]; p.dst_kind = h[5]; p.nseg = h[7];
    const int guard = h[8];
    p.row = 1 + p.C * p.W;
    p.S = (int64_t)p.H * p.row;
    p.S_pad = (p.S + 15) / 16 * 16;
    int64_t* seg = block<int64_t>((size_t)p.nseg * PNGD_SEG_WORDS, 0);
    int32_t* image_seg = block<int32_t>((size_t)p.B + 1, 0);
    uint8_t* payload = block<uint8_t>((size_t)payload_bytes, 0);
    if (fread(seg, 8, (size_t)p.nseg * PNGD_SEG_WORDS, f) != (size_t)p.nseg * PNGD_SEG_WORDS || fread(image_seg, 4, (size_t)p.B + 1, f) != (size_t)p.B + 1 ||
        fread(payload, 1, (size_t)payload_bytes, f) != (size_t)payload_bytes)
        return 3;
    fclose(f);
    const size_t esz = p.dst_kind == GP_PNG_DECODE_DST_F32 ? 4 : 1;
    p.dst_stride = (int64_t)p.C_out * p.H * p.W + guard;
    uint8_t* dst = block<uint8_t>((size_t)p.B * p.dst_stride * esz, 0xa5);
    p.payload = payload; p.payload_bytes = payload_bytes; p.seg = seg; p.image_seg = image_seg; p.bg = h[6] ? bg : nullptr;
    p.dst = dst;
    p.status = block<uint32_t>((size_t)p.B, 0xee);
    p.mode = block<uint32_t>((size_t)p.B, 0xee);
    p.filt = block<uint8_t>((size_t)p.B * p.S_pad, 0xee);
    p.info = block<uint32_t>((size_t)p.nseg * PNGD_INFO_WORDS, 0xee);
    static PngdInflateShared is;
    static PngdStatusShared ss;
    static PngdUnfilterShared us;
    for (int k = 0; k < p.nseg; ++k) pngd_inflate_block(is, p, k);
    for (int b = 0; b < p.B; ++b) pngd_status_block(ss, p, b);
    for (int b = 0; b < p.B; ++b) pngd_unfilter_block(us, p, b);
    for (int b = 0; b < p.B; ++b)
        for (int y = 0; y < p.H; ++y)
            for (int x = 0; x < p.W; ++x) pngd_convert_pixel(p, b, y, x);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(p.status, 4, (size_t)p.B, f) != (size_t)p.B || fwrite(p.mode, 4, (size_t)p.B, f) != (size_t)p.B ||
        fwrite(dst, esz, (size_t)p.B * p.dst_stride, f) != (size_t)p.B * p.dst_stride)
        return 6;
    fclose(f);
    free(seg); free(image_seg); free(payload); free(dst); free(p.status); free(p.mode); free(p.filt); free(p.info);
    return 0;
}
