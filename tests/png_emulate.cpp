// The PNG encoder's workgroup programs (csrc/png_core.h) run on the CPU, every phase as a loop over the lanes:
//   png_emulate H W src_kind flags in.raw out.png      (in.raw: [3][H][W] float32 or uint8)
// tests/test_png_host.py builds this with the host compiler and holds the files against Pillow and zlib.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../gaussianprediction_amd/csrc/png_core.h"

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    PngPlan p{};
    p.B = 1; p.H = atoi(argv[1]); p.W = atoi(argv[2]); p.src_kind = atoi(argv[3]); p.flags = (uint32_t)atoi(argv[4]);
    p.row = 1 + 3 * p.W;
    p.S = (int64_t)p.H * p.row;
    p.S_pad = (p.S + 15) / 16 * 16;
    p.NB = (int)((p.S + PNG_BAND - 1) / PNG_BAND);
    const size_t elems = (size_t)3 * p.H * p.W, esz = p.src_kind == GP_PNG_SRC_U8 ? 1 : 4;
    std::vector<uint8_t> src(elems * esz);
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(src.data(), 1, src.size(), f) != src.size()) return 3;
    fclose(f);
    const size_t bound = (size_t)(p.S + 17 * (int64_t)p.NB + 56 + 7) / 8 * 8;
    std::vector<uint8_t> filt((size_t)p.S_pad, 0xee), comp((size_t)p.NB * PNG_COMP_STRIDE, 0xee), out(bound, 0xcc);
    std::vector<uint32_t> info((size_t)p.NB * 4), chunk_off((size_t)p.NB), adler(1), sizes(1);
    p.src = src.data(); p.filt = filt.data(); p.comp = comp.data(); p.info = info.data(); p.chunk_off = chunk_off.data();
    p.adler = adler.data(); p.out = out.data(); p.out_stride = (int64_t)bound; p.sizes = sizes.data();
    static PngFilterShared fs;
    static PngBandShared bs;
    static PngLayoutShared ls;
    static PngChunkShared cs;
    for (int y = 0; y < p.H; ++y) png_filter_block(fs, p, 0, y);
    for (int k = 0; k < p.NB; ++k) png_band_block(bs, p, 0, k);
    png_layout_block(ls, p, 0);
    for (int k = 0; k < p.NB; ++k) png_chunk_block(cs, p, 0, k);
    if (sizes[0] > bound) return 4;
    for (size_t i = sizes[0]; i < bound; ++i)
        if (out[i] != 0xcc) return 5;                 // nothing is written at or beyond the file's length
    f = fopen(argv[6], "wb");
    if (!f || fwrite(out.data(), 1, sizes[0], f) != sizes[0]) return 6;
    fclose(f);
    return 0;
}
