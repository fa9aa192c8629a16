// The JPEG encoder's workgroup programs (csrc/jpeg_core.h) run on the CPU, every phase as a loop over the lanes:
//   jpeg_emulate H W src_kind subsampling qt.bin in.raw out.jpg      (in.raw: [3][H][W] float32 or uint8; qt.bin: the luminance and the
//   jpeg_emulate tables quality out.bin                               chrominance table, 64 bytes each in natural order)
// tests/test_jpeg_host.py builds this with the host compiler and holds the files against Pillow and its own entropy decoder.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../gaussianprediction_amd/csrc/jpeg_core.h"

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "tables")) {
        uint8_t qt[128];
        jpg_quant_tables(atoi(argv[2]), qt, qt + 64);
        FILE* f = fopen(argv[3], "wb");
        if (!f || fwrite(qt, 1, 128, f) != 128) return 6;
        fclose(f);
        return 0;
    }
    if (argc != 8) return 2;
    JpgPlan p{};
    jpg_plan_sizes(p, 1, atoi(argv[1]), atoi(argv[2]), atoi(argv[4]));
    p.src_kind = atoi(argv[3]);
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(p.qt, 1, 128, f) != 128) return 3;
    fclose(f);
    const size_t elems = (size_t)3 * p.H * p.W, esz = p.src_kind == GP_PNG_SRC_U8 ? 1 : 4;
    std::vector<uint8_t> src(elems * esz);
    f = fopen(argv[6], "rb");
    if (!f || fread(src.data(), 1, src.size(), f) != src.size()) return 3;
    fclose(f);
    if (jpg_build_header(p) != JPG_HEAD) return 7;
    const size_t bound = (size_t)jpg_bound_of(p);
    std::vector<uint8_t> seg((size_t)p.nseg * p.seg_stride, 0xee), out(bound, 0xcc);
    std::vector<uint32_t> seg_len((size_t)p.nseg), seg_off((size_t)p.nseg), sizes(1);
    p.src = src.data(); p.seg = seg.data(); p.seg_len = seg_len.data(); p.seg_off = seg_off.data();
    p.out = out.data(); p.out_stride = (int64_t)bound; p.sizes = sizes.data();
    static JpgSegShared ss;
    static JpgLayoutShared ls;
    for (int s = 0; s < p.nseg; ++s) {
        memset(&ss, 0xee, sizeof ss);                 // (LDS is uninitialised on the device)
        jpg_segment_block(ss, p, 0, s);
        if (seg_len[s] > p.seg_stride) return 8;
    }
    jpg_layout_block(ls, p, 0);
    for (int s = 0; s < p.nseg; ++s) jpg_copy_block(p, 0, s);
    if (sizes[0] > bound) return 4;
    for (size_t i = sizes[0]; i < bound; ++i)
        if (out[i] != 0xcc) return 5;                 // nothing is written at or beyond the file's length
    f = fopen(argv[7], "wb");
    if (!f || fwrite(out.data(), 1, sizes[0], f) != sizes[0]) return 6;
    fclose(f);
    return 0;
}
