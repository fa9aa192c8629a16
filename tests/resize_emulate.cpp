// The resize kernels' programs (csrc/resize_core.h) run on the CPU, every phase as a loop over the lanes, over the grids the C entry
// launches:
//   resize_emulate job.bin out.bin
// job.bin: int32 B, C, H, W, Ho, Wo, filter, alpha_mode, dst_kind, src_gap, guard; then B images [C][H][W] of bytes.
// out.bin: int32 path; then B slots of C * Ho * Wo + guard elements (filled with 0xa5 before the run).
// The images lie src_gap bytes apart.  Every buffer -- the tables, the LDS of a fused workgroup, the scratch -- is its own heap block
// of exactly the size the C entry asks for, so that -fsanitize=address,undefined (how tests/test_resize_host.py builds this where the
// host compiler can) sees any access outside them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../gaussianprediction_amd/csrc/resize_core.h"

template <class T>
static T* block(size_t n, int fill) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (!p) exit(7);
    memset(p, fill, n * sizeof(T));
    return p;
}

static unsigned blocks(int n, int per) { return (unsigned)((n + per - 1) / per); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t h[11];
    if (fread(h, 4, 11, f) != 11) return 3;
    const int B = h[0], C = h[1], H = h[2], W = h[3], Ho = h[4], Wo = h[5], filter = h[6], alpha_mode = h[7], dst_kind = h[8], src_gap = h[9], guard = h[10];
    RsAxis ax, ay;
    if (B < 1 || (C != 1 && C != 3 && C != 4) || (alpha_mode && C != 4) || rs_axis(ax, W, Wo, filter) || rs_axis(ay, H, Ho, filter)) return 4;
    const size_t image = (size_t)C * H * W, src_stride = image + src_gap, elem = dst_kind == GP_RESIZE_DST_F32 ? 4 : 1;
    const size_t slot = (size_t)C * Ho * Wo + guard;
    uint8_t* src = block<uint8_t>((B - 1) * src_stride + image, 0x5a);
    for (int b = 0; b < B; ++b)
        if (fread(src + b * src_stride, 1, image, f) != image) return 3;
    fclose(f);
    uint8_t* dst = block<uint8_t>(B * slot * elem, 0xa5);
    int rows;
    RsPlan p{};
    p.B = B; p.C = C; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo;
    p.alpha_mode = alpha_mode; p.dst_kind = dst_kind;
    p.path = rs_path(ax, ay, &rows);
    p.rows = rows;
    p.src = src; p.src_stride = (int64_t)src_stride; p.dst = dst; p.dst_stride = (int64_t)(slot * elem);
    double* w = block<double>(ax.ksize > ay.ksize ? ax.ksize : ay.ksize, 0);
    if (W != Wo) {
        int32_t* xb = block<int32_t>(2 * (size_t)Wo, 0x7f), *xk = block<int32_t>((size_t)Wo * ax.ksize, 0x7f);
        rs_coeffs(ax, xb, xk, w);
        p.xb = xb; p.xk = xk; p.xtaps = ax.ksize;
    }
    if (H != Ho) {
        int32_t* yb = block<int32_t>(2 * (size_t)Ho, 0x7f), *yk = block<int32_t>((size_t)Ho * ay.ksize, 0x7f);
        rs_coeffs(ay, yb, yk, w);
        p.yb = yb; p.yk = yk; p.ytaps = ay.ksize;
    }
    if (p.path == GP_RESIZE_PATH_TWO_LAUNCH) p.mid = block<uint8_t>((size_t)B * C * H * Wo, 0x3c);
    const unsigned planes = (unsigned)(B * C);
    // a launch of one-lane-per-sample programs: grid (gx, gy, gz) of RS_BLOCK lanes
    auto launch = [&](void (*program)(const RsPlan&, int, int, int), unsigned gx, unsigned gy, unsigned gz) {
        for (unsigned z = 0; z < gz; ++z)
            for (unsigned y = 0; y < gy; ++y)
                for (unsigned x = 0; x < gx * RS_BLOCK; ++x) program(p, (int)x, (int)y, (int)z);
    };
    switch (p.path) {
        case GP_RESIZE_PATH_COPY: launch(rs_copy_sample, blocks(W, RS_BLOCK), H, planes); break;
        case GP_RESIZE_PATH_HORIZONTAL: launch(rs_horizontal_sample, blocks(Wo, RS_BLOCK), H, planes); break;
        case GP_RESIZE_PATH_VERTICAL: launch(rs_vertical_sample, blocks(Wo, RS_BLOCK), Ho, planes); break;
        case GP_RESIZE_PATH_TWO_LAUNCH:
            launch(rs_horizontal_sample, blocks(Wo, RS_BLOCK), H, planes);
            launch(rs_vertical_sample, blocks(Wo, RS_BLOCK), Ho, planes);
            break;
        case GP_RESIZE_PATH_FUSED: {
            const size_t lds_bytes = (size_t)rs_fused_lds(ax, ay, &rows);
            if (lds_bytes > RS_LDS_BUDGET || lds_bytes % 4) return 5;
            for (unsigned z = 0; z < (alpha_mode ? (unsigned)B : planes); ++z)
                for (unsigned y = 0; y < blocks(Ho, GP_RESIZE_TILE_H); ++y)
                    for (unsigned x = 0; x < blocks(Wo, GP_RESIZE_TILE_W); ++x) {
                        int32_t* lds = block<int32_t>(lds_bytes / 4, 0x7f);      // (uninitialised on a device: garbage here)
                        rs_fused_block(lds, p, (int)x, (int)y, (int)z);
                        free(lds);
                    }
            break;
        }
        default: return 6;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 3;
    const int32_t path = p.path;
    fwrite(&path, 4, 1, f);
    fwrite(dst, elem, B * slot, f);
    fclose(f);
    free(src); free(dst); free(w); free(p.mid);
    free((void*)p.xb); free((void*)p.xk); free((void*)p.yb); free((void*)p.yk);
    return 0;
}
