// The voxel downsample's programs (csrc/voxel_core.h) in a stand-alone build on the CPU: what gp_voxel_downsample_host runs inside the
// library, here as a program of its own so that it can be built with -fsanitize=address,undefined (how tests/test_voxel_host.py builds
// this where the host compiler can) and run as a child process:
//   voxel_emulate job.bin out.bin
// job.bin: int64 n; int32 has_colors, has_normals; double voxel_size; then points, colours, normals, each [n][3] doubles where present.
// out.bin: int32 rc (0, or the refusal's code: vx_refusal); int64 M; then the M rows of points, colours, normals where present and the
// int32 index [M][3].  Every buffer is its own heap block of exactly n rows.
#include <stdio.h>
#include <stdlib.h>

#include "../gaussianprediction_amd/csrc/voxel_core.h"

template <class T>
static T* block(size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (!p) exit(7);
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t n;
    int32_t has[2];
    double voxel_size;
    if (fread(&n, 8, 1, f) != 1 || fread(has, 4, 2, f) != 2 || fread(&voxel_size, 8, 1, f) != 1 || n < 0) return 3;
    const size_t cells = (size_t)n * 3;
    double *src[3] = {nullptr, nullptr, nullptr}, *dst[3] = {nullptr, nullptr, nullptr};
    for (int a = 0; a < 3; ++a) {
        if (a > 0 && !has[a - 1]) continue;
        src[a] = block<double>(cells);
        dst[a] = block<double>(cells);
        if (fread(src[a], 8, cells, f) != cells) return 3;
    }
    fclose(f);
    int32_t* index = block<int32_t>(cells);
    int64_t m = 0;
    const int32_t rc = vx_downsample_host(n, src[0], src[1], src[2], voxel_size, dst[0], dst[1], dst[2], index, &m);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 5;
    fwrite(&rc, 4, 1, o);
    fwrite(&m, 8, 1, o);
    if (!rc) {
        for (int a = 0; a < 3; ++a)
            if (dst[a]) fwrite(dst[a], 8, (size_t)m * 3, o);
        fwrite(index, 4, (size_t)m * 3, o);
    }
    if (fclose(o)) return 5;
    for (int a = 0; a < 3; ++a) { free(src[a]); free(dst[a]); }
    free(index);
    return 0;
}
