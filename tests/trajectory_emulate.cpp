// trajectory_emulate.cpp -- the programs of gaussianprediction_amd/csrc/trajectory_core.h on a CPU, point by point as the kernels'
// lanes run them, in a stand-alone program (tests/test_trajectory_host.py builds it under the sanitizers and runs it as a child).
//   trajectory_emulate JOB OUT
// JOB:  int32 H, W; int64 N, P, S; int32 has_idx, has_base; float min_depth; float view[15] (R, t, f, cx, cy);
//       int32 idx[P] if has_idx; float colors[P][3]; float base[3][H][W] if has_base; float xyz[S][N][3]
// OUT:  int32 rc (1: refused, and nothing follows); int32 px[S][P][2]; uint32 owner[H][W]; float image[3][H][W]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../gaussianprediction_amd/csrc/trajectory_core.h"

struct HostClaim {
    uint32_t* owner;
    int64_t plane;
    uint32_t key;
    void operator()(int64_t offset) const {
        if (offset < 0 || offset >= plane) abort();          // (the kernels' atomic has no such test: a claim outside the image is a bug)
        if (owner[offset] < key) owner[offset] = key;
    }
};

template <typename T>
static void get(FILE* fp, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short job file\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    int32_t H, W, has_idx, has_base;
    int64_t N, P, S;
    float min_depth;
    gp_traj_view view;
    get(fp, &H, 1); get(fp, &W, 1); get(fp, &N, 1); get(fp, &P, 1); get(fp, &S, 1); get(fp, &has_idx, 1); get(fp, &has_base, 1);
    get(fp, &min_depth, 1); get(fp, view.R, 9); get(fp, view.t, 3); get(fp, &view.f, 1); get(fp, &view.cx, 1); get(fp, &view.cy, 1);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    int32_t rc = 0;
    for (int64_t s = 0; s < (S > 0 ? S : 1); ++s)
        if (tj_refusal(N, P, s, H, W, has_idx != 0)) rc = 1;
    fwrite(&rc, 4, 1, out);
    if (rc) { fclose(out); return 0; }
    const int64_t plane = (int64_t)H * W;
    std::vector<int32_t> idx(has_idx ? P : 0);
    std::vector<float> colors(P * 3), base(has_base ? plane * 3 : 0), xyz(N * 3), image(plane * 3);
    std::vector<TjPixel> px(P);
    std::vector<uint32_t> owner(plane, 0u);
    get(fp, idx.data(), idx.size()); get(fp, colors.data(), colors.size()); get(fp, base.data(), base.size());
    for (int64_t s = 0; s < S; ++s) {
        get(fp, xyz.data(), xyz.size());
        for (int64_t j = 0; j < P; ++j) {
            const uint32_t row = has_idx ? (uint32_t)idx[j] : (uint32_t)j;
            HostClaim claim = {owner.data(), plane, (uint32_t)(s * P) + (uint32_t)j + 1u};
            TjPixel prev = {TJ_NONE, TJ_NONE};
            if (s > 0) prev = px[j];
            px[j] = tj_point_step(view, row < (uint64_t)N ? xyz.data() + (size_t)row * 3 : nullptr, min_depth, s == 0, prev, W, H, claim);
        }
        if (P) fwrite(px.data(), sizeof(TjPixel), P, out);
    }
    for (int64_t p = 0; p < plane; ++p)
        for (int ch = 0; ch < 3; ++ch)
            image[ch * plane + p] = tj_resolve_pixel(owner[p], P ? colors.data() : nullptr, P, has_base ? base.data() : nullptr, p, plane, ch);
    fwrite(owner.data(), 4, plane, out);
    fwrite(image.data(), 4, plane * 3, out);
    fclose(out);
    fclose(fp);
    return 0;
}
