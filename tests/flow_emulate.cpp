// flow_emulate.cpp -- the programs of gaussianprediction_amd/csrc/flow_core.h on a CPU, element by element in the kernels' tile order,
// in a stand-alone program (tests/test_flow_host.py builds it under the sanitizers and runs it as a child).
//   flow_emulate JOB OUT
// JOB begins with int32 op; everything else is little-endian and packed:
//   0 project   int32 W0, H0, W1, H1; int64 N; float v0[16], p0[16], v1[16], p1[16]; float xyz0[N][3], xyz1[N][3]   -> float out[N][3]
//   1 resolve   int32 H, W; float alpha_min; float composite[3][H][W]                       -> float flow[2][H][W], alpha[H][W]; uint8 valid[H][W]
//   2 colorize  int32 H, W, has_valid; float max_flow, bg[3]; float flow[2][H][W]; uint8 valid[H][W] if has_valid   -> float scale; float out[3][H][W]
//   3 metrics   int32 B, H, W, has_mask; float flow[B][2][H][W], gt[B][2][H][W]; uint8 mask[B][H][W] if has_mask      -> double table[B][8]
//   4 warp      int32 C, H, W; float image[C][H][W], flow[2][H][W]                          -> float out[C][H][W]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../gaussianprediction_amd/csrc/flow_core.h"

template <typename T>
static void get(FILE* fp, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short job file\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short write\n"); exit(2); }
}

#define BLOCK 256
#define PER_LANE (GP_FLOW_TILE / BLOCK)

// the workgroup's sum of 256 lane values as fl_metric_kernel forms it: xor butterflies in the four waves, then (w0 + w1) + (w2 + w3)
static double block_sum(const float* lane) {
    float w[4];
    for (int wave = 0; wave < 4; ++wave) {
        float v[64], n[64];
        for (int l = 0; l < 64; ++l) v[l] = lane[wave * 64 + l];
        for (int d = 32; d >= 1; d >>= 1) {
            for (int l = 0; l < 64; ++l) n[l] = v[l] + v[l ^ d];
            for (int l = 0; l < 64; ++l) v[l] = n[l];
        }
        w[wave] = v[0];
    }
    return (double)((w[0] + w[1]) + (w[2] + w[3]));
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!fp || !out) return 2;
    int32_t op;
    get(fp, &op, 1);
    if (op == 0) {
        int32_t W0, H0, W1, H1;
        int64_t N;
        float v0[16], p0[16], v1[16], p1[16];
        get(fp, &W0, 1); get(fp, &H0, 1); get(fp, &W1, 1); get(fp, &H1, 1); get(fp, &N, 1);
        get(fp, v0, 16); get(fp, p0, 16); get(fp, v1, 16); get(fp, p1, 16);
        std::vector<float> a(N * 3), b(N * 3), o(N * 3);
        get(fp, a.data(), a.size()); get(fp, b.data(), b.size());
        for (int64_t i = 0; i < N; ++i) fl_project_row(v0, p0, W0, H0, v1, p1, W1, H1, &a[i * 3], &b[i * 3], &o[i * 3]);
        put(out, o.data(), o.size());
    } else if (op == 1) {
        int32_t H, W;
        float alpha_min;
        get(fp, &H, 1); get(fp, &W, 1); get(fp, &alpha_min, 1);
        if (fl_refuse_plane(H, W)) return 3;
        const size_t plane = (size_t)H * W;
        std::vector<float> c(3 * plane), flow(2 * plane), alpha(plane);
        std::vector<uint8_t> valid(plane);
        get(fp, c.data(), c.size());
        for (size_t p = 0; p < plane; ++p) {
            const FlResolved r = fl_resolve_pixel(c[p], c[plane + p], c[2 * plane + p], alpha_min);
            flow[p] = r.u; flow[plane + p] = r.v; alpha[p] = r.alpha; valid[p] = r.valid;
        }
        put(out, flow.data(), flow.size()); put(out, alpha.data(), alpha.size()); put(out, valid.data(), valid.size());
    } else if (op == 2) {
        int32_t H, W, has_valid;
        float max_flow, bg[3];
        get(fp, &H, 1); get(fp, &W, 1); get(fp, &has_valid, 1); get(fp, &max_flow, 1); get(fp, bg, 3);
        if (fl_refuse_plane(H, W)) return 3;
        const size_t plane = (size_t)H * W;
        std::vector<float> flow(2 * plane), o(3 * plane), wheel(GP_FLOW_WHEEL * 3);
        std::vector<uint8_t> valid(has_valid ? plane : 0);
        get(fp, flow.data(), flow.size()); get(fp, valid.data(), valid.size());
        const uint8_t* vp = has_valid ? valid.data() : nullptr;
        for (int k = 0; k < GP_FLOW_WHEEL * 3; ++k) wheel[k] = fl_wheel(k / 3, k % 3);
        float scale_word = max_flow;
        if (!(max_flow > 0.f)) {                       // fl_max_kernel: workgroups of GP_FLOW_TILE pixels, lane t its pixels t + 256 u
            uint32_t best = 0u;
            for (size_t tile = 0; tile * GP_FLOW_TILE < plane; ++tile)
                for (int t = 0; t < BLOCK; ++t)
                    for (int u = 0; u < PER_LANE; ++u) {
                        const size_t p = tile * GP_FLOW_TILE + (size_t)u * BLOCK + t;
                        if (p < plane && fl_coloured(flow[p], flow[plane + p], vp, (int64_t)p)) {
                            const uint32_t b = fl_magnitude_bits(flow[p], flow[plane + p]);
                            best = b > best ? b : best;
                        }
                    }
            memcpy(&scale_word, &best, 4);
        }
        const float s = fl_scale_of(max_flow, scale_word);
        for (size_t p = 0; p < plane; ++p) {
            float col[3] = {bg[0], bg[1], bg[2]};
            if (fl_coloured(flow[p], flow[plane + p], vp, (int64_t)p)) fl_color(flow[p], flow[plane + p], s, wheel.data(), col);
            for (int c = 0; c < 3; ++c) o[c * plane + p] = col[c];
        }
        put(out, &scale_word, 1); put(out, o.data(), o.size());
    } else if (op == 3) {
        int32_t B, H, W, has_mask;
        get(fp, &B, 1); get(fp, &H, 1); get(fp, &W, 1); get(fp, &has_mask, 1);
        if (B <= 0 || fl_refuse_plane(H, W)) return 3;
        const size_t plane = (size_t)H * W, tiles = (size_t)fl_tiles(H, W);
        std::vector<float> flow((size_t)B * 2 * plane), gt((size_t)B * 2 * plane);
        std::vector<uint8_t> mask(has_mask ? (size_t)B * plane : 0);
        get(fp, flow.data(), flow.size()); get(fp, gt.data(), gt.size()); get(fp, mask.data(), mask.size());
        std::vector<double> slots((size_t)B * tiles * GP_FLOW_SUMS), table((size_t)B * GP_FLOW_COLUMNS);
        for (int32_t b = 0; b < B; ++b) {
            const float* f = &flow[(size_t)b * 2 * plane];
            const float* g = &gt[(size_t)b * 2 * plane];
            const uint8_t* mk = has_mask ? &mask[(size_t)b * plane] : nullptr;
            for (size_t tile = 0; tile < tiles; ++tile) {
                float lanes[GP_FLOW_SUMS][BLOCK];
                for (int t = 0; t < BLOCK; ++t) {
                    float acc[GP_FLOW_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    for (int u = 0; u < PER_LANE; ++u) {
                        const size_t p = tile * GP_FLOW_TILE + (size_t)u * BLOCK + t;
                        if (p < plane) fl_metric_terms(f[p], f[plane + p], g[p], g[plane + p], !mk || mk[p] != 0, acc);
                    }
                    for (int q = 0; q < GP_FLOW_SUMS; ++q) lanes[q][t] = acc[q];
                }
                for (int q = 0; q < GP_FLOW_SUMS; ++q) slots[((size_t)b * tiles + tile) * GP_FLOW_SUMS + q] = block_sum(lanes[q]);
            }
            // fl_metric_finalize: lane t the slots t, t + 256, ...; then the tree of strides 128 .. 1
            double sum[GP_FLOW_SUMS][BLOCK];
            for (int t = 0; t < BLOCK; ++t)
                for (int q = 0; q < GP_FLOW_SUMS; ++q) {
                    double a = 0.0;
                    for (size_t k = t; k < tiles; k += BLOCK) a += slots[((size_t)b * tiles + k) * GP_FLOW_SUMS + q];
                    sum[q][t] = a;
                }
            for (int stride = BLOCK / 2; stride >= 1; stride >>= 1)
                for (int t = 0; t < stride; ++t)
                    for (int q = 0; q < GP_FLOW_SUMS; ++q) sum[q][t] += sum[q][t + stride];
            double s[GP_FLOW_SUMS];
            for (int q = 0; q < GP_FLOW_SUMS; ++q) s[q] = sum[q][0];
            fl_metric_row(s, &table[(size_t)b * GP_FLOW_COLUMNS]);
        }
        put(out, table.data(), table.size());
    } else if (op == 4) {
        int32_t C, H, W;
        get(fp, &C, 1); get(fp, &H, 1); get(fp, &W, 1);
        if (C <= 0 || fl_refuse_plane(H, W)) return 3;
        const size_t plane = (size_t)H * W;
        std::vector<float> image((size_t)C * plane), flow(2 * plane), o((size_t)C * plane);
        get(fp, image.data(), image.size()); get(fp, flow.data(), flow.size());
        for (size_t p = 0; p < plane; ++p) {
            const int32_t y = (int32_t)(p / (size_t)W), x = (int32_t)(p - (size_t)y * W);
            for (int32_t c = 0; c < C; ++c) o[(size_t)c * plane + p] = fl_warp_pixel(&image[(size_t)c * plane], H, W, x, y, flow[p], flow[plane + p]);
        }
        put(out, o.data(), o.size());
    } else {
        return 2;
    }
    fclose(out);
    fclose(fp);
    return 0;
}
