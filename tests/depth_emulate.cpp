// depth_emulate.cpp -- the programs of gaussianprediction_amd/csrc/depth_core.h on a CPU, element by element in the kernels' tile order,
// in a stand-alone program (tests/test_depth_host.py builds it under the sanitizers and runs it as a child).
//   depth_emulate JOB OUT
// JOB begins with int32 op; everything else is little-endian and packed:
//   0 resolve    int32 H, W; float alpha_min; float accum[H][W], alpha[H][W]                       -> float depth[H][W]; uint8 valid[H][W]
//   1 colorize   int32 H, W, has_valid, mode; float lo, hi, bg[3]; float depth[H][W], lut[256][3]; uint8 valid[H][W] if has_valid
//                                                                                                   -> float range[2]; float out[3][H][W]
//   2 normals    int32 H, W, has_valid; float tanfovx, tanfovy, bg[3]; float depth[H][W]; uint8 valid[H][W] if has_valid
//                                                                     -> float normals[3][H][W]; uint8 nvalid[H][W]; float picture[3][H][W]
//   3 unproject  int32 H, W, has_valid, has_image; float tanfovx, tanfovy, cam2world[16]; float depth[H][W]; uint8 valid[H][W] if has_valid;
//                float image[3][H][W] if has_image
//                -> int32 count; float points[H*W][3]; float colors[H*W][3] if has_image; int32 index[H*W]   (rows beyond count: -7)
//   4 metrics    int32 B, H, W, has_mask, has_scale; float gt_min, gt_max; float pred[B][H][W], gt[B][H][W]; uint8 mask[B][H][W] if has_mask;
//                float scale[B] if has_scale                                                        -> double table[B][12]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../gaussianprediction_amd/csrc/depth_core.h"

template <typename T>
static void get(FILE* fp, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short job file\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short write\n"); exit(2); }
}

// the workgroup's sum of 256 lane values as dp_metric_kernel forms it: xor butterflies in the four waves, then (w0 + w1) + (w2 + w3)
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
    int32_t op, H, W;
    get(fp, &op, 1);
    if (op < 0 || op > 4) return 2;
    if (op == 4) {
        int32_t B, has_mask, has_scale;
        float gt_min, gt_max;
        get(fp, &B, 1); get(fp, &H, 1); get(fp, &W, 1); get(fp, &has_mask, 1); get(fp, &has_scale, 1); get(fp, &gt_min, 1); get(fp, &gt_max, 1);
        if (B <= 0 || B > 65535 || dp_refuse_plane(H, W)) return 3;
        const size_t plane = (size_t)H * W, tiles = (size_t)dp_tiles(H, W);
        std::vector<float> pred((size_t)B * plane), gt((size_t)B * plane), scale(has_scale ? B : 0);
        std::vector<uint8_t> mask(has_mask ? (size_t)B * plane : 0);
        get(fp, pred.data(), pred.size()); get(fp, gt.data(), gt.size()); get(fp, mask.data(), mask.size()); get(fp, scale.data(), scale.size());
        std::vector<double> slots((size_t)B * tiles * GP_DEPTH_SUMS), table((size_t)B * GP_DEPTH_COLUMNS);
        for (int32_t b = 0; b < B; ++b) {
            const float* d = &pred[(size_t)b * plane];
            const float* g = &gt[(size_t)b * plane];
            const uint8_t* mk = has_mask ? &mask[(size_t)b * plane] : nullptr;
            const float* sc = has_scale ? &scale[b] : nullptr;
            for (size_t tile = 0; tile < tiles; ++tile) {
                float lanes[GP_DEPTH_SUMS][DP_BLOCK];
                for (int t = 0; t < DP_BLOCK; ++t) {
                    float acc[GP_DEPTH_SUMS];
                    for (int q = 0; q < GP_DEPTH_SUMS; ++q) acc[q] = 0.f;
                    for (int u = 0; u < DP_PER_LANE; ++u) {
                        const size_t p = (size_t)dp_tile_pixel((int64_t)tile, u, t);
                        if (p < plane) dp_metric_terms(d[p], g[p], !mk || mk[p] != 0, sc, gt_min, gt_max, acc);
                    }
                    for (int q = 0; q < GP_DEPTH_SUMS; ++q) lanes[q][t] = acc[q];
                }
                for (int q = 0; q < GP_DEPTH_SUMS; ++q) slots[((size_t)b * tiles + tile) * GP_DEPTH_SUMS + q] = block_sum(lanes[q]);
            }
            // dp_metric_finalize: lane t the slots t, t + 256, ...; then the tree of strides 128 .. 1
            static double sum[GP_DEPTH_SUMS][DP_BLOCK];
            for (int t = 0; t < DP_BLOCK; ++t)
                for (int q = 0; q < GP_DEPTH_SUMS; ++q) {
                    double a = 0.0;
                    for (size_t k = t; k < tiles; k += DP_BLOCK) a += slots[((size_t)b * tiles + k) * GP_DEPTH_SUMS + q];
                    sum[q][t] = a;
                }
            for (int stride = DP_BLOCK / 2; stride >= 1; stride >>= 1)
                for (int t = 0; t < stride; ++t)
                    for (int q = 0; q < GP_DEPTH_SUMS; ++q) sum[q][t] += sum[q][t + stride];
            double s[GP_DEPTH_SUMS];
            for (int q = 0; q < GP_DEPTH_SUMS; ++q) s[q] = sum[q][0];
            dp_metric_row(s, &table[(size_t)b * GP_DEPTH_COLUMNS]);
        }
        put(out, table.data(), table.size());
        fclose(out);
        fclose(fp);
        return 0;
    }
    get(fp, &H, 1); get(fp, &W, 1);
    if (dp_refuse_plane(H, W)) return 3;
    const size_t plane = (size_t)H * W, tiles = (size_t)dp_tiles(H, W);
    if (op == 0) {
        float alpha_min;
        get(fp, &alpha_min, 1);
        std::vector<float> accum(plane), alpha(plane), depth(plane);
        std::vector<uint8_t> valid(plane);
        get(fp, accum.data(), plane); get(fp, alpha.data(), plane);
        for (size_t p = 0; p < plane; ++p) {
            const DpResolved r = dp_resolve_pixel(accum[p], alpha[p], alpha_min);
            depth[p] = r.depth; valid[p] = r.valid;
        }
        put(out, depth.data(), plane); put(out, valid.data(), plane);
    } else if (op == 1) {
        int32_t has_valid, mode;
        float lo, hi, bg[3];
        get(fp, &has_valid, 1); get(fp, &mode, 1); get(fp, &lo, 1); get(fp, &hi, 1); get(fp, bg, 3);
        std::vector<float> depth(plane), lut(GP_DEPTH_LUT * 3), o(3 * plane);
        std::vector<uint8_t> valid(has_valid ? plane : 0);
        get(fp, depth.data(), plane); get(fp, lut.data(), lut.size()); get(fp, valid.data(), valid.size());
        const uint8_t* vp = has_valid ? valid.data() : nullptr;
        uint32_t lo_bits = DP_RANGE_LO_INIT, hi_bits = DP_RANGE_HI_INIT;
        if (!(lo < hi)) {                              // dp_range_kernel: workgroups of GP_DEPTH_TILE pixels, lane t its pixels t + 256 u
            for (size_t tile = 0; tile < tiles; ++tile)
                for (int t = 0; t < DP_BLOCK; ++t)
                    for (int u = 0; u < DP_PER_LANE; ++u) {
                        const size_t p = (size_t)dp_tile_pixel((int64_t)tile, u, t);
                        float v;
                        if (p < plane && dp_value(depth[p], vp, (int64_t)p, mode, &v)) {
                            const uint32_t b = dp_bits(v);
                            lo_bits = b < lo_bits ? b : lo_bits;
                            hi_bits = b > hi_bits ? b : hi_bits;
                        }
                    }
        }
        float range[2];
        dp_range_of(lo, hi, lo_bits, hi_bits, range);
        for (size_t p = 0; p < plane; ++p) {
            float col[3] = {bg[0], bg[1], bg[2]}, v;
            if (dp_value(depth[p], vp, (int64_t)p, mode, &v)) {
                const int row = dp_lut_row(v, range[0], range[1]);
                if (row < 0 || row >= GP_DEPTH_LUT) return 4;
                for (int c = 0; c < 3; ++c) col[c] = lut[row * 3 + c];
            }
            for (int c = 0; c < 3; ++c) o[c * plane + p] = col[c];
        }
        put(out, range, 2); put(out, o.data(), o.size());
    } else if (op == 2) {
        int32_t has_valid;
        float tanfovx, tanfovy, bg[3];
        get(fp, &has_valid, 1); get(fp, &tanfovx, 1); get(fp, &tanfovy, 1); get(fp, bg, 3);
        std::vector<float> depth(plane), n(3 * plane), pic(3 * plane);
        std::vector<uint8_t> valid(has_valid ? plane : 0), nvalid(plane);
        get(fp, depth.data(), plane); get(fp, valid.data(), valid.size());
        for (size_t p = 0; p < plane; ++p) {
            const int32_t y = (int32_t)(p / (size_t)W), x = (int32_t)(p - (size_t)y * W);
            float v[3];
            nvalid[p] = dp_normal(depth.data(), has_valid ? valid.data() : nullptr, x, y, tanfovx, tanfovy, W, H, v);
            for (int c = 0; c < 3; ++c) {
                n[c * plane + p] = v[c];
                pic[c * plane + p] = nvalid[p] ? v[c] * 0.5f + 0.5f : bg[c];
            }
        }
        put(out, n.data(), n.size()); put(out, nvalid.data(), plane); put(out, pic.data(), pic.size());
    } else {
        int32_t has_valid, has_image;
        float tanfovx, tanfovy, m[16];
        get(fp, &has_valid, 1); get(fp, &has_image, 1); get(fp, &tanfovx, 1); get(fp, &tanfovy, 1); get(fp, m, 16);
        std::vector<float> depth(plane), image(has_image ? 3 * plane : 0), points(3 * plane, -7.f), colors(has_image ? 3 * plane : 0, -7.f);
        std::vector<uint8_t> valid(has_valid ? plane : 0);
        std::vector<int32_t> index(plane, -7);
        get(fp, depth.data(), plane); get(fp, valid.data(), valid.size()); get(fp, image.data(), image.size());
        const uint8_t* vp = has_valid ? valid.data() : nullptr;
        // dp_count_kernel: sixteen ballots a tile, in the lanes' order
        std::vector<uint32_t> counts(tiles), chunk(tiles * DP_CHUNKS, 0u);
        for (size_t tile = 0; tile < tiles; ++tile) {
            for (int u = 0; u < DP_PER_LANE; ++u)
                for (int t = 0; t < DP_BLOCK; ++t) {
                    const size_t p = (size_t)dp_tile_pixel((int64_t)tile, u, t);
                    if (p < plane && (!vp || vp[p] != 0)) chunk[tile * DP_CHUNKS + dp_chunk(u, t)] += 1u;
                }
            uint32_t n = 0;
            for (int c = 0; c < DP_CHUNKS; ++c) n += chunk[tile * DP_CHUNKS + c];
            counts[tile] = n;
        }
        // dp_scan_kernel: exclusive, ascending
        uint32_t carry = 0;
        for (size_t tile = 0; tile < tiles; ++tile) { const uint32_t a = counts[tile]; counts[tile] = carry; carry += a; }
        const int32_t count = (int32_t)carry;
        // dp_place_kernel: the tile's offset + the chunks before the pixel's own + the set bits below its lane
        for (size_t tile = 0; tile < tiles; ++tile)
            for (int u = 0; u < DP_PER_LANE; ++u) {
                uint32_t below[4] = {0u, 0u, 0u, 0u};          // per wave, as the lanes are walked in ascending order
                for (int t = 0; t < DP_BLOCK; ++t) {
                    const size_t p = (size_t)dp_tile_pixel((int64_t)tile, u, t);
                    if (!(p < plane && (!vp || vp[p] != 0))) continue;
                    uint32_t before = 0;
                    for (int c = 0; c < dp_chunk(u, t); ++c) before += chunk[tile * DP_CHUNKS + c];
                    const size_t row = (size_t)counts[tile] + before + below[t / 64]++;
                    if (row >= (size_t)count) return 4;
                    const int32_t y = (int32_t)(p / (size_t)W), x = (int32_t)(p - (size_t)y * W);
                    const DpVec X = dp_world(m, dp_point(x, y, depth[p], tanfovx, tanfovy, W, H));
                    points[row * 3] = X.x; points[row * 3 + 1] = X.y; points[row * 3 + 2] = X.z;
                    if (has_image) for (int c = 0; c < 3; ++c) colors[row * 3 + c] = image[c * plane + p];
                    index[row] = (int32_t)p;
                }
            }
        put(out, &count, 1); put(out, points.data(), points.size()); put(out, colors.data(), colors.size()); put(out, index.data(), plane);
    }
    fclose(out);
    fclose(fp);
    return 0;
}
