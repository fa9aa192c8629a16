// tsdf_emulate.cpp -- the programs of gaussianprediction_amd/csrc/tsdf_core.h on a CPU, point by point, in a stand-alone program
// (tests/test_tsdf_host.py builds it under the sanitizers and runs it as a child).
//   tsdf_emulate JOB OUT
// JOB begins with int32 op; everything else is little-endian and packed:
//   0 integrate  int32 nx, ny, nz, has_color, V, H, W, has_valid; float origin[3], voxel, trunc, z_min, view_weight, weight_max;
//                V x (float world_view[16], tanfovx, tanfovy); float tsdf[n], weight[n]; float color[3][n] if has_color;
//                float depth[V][H][W]; uint8 valid[V][H][W] if has_valid; float image[V][3][H][W] if has_color
//                                                                        -> float tsdf[n], weight[n]; float color[3][n] if has_color
//   1 extract    int32 nx, ny, nz, has_color; float origin[3], voxel, iso, min_weight; float tsdf[n], weight[n]; float color[3][n] if has_color
//                -> int32 counts[2]; float vertices[counts[0]][3]; float colors[counts[0]][3] if has_color; int32 faces[counts[1]][3]
// The ranks are the running sums over the points in ascending order: what the tiles' offsets and the scans inside a tile add up to.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../gaussianprediction_amd/csrc/tsdf_core.h"

template <typename T>
static void get(FILE* fp, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short job file\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short write\n"); exit(2); }
}

static void ijk(const TsGrid& g, int64_t n, int32_t* i, int32_t* j, int32_t* k) {
    *i = (int32_t)(n % g.nx);
    *j = (int32_t)((n / g.nx) % g.ny);
    *k = (int32_t)(n / ((int64_t)g.nx * g.ny));
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!fp || !out) return 2;
    int32_t op, dims[3], has_color;
    get(fp, &op, 1); get(fp, dims, 3); get(fp, &has_color, 1);
    if (op < 0 || op > 1 || ts_refuse_dims(dims[0], dims[1], dims[2])) return 3;
    gp_tsdf_volume vol;
    vol.nx = dims[0]; vol.ny = dims[1]; vol.nz = dims[2];
    const size_t n_points = (size_t)vol.nx * vol.ny * vol.nz;
    std::vector<float> tsdf(n_points), weight(n_points), color(has_color ? 3 * n_points : 0);
    vol.tsdf = tsdf.data(); vol.weight = weight.data(); vol.color = has_color ? color.data() : nullptr;
    if (op == 0) {
        int32_t V, H, W, has_valid;
        float head[8];
        get(fp, &V, 1); get(fp, &H, 1); get(fp, &W, 1); get(fp, &has_valid, 1); get(fp, head, 8);
        vol.origin_x = head[0]; vol.origin_y = head[1]; vol.origin_z = head[2]; vol.voxel = head[3]; vol.trunc = head[4];
        const float z_min = head[5], view_weight = head[6], weight_max = head[7];
        if (ts_refuse_volume(&vol) || V < 1 || V > GP_TSDF_MAX_VIEWS || H <= 0 || W <= 0) return 3;
        std::vector<float> views((size_t)V * 18);
        get(fp, views.data(), views.size());
        const size_t plane = (size_t)H * W;
        std::vector<float> depth(V * plane), image(has_color ? V * 3 * plane : 0);
        std::vector<uint8_t> valid(has_valid ? V * plane : 0);
        get(fp, tsdf.data(), n_points); get(fp, weight.data(), n_points); get(fp, color.data(), color.size());
        get(fp, depth.data(), depth.size()); get(fp, valid.data(), valid.size()); get(fp, image.data(), image.size());
        const TsGrid g = ts_grid_of(&vol);
        for (size_t n = 0; n < n_points; ++n) {
            int32_t i, j, k;
            ijk(g, (int64_t)n, &i, &j, &k);
            const float x = ts_coord(i, g.voxel, g.ox), y = ts_coord(j, g.voxel, g.oy), z = ts_coord(k, g.voxel, g.oz);
            TsVoxel p;
            p.tsdf = tsdf[n]; p.w = weight[n];
            for (int c = 0; c < 3; ++c) p.c[c] = has_color ? color[c * n_points + n] : 0.f;
            for (int32_t v = 0; v < V; ++v)
                ts_integrate_view(p, x, y, z, &views[(size_t)v * 18], views[(size_t)v * 18 + 16], views[(size_t)v * 18 + 17], &depth[v * plane],
                                  has_valid ? &valid[v * plane] : nullptr, has_color ? &image[v * 3 * plane] : nullptr, H, W, vol.trunc, z_min, view_weight,
                                  weight_max);
            tsdf[n] = p.tsdf; weight[n] = p.w;
            for (int c = 0; c < 3 && has_color; ++c) color[c * n_points + n] = p.c[c];
        }
        put(out, tsdf.data(), n_points); put(out, weight.data(), n_points); put(out, color.data(), color.size());
    } else {
        float head[6];
        get(fp, head, 6);
        vol.origin_x = head[0]; vol.origin_y = head[1]; vol.origin_z = head[2]; vol.voxel = head[3]; vol.trunc = 1.f;
        const float iso = head[4], min_weight = head[5];
        if (ts_refuse_volume(&vol)) return 3;
        get(fp, tsdf.data(), n_points); get(fp, weight.data(), n_points); get(fp, color.data(), color.size());
        const TsGrid g = ts_grid_of(&vol);
        std::vector<uint8_t> active(n_points), marks(n_points), tris(n_points);
        std::vector<uint32_t> first_vertex(n_points), first_tri(n_points);
        for (size_t n = 0; n < n_points; ++n) {                        // ts_active_kernel
            int32_t i, j, k;
            ijk(g, (int64_t)n, &i, &j, &k);
            active[n] = ts_cell_active(tsdf.data(), weight.data(), g, (int64_t)n, i, j, k, min_weight);
        }
        uint32_t nv = 0, nt = 0;
        for (size_t n = 0; n < n_points; ++n) {                        // ts_mark_kernel, ts_scan_kernel and ts_rank_kernel
            int32_t i, j, k;
            ijk(g, (int64_t)n, &i, &j, &k);
            const int corners = ts_corners_inside(tsdf.data(), g, (int64_t)n, i, j, k, iso);
            marks[n] = ts_edge_marks(active.data(), g, (int64_t)n, i, j, k, corners);
            tris[n] = active[n] ? (uint8_t)ts_cell_triangles(corners) : (uint8_t)0;
            first_vertex[n] = nv; first_tri[n] = nt;
            for (int e = 0; e < GP_TSDF_EDGES; ++e) nv += (marks[n] >> e) & 1;
            nt += tris[n];
        }
        const int32_t counts[2] = {(int32_t)nv, (int32_t)nt};
        std::vector<float> vertices((size_t)nv * 3), colors(has_color ? (size_t)nv * 3 : 0);
        std::vector<int32_t> faces((size_t)nt * 3);
        for (size_t n = 0; n < n_points; ++n) {                        // ts_vertex_kernel and ts_face_kernel
            int32_t i, j, k;
            ijk(g, (int64_t)n, &i, &j, &k);
            size_t row = first_vertex[n];
            for (int e = 0; e < GP_TSDF_EDGES; ++e) {
                if (!((marks[n] >> e) & 1)) continue;
                float col[3];
                ts_vertex(tsdf.data(), vol.color, g, (int64_t)n, i, j, k, e, iso, &vertices[row * 3], col);
                for (int c = 0; c < 3 && has_color; ++c) colors[row * 3 + c] = col[c];
                ++row;
            }
            if (tris[n] == 0) continue;
            const int corners = ts_corners_inside(tsdf.data(), g, (int64_t)n, i, j, k, iso);
            if (ts_cell_faces(marks.data(), first_vertex.data(), g, (int64_t)n, corners, tris[n], &faces[(size_t)first_tri[n] * 3]) != tris[n]) return 4;
        }
        for (int32_t f : faces)
            if (f < 0 || f >= counts[0]) return 4;
        put(out, counts, 2); put(out, vertices.data(), vertices.size()); put(out, colors.data(), colors.size()); put(out, faces.data(), faces.size());
    }
    fclose(out);
    fclose(fp);
    return 0;
}
