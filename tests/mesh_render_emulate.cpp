// mesh_render_emulate.cpp -- the programs of gaussianprediction_amd/csrc/mesh_render_core.h on a CPU, element by element, in a
// stand-alone program (tests/test_mesh_render_host.py builds it under the sanitizers and runs it as a child).
//   mesh_render_emulate JOB OUT
// JOB: int32 nv, nf, H, W, cull, C, backwards, 0; float z_near, tanfovx, tanfovy, ambient, shade_background[3], 0, background[8];
// float world_view[16], vertices[nv][3]; int32 faces[nf][3]; float attributes[nv][C].  Everything is little-endian and packed; every
// array has exactly its stated size, so that an index the programs fail to check is an error of the sanitizers.
//   -> int32 counts[8], coverage[H][W], face[H][W]; float depth[H][W]; uint8 valid[H][W]; float bary[3][H][W]; and with C >= 3:
//      float interpolated[C][H][W], normals[3][H][W]; uint8 nvalid[H][W]; float shaded[3][H][W] (the shade of the first three channels)
// The faces are taken in ascending order, or with `backwards` in descending order: no result may depend on it.  A wide face is
// drawn as the device draws it, piece by piece and lane by lane.  Exit 3: a refusal (its words on stderr).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../gaussianprediction_amd/csrc/mesh_render_core.h"

template <typename T>
static void get(FILE* fp, std::vector<T>& v) {
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), fp) != v.size()) { fprintf(stderr, "short job file\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const std::vector<T>& v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), fp) != v.size()) { fprintf(stderr, "short write\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!fp || !out) return 2;
    std::vector<int32_t> head(8);
    std::vector<float> real(16), m(16);
    get(fp, head); get(fp, real); get(fp, m);
    const int64_t nv = head[0], nf = head[1];
    const int32_t H = head[2], W = head[3], cull = head[4], C = head[5];
    const bool backwards = head[6] != 0;
    const char* why = mr_refuse_sizes(nv, nf, H, W);
    if (!why) why = mr_refuse_raster(real[1], real[2], real[0], cull);
    if (!why && (C < 0 || C > GP_MESH_RENDER_MAX_CHANNELS)) why = "C must be 1 .. 8";
    if (why) { fprintf(stderr, "%s\n", why); return 3; }
    MrView view;
    view.tanfovx = real[1]; view.tanfovy = real[2]; view.z_near = real[0]; view.W = W; view.H = H; view.cull = cull;
    const int64_t plane = (int64_t)H * W;
    std::vector<float> vertices(3 * nv), attributes(nv * C);
    std::vector<int32_t> faces(3 * nf);
    get(fp, vertices); get(fp, faces); get(fp, attributes);

    std::vector<MrVertex> records(nv);
    for (int64_t v = 0; v < nv; ++v) records[v] = mr_vertex(m.data(), &vertices[3 * v], view);                          // mr_vertex_kernel
    std::vector<int32_t> counts(GP_MESH_RENDER_COUNT_WORDS, 0), coverage(plane, 0);
    std::vector<unsigned long long> vis(plane, MR_EMPTY_KEY);
    std::vector<uint32_t> wide_list;
    wide_list.reserve(nf);
    for (int64_t k = 0; k < nf; ++k) {                                                                                 // mr_face_kernel
        const int64_t f = backwards ? nf - 1 - k : k;
        MrFace t;
        const int what = mr_classify(faces.data(), f, nv, records.data(), view, t);
        ms_atomic_add(&counts[mr_count_word(what)], 1);
        if (what != MR_DRAW) continue;
        const int64_t pixels = mr_box_pixels(t);
        if (pixels > GP_MESH_RENDER_NARROW_MAX) {
            ms_atomic_add(&counts[GP_MESH_RENDER_WIDE], 1);
            wide_list.push_back((uint32_t)f);
        } else if (pixels > 0) {
            mr_draw_narrow(t, f, W, vis.data(), coverage.data());
        }
    }
    for (size_t e = 0; e < wide_list.size(); ++e)                                                                      // mr_wide_kernel
        for (int piece = GP_MESH_RENDER_SPLIT - 1; piece >= 0; --piece) {
            MrFace t;
            if (mr_classify(faces.data(), wide_list[e], nv, records.data(), view, t) != MR_DRAW) return 4;
            for (int lane = 0; lane < 64; ++lane) mr_draw_wide_lane(t, wide_list[e], piece, lane, W, vis.data(), coverage.data());
        }
    std::vector<int32_t> face(plane);
    std::vector<float> depth(plane), bary(3 * plane);
    std::vector<uint8_t> valid(plane);
    for (int64_t p = 0; p < plane; ++p)                                                                                // mr_resolve_kernel
        mr_resolve_pixel(vis.data(), faces.data(), nv, nf, records.data(), view, (int32_t)(p % W), (int32_t)(p / W), face.data(), depth.data(), valid.data(), bary.data());
    put(out, counts); put(out, coverage); put(out, face); put(out, depth); put(out, valid); put(out, bary);
    if (C >= 3) {
        std::vector<float> image(C * plane), normals(3 * plane), shaded(3 * plane);
        std::vector<uint8_t> nvalid(plane);
        for (int64_t p = 0; p < plane; ++p) {
            mr_interpolate_pixel(attributes.data(), C, faces.data(), nv, nf, records.data(), face.data(), valid.data(), bary.data(), &real[8], p, plane, image.data());
            float n[3];
            nvalid[p] = mr_normal_pixel(vertices.data(), faces.data(), nv, nf, m.data(), view, face.data(), depth.data(), valid.data(), (int32_t)(p % W), (int32_t)(p / W), n);
            for (int c = 0; c < 3; ++c) normals[c * plane + p] = n[c];
        }
        for (int64_t p = 0; p < plane; ++p)
            mr_shade_pixel(image.data(), normals.data(), nvalid.data(), depth.data(), view, real[3], &real[4], (int32_t)(p % W), (int32_t)(p / W), shaded.data());
        put(out, image); put(out, normals); put(out, nvalid); put(out, shaded);
    }
    fclose(out);
    fclose(fp);
    return 0;
}
