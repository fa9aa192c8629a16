// mesh_emulate.cpp -- the programs of gaussianprediction_amd/csrc/mesh_core.h on a CPU, element by element, in a stand-alone program
// (tests/test_mesh_host.py builds it under the sanitizers and runs it as a child).
//   mesh_emulate JOB OUT
// JOB begins with int32 op, nv, nf; everything is little-endian and packed; every array has exactly its stated size, so that an index
// the programs fail to check is an error of the sanitizers:
//   0 components  int32 faces[nf][3]  -> int32 state[4], vertex_label[nv], face_label[nf], labels[C], vertex_counts[C], face_counts[C]
//   1 filter      int32 C, min_triangles, keep_largest, k; int32 faces[nf][3], vertex_label[nv], labels[C], face_counts[C]; float rows[nv][k]
//                 -> int32 counts[3] (status, vertices, faces), vertex_index[], face_index[], faces_out[][3]; float rows_out[][k]
//   2 normals     float vertices[nv][3]; int32 faces[nf][3]  -> int32 status; float normals[nv][3]
// The rounds of op 0 are SYNCHRONOUS: every load of a hook or jump launch sees the array as the launch found it, every atomicMin and
// store lands in the live one -- the stalest a device can be; state[3] is the rounds that took.  The ranks are running sums over the
// elements in ascending order: what the tiles' offsets and the ballot ranks inside a tile add up to.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../gaussianprediction_amd/csrc/mesh_core.h"

template <typename T>
static void get(FILE* fp, std::vector<T>& v) {
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), fp) != v.size()) { fprintf(stderr, "short job file\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short write\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const std::vector<T>& v) { put(fp, v.data(), v.size()); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!fp || !out) return 2;
    std::vector<int32_t> head(3);
    get(fp, head);
    const int32_t op = head[0];
    const int64_t nv = head[1], nf = head[2];
    if (op < 0 || op > 2 || ms_refuse_sizes(nv, nf)) return 3;
    if (op == 0) {
        std::vector<int32_t> faces(3 * nf), parent(nv), face_label(nf), state(GP_MESH_STATE_WORDS, 0);
        get(fp, faces);
        std::iota(parent.begin(), parent.end(), 0);
        for (bool open = true; open;) {
            if (state[GP_MESH_ROUNDS] >= 100000) return 4;
            std::vector<int32_t> seen = parent;                                                                  // ms_hook_kernel
            for (int64_t f = 0; f < nf; ++f) ms_hook_face(seen.data(), parent.data(), faces.data(), f, nv, state.data());
            seen = parent;                                                                                       // ms_jump_kernel
            for (int64_t v = 0; v < nv; ++v) ms_jump(seen.data(), parent.data(), v);
            open = false;                                                                                        // ms_settle_kernel
            for (int64_t f = 0; f < nf; ++f) open = open || ms_unsettled_face(parent.data(), faces.data(), f, nv);
            for (int64_t v = 0; v < nv; ++v) open = open || ms_unsettled_vertex(parent.data(), v);
            state[GP_MESH_ROUNDS] += 1;
        }
        state[GP_MESH_CONVERGED] = 1;
        std::vector<int32_t> vcount(nv, 0), fcount(nv, 0), labels, vcounts, fcounts;
        for (int64_t v = 0; v < nv; ++v) ms_atomic_add(&vcount[parent[v]], 1);                                   // ms_count_kernel
        for (int64_t f = 0; f < nf; ++f) {
            face_label[f] = ms_face_label(parent.data(), faces.data(), f, nv, state.data());
            if (face_label[f] >= 0) ms_atomic_add(&fcount[face_label[f]], 1);
        }
        for (int64_t v = 0; v < nv; ++v)                                                                         // the compaction, ms_table_kernel
            if (parent[v] == v) { labels.push_back((int32_t)v); vcounts.push_back(vcount[v]); fcounts.push_back(fcount[v]); }
        state[GP_MESH_COUNT] = (int32_t)labels.size();
        put(out, state); put(out, parent); put(out, face_label); put(out, labels); put(out, vcounts); put(out, fcounts);
    } else if (op == 1) {
        std::vector<int32_t> more(4);
        get(fp, more);
        const int64_t C = more[0], k = more[3];
        const int32_t min_triangles = more[1], keep_largest = more[2];
        if (C < 0 || C > nv || k < 1) return 3;
        std::vector<int32_t> faces(3 * nf), vertex_label(nv), labels(C), face_counts(C), counts(3, 0);
        std::vector<float> rows(nv * k);
        get(fp, faces); get(fp, vertex_label); get(fp, labels); get(fp, face_counts); get(fp, rows);
        std::vector<uint32_t> order(C);
        std::iota(order.begin(), order.end(), 0u);
        if (keep_largest >= 0)                                                                                   // ms_count_key_kernel and the stable sort
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
                return 0x7fffffffu - (uint32_t)std::max(face_counts[a], 0) < 0x7fffffffu - (uint32_t)std::max(face_counts[b], 0);
            });
        std::vector<uint8_t> keep_label(nv, 0), keep_vertex(nv), keep_face(nf);
        for (int64_t pos = 0; pos < C; ++pos) {                                                                  // ms_keep_label_kernel
            const uint32_t c = order[pos];
            if (!ms_index_ok(labels[c], nv)) { counts[GP_MESH_STATUS] = 1; continue; }
            keep_label[labels[c]] = ms_keep_component(face_counts[c], min_triangles, keep_largest, pos);
        }
        for (int64_t v = 0; v < nv; ++v) keep_vertex[v] = ms_keep_vertex(keep_label.data(), vertex_label.data(), v, nv, counts.data());
        for (int64_t f = 0; f < nf; ++f) keep_face[f] = ms_keep_face(keep_vertex.data(), faces.data(), f, nv, counts.data());
        std::vector<uint32_t> rank_vertex(nv), rank_face(nf);
        uint32_t kept_v = 0, kept_f = 0;
        for (int64_t v = 0; v < nv; ++v) { rank_vertex[v] = kept_v; kept_v += keep_vertex[v] != 0; }
        for (int64_t f = 0; f < nf; ++f) { rank_face[f] = kept_f; kept_f += keep_face[f] != 0; }
        counts[1] = (int32_t)kept_v; counts[2] = (int32_t)kept_f;
        std::vector<int32_t> vertex_index(kept_v), face_index(kept_f), faces_out(3 * (size_t)kept_f);
        std::vector<float> rows_out((size_t)kept_v * k);
        for (int64_t v = 0; v < nv; ++v) {                                                                       // ms_apply_vertex_kernel, ms_gather_kernel
            if (!keep_vertex[v]) continue;
            vertex_index[rank_vertex[v]] = (int32_t)v;
            for (int64_t j = 0; j < k; ++j) rows_out[rank_vertex[v] * k + j] = rows[v * k + j];
        }
        for (int64_t f = 0; f < nf; ++f) {                                                                       // ms_apply_face_kernel
            if (!keep_face[f]) continue;
            face_index[rank_face[f]] = (int32_t)f;
            ms_remap_face(faces.data(), f, rank_vertex.data(), &faces_out[3 * (size_t)rank_face[f]]);
        }
        put(out, counts); put(out, vertex_index); put(out, face_index); put(out, faces_out); put(out, rows_out);
    } else {
        std::vector<float> vertices(3 * nv), face_vectors(3 * nf), normals(3 * nv);
        std::vector<int32_t> faces(3 * nf), state(GP_MESH_STATE_WORDS, 0);
        get(fp, vertices); get(fp, faces);
        for (int64_t f = 0; f < nf; ++f) (void)ms_face_vector(vertices.data(), faces.data(), f, nv, &face_vectors[3 * f], state.data());
        std::vector<uint32_t> keys(3 * nf), incidences(3 * nf), begin(nv, 0), end(nv, 0);
        for (int64_t i = 0; i < 3 * nf; ++i) keys[i] = ms_incidence_key(faces.data(), i, nv);
        std::iota(incidences.begin(), incidences.end(), 0u);
        std::stable_sort(incidences.begin(), incidences.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
        for (int64_t i = 0; i < 3 * nf; ++i) {                                                                   // ms_bounds_kernel
            const uint32_t key = keys[incidences[i]];
            if (key >= (uint32_t)nv) continue;
            if (i == 0 || keys[incidences[i - 1]] != key) begin[key] = (uint32_t)i;
            if (i == 3 * nf - 1 || keys[incidences[i + 1]] != key) end[key] = (uint32_t)i + 1;
        }
        for (int64_t v = 0; v < nv; ++v) ms_vertex_normal(face_vectors.data(), incidences.data(), begin[v], end[v], &normals[3 * v]);
        put(out, state.data(), 1); put(out, normals);
    }
    fclose(out);
    fclose(fp);
    return 0;
}
