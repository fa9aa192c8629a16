// mesh_simplify_emulate.cpp -- the programs of gaussianprediction_amd/csrc/mesh_simplify_core.h on a CPU, element by element, in a
// stand-alone program (tests/test_mesh_simplify_host.py builds it under the sanitizers and runs it as a child).
//   mesh_simplify_emulate JOB OUT
// JOB begins with int32 op, nv, nf; everything is little-endian and packed; every array has exactly its stated size, so that an index
// the programs fail to check is an error of the sanitizers:
//   0 bounds    float vertices[nv][3]  -> double record[8]
//   1 simplify  int32 mode, contraction, drop_zero_area, drop_duplicates, keep_unreferenced, k; double voxel_size, bounds[6];
//               float vertices[nv][3]; int32 faces[nf][3]; float rows[nv][k]
//               -> int32 counts[8]; float vertices_out[nv'][3]; int32 faces_out[nf'][3], vertex_map[nv], face_index[nf'],
//                  vertex_counts[nv']; float rows_out[nv'][k]
// The sorts are std::stable_sort a word at a time, least significant first, as the device's passes; the ranks are running sums over
// the elements in ascending order: what the tiles' offsets and the ballot ranks inside a tile add up to.  Exit 3: a refusal (its
// words on stderr).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../gaussianprediction_amd/csrc/mesh_simplify_core.h"

template <typename T>
static void get(FILE* fp, std::vector<T>& v) {
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), fp) != v.size()) { fprintf(stderr, "short job file\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const std::vector<T>& v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), fp) != v.size()) { fprintf(stderr, "short write\n"); exit(2); }
}

static std::vector<uint32_t> ranks(const std::vector<uint8_t>& keep, int32_t* total) {
    std::vector<uint32_t> rank(keep.size());
    uint32_t kept = 0;
    for (size_t e = 0; e < keep.size(); ++e) { rank[e] = kept; kept += keep[e] != 0; }
    *total = (int32_t)kept;
    return rank;
}

// mz_sort3: three stable passes, word 2 first
static std::vector<uint32_t> sort3(const uint32_t* keys, int64_t n) {
    std::vector<uint32_t> order, k(n), e(n);
    for (int word = 2; word >= 0; --word) {
        for (int64_t i = 0; i < n; ++i) k[i] = mz_sort_word(keys, order.empty() ? nullptr : order.data(), i, word, &e[i]);
        std::vector<uint32_t> at(n);
        std::iota(at.begin(), at.end(), 0u);
        std::stable_sort(at.begin(), at.end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
        order.resize(n);
        for (int64_t i = 0; i < n; ++i) order[i] = e[at[i]];
    }
    return order;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!fp || !out) return 2;
    std::vector<int32_t> head(3);
    get(fp, head);
    const int32_t op = head[0];
    const int64_t nv = head[1], nf = head[2];
    if (op < 0 || op > 1 || ms_refuse_sizes(nv, nf)) return 3;
    if (op == 0) {
        std::vector<float> vertices(3 * nv), acc(MZ_BOUNDS_WORDS);
        std::vector<double> record(GP_MESH_SIMPLIFY_RECORD_WORDS);
        get(fp, vertices);
        // mz_bounds_partial_kernel: partial results over strided vertices, then merged
        std::vector<std::vector<float>> partial(7, std::vector<float>(MZ_BOUNDS_WORDS));
        for (size_t b = 0; b < partial.size(); ++b) {
            mz_bounds_start(partial[b].data());
            for (int64_t v = (int64_t)b; v < nv; v += (int64_t)partial.size()) mz_bounds_fold(partial[b].data(), &vertices[3 * v]);
        }
        mz_bounds_start(acc.data());
        for (const auto& p : partial) mz_bounds_merge(acc.data(), p.data());
        mz_bounds_record(acc.data(), record.data());
        put(out, record);
    } else {
        std::vector<int32_t> more(6);
        std::vector<double> real(7);
        get(fp, more); get(fp, real);
        const int32_t mode = more[0], drop_zero_area = more[2], drop_duplicates = more[3], keep_unreferenced = more[4];
        int32_t contraction = more[1];
        const int64_t k = more[5];
        if (k < 0) return 3;
        MzGrid grid;
        const char* why = mz_plan_grid(grid, mode, real[0], real.data() + 1);
        if (why) { fprintf(stderr, "%s\n", why); return 3; }
        if (mode == GP_MESH_SIMPLIFY_WELD) contraction = GP_MESH_SIMPLIFY_FIRST;
        std::vector<float> vertices(3 * nv), rows(nv * k);
        std::vector<int32_t> faces(3 * nf), counts(GP_MESH_SIMPLIFY_COUNT_WORDS, 0), words(8, 0);
        get(fp, vertices); get(fp, faces); get(fp, rows);
        std::vector<uint32_t> keys(3 * nv);
        for (int64_t v = 0; v < nv; ++v) mz_key(grid, &vertices[3 * v], &keys[3 * v], counts.data());                         // mz_key_kernel
        const std::vector<uint32_t> order = sort3(keys.data(), nv);
        std::vector<uint32_t> members(nv);
        std::vector<uint8_t> head_pos(nv), head_vertex(nv);
        for (int64_t i = 0; i < nv; ++i) {                                                                               // mz_head_kernel
            members[i] = order[i];
            head_pos[i] = mz_is_head(keys.data(), order.data(), i);
            head_vertex[order[i]] = head_pos[i];
        }
        const std::vector<uint32_t> rank_pos = ranks(head_pos, &words[MZ_WORD_SPARE]), rank_vertex = ranks(head_vertex, &words[MZ_WORD_CLUSTERS]);
        const int64_t C = words[MZ_WORD_CLUSTERS];
        counts[GP_MESH_SIMPLIFY_CLUSTERS] = (int32_t)C;
        std::vector<uint32_t> seg_begin(words[MZ_WORD_SPARE]), begin(C), end(C);
        std::vector<int32_t> seg_cluster(words[MZ_WORD_SPARE]), cluster(nv);
        for (int64_t i = 0; i < nv; ++i) {                                                                               // mz_segment_kernel
            if (!head_pos[i]) continue;
            const uint32_t s = mz_segment(rank_pos[i], true);
            seg_begin.at(s) = (uint32_t)i;
            seg_cluster.at(s) = (int32_t)rank_vertex[members[i]];
        }
        for (int64_t i = 0; i < nv; ++i) {                                                                               // mz_cluster_kernel
            const bool h = head_pos[i] != 0;
            const uint32_t s = mz_segment(rank_pos[i], h), segments = (uint32_t)words[MZ_WORD_SPARE];
            if (s >= segments) return 4;
            const int32_t c = seg_cluster[s];
            cluster[members[i]] = c;
            if (h) { begin.at(c) = (uint32_t)i; end.at(c) = s + 1 < segments ? seg_begin[s + 1] : (uint32_t)nv; }
        }
        std::vector<float> positions(3 * C);
        for (int64_t i = 0; i < 3 * C; ++i) mz_contract(vertices.data(), 3, i % 3, members.data(), begin[i / 3], end[i / 3], contraction, &positions[i]);      // mz_contract_kernel
        std::vector<uint8_t> keep_cluster(C, keep_unreferenced ? 1 : 0), keep_face(nf);
        std::vector<int32_t> rot(3 * nf);
        for (int64_t f = 0; f < nf; ++f) {                                                                               // mz_face_kernel
            const int what = mz_face_class(faces.data(), f, nv, cluster.data(), positions.data(), drop_zero_area, &rot[3 * f], counts.data());
            keep_face[f] = what == MZ_KEPT;
            if (what == MZ_COLLAPSED) ms_atomic_add(&counts[GP_MESH_SIMPLIFY_COLLAPSED], 1);
            if (what == MZ_ZERO_AREA) ms_atomic_add(&counts[GP_MESH_SIMPLIFY_ZERO_AREA], 1);
        }
        if (drop_duplicates) {
            const std::vector<uint32_t> by_triple = sort3((const uint32_t*)rot.data(), nf);
            for (int64_t i = 0; i < nf; ++i)                                                                             // mz_duplicate_kernel
                if (mz_is_duplicate((const uint32_t*)rot.data(), by_triple.data(), i, nv)) {
                    keep_face[by_triple[i]] = 0;
                    ms_atomic_add(&counts[GP_MESH_SIMPLIFY_DUPLICATES], 1);
                }
        }
        if (!keep_unreferenced)
            for (int64_t f = 0; f < nf; ++f)                                                                             // mz_mark_kernel
                if (keep_face[f])
                    for (int c = 0; c < 3; ++c) keep_cluster.at(cluster[faces[3 * f + c]]) = 1;
        const std::vector<uint32_t> rank_cluster = ranks(keep_cluster, &counts[GP_MESH_SIMPLIFY_VERTICES]), rank_face = ranks(keep_face, &counts[GP_MESH_SIMPLIFY_FACES]);
        const int64_t nv2 = counts[GP_MESH_SIMPLIFY_VERTICES], nf2 = counts[GP_MESH_SIMPLIFY_FACES];
        std::vector<float> vertices_out(3 * nv2), rows_out(nv2 * k);
        std::vector<int32_t> faces_out(3 * nf2), vertex_map(nv), face_index(nf2), vertex_counts(nv2);
        for (int64_t v = 0; v < nv; ++v) vertex_map[v] = keep_cluster[cluster[v]] ? (int32_t)rank_cluster[cluster[v]] : -1;      // mz_apply_vertex_kernel
        for (int64_t c = 0; c < C; ++c) {
            if (!keep_cluster[c]) continue;
            const size_t r = rank_cluster[c];
            for (int a = 0; a < 3; ++a) vertices_out.at(3 * r + a) = positions[3 * c + a];
            vertex_counts.at(r) = (int32_t)(end[c] - begin[c]);
            for (int64_t j = 0; j < k; ++j) mz_contract(rows.data(), k, j, members.data(), begin[c], end[c], contraction, &rows_out.at(r * k + j));      // mz_rows_kernel
        }
        for (int64_t f = 0; f < nf; ++f) {                                                                               // mz_apply_face_kernel
            if (!keep_face[f]) continue;
            const size_t r = rank_face[f];
            face_index.at(r) = (int32_t)f;
            for (int c = 0; c < 3; ++c) faces_out.at(3 * r + c) = (int32_t)rank_cluster[cluster[faces[3 * f + c]]];
        }
        put(out, counts); put(out, vertices_out); put(out, faces_out); put(out, vertex_map); put(out, face_index); put(out, vertex_counts); put(out, rows_out);
    }
    fclose(out);
    fclose(fp);
    return 0;
}
