// mesh_smooth_emulate.cpp -- the programs of gaussianprediction_amd/csrc/mesh_smooth_core.h on a CPU, element by element, in a
// stand-alone program (tests/test_mesh_smooth_host.py builds it under the sanitizers and runs it as a child).
//   mesh_smooth_emulate JOB OUT
// JOB: int32 nv, nf, k, method, boundary, iterations; double lambda_, mu; int32 faces[nf][3]; float rows[nv][k] (k = 0: none).
// Everything is little-endian and packed; every array has exactly its stated size, so that an index the programs fail to check is an
// error of the sanitizers.
// OUT: int32 counts[8], edge[E][2], face_count[E], wind[E], offsets[nv + 1], neighbors[2E]; uint8 vertex_flags[nv]; int32 pinned;
//      float smoothed[nv][k], umbrella[nv][k]
// The sort is std::stable_sort a word at a time, the second end first, as the device's passes; the ranks are running sums over the
// elements in ascending order: what the tiles' offsets and the ballot ranks inside a tile add up to.  Exit 3: a refusal (its words on
// stderr).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../gaussianprediction_amd/csrc/mesh_smooth_core.h"

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

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!fp || !out) return 2;
    std::vector<int32_t> head(6);
    std::vector<double> real(2);
    get(fp, head); get(fp, real);
    const int64_t nv = head[0], nf = head[1], k = head[2];
    const int32_t method = head[3], boundary = head[4], iterations = head[5];
    const char* why = mt_refuse_sizes(nv, nf);
    if (!why && k != 0) why = mt_refuse_rows(nv, k);
    if (!why) why = mt_refuse_options(method, boundary, iterations, real[0], real[1]);
    if (why) { fprintf(stderr, "%s\n", why); return 3; }
    std::vector<int32_t> faces(3 * nf), counts(GP_MESH_SMOOTH_COUNT_WORDS, 0), words(8, 0);
    std::vector<float> rows(nv * k);
    get(fp, faces); get(fp, rows);
    const int64_t n6 = 6 * nf;
    for (int64_t f = 0; f < nf; ++f) {                                                                               // mt_tally_kernel
        int32_t degenerate;
        if (mt_face_tally(faces.data(), f, nv, counts.data(), &degenerate)) ms_atomic_add(&counts[GP_MESH_SMOOTH_FACES], 1);
        ms_atomic_add(&counts[GP_MESH_SMOOTH_DEGENERATE], degenerate);
    }
    std::vector<uint32_t> order, key(n6), element(n6);
    for (int word = 1; word >= 0; --word) {                                                                         // mt_sort_word_kernel and the sort
        for (int64_t i = 0; i < n6; ++i) key[i] = mt_sort_word(faces.data(), order.empty() ? nullptr : order.data(), i, word, nv, &element[i]);
        std::vector<uint32_t> at(n6);
        std::iota(at.begin(), at.end(), 0u);
        std::stable_sort(at.begin(), at.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
        order.resize(n6);
        for (int64_t i = 0; i < n6; ++i) order[i] = element[at[i]];
    }
    std::vector<uint32_t> first(n6), second(n6);
    for (int64_t i = 0; i < n6; ++i) {                                                                              // mt_gather_kernel
        mt_entry(faces.data(), order[i], nv, &first[i], &second[i]);
        second[i] |= (order[i] & 1u) ? MT_DIRECTION : 0u;
    }
    std::vector<uint8_t> head_adj(n6), head_edge(n6), mark_boundary(nv, 0), mark_nonmanifold(nv, 0);
    for (int64_t i = 0; i < n6; ++i) {                                                                              // mt_head_kernel
        const bool h = mt_is_head(first.data(), second.data(), i, nv);
        const uint32_t lo = first[i], hi = mt_end(second[i]);
        head_adj[i] = h;
        head_edge[i] = h && lo < hi;
        if (mt_starts_vertex(first.data(), i, nv)) ms_atomic_add(&counts[GP_MESH_SMOOTH_VERTICES], 1);
        if (!head_edge[i]) continue;
        int32_t c, w;
        mt_run(first.data(), second.data(), i, n6, &c, &w);
        if (mt_is_boundary(c)) { ms_atomic_add(&counts[GP_MESH_SMOOTH_BOUNDARY], 1); mark_boundary.at(lo) = 1; mark_boundary.at(hi) = 1; }
        if (mt_is_nonmanifold(c)) { ms_atomic_add(&counts[GP_MESH_SMOOTH_NONMANIFOLD], 1); mark_nonmanifold.at(lo) = 1; mark_nonmanifold.at(hi) = 1; }
        if (mt_is_inconsistent(c, w)) ms_atomic_add(&counts[GP_MESH_SMOOTH_INCONSISTENT], 1);
    }
    const std::vector<uint32_t> rank_adj = ranks(head_adj, &words[MT_WORD_ADJ]), rank_edge = ranks(head_edge, &counts[GP_MESH_SMOOTH_EDGES]);
    const int64_t ne = counts[GP_MESH_SMOOTH_EDGES];
    if (words[MT_WORD_ADJ] != 2 * ne) return 4;
    std::vector<int32_t> edge(2 * ne), face_count(ne), wind(ne), offsets(nv + 1), neighbors(2 * ne);
    std::vector<uint32_t> adj_src(2 * ne);
    std::vector<uint8_t> flags(nv);
    for (int64_t i = 0; i < n6; ++i) {                                                                              // mt_apply_kernel
        if (!head_adj[i]) continue;
        adj_src.at(rank_adj[i]) = first[i];
        neighbors.at(rank_adj[i]) = (int32_t)mt_end(second[i]);
        if (!head_edge[i]) continue;
        const size_t e = rank_edge[i];
        edge.at(2 * e) = (int32_t)first[i];
        edge.at(2 * e + 1) = (int32_t)mt_end(second[i]);
        mt_run(first.data(), second.data(), i, n6, &face_count.at(e), &wind.at(e));
    }
    for (int64_t v = 0; v <= nv; ++v) {                                                                             // mt_vertex_kernel
        const int64_t begin = mt_lower_bound(adj_src.data(), 2 * ne, v);
        offsets[v] = (int32_t)begin;
        if (v < nv) flags[v] = mt_flags(mark_boundary[v], mark_nonmanifold[v], mt_lower_bound(adj_src.data(), 2 * ne, v + 1) - begin);
    }
    const uint8_t mask = boundary == GP_MESH_SMOOTH_FIXED ? (GP_MESH_SMOOTH_FLAG_BOUNDARY | GP_MESH_SMOOTH_FLAG_NONMANIFOLD) : 0;
    std::vector<int32_t> pinned(1, 0);
    for (int64_t v = 0; v < nv; ++v) pinned[0] += mt_is_pinned(flags.data(), mask, v);                                 // mt_pinned_kernel
    // gp_mesh_smooth_steps: ping-pong between two buffers, the last step into the output; the input is const
    const std::vector<float>& src = rows;
    std::vector<float> smoothed(nv * k), umbrella(nv * k), buf[2] = {std::vector<float>(nv * k), std::vector<float>(nv * k)};
    const int64_t steps = mt_steps(method, iterations);
    if (steps == 0) smoothed = src;
    const float* from = src.data();
    for (int64_t step = 0; step < steps; ++step) {
        float* to = step + 1 == steps ? smoothed.data() : buf[step & 1].data();
        for (int64_t i = 0; i < nv * k; ++i)                                                                        // mt_step_kernel
            mt_step(from, nv, k, i / k, i % k, offsets.data(), neighbors.data(), 2 * ne, flags.data(), mask, mt_factor(method, step, real[0], real[1]), to);
        from = to;
    }
    for (int64_t i = 0; i < nv * k; ++i) mt_umbrella(src.data(), nv, k, i / k, i % k, offsets.data(), neighbors.data(), 2 * ne, umbrella.data());      // mt_umbrella_kernel
    put(out, counts); put(out, edge); put(out, face_count); put(out, wind); put(out, offsets); put(out, neighbors); put(out, flags); put(out, pinned);
    put(out, smoothed); put(out, umbrella);
    fclose(out);
    fclose(fp);
    return 0;
}
