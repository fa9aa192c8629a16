// volume_emulate.cpp -- the programs of gaussianprediction_amd/csrc/volume_core.h on a CPU, element by element, in a stand-alone
// program (tests/test_volume_host.py builds it under the sanitizers and runs it as a child).
//   volume_emulate JOB OUT
// JOB (everything little-endian and packed; every array has exactly its stated size, so that an index the programs fail to check is
// an error of the sanitizers):
//   int32 nv, nf, ne, nq, leaf, nx, ny, nz, ncmp, 0, 0, 0; float ox, oy, oz, voxel;
//   float vertices[nv][3]; int32 faces[nf][3]; float queries[nq][3];
//   int32 face_edges[nf][3]; double edge_normal[ne][3]; double vertex_normal[nv][3]      (gp_sdf_tables' outputs for the mesh; read by the lattice only)
//   float a[ncmp]; float b[ncmp]
//   -> float dist2[nq]; int32 face[nq]; int32 region[nq]; float closest[nq][3]; float bary[nq][2]; int64 stats[8];
//      float sdf[nz][ny][nx]; int64 lattice_stats[16]        (only where nx > 0)
//      int64 counts[6]
//   nx = ny = nz = 0: no lattice.  leaf: the records of a leaf (the library's is GP_VOLUME_LEAF; no result may depend on it).
// Exit 3: a refusal (its words on stderr).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../gaussianprediction_amd/csrc/volume_core.h"

template <typename T>
static void get(FILE* fp, std::vector<T>& v) {
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), fp) != v.size()) { fprintf(stderr, "short job file\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const std::vector<T>& v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), fp) != v.size()) { fprintf(stderr, "short write\n"); exit(2); }
}
static int refuse(const char* why) { fprintf(stderr, "%s\n", why); return 3; }

static void add(std::vector<int64_t>& stats, const VlTally& t, bool bad) {
    stats[GP_VOLUME_NODES] += (int64_t)t.nodes;
    stats[GP_VOLUME_CANDIDATES] += (int64_t)t.candidates;
    if (t.stack > stats[GP_VOLUME_MAX_STACK]) stats[GP_VOLUME_MAX_STACK] = t.stack;
    if (t.overflow) stats[GP_VOLUME_STATUS] = 1;
    if (bad) ++stats[GP_VOLUME_EXCLUDED_QUERIES];
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!fp || !out) return 2;
    std::vector<int32_t> head(12);
    std::vector<float> real(4);
    get(fp, head); get(fp, real);
    const int64_t nv = head[0], nf = head[1], ne = head[2], nq = head[3], leaf = head[4], nx = head[5], ny = head[6], nz = head[7], ncmp = head[8];
    const bool lattice = nx != 0 || ny != 0 || nz != 0;
    const char* why = sd_refuse_tables(nv, nf, ne);
    if (!why) why = gm_refuse_count(nq);
    if (!why) why = gm_refuse_count(ncmp);
    if (!why && (leaf < 1 || leaf > 64)) why = "leaf must be 1 .. 64";
    if (!why && lattice) why = vl_refuse_lattice(real[0], real[1], real[2], real[3], nx, ny, nz);
    if (why) return refuse(why);
    std::vector<float> vertices(3 * nv), queries(3 * nq), a(ncmp), b(ncmp);
    std::vector<int32_t> faces(3 * nf), face_edges(3 * nf);
    std::vector<double> edge_normal(3 * ne), vertex_normal(3 * nv);
    get(fp, vertices); get(fp, faces); get(fp, queries); get(fp, face_edges); get(fp, edge_normal); get(fp, vertex_normal); get(fp, a); get(fp, b);

    // gp_volume_tree
    std::vector<SfFace> records(nf), sorted(nf);
    uint32_t words[VL_WORDS] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (int64_t f = 0; f < nf; ++f) {                                                           // vl_prepare_kernel
        if (!sf_record(vertices.data(), faces.data(), f, nv, &records[f])) continue;
        const SfFace& r = records[f];
        for (int k = 0; k < 3; ++k) {
            const float c[3] = {r.a[k] + 0.f, r.b[k] + 0.f, r.c[k] + 0.f};
            for (int j = 0; j < 3; ++j) {
                const uint32_t o = gm_ordered(c[j]);
                uint32_t bits;
                const float m = fabsf(c[j]);
                memcpy(&bits, &m, 4);
                if (o < words[k]) words[k] = o;
                if (o > words[3 + k]) words[3 + k] = o;
                if (bits > words[VL_WORD_M]) words[VL_WORD_M] = bits;
            }
        }
        ++words[VL_WORD_USABLE];
    }
    std::vector<uint32_t> keys(nf), order(nf);
    for (int64_t f = 0; f < nf; ++f) keys[f] = vl_key(records[f], words);                        // vl_key_kernel
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });      // the stable radix sort
    for (int64_t i = 0; i < nf; ++i) sorted[i] = records[order[i]];                              // vl_gather_kernel
    const VlTree t = vl_tree(nf, leaf);
    std::vector<VlBox> boxes(t.boxes);
    for (uint32_t i = 0; i < t.count[0]; ++i) vl_leaf_box(sorted.data(), t, i, &boxes[t.offset[0] + i]);      // vl_leaf_kernel
    for (uint32_t level = 1; level < t.levels; ++level)                                                       // vl_level_kernel
        for (uint32_t i = 0; i < t.count[level]; ++i) vl_union(boxes.data(), t, level, i, &boxes[t.offset[level] + i]);
    const uint32_t usable = words[VL_WORD_USABLE];
    float M;
    memcpy(&M, &words[VL_WORD_M], 4);

    const auto finish = [&](std::vector<int64_t>& stats) {
        stats[GP_VOLUME_EXCLUDED_FACES] = nf - usable;
        stats[GP_VOLUME_LEVELS] = t.levels;
        stats[GP_VOLUME_LEAVES] = t.count[0];
    };
    std::vector<float> dist2(nq), closest(3 * nq), bary(2 * nq);
    std::vector<int32_t> face(nq), region(nq);
    std::vector<int64_t> stats(GP_VOLUME_STAT_WORDS, 0);
    for (int64_t i = 0; i < nq; ++i) {                                                           // vl_query_kernel
        VlTally tally;
        vl_query(t, boxes.data(), sorted.data(), usable, M, &queries[3 * i], &dist2[i], &face[i], &region[i], &closest[3 * i], &bary[2 * i], &tally);
        add(stats, tally, !gm_usable(&queries[3 * i]));
    }
    finish(stats);
    put(out, dist2); put(out, face); put(out, region); put(out, closest); put(out, bary); put(out, stats);

    if (lattice) {                                                                               // vl_lattice_kernel
        const int64_t n = nx * ny * nz;
        std::vector<float> sdf(n);
        std::vector<int64_t> ls(GP_VOLUME_LATTICE_WORDS, 0);
        for (int64_t i = 0; i < n; ++i) {
            float p[3];
            int8_t sg;
            int32_t kind;
            VlTally tally;
            vl_point(i, (int32_t)nx, (int32_t)ny, real[0], real[1], real[2], real[3], p);
            const int row = vl_lattice_point(t, boxes.data(), sorted.data(), usable, M, p, vertices.data(), faces.data(), nv, nf, face_edges.data(), edge_normal.data(), ne,
                                             vertex_normal.data(), &sdf[i], &sg, &kind, &tally);
            add(ls, tally, !gm_usable(p));
            int64_t* s = ls.data() + GP_VOLUME_STAT_WORDS;
            if (row == SD_ROW_EXCLUDED) ++s[GP_SDF_EXCLUDED];
            if (row == SD_ROW_FOREIGN) { ++s[GP_SDF_UNDETERMINED]; s[GP_SDF_STATUS] = 1; }
            if (row == SD_ROW_SIGNED) {
                ++s[GP_SDF_FACE + kind];
                ++s[sg < 0 ? GP_SDF_INSIDE : (sg > 0 ? GP_SDF_OUTSIDE : GP_SDF_UNDETERMINED)];
            }
        }
        finish(ls);
        put(out, sdf); put(out, ls);
    }

    std::vector<int64_t> counts(GP_VOLUME_COUNT_WORDS, 0);                                       // vl_compare_kernel
    for (int64_t i = 0; i < ncmp; ++i) {
        const uint32_t bits = vl_compare(a[i], b[i]);
        for (int w = 0; w < GP_VOLUME_POINTS; ++w) counts[w] += (bits >> w) & 1u;
    }
    counts[GP_VOLUME_POINTS] = ncmp;
    put(out, counts);
    fclose(out);
    fclose(fp);
    return 0;
}
