// surface_emulate.cpp -- the programs of gaussianprediction_amd/csrc/surface_core.h on a CPU, element by element, in a stand-alone
// program (tests/test_surface_host.py builds it under the sanitizers and runs it as a child).
//   surface_emulate JOB OUT
// JOB (everything little-endian and packed; every array has exactly its stated size, so that an index the programs fail to check is
// an error of the sanitizers):
//   int32 nv, nf, nq, wide_cells, backwards, short_by, 0, 0; float cell, 0; float vertices[nv][3]; int32 faces[nf][3]; float queries[nq][3]
//   -> float dist2[nq]; int32 face[nq]; int32 region[nq]; float closest[nq][3]; float bary[nq][2]; int64 stats[12]; int32 dims[3], cells
//   backwards: the faces enter their cells and the wide list in descending order -- no result may depend on the order inside either
//   short_by:  the pair array is that many entries smaller than the pairs (> 0: the fill is refused and writes nothing)
// Exit 3: a refusal (its words on stderr).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../gaussianprediction_amd/csrc/surface_core.h"

template <typename T>
static void get(FILE* fp, std::vector<T>& v) {
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), fp) != v.size()) { fprintf(stderr, "short job file\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const std::vector<T>& v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), fp) != v.size()) { fprintf(stderr, "short write\n"); exit(2); }
}
static int refuse(const char* why) { fprintf(stderr, "%s\n", why); return 3; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!fp || !out) return 2;
    std::vector<int32_t> head(8);
    std::vector<float> real(2);
    get(fp, head); get(fp, real);
    const int64_t nv = head[0], nf = head[1], nq = head[2];
    const int32_t wide_cells = head[3];
    const bool backwards = head[4] != 0;
    const int64_t short_by = head[5];
    const float cell = real[0];
    const char* why = gm_refuse_mesh(nv, nf);
    if (!why) why = sf_refuse_grid(nf, cell);
    if (!why) why = sf_refuse_wide(wide_cells);
    if (!why) why = gm_refuse_count(nq);
    if (why) return refuse(why);
    std::vector<float> vertices(3 * nv), queries(3 * nq);
    std::vector<int32_t> faces(3 * nf);
    get(fp, vertices); get(fp, faces); get(fp, queries);

    std::vector<SfFace> records(nf);
    uint32_t words[SF_WORDS] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (int64_t f = 0; f < nf; ++f) {                                                           // sf_prepare_kernel
        if (!sf_record(vertices.data(), faces.data(), f, nv, &records[f])) continue;
        const SfFace& r = records[f];
        for (int a = 0; a < 3; ++a) {
            const uint32_t o[3] = {gm_ordered(r.a[a] + 0.f), gm_ordered(r.b[a] + 0.f), gm_ordered(r.c[a] + 0.f)};
            for (int k = 0; k < 3; ++k) {
                if (o[k] < words[a]) words[a] = o[k];
                if (o[k] > words[3 + a]) words[3 + a] = o[k];
            }
        }
        ++words[SF_WORD_USABLE];
    }
    GmGrid g;
    sf_derive(words, words[SF_WORD_USABLE], nf, cell, &g);                                       // sf_derive_kernel
    if (g.cells > sf_cell_capacity(nf, cell)) return 4;
    std::vector<uint32_t> start(g.cells + 1, 0);
    for (int64_t f = 0; f < nf; ++f) {                                                           // sf_count_kernel
        if (records[f].face < 0) continue;
        int32_t lo[3], hi[3];
        sf_box(g, records[f], lo, hi);
        if (sf_box_cells(lo, hi) > wide_cells) { ++words[SF_WORD_WIDE]; continue; }
        for (int32_t z = lo[2]; z <= hi[2]; ++z)
            for (int32_t y = lo[1]; y <= hi[1]; ++y)
                for (int32_t x = lo[0]; x <= hi[0]; ++x) ++start[sf_key(g, x, y, z)];
    }
    uint32_t run = 0;
    for (int64_t k = 0; k <= g.cells; ++k) { const uint32_t c = start[k]; start[k] = run; run += c; }      // the scan
    words[SF_WORD_PAIRS] = run;                                                                  // sf_sizes_kernel
    const int64_t capacity = (int64_t)run - short_by;
    if (capacity < 0) return refuse("short_by exceeds the pairs");
    words[SF_WORD_STATUS] = (int64_t)run > capacity ? GP_SURFACE_REFUSED_CAPACITY : 0;           // sf_status_kernel
    std::vector<int32_t> pairs(capacity), wide(words[SF_WORD_WIDE]);
    std::vector<uint32_t> cursor(start);
    uint32_t nwide = 0;
    for (int64_t k = 0; k < nf; ++k) {                                                           // the wide list; sf_fill_kernel
        const int64_t f = backwards ? nf - 1 - k : k;
        if (records[f].face < 0) continue;
        int32_t lo[3], hi[3];
        sf_box(g, records[f], lo, hi);
        if (sf_box_cells(lo, hi) > wide_cells) { wide[nwide++] = (int32_t)f; continue; }
        if (words[SF_WORD_STATUS] != 0) continue;
        for (int32_t z = lo[2]; z <= hi[2]; ++z)
            for (int32_t y = lo[1]; y <= hi[1]; ++y)
                for (int32_t x = lo[0]; x <= hi[0]; ++x) pairs[cursor[sf_key(g, x, y, z)]++] = (int32_t)f;
    }
    std::vector<float> dist2(nq), closest(3 * nq), bary(2 * nq);
    std::vector<int32_t> face(nq), region(nq);
    std::vector<int64_t> stats(GP_SURFACE_STAT_WORDS, 0);
    for (int64_t i = 0; i < nq; ++i) {                                                           // sf_query_kernel
        uint64_t seen;
        int32_t ring, swept;
        sf_query(g, nf, words[SF_WORD_STATUS] != 0, start.data(), pairs.data(), records.data(), wide.data(), nwide, &queries[3 * i], &dist2[i], &face[i], &region[i],
                 &closest[3 * i], &bary[2 * i], &seen, &ring, &swept);
        stats[GP_SURFACE_CANDIDATES] += (int64_t)seen;
        if (ring > stats[GP_SURFACE_MAX_RING]) stats[GP_SURFACE_MAX_RING] = ring;
        stats[GP_SURFACE_SWEPT] += swept;
        if (!gm_usable(&queries[3 * i])) ++stats[GP_SURFACE_EXCLUDED_QUERIES];
    }
    stats[GP_SURFACE_EXCLUDED_FACES] = g.excluded;
    for (int a = 0; a < 3; ++a) stats[GP_SURFACE_DIM_X + a] = g.dims[a];
    stats[GP_SURFACE_PAIRS] = words[SF_WORD_PAIRS];
    stats[GP_SURFACE_WIDE] = words[SF_WORD_WIDE];
    stats[GP_SURFACE_STATUS] = words[SF_WORD_STATUS];
    std::vector<int32_t> dims = {g.dims[0], g.dims[1], g.dims[2], g.cells};
    put(out, dist2); put(out, face); put(out, region); put(out, closest); put(out, bary); put(out, stats); put(out, dims);
    fclose(out);
    fclose(fp);
    return 0;
}
