// geometry_emulate.cpp -- the programs of gaussianprediction_amd/csrc/geometry_core.h on a CPU, element by element, in a stand-alone
// program (tests/test_geometry_host.py builds it under the sanitizers and runs it as a child).
//   geometry_emulate JOB OUT
// JOB: int32 mode, then per mode (everything little-endian and packed; every array has exactly its stated size, so that an index the
// programs fail to check is an error of the sanitizers):
//   0 samples   int32 nv, nf, n, C, 0, 0, 0; uint64 seed; float vertices[nv][3]; int32 faces[nf][3]; float attributes[nv][C]
//               -> int32 counts[8]; float points[n][3]; int32 face[n]; float bary[n][2]; float interpolated[n][C]
//   1 nearest   int32 np, nq, backwards, 0, 0, 0, 0; float cell, 0; float points[np][3], queries[nq][3]
//               -> float dist2[nq]; int32 index[nq]; int64 stats[8]; int32 dims[3], cells
//               (backwards: the points enter their cells in descending order -- no result may depend on the order inside a cell)
//   2 metrics   int32 n_ab, n_ba, nt, 0, 0, 0, 0; float thresholds[8]; float dist2_ab[n_ab], dist2_ba[n_ba]
//               -> double table[37]
// The reductions run in the order the device's run: tiles, lanes, butterflies, slots.  Exit 3: a refusal (its words on stderr).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../gaussianprediction_amd/csrc/geometry_core.h"

template <typename T>
static void get(FILE* fp, std::vector<T>& v) {
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), fp) != v.size()) { fprintf(stderr, "short job file\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const std::vector<T>& v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), fp) != v.size()) { fprintf(stderr, "short write\n"); exit(2); }
}
static int refuse(const char* why) { fprintf(stderr, "%s\n", why); return 3; }

static int samples(FILE* fp, FILE* out, const std::vector<int32_t>& head) {
    const int64_t nv = head[1], nf = head[2], n = head[3];
    const int32_t C = head[4];
    std::vector<uint64_t> seed(1);
    get(fp, seed);
    const char* why = gm_refuse_mesh(nv, nf);
    if (!why) why = gm_refuse_count(n);
    if (!why && n < 1) why = "n must be >= 1";
    if (!why && (C < 0 || C > GP_GEOMETRY_MAX_CHANNELS)) why = "C must be 1 .. 8";
    if (why) return refuse(why);
    std::vector<float> vertices(3 * nv), attributes(nv * C);
    std::vector<int32_t> faces(3 * nf);
    get(fp, vertices); get(fp, faces); get(fp, attributes);
    std::vector<int32_t> counts(GP_GEOMETRY_COUNT_WORDS, 0);
    std::vector<double> areas(nf);
    std::vector<uint64_t> prefix(nf);
    uint64_t max_bits = 0;
    for (int64_t f = 0; f < nf; ++f) {                                                           // gm_area_kernel
        double a;
        const int what = gm_face_area(vertices.data(), faces.data(), f, nv, &a);
        areas[f] = what == GM_FACE_OK ? a : -1.0;
        if (what == GM_FACE_BAD_INDEX) ++counts[GP_GEOMETRY_BAD_INDEX];
        if (what == GM_FACE_NON_FINITE) ++counts[GP_GEOMETRY_NON_FINITE];
        if (what == GM_FACE_OK && gm_double_bits(a) > max_bits) max_bits = gm_double_bits(a);
    }
    const double scale = gm_scale(max_bits);
    uint64_t total = 0;
    for (int64_t f = 0; f < nf; ++f) {                                                           // gm_weight_kernel, the scans
        const uint64_t w = areas[f] > 0.0 ? gm_weight(areas[f], scale) : 0;
        if (areas[f] >= 0.0 && w == 0) ++counts[GP_GEOMETRY_ZERO_WEIGHT];
        total += w;
        prefix[f] = total;
    }
    const GmSampleHead h = gm_sample_head(total, n);
    counts[GP_GEOMETRY_STATUS] = h.status;
    std::vector<float> points(3 * n), bary(2 * n), inter(n * C);
    std::vector<int32_t> face(n);
    for (int64_t i = 0; i < n; ++i) {
        gm_sample(vertices.data(), faces.data(), nv, nf, prefix.data(), h, seed[0], i, points.data(), face.data(), bary.data());
        if (C > 0) gm_interpolate(attributes.data(), C, faces.data(), nv, nf, face.data(), bary.data(), i, inter.data());
    }
    put(out, counts); put(out, points); put(out, face); put(out, bary); put(out, inter);
    return 0;
}

static int nearest(FILE* fp, FILE* out, const std::vector<int32_t>& head) {
    const int64_t np = head[1], nq = head[2];
    const bool backwards = head[3] != 0;
    std::vector<float> real(2);
    get(fp, real);
    const float cell = real[0];
    const char* why = gm_refuse_cloud(np, cell);
    if (!why) why = gm_refuse_count(nq);
    if (why) return refuse(why);
    std::vector<float> points(3 * np), queries(3 * nq);
    get(fp, points); get(fp, queries);
    uint32_t words[7] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u};
    for (int64_t j = 0; j < np; ++j) {                                                           // gm_bounds_kernel
        const float* p = &points[3 * j];
        if (!gm_usable(p)) continue;
        for (int a = 0; a < 3; ++a) {
            const uint32_t o = gm_ordered(p[a] + 0.f);
            if (o < words[a]) words[a] = o;
            if (o > words[3 + a]) words[3 + a] = o;
        }
        ++words[6];
    }
    GmGrid g;
    gm_derive(words, words[6], np, cell, &g);                                                    // gm_derive_kernel
    if (g.cells > gm_cell_capacity(np, cell)) return 4;
    std::vector<uint32_t> start(g.cells + 1, 0), cursor(g.cells + 1);
    for (int64_t j = 0; j < np; ++j)                                                             // gm_count_kernel
        if (gm_usable(&points[3 * j])) ++start[gm_key(g, &points[3 * j])];
    uint32_t run = 0;
    for (int64_t k = 0; k <= g.cells; ++k) { const uint32_t c = start[k]; start[k] = cursor[k] = run; run += c; }
    std::vector<GmRecord> records(words[6]);
    for (int64_t k = 0; k < np; ++k) {                                                           // gm_scatter_kernel
        const int64_t j = backwards ? np - 1 - k : k;
        const float* p = &points[3 * j];
        if (!gm_usable(p)) continue;
        GmRecord r;
        r.x = p[0]; r.y = p[1]; r.z = p[2]; r.index = (int32_t)j;
        records[cursor[gm_key(g, p)]++] = r;
    }
    std::vector<float> dist2(nq);
    std::vector<int32_t> index(nq);
    std::vector<int64_t> stats(GP_GEOMETRY_STAT_WORDS, 0);
    for (int64_t i = 0; i < nq; ++i) {                                                           // gm_query_kernel
        uint64_t seen;
        int32_t ring, swept;
        gm_query(g, start.data(), records.data(), &queries[3 * i], &dist2[i], &index[i], &seen, &ring, &swept);
        stats[GP_GEOMETRY_CANDIDATES] += (int64_t)seen;
        if (ring > stats[GP_GEOMETRY_MAX_RING]) stats[GP_GEOMETRY_MAX_RING] = ring;
        stats[GP_GEOMETRY_SWEPT] += swept;
        if (!gm_usable(&queries[3 * i])) ++stats[GP_GEOMETRY_EXCLUDED_QUERIES];
    }
    stats[GP_GEOMETRY_EXCLUDED_POINTS] = g.excluded;
    for (int a = 0; a < 3; ++a) stats[GP_GEOMETRY_DIM_X + a] = g.dims[a];
    std::vector<int32_t> dims = {g.dims[0], g.dims[1], g.dims[2], g.cells};
    put(out, dist2); put(out, index); put(out, stats); put(out, dims);
    return 0;
}

static void tile_slots(const std::vector<float>& d2, const GmThresholds& th, std::vector<double>& slots) {      // gm_metric_kernel
    const int64_t n = (int64_t)d2.size();
    for (int64_t tile = 0; tile < gm_tiles(n); ++tile) {
        double t[GM_BLOCK][GM_TERMS];
        for (int lane = 0; lane < GM_BLOCK; ++lane) {
            for (int q = 0; q < GM_TERMS; ++q) t[lane][q] = 0.0;
            for (int u = 0; u < GM_PER_LANE; ++u) {
                const int64_t k = tile * GM_TILE + u * GM_BLOCK + lane;
                if (k >= n) continue;
                double e[GM_TERMS];
                gm_terms(d2[k], th, e);
                for (int q = 0; q < GM_TERMS; ++q) t[lane][q] = gm_join(q, t[lane][q], e[q]);
            }
        }
        for (int s = 32; s >= 1; s >>= 1) {
            double o[GM_BLOCK][GM_TERMS];
            for (int lane = 0; lane < GM_BLOCK; ++lane)
                for (int q = 0; q < GM_TERMS; ++q) o[lane][q] = gm_join(q, t[lane][q], t[lane ^ s][q]);
            memcpy(t, o, sizeof(t));
        }
        for (int q = 0; q < GM_TERMS; ++q) slots.push_back(gm_join(q, gm_join(q, t[0][q], t[64][q]), gm_join(q, t[128][q], t[192][q])));
    }
}

static void totals(const double* slots, int64_t tiles, double* total) {                                        // gm_metric_final_kernel
    double s[GM_BLOCK][GM_TERMS];
    for (int lane = 0; lane < GM_BLOCK; ++lane) {
        for (int q = 0; q < GM_TERMS; ++q) s[lane][q] = 0.0;
        for (int64_t k = lane; k < tiles; k += GM_BLOCK)
            for (int q = 0; q < GM_TERMS; ++q) s[lane][q] = gm_join(q, s[lane][q], slots[k * GM_TERMS + q]);
    }
    for (int stride = GM_BLOCK / 2; stride >= 1; stride >>= 1)
        for (int lane = 0; lane < stride; ++lane)
            for (int q = 0; q < GM_TERMS; ++q) s[lane][q] = gm_join(q, s[lane][q], s[lane + stride][q]);
    for (int q = 0; q < GM_TERMS; ++q) total[q] = s[0][q];
}

static int metrics(FILE* fp, FILE* out, const std::vector<int32_t>& head) {
    const int64_t n_ab = head[1], n_ba = head[2];
    const int32_t nt = head[3];
    std::vector<float> th(8);
    get(fp, th);
    const char* why = gm_refuse_count(n_ab);
    if (!why) why = gm_refuse_count(n_ba);
    if (!why && (nt < 0 || nt > GP_GEOMETRY_MAX_THRESHOLDS)) why = "nt must be 0 .. 8";
    if (why) return refuse(why);
    GmThresholds t;
    t.nt = nt;
    for (int k = 0; k < 8; ++k) {
        t.v[k] = k < nt ? th[k] : 0.f;
        if (t.v[k] != t.v[k]) return refuse("a threshold is NaN");
    }
    std::vector<float> ab(n_ab), ba(n_ba);
    get(fp, ab); get(fp, ba);
    std::vector<double> slots_ab, slots_ba, total(2 * GM_TERMS), row(GP_GEOMETRY_COLUMNS);
    tile_slots(ab, t, slots_ab);
    tile_slots(ba, t, slots_ba);
    totals(slots_ab.data(), gm_tiles(n_ab), &total[0]);
    totals(slots_ba.data(), gm_tiles(n_ba), &total[GM_TERMS]);
    gm_row(total.data(), nt, row.data());
    put(out, row);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!fp || !out) return 2;
    std::vector<int32_t> head(8);
    get(fp, head);
    int rc = 2;
    if (head[0] == 0) rc = samples(fp, out, head);
    else if (head[0] == 1) rc = nearest(fp, out, head);
    else if (head[0] == 2) rc = metrics(fp, out, head);
    fclose(out);
    fclose(fp);
    return rc;
}
