// meanshift_emulate.cpp -- the programs of gaussianprediction_amd/csrc/meanshift_core.h on a CPU, in a stand-alone program
// (tests/test_meanshift_host.py builds it under the sanitizers and runs it as a child).  The loops walk the tiles the kernels walk.
//   meanshift_emulate JOB OUT
// JOB starts with int32 mode:
//   0 cluster    int64 N, S; int32 D, max_iter; double bandwidth; float X[N][D], seeds[S][D]
//                -> float seed_centers[S][D]; int32 seed_counts[S], seed_iterations[S]; int32 K; float centres[K][D]; int32 counts[K]
//   1 bandwidth  int64 N; int32 D; double quantile; float X[N][D]    -> float kth[N]; double bandwidth
//   2 refusals   int32 count; per query int32 kind (0 sizes: N, S, D; 1 max_iter: a; 2 rounds: a; 3 quantile: q), int64 a, b, c; double q
//                -> per query char text[96] (empty: accepted)
//   3 radius     int32 n; double bandwidth[n]    -> float t[n]; int32 ok[n]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../gaussianprediction_amd/csrc/meanshift_core.h"

template <typename T>
static void get(FILE* fp, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short job file\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short write\n"); exit(2); }
}

// every seed's steps, as ms_step_kernel<DP> runs one: the points through a tile of MS_TILE_FLOATS / DP padded rows, in ascending order
template <int DP>
static void shift(const std::vector<float>& X, int64_t N, int D, int64_t S, double bandwidth, int max_iter, std::vector<float>& m,
                  std::vector<int32_t>& counts, std::vector<int32_t>& its) {
    const float radius2 = ms_radius2(bandwidth);
    const int tile_rows = MS_TILE_FLOATS / DP;
    std::vector<float> tile((size_t)tile_rows * DP);
    for (int64_t s = 0; s < S; ++s) {
        bool done = false;
        for (int step = 0; step <= max_iter && !done; ++step) {
            MsSeed<DP> seed;
            ms_seed_begin(seed);
            for (int j = 0; j < DP; ++j) seed.m[j] = j < D ? m[s * D + j] : 0.0f;
            for (int64_t r0 = 0; r0 < N; r0 += tile_rows) {
                const int rows = (int)(N - r0 < tile_rows ? N - r0 : tile_rows);
                for (int e = 0; e < rows * DP; ++e) tile[e] = e % DP < D ? X[(r0 + e / DP) * D + e % DP] : 0.0f;
                for (int p = 0; p < rows; ++p) ms_seed_point(seed, tile.data() + (size_t)p * DP, radius2);
            }
            int it = its[s], count;
            done = ms_seed_end(seed, bandwidth, max_iter, &it, &count);
            counts[s] = count;
            its[s] = it;
            if (count > 0)
                for (int j = 0; j < D; ++j) m[s * D + j] = seed.m[j];
        }
        if (!done) abort();                                       // (max_iter + 1 steps finish every seed)
    }
}

static void cluster(FILE* fp, FILE* out) {
    int64_t N, S;
    int32_t D, max_iter;
    double bandwidth;
    get(fp, &N, 1); get(fp, &S, 1); get(fp, &D, 1); get(fp, &max_iter, 1); get(fp, &bandwidth, 1);
    if (ms_size_refusal(N, S, D) || ms_max_iter_refusal(max_iter) || !ms_bandwidth_ok(bandwidth)) exit(3);
    std::vector<float> X((size_t)N * D), m((size_t)S * D);
    get(fp, X.data(), X.size()); get(fp, m.data(), m.size());
    std::vector<int32_t> counts(S, 0), its(S, 0);
    switch (ms_dp(D)) {
        case 4: shift<4>(X, N, D, S, bandwidth, max_iter, m, counts, its); break;
        case 8: shift<8>(X, N, D, S, bandwidth, max_iter, m, counts, its); break;
        case 16: shift<16>(X, N, D, S, bandwidth, max_iter, m, counts, its); break;
        case 32: shift<32>(X, N, D, S, bandwidth, max_iter, m, counts, its); break;
        default: shift<64>(X, N, D, S, bandwidth, max_iter, m, counts, its); break;
    }
    put(out, m.data(), m.size()); put(out, counts.data(), counts.size()); put(out, its.data(), its.size());
    // pick and suppress, as the merge kernels do it
    const float radius2 = ms_radius2(bandwidth);
    std::vector<char> alive(S);
    for (int64_t s = 0; s < S; ++s) alive[s] = counts[s] > 0;
    std::vector<float> centres;
    std::vector<int32_t> kept;
    for (int64_t w = -1;;) {
        int64_t b = -1;
        for (int64_t s = 0; s < S; ++s) {
            if (!alive[s]) continue;
            if (w >= 0 && (s == w || ms_dist2(m.data() + s * D, m.data() + w * D, D) <= radius2)) { alive[s] = 0; continue; }
            if (b < 0 || ms_precedes(counts[s], m.data() + s * D, s, counts[b], m.data() + b * D, b, D)) b = s;
        }
        if (b < 0) break;
        centres.insert(centres.end(), m.begin() + b * D, m.begin() + (b + 1) * D);
        kept.push_back(counts[b]);
        w = b;
    }
    const int32_t K = (int32_t)kept.size();
    put(out, &K, 1); put(out, centres.data(), centres.size()); put(out, kept.data(), kept.size());
}

// the four passes as ms_select_kernel runs them: per pass a 256-bin count over the keys that share the prefix, the distances recomputed
static void bandwidth(FILE* fp, FILE* out) {
    int64_t N;
    int32_t D;
    double quantile;
    get(fp, &N, 1); get(fp, &D, 1); get(fp, &quantile, 1);
    if (ms_size_refusal(N, 1, D) || ms_quantile_refusal(quantile)) exit(3);
    std::vector<float> X((size_t)N * D), kth(N);
    get(fp, X.data(), X.size());
    const int LD = D | 1, tile_rows = MS_TILE_FLOATS / LD;
    std::vector<float> tile((size_t)tile_rows * LD, -777.0f);
    for (int64_t q = 0; q < N; ++q) {
        MsTarget target = {0u, (uint32_t)ms_kth_rank(N, quantile)};
        for (int pass = 0; pass < 4; ++pass) {
            uint32_t hist[256];
            memset(hist, 0, sizeof(hist));
            for (int64_t r0 = 0; r0 < N; r0 += tile_rows) {
                const int rows = (int)(N - r0 < tile_rows ? N - r0 : tile_rows);
                for (int e = 0; e < rows * D; ++e) tile[(size_t)(e / D) * LD + e % D] = X[r0 * D + e];
                for (int p = 0; p < rows; ++p) {
                    const uint32_t key = ms_key(ms_dist2(X.data() + q * D, tile.data() + (size_t)p * LD, D));
                    if (ms_key_matches(key, target, pass)) ++hist[(key >> (24 - 8 * pass)) & 255u];
                }
            }
            target = ms_select_step(target, hist, pass);
        }
        kth[q] = ms_kth_value(target);
    }
    double sum = 0.0;
    for (int64_t q = 0; q < N; ++q) sum += (double)kth[q];
    const double bw = sum / (double)N;
    put(out, kth.data(), kth.size()); put(out, &bw, 1);
}

static void refusals(FILE* fp, FILE* out) {
    int32_t count;
    get(fp, &count, 1);
    for (int n = 0; n < count; ++n) {
        int32_t kind;
        int64_t a[3];
        double q;
        get(fp, &kind, 1); get(fp, a, 3); get(fp, &q, 1);
        const char* why = kind == 0 ? ms_size_refusal(a[0], a[1], a[2]) : kind == 1 ? ms_max_iter_refusal(a[0]) : kind == 2 ? ms_rounds_refusal(a[0]) : ms_quantile_refusal(q);
        char text[96];
        memset(text, 0, sizeof(text));
        if (why) strncpy(text, why, sizeof(text) - 1);
        put(out, text, sizeof(text));
    }
}

static void radius(FILE* fp, FILE* out) {
    int32_t n;
    get(fp, &n, 1);
    std::vector<double> bw(n);
    get(fp, bw.data(), bw.size());
    std::vector<float> t(n);
    std::vector<int32_t> ok(n);
    for (int i = 0; i < n; ++i) {
        t[i] = ms_radius2(bw[i]);
        ok[i] = ms_bandwidth_ok(bw[i]) ? 1 : 0;
    }
    put(out, t.data(), t.size()); put(out, ok.data(), ok.size());
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!fp || !out) return 2;
    int32_t mode;
    get(fp, &mode, 1);
    if (mode == 0) cluster(fp, out);
    else if (mode == 1) bandwidth(fp, out);
    else if (mode == 2) refusals(fp, out);
    else if (mode == 3) radius(fp, out);
    else return 2;
    fclose(out);
    fclose(fp);
    return 0;
}
