// pca_emulate.cpp -- the programs of gaussianprediction_amd/csrc/pca_core.h on a CPU, in a stand-alone program
// (tests/test_pca_host.py builds it under the sanitizers and runs it as a child).
//   pca_emulate JOB OUT
// JOB starts with int32 mode:
//   0 jacobi    int32 D, dim; double C[D][D]
//               -> int32 sweeps; double eigenvalue[D] (the diagonal, in the iteration's order); double Vt[D][D] (eigenvectors in rows);
//                  per k < dim: int32 row of Vt, double sign
//   1 project   int64 N; int32 D, dim; float X[N][D], mean[D], components[dim][D]    -> float Y[N][dim]
//   2 select    int64 M; int32 nq; double qs[2]; float values[M]
//               -> int32 refused (1: nothing follows); float selected[nq][2]; float out[nq]
//   3 refusals  int32 count; per query int32 kind (0 fit: N, D, dim; 1 percentiles: M, nq, with q0, q1; 2 colorize: N, dim), int64 a, b, c; double q0, q1
//               -> per query char text[96] (empty: accepted)
//   4 colours   int32 n; float q1, q99; float x[n]    -> float vis[n], clipped[n]; int32 lut_index[n]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../gaussianprediction_amd/csrc/pca_core.h"

struct HostTeam {
    int rank, size;
    void sync() const {}
};

template <typename T>
static void get(FILE* fp, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short job file\n"); exit(2); }
}
template <typename T>
static void put(FILE* fp, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, fp) != n) { fprintf(stderr, "short write\n"); exit(2); }
}

static void jacobi(FILE* fp, FILE* out) {
    int32_t D, dim;
    get(fp, &D, 1); get(fp, &dim, 1);
    std::vector<double> C((size_t)D * D), V((size_t)D * D), work(PCA_JACOBI_WORK), lam(D);
    get(fp, C.data(), C.size());
    const int lda = D + 3;                                      // (any stride >= D: the entries beyond D are never touched)
    std::vector<double> A((size_t)D * lda, -777.0);
    for (int j = 0; j < D; ++j)
        for (int k = 0; k < D; ++k) A[(size_t)j * lda + k] = C[(size_t)j * D + k];
    HostTeam team = {0, 1};
    const int32_t sweeps = pca_jacobi(A.data(), lda, V.data(), D, work.data(), team);
    for (int j = 0; j < D; ++j) {
        lam[j] = A[(size_t)j * lda + j];
        for (int k = D; k < lda; ++k)
            if (A[(size_t)j * lda + k] != -777.0) abort();
    }
    put(out, &sweeps, 1); put(out, lam.data(), lam.size()); put(out, V.data(), V.size());
    for (int k = 0; k < dim; ++k) {
        double sign;
        const int32_t col = pca_pick_component(A.data(), lda, V.data(), D, k, &sign);
        put(out, &col, 1); put(out, &sign, 1);
    }
}

static void project(FILE* fp, FILE* out) {
    int64_t N;
    int32_t D, dim;
    get(fp, &N, 1); get(fp, &D, 1); get(fp, &dim, 1);
    std::vector<float> X((size_t)N * D), mean(D), comp((size_t)dim * D), Y((size_t)N * dim);
    get(fp, X.data(), X.size()); get(fp, mean.data(), mean.size()); get(fp, comp.data(), comp.size());
    for (int64_t i = 0; i < N; ++i)
        for (int k = 0; k < dim; ++k) Y[i * dim + k] = pca_project_row(X.data() + i * D, mean.data(), comp.data() + (size_t)k * D, D);
    put(out, Y.data(), Y.size());
}

// the four passes as the kernels run them: per pass one 256-bin count per target over the keys that share its prefix
static void select(FILE* fp, FILE* out) {
    int64_t M;
    int32_t nq;
    double qs[2];
    get(fp, &M, 1); get(fp, &nq, 1); get(fp, qs, 2);
    int32_t refused = pca_percentile_refusal(M, nq, qs) ? 1 : 0;
    put(out, &refused, 1);
    if (refused) return;
    std::vector<float> values(M);
    get(fp, values.data(), values.size());
    PcaTarget target[4];
    double frac[2];
    for (int k = 0; k < nq; ++k) {
        uint32_t lo, hi;
        pca_rank(qs[k], M, &lo, &hi, &frac[k]);
        target[2 * k] = {0u, lo};
        target[2 * k + 1] = {0u, hi};
    }
    for (int pass = 0; pass < 4; ++pass)
        for (int u = 0; u < 2 * nq; ++u) {
            std::vector<uint32_t> hist(256, 0u);
            for (int64_t i = 0; i < M; ++i) {
                const uint32_t key = pca_key(values[i]);
                if (pca_key_matches(key, target[u], pass)) ++hist[(key >> (24 - 8 * pass)) & 255u];
            }
            target[u] = pca_select_step(target[u], hist.data(), pass);
        }
    float selected[4], q[2];
    for (int u = 0; u < 2 * nq; ++u) selected[u] = pca_unkey(target[u].prefix);
    for (int k = 0; k < nq; ++k) q[k] = pca_interpolate(selected[2 * k], selected[2 * k + 1], frac[k]);
    put(out, selected, 2 * nq); put(out, q, nq);
}

static void refusals(FILE* fp, FILE* out) {
    int32_t count;
    get(fp, &count, 1);
    for (int n = 0; n < count; ++n) {
        int32_t kind;
        int64_t a[3];
        double q[2];
        get(fp, &kind, 1); get(fp, a, 3); get(fp, q, 2);
        const char* why = kind == 0 ? pca_refusal(a[0], a[1], a[2]) : kind == 1 ? pca_percentile_refusal(a[0], a[1], q) : pca_colorize_refusal(a[0], a[1]);
        char text[96];
        memset(text, 0, sizeof(text));
        if (why) strncpy(text, why, sizeof(text) - 1);
        put(out, text, sizeof(text));
    }
}

static void colours(FILE* fp, FILE* out) {
    int32_t n;
    float q1, q99;
    get(fp, &n, 1); get(fp, &q1, 1); get(fp, &q99, 1);
    std::vector<float> x(n), vis(n), clipped(n);
    std::vector<int32_t> index(n);
    get(fp, x.data(), x.size());
    for (int i = 0; i < n; ++i) {
        vis[i] = pca_vis(x[i], q1, q99);
        clipped[i] = pca_clip01(vis[i]);
        index[i] = pca_lut_index(x[i]);
    }
    put(out, vis.data(), vis.size()); put(out, clipped.data(), clipped.size()); put(out, index.data(), index.size());
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!fp || !out) return 2;
    int32_t mode;
    get(fp, &mode, 1);
    if (mode == 0) jacobi(fp, out);
    else if (mode == 1) project(fp, out);
    else if (mode == 2) select(fp, out);
    else if (mode == 3) refusals(fp, out);
    else if (mode == 4) colours(fp, out);
    else return 2;
    fclose(out);
    fclose(fp);
    return 0;
}
