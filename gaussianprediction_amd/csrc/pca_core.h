// pca_core.h -- the programs of the PCA colouring (csrc/gp_pca.h), shared by the kernels of pca_kernels.hip and by the stand-alone CPU
// build the tests run under the sanitizers (tests/pca_emulate.cpp).
//
//   pca_refusal / pca_percentile_refusal / pca_colorize_refusal   the argument checks, as text (NULL: accepted)
//   pca_rotation, pca_jacobi      one Jacobi rotation's (c, s); the sweeps of a symmetric matrix, run by a TEAM (below)
//   pca_pick_component            the k-th largest eigenvalue's eigenvector (a row of Vt) and the sign of its component
//   pca_project_row               one y_ik
//   pca_key / pca_unkey, pca_select_step, pca_rank, pca_interpolate   the radix select and the percentile
//   pca_vis, pca_clip01, pca_lut_index   the colours and the table lookup
// The file must be compiled with -ffp-contract=off: pca_project_row and pca_vis round once per operation.
//
// A TEAM is the set of workers that runs pca_jacobi together: `rank` of `size`, and sync(), after which every worker sees what the
// others stored.  On the device it is one workgroup (sync = __syncthreads), on the host one worker whose sync does nothing.  Work is
// dealt item by item (item i to worker i % size), the items of one phase touch disjoint entries, and every worker computes the
// phase-independent scalars for itself, so the result does not depend on the team's size: the host run and the device run of one matrix
// give equal bytes.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gp_pca.h"

#if defined(__HIPCC__)
#define PCA_FN __host__ __device__ inline
#else
#define PCA_FN inline
#endif

#define PCA_MAX_SWEEPS 30              // the sweeps of pca_jacobi end here whatever the matrix holds (non-finite input terminates)
#define PCA_CHUNK GP_PCA_CHUNK_ROWS
#define PCA_JACOBI_WORK (4 * 64 + 128 + 2)   // doubles of team-shared work space of pca_jacobi
#define PCA_MAX_PARTS 256              // workgroups of the mean and Gram kernels: workgroup b takes chunks b, b + parts, ...

// ---- the argument checks, worded once ------------------------------------------------------------------------------------------
inline const char* pca_refusal(int64_t N, int64_t D, int64_t dim) {
    if (N < 2) return "N must be >= 2";
    if (D < 1 || D > GP_PCA_MAX_D) return "D must be in 1 .. 128";
    if (dim < 1 || dim > GP_PCA_MAX_DIM || dim > D || dim > N) return "dim must be in 1 .. min(8, D, N)";
    if (N * dim >= 0x80000000LL) return "N*dim must be below 2^31";
    return nullptr;
}

inline const char* pca_percentile_refusal(int64_t M, int64_t nq, const double* qs) {
    if (M < 1 || M >= 0x80000000LL) return "M must be in 1 .. 2^31 - 1";
    if (nq < 1 || nq > GP_PCA_MAX_Q) return "the number of percentiles must be 1 or 2";
    for (int64_t k = 0; k < nq; ++k)
        if (!(qs[k] >= 0.0 && qs[k] <= 100.0)) return "a percentile must be in 0 .. 100";
    return nullptr;
}

inline const char* pca_colorize_refusal(int64_t N, int64_t dim) {
    if (N < 1) return "N must be >= 1";
    if (dim != 3 && dim != 5) return "colours need dim 3 or 5";
    if (N * dim >= 0x80000000LL) return "N*dim must be below 2^31";
    return nullptr;
}

PCA_FN int64_t pca_parts(int64_t N) {
    const int64_t chunks = (N + PCA_CHUNK - 1) / PCA_CHUNK;
    return chunks < PCA_MAX_PARTS ? chunks : PCA_MAX_PARTS;
}

// ---- Jacobi ----------------------------------------------------------------------------------------------------------------------
// (c, s) of the rotation J = [[c, s], [-s, c]] on rows and columns (p, q) that zeroes entry (p, q) of J^T A J.
PCA_FN void pca_rotation(double app, double aqq, double apq, double* c, double* s) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = fabs(theta);
    double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    *c = 1.0 / sqrt(t * t + 1.0);
    *s = t * *c;
}

// The pair i of step `step` of a round-robin over n players (n even): every two players meet once in n - 1 steps, the n / 2 pairs of one
// step are disjoint.  p < q.
PCA_FN void pca_pair(int n, int step, int i, int* p, int* q) {
    const int m = n - 1;
    const int a = i == 0 ? m : (step + i) % m, b = (step - i + m) % m;
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

// Cyclic Jacobi on A [D] rows of stride lda >= D (symmetric, destroyed: its diagonal ends as the eigenvalues) with Vt [D][D] ending as the
// eigenvectors in its ROWS (the lanes that rotate two eigenvectors then walk along rows of Vt, and with an odd lda down a column of A
// without a bank conflict).  work: PCA_JACOBI_WORK doubles shared by the team.  One sweep is n - 1 steps of n / 2 disjoint rotations (n = D rounded up
// to even; the pair with the padding player is skipped); a rotation is applied where |a_pq| > 1e-14 * ||A||_F / D, and its entry is then
// stored as an exact zero.  A sweep that applied none ends the loop: the off-diagonal part is then below 1e-14 * ||A||_F, inside the
// contract ||A v - lambda v|| <= 1e-12 * ||A||_F.  Returns the sweeps run.
template <typename Team>
PCA_FN int pca_jacobi(double* A, int lda, double* Vt, int D, double* work, Team team) {
    double* cs = work;                  // [64][4]: c, s, p, q of the step's pairs (p and q are small integers, exact as doubles)
    double* rows = work + 256;          // [128]
    double* flag = work + 384;          // [2]: a rotation was applied in this sweep, alternating by sweep
    const int n = (D + 1) & ~1, half = n / 2;
    for (int e = team.rank; e < D * D; e += team.size) Vt[e] = (e / D == e % D) ? 1.0 : 0.0;
    for (int r = team.rank; r < D; r += team.size) {
        double acc = 0.0;
        for (int k = 0; k < D; ++k) acc += A[r * lda + k] * A[r * lda + k];
        rows[r] = acc;
    }
    if (team.rank == 0) flag[0] = flag[1] = 0.0;
    team.sync();
    double fro = 0.0;
    for (int r = 0; r < D; ++r) fro += rows[r];
    const double thr = 1e-14 * sqrt(fro) / D;
    int sweep = 0;
    for (; sweep < PCA_MAX_SWEEPS; ++sweep) {
        for (int step = 0; step < n - 1; ++step) {
            for (int i = team.rank; i < half; i += team.size) {
                int p, q;
                pca_pair(n, step, i, &p, &q);
                double c = 1.0, s = 0.0;
                if (q < D && fabs(A[p * lda + q]) > thr) {
                    pca_rotation(A[p * lda + p], A[q * lda + q], A[p * lda + q], &c, &s);
                    flag[sweep & 1] = 1.0;
                }
                cs[4 * i] = c;
                cs[4 * i + 1] = s;
                cs[4 * i + 2] = (double)p;
                cs[4 * i + 3] = (double)q;
            }
            team.sync();
            // columns: A <- A J and V <- V J; item (i, r) owns entries (r, p) and (r, q) of A and V
            for (int e = team.rank; e < half * D; e += team.size) {
                const int i = e / D, r = e - i * D;
                const double c = cs[4 * i], s = cs[4 * i + 1];
                if (s == 0.0) continue;
                const int p = (int)cs[4 * i + 2], q = (int)cs[4 * i + 3];
                const double ap = A[r * lda + p], aq = A[r * lda + q], vp = Vt[p * D + r], vq = Vt[q * D + r];
                A[r * lda + p] = c * ap - s * aq;
                A[r * lda + q] = s * ap + c * aq;
                Vt[p * D + r] = c * vp - s * vq;
                Vt[q * D + r] = s * vp + c * vq;
            }
            team.sync();
            // rows: A <- J^T A; item (i, k) owns entries (p, k) and (q, k)
            for (int e = team.rank; e < half * D; e += team.size) {
                const int i = e / D, k = e - i * D;
                const double c = cs[4 * i], s = cs[4 * i + 1];
                if (s == 0.0) continue;
                const int p = (int)cs[4 * i + 2], q = (int)cs[4 * i + 3];
                const double ap = A[p * lda + k], aq = A[q * lda + k];
                A[p * lda + k] = k == q ? 0.0 : c * ap - s * aq;
                A[q * lda + k] = k == p ? 0.0 : s * ap + c * aq;
            }
            team.sync();
        }
        const bool rotated = flag[sweep & 1] != 0.0;
        team.sync();                                          // (every worker has read the flag before it is cleared ...)
        if (team.rank == 0) flag[sweep & 1] = 0.0;            // (... for the sweep after the next, which sets it many syncs later)
        if (!rotated) { ++sweep; break; }
    }
    return sweep;
}

// ---- order and sign ----------------------------------------------------------------------------------------------------------------
// The row of Vt that is component k: the k-th in descending eigenvalue A[j][j], the lower row first among equals; *sign is +-1 so that
// the entry of largest magnitude of the row is positive, the first such entry on a tie (decided in float64, before rounding).
PCA_FN int pca_pick_component(const double* A, int lda, const double* Vt, int D, int k, double* sign) {
    int col = 0;
    for (int j = 0; j < D; ++j) {
        const double lj = A[j * lda + j];
        int before = 0;                                 // eigenvalues that come before j
        for (int m = 0; m < D; ++m) {
            const double lm = A[m * lda + m];
            before += (lm > lj || (lm == lj && m < j)) ? 1 : 0;
        }
        if (before == k) col = j;
    }
    double best = -1.0, value = 1.0;
    for (int r = 0; r < D; ++r) {
        const double v = Vt[col * D + r];
        if (fabs(v) > best) { best = fabs(v); value = v; }
    }
    *sign = value < 0.0 ? -1.0 : 1.0;
    return col;
}

// ---- projection ----------------------------------------------------------------------------------------------------------------------
// y_ik: x, mean and c are rows of D floats; j ascending, a multiply and an add per term.
PCA_FN float pca_project_row(const float* x, const float* mean, const float* c, int D) {
    float y = 0.0f;
    for (int j = 0; j < D; ++j) y = y + (x[j] - mean[j]) * c[j];
    return y;
}

// ---- radix select --------------------------------------------------------------------------------------------------------------------
// float32 total order as unsigned keys: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.
PCA_FN uint32_t pca_key(float v) {
    union { float f; uint32_t u; } b;
    b.f = v;
    return (b.u & 0x80000000u) ? ~b.u : (b.u | 0x80000000u);
}
PCA_FN float pca_unkey(uint32_t k) {
    union { float f; uint32_t u; } b;
    b.u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return b.f;
}

struct PcaTarget { uint32_t prefix, rank; };      // the key bits decided so far (the high 8 * pass bits), the rank among the keys that share them

// One step: hist[256] counts the next 8 bits of the keys that share t.prefix; the bin that holds rank t.rank becomes the next 8 bits.
PCA_FN PcaTarget pca_select_step(PcaTarget t, const uint32_t* hist, int pass) {
    uint32_t before = 0, digit = 255, base = 0;
    bool found = false;
    for (uint32_t b = 0; b < 256; ++b) {
        const uint32_t h = hist[b];
        if (!found && t.rank - before < h) { digit = b; base = before; found = true; }
        before += h;
    }
    PcaTarget r;
    r.prefix = t.prefix | (digit << (24 - 8 * pass));
    r.rank = found ? t.rank - base : 0;
    return r;
}

// whether key belongs to the histogram of target t in pass `pass`
PCA_FN bool pca_key_matches(uint32_t key, PcaTarget t, int pass) {
    return pass == 0 || ((key ^ t.prefix) >> (32 - 8 * pass)) == 0;
}

// pos = q / 100 * (M - 1); lo = floor, hi = ceil, *frac = pos - lo
PCA_FN void pca_rank(double q, int64_t M, uint32_t* lo, uint32_t* hi, double* frac) {
    const double pos = q / 100.0 * (double)(M - 1);
    const double f = floor(pos);
    *lo = (uint32_t)f;
    *hi = (uint32_t)ceil(pos);
    *frac = pos - f;
}

PCA_FN float pca_interpolate(float v_lo, float v_hi, double frac) {
    return (float)((double)v_lo + ((double)v_hi - (double)v_lo) * frac);
}

// ---- colours --------------------------------------------------------------------------------------------------------------------------
PCA_FN float pca_vis(float y, float q1, float q99) { return (y - q1) / (q99 - q1); }       // (q99 == q1: the IEEE result, as the reference)
PCA_FN float pca_clip01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }       // (a NaN stays a NaN, as numpy's clip)

// the row of the 256-entry table for x, or -1 for a NaN (whose colour is (0, 0, 0))
PCA_FN int pca_lut_index(float x) {
    if (x != x) return -1;
    if (x < 0.0f) return 0;
    if (x >= 1.0f) return 255;
    return (int)(x * 256.0f);
}
