// meanshift_core.h -- the per-element programs of the mean-shift clustering (csrc/gp_meanshift.h), shared by the kernels of
// meanshift_kernels.hip and by the stand-alone CPU build the tests run under the sanitizers (tests/meanshift_emulate.cpp).
//
//   ms_size_refusal / ms_quantile_refusal / ms_max_iter_refusal / ms_rounds_refusal   the argument checks, as text (NULL: accepted)
//   ms_dp                                 D padded to the register width of the step: 4, 8, 16, 32 or 64
//   ms_dist2, ms_radius2, ms_bandwidth_ok the squared distance, the threshold t of `within`, the test of a bandwidth read on the device
//   ms_kth_rank, ms_key / ms_unkey, ms_key_matches, ms_select_step, ms_kth_value   the radix select of the k-th distance
//   MsSeed<DP>, ms_seed_begin / ms_seed_point / ms_seed_end   one seed's step: the members' float64 sums in ascending row order
//   ms_precedes                           the precedence of the merge
// The file must be compiled with -ffp-contract=off: every operation rounds once.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gp_meanshift.h"

#if defined(__HIPCC__)
#define MS_FN __host__ __device__ inline
#else
#define MS_FN inline
#endif

#define MS_TILE_FLOATS 8192           // the points go through LDS 32 KB at a time: 8192 / DP rows of the step, 8192 / (D | 1) of the select

// ---- the argument checks, worded once ------------------------------------------------------------------------------------------
inline const char* ms_size_refusal(int64_t N, int64_t S, int64_t D) {
    if (D < 1 || D > GP_MEANSHIFT_MAX_D) return "D must be in 1 .. 64";
    if (N < 1 || N >= 0x80000000LL) return "N must be in 1 .. 2^31 - 1";
    if (S < 1 || S >= 0x80000000LL) return "S must be in 1 .. 2^31 - 1";
    if (N * D >= 0x80000000LL) return "N*D must be below 2^31";
    if (S * D >= 0x80000000LL) return "S*D must be below 2^31";
    return nullptr;
}

inline const char* ms_quantile_refusal(double quantile) { return quantile > 0.0 && quantile <= 1.0 ? nullptr : "quantile must be in (0, 1]"; }

inline const char* ms_max_iter_refusal(int64_t max_iter) {
    return max_iter >= 0 && max_iter <= GP_MEANSHIFT_MAX_ITER ? nullptr : "max_iter must be in 0 .. 10000";
}

inline const char* ms_rounds_refusal(int64_t rounds) {
    return rounds >= 1 && rounds <= GP_MEANSHIFT_MAX_CENTRES ? nullptr : "rounds must be in 1 .. 4096";
}

MS_FN int ms_dp(int D) { return D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64; }

// ---- the distance ------------------------------------------------------------------------------------------------------------------
MS_FN float ms_dist2(const float* a, const float* b, int D) {
    float acc = 0.0f;
    for (int j = 0; j < D; ++j) {
        const float t = a[j] - b[j];
        acc = acc + t * t;
    }
    return acc;
}

MS_FN uint32_t ms_key(float v) {           // (a squared distance is >= +0: its bits order as unsigned integers; a NaN sorts last)
    union { float f; uint32_t u; } b;
    b.f = v;
    return b.u;
}
MS_FN float ms_unkey(uint32_t k) {
    union { float f; uint32_t u; } b;
    b.u = k;
    return b.f;
}

MS_FN bool ms_bandwidth_ok(double bandwidth) { return bandwidth > 0.0 && bandwidth <= 1.7976931348623157e308; }

// The largest float32 t with sqrtf(t) <= (float)bandwidth, for a bandwidth that ms_bandwidth_ok: d2 <= t is sqrtf(d2) <= (float)bandwidth.
// bw * bw is within a few units of it; the walks are bounded so that any input terminates.
MS_FN float ms_radius2(double bandwidth) {
    const float bw = (float)bandwidth;
    uint32_t k = ms_key(bw * bw);
    if (k > 0x7F7FFFFFu) k = 0x7F7FFFFFu;                            // (bw * bw overflowed: start at the largest finite float)
    for (int n = 0; n < 8 && k > 0u && sqrtf(ms_unkey(k)) > bw; ++n) --k;
    for (int n = 0; n < 8 && k < 0x7F7FFFFFu && sqrtf(ms_unkey(k + 1u)) <= bw; ++n) ++k;
    return ms_unkey(k);
}

// ---- the radix select of the k-th smallest distance ---------------------------------------------------------------------------------
MS_FN int64_t ms_kth_rank(int64_t N, double quantile) {                // zero-based: k - 1 with k = max(1, (int)(N * quantile))
    const int64_t k = (int64_t)((double)N * quantile);
    return k < 1 ? 0 : (k > N ? N - 1 : k - 1);
}

struct MsTarget { uint32_t prefix, rank; };      // the key bits decided so far (the high 8 * pass bits), the rank among the keys that share them

MS_FN bool ms_key_matches(uint32_t key, MsTarget t, int pass) { return pass == 0 || ((key ^ t.prefix) >> (32 - 8 * pass)) == 0; }

// hist[256] counts the next 8 bits of the keys that share t.prefix; the bin that holds rank t.rank becomes the next 8 bits.
template <typename Count>
MS_FN MsTarget ms_select_step(MsTarget t, const Count* hist, int pass) {
    uint32_t before = 0, digit = 255, base = 0;
    bool found = false;
    for (uint32_t b = 0; b < 256; ++b) {
        const uint32_t h = (uint32_t)hist[b];
        if (!found && t.rank - before < h) { digit = b; base = before; found = true; }
        before += h;
    }
    MsTarget r;
    r.prefix = t.prefix | (digit << (24 - 8 * pass));
    r.rank = found ? t.rank - base : 0;
    return r;
}

MS_FN float ms_kth_value(MsTarget t) { return sqrtf(ms_unkey(t.prefix)); }      // (sqrtf is monotone: the k-th distance is the root of the k-th square)

// ---- one seed's step ---------------------------------------------------------------------------------------------------------------
// m and the rows are padded with zeros from D to DP: a padding column adds +0 to every sum, which changes nothing.
template <int DP>
struct MsSeed {
    float m[DP];
    double sum[DP];
    int n;
};

template <int DP>
MS_FN void ms_seed_begin(MsSeed<DP>& s) {
#pragma unroll
    for (int j = 0; j < DP; ++j) s.sum[j] = 0.0;
    s.n = 0;
}

// the rows must come in ascending order: the float64 sums are then those of the definition
template <int DP>
MS_FN void ms_seed_point(MsSeed<DP>& s, const float* x, float radius2) {
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < DP; ++j) {
        const float t = x[j] - s.m[j];
        acc = acc + t * t;
    }
    if (acc <= radius2) {
#pragma unroll
        for (int j = 0; j < DP; ++j) s.sum[j] += (double)x[j];
        ++s.n;
    }
}

// Ends the step: m and *count are updated; returns whether the seed is finished; *it is incremented where it is not.
template <int DP>
MS_FN bool ms_seed_end(MsSeed<DP>& s, double bandwidth, int max_iter, int* it, int* count) {
    *count = s.n;
    if (s.n == 0) return true;
    const double n = (double)s.n;
    double shift2 = 0.0;
#pragma unroll
    for (int j = 0; j < DP; ++j) {
        const float m_new = (float)(s.sum[j] / n);
        const double d = (double)m_new - (double)s.m[j];
        shift2 = shift2 + d * d;
        s.m[j] = m_new;
    }
    if (sqrt(shift2) <= 1e-3 * bandwidth || *it >= max_iter) return true;
    *it += 1;
    return false;
}

// ---- the merge's precedence ----------------------------------------------------------------------------------------------------------
// whether seed a comes before seed b: count descending, then the centre lexicographically, larger first, then the lower index
MS_FN bool ms_precedes(int count_a, const float* a, int64_t index_a, int count_b, const float* b, int64_t index_b, int D) {
    if (count_a != count_b) return count_a > count_b;
    for (int j = 0; j < D; ++j)
        if (a[j] != b[j]) return a[j] > b[j];
    return index_a < index_b;
}
