// kmeans_kernels.hip -- deterministic Lloyd k-means on the device (include/gp_kmeans.h), gfx950.
//
//   km_rows_kernel<DP, ASSIGN, ACCUM>   a workgroup owns a contiguous range of rows and walks it in batches of 256: a lane holds one
//                      row in registers (DP = D rounded up, the tail zero: (0 - 0)^2 adds +0 to a non-negative sum, so the padded
//                      sum has the bits of the D-term one).
//                      ASSIGN: the centres sit in LDS, a tile of KM_CT floats at a time; every lane reads the SAME centre address
//                      (a broadcast: no bank conflict) as float4 and keeps the running minimum: the ids do not depend on the tile size.
//                      ACCUM: the batch goes through LDS, 64 (or 32) rows at a time; lane (g, d) of the accumulate role walks those
//                      rows IN ORDER and adds column d of the rows whose cluster it owns (k mod G == g) into a double table in LDS,
//                      a tile of KM_AT doubles of the clusters at a time; a (cluster, column) cell has one owner, so the order of its
//                      additions is the row order.  The table goes to this workgroup's partial sums.  With one table tile (K * DP <=
//                      KM_AT) X is read once; a further tile reads the range again (ids then come from memory).
//   km_finish_kernel   one wave per cluster: adds the partial sums in workgroup order, forms the mean (or the new centre and its shift)
//   km_total_kernel    one workgroup: the shifts in cluster order, shift^2 against tol, the status words
// No atomics, no host reads; plain (vector) stores only.
#include "gp_common.h"

#include "../../include/gp_kmeans.h"

#define KM_BLOCK GP_KMEANS_BLOCK
#define KM_CT 5400                        // floats of a centre tile in LDS (150 centres of 36)
#define KM_AT 5400                        // doubles of a tile of the sum table in LDS
#define KM_MAX_WG 512                     // workgroups of the row kernel: one resident round at two per CU
#define KM_PARTIAL_BYTES (24u << 20)      // the partial sums stay below this where one workgroup's table allows it
static_assert(KM_BLOCK == 256, "a batch is one row per lane of four waves");

// ------------------------------------------------------------------------------------------------
// rows: assignment and per-workgroup partial sums
// ------------------------------------------------------------------------------------------------
template <int DP, bool ASSIGN, bool ACCUM>
__global__ __launch_bounds__(KM_BLOCK) void km_rows_kernel(uint64_t N, int D, const float* __restrict__ X, int K, const float* __restrict__ centres,
                                                          int32_t* ids, float* __restrict__ d2out, uint64_t rows_per_wg,
                                                          double* __restrict__ psum, int32_t* __restrict__ pcnt,
                                                          const uint32_t* __restrict__ status, int honour) {
    static_assert(DP % 4 == 0 && DP <= 64, "rows are moved as float4");
    constexpr int KT = KM_CT / DP;                 // centres per tile
    constexpr int AK = KM_AT / DP;                 // clusters per tile of the sum table
    constexpr int G = KM_BLOCK / DP;               // cluster groups of the accumulate role
    constexpr int SR = DP <= 36 ? 64 : 32;         // rows per sub-round through LDS
    __shared__ __attribute__((aligned(16))) float s_c[ASSIGN ? KT * DP : 4];
    __shared__ __attribute__((aligned(16))) float s_x[ACCUM ? SR * DP : 4];
    __shared__ double s_acc[ACCUM ? AK * DP : 1];
    __shared__ int s_cnt[ACCUM ? AK : 1];
    __shared__ int s_id[ACCUM ? KM_BLOCK : 1];

    if (honour && status[GP_KMEANS_ST_CONVERGED]) return;      // (uniform: before any barrier)
    const int t = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * rows_per_wg;
    const uint64_t row1 = (row0 + rows_per_wg < N) ? row0 + rows_per_wg : N;
    const int g = t / DP, dd = t % DP;
    const int n_tiles = ACCUM ? (K + AK - 1) / AK : 1;
    int staged = -1;                                            // first centre of the tile in s_c

    for (int j = 0; j < n_tiles; ++j) {
        const int abase = j * AK;
        const int ak = (K - abase < AK) ? K - abase : AK;
        if (ACCUM) {
            for (int e = t; e < ak * DP; e += KM_BLOCK) s_acc[e] = 0.0;
            for (int e = t; e < ak; e += KM_BLOCK) s_cnt[e] = 0;
        }
        for (uint64_t b0 = row0; b0 < row1; b0 += KM_BLOCK) {
            const uint64_t i = b0 + t;
            const bool live = i < row1;
            float x[DP];
#pragma unroll
            for (int d = 0; d < DP; ++d) x[d] = (live && d < D) ? X[i * (uint64_t)D + d] : 0.f;
            int id = -1;
            if (ASSIGN && j == 0) {
                float best = __builtin_inff();
                int bk = 0;
                for (int cb = 0; cb < K; cb += KT) {
                    const int kt = (K - cb < KT) ? K - cb : KT;
                    if (staged != cb) {
                        __syncthreads();                        // the readers of the tile before are done
                        for (int e = t; e < kt * DP; e += KM_BLOCK) {
                            const int k = e / DP, d = e % DP;
                            s_c[e] = (d < D) ? centres[(size_t)(cb + k) * D + d] : 0.f;
                        }
                        __syncthreads();
                        staged = cb;
                    }
#pragma unroll 2
                    for (int k = 0; k < kt; ++k) {
                        const float4* c4 = reinterpret_cast<const float4*>(s_c + k * DP);
                        float acc = 0.f;
#pragma unroll
                        for (int q = 0; q < DP / 4; ++q) {
                            const float4 c = c4[q];
                            const float t0 = x[4 * q] - c.x, t1 = x[4 * q + 1] - c.y, t2 = x[4 * q + 2] - c.z, t3 = x[4 * q + 3] - c.w;
                            acc = acc + t0 * t0;
                            acc = acc + t1 * t1;
                            acc = acc + t2 * t2;
                            acc = acc + t3 * t3;
                        }
                        if (acc < best) {                       // strict: a tie keeps the lower k, a NaN never wins
                            best = acc;
                            bk = cb + k;
                        }
                    }
                }
                if (live) {
                    ids[i] = bk;
                    if (d2out) d2out[i] = best;
                    id = bk;
                }
            } else if (ACCUM && live) {
                id = ids[i];
            }
            if (ACCUM) {
                __syncthreads();                                // the batch before is summed (and the table is zero)
                s_id[t] = id;
                for (int sub = 0; sub < KM_BLOCK / SR; ++sub) {
                    if (b0 + (uint64_t)sub * SR >= row1) break;  // (uniform)
                    if (sub) __syncthreads();
                    if (t / SR == sub) {
                        float4* dst = reinterpret_cast<float4*>(s_x + (t % SR) * DP);
#pragma unroll
                        for (int q = 0; q < DP / 4; ++q) dst[q] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
                    }
                    __syncthreads();
                    if (g < G) {
                        for (int r = 0; r < SR; ++r) {
                            const int kk = s_id[sub * SR + r] - abase;
                            if ((unsigned)kk < (unsigned)ak && kk % G == g) {
                                s_acc[kk * DP + dd] += (double)s_x[r * DP + dd];
                                if (dd == 0) s_cnt[kk] += 1;
                            }
                        }
                    }
                }
            }
        }
        if (ACCUM) {
            __syncthreads();
            const size_t wg = blockIdx.x;
            for (int e = t; e < ak * D; e += KM_BLOCK) {
                const int k = e / D, d = e % D;
                psum[(wg * K + abase + k) * D + d] = s_acc[k * DP + d];
            }
            for (int e = t; e < ak; e += KM_BLOCK) pcnt[wg * K + abase + e] = s_cnt[e];
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// the partial sums in workgroup order -> mean (MODE 0) or new centre + shift (MODE 1)
// ------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(GP_WAVE) void km_finish_kernel(int K, int D, uint32_t nb, const double* __restrict__ psum, const int32_t* __restrict__ pcnt,
                                                           float* out, int32_t* __restrict__ counts, double* __restrict__ shift,
                                                           const uint32_t* __restrict__ status, int honour) {
    __shared__ double s_sq[GP_WAVE];
    if (honour && status[GP_KMEANS_ST_CONVERGED]) return;
    const int k = blockIdx.x, d = threadIdx.x;
    int64_t count = 0;
    for (uint32_t b = 0; b < nb; ++b) count += pcnt[(size_t)b * K + k];
    double sum = 0.0;
    if (d < D) {
#pragma unroll 8
        for (uint32_t b = 0; b < nb; ++b) sum += psum[((size_t)b * K + k) * D + d];
    }
    if (d == 0 && counts) counts[k] = (int32_t)count;
    if (MODE == 0) {
        if (d < D) out[(size_t)k * D + d] = count > 0 ? (float)(sum / (double)count) : 0.f;
    } else {
        double diff = 0.0;
        if (d < D) {
            const float old = out[(size_t)k * D + d];
            const float nw = count > 0 ? (float)(sum / (double)count) : old;
            out[(size_t)k * D + d] = nw;
            diff = (double)nw - (double)old;
        }
        s_sq[d] = diff * diff;
        __syncthreads();
        if (d == 0) {
            double q = 0.0;
            for (int e = 0; e < D; ++e) q += s_sq[e];
            shift[k] = sqrt(q);
        }
    }
}

__global__ __launch_bounds__(KM_BLOCK) void km_total_kernel(int K, const double* __restrict__ shift, double tol, uint32_t* status) {
    __shared__ double s_part[KM_BLOCK];
    if (status[GP_KMEANS_ST_CONVERGED]) return;
    const int t = threadIdx.x, per = (K + KM_BLOCK - 1) / KM_BLOCK;
    double p = 0.0;
    for (int k = t * per; k < (t + 1) * per && k < K; ++k) p += shift[k];
    s_part[t] = p;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int e = 0; e < KM_BLOCK; ++e) s += s_part[e];
        const double s2 = s * s;
        status[GP_KMEANS_ST_ITERATIONS] += 1u;
        *reinterpret_cast<double*>(status + GP_KMEANS_ST_SHIFT2) = s2;
        if (s2 <= tol) status[GP_KMEANS_ST_CONVERGED] = 1u;
    }
}

// ------------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------------
struct KmPlan {
    uint32_t nb;        // workgroups of the row kernel
    uint64_t rows;      // rows of one workgroup, a multiple of KM_BLOCK
};

static KmPlan km_plan(int64_t N, int D, int K) {
    const uint64_t batches = ((uint64_t)N + KM_BLOCK - 1) / KM_BLOCK;
    const uint64_t per_wg = (uint64_t)K * D * sizeof(double) + (uint64_t)K * sizeof(int32_t);
    uint64_t target = KM_PARTIAL_BYTES / per_wg;
    if (target < 1) target = 1;
    if (target > KM_MAX_WG) target = KM_MAX_WG;
    if (target > batches) target = batches;
    KmPlan p;
    p.rows = (batches + target - 1) / target * KM_BLOCK;
    p.nb = (uint32_t)(((uint64_t)N + p.rows - 1) / p.rows);
    return p;
}

struct KmScratch {
    double* psum;
    int32_t* pcnt;
    double* shift;
    float* mean;        // where gp_kmeans_run puts a mean nobody asked for
    size_t bytes;
    KmScratch(void* p, int64_t N, int D, int K) {
        const KmPlan pl = km_plan(N, D, K);
        GpCarver c(p);
        psum = c.take<double>((size_t)pl.nb * K * D);
        pcnt = c.take<int32_t>((size_t)pl.nb * K);
        shift = c.take<double>((size_t)K);
        mean = c.take<float>((size_t)K * D);
        bytes = c.bytes();
    }
};

static int km_pad(int D) {
    static const int pads[] = {4, 8, 16, 32, 36, 48, 64};
    for (int p : pads)
        if (D <= p) return p;
    return 0;
}

template <bool ASSIGN, bool ACCUM>
static int km_launch_rows(const KmPlan& pl, int64_t N, int D, const float* X, int K, const float* centres, int32_t* ids, float* d2,
                          double* psum, int32_t* pcnt, const uint32_t* status, int honour, hipStream_t s) {
#define KM_CASE_(DP)                                                                                                                          \
    case DP:                                                                                                                                  \
        hipLaunchKernelGGL((km_rows_kernel<DP, ASSIGN, ACCUM>), dim3(pl.nb), dim3(KM_BLOCK), 0, s, (uint64_t)N, D, X, K, centres, ids, d2, pl.rows, \
                           psum, pcnt, status, honour);                                                                                       \
        break;
    switch (km_pad(D)) {
        KM_CASE_(4) KM_CASE_(8) KM_CASE_(16) KM_CASE_(32) KM_CASE_(36) KM_CASE_(48) KM_CASE_(64)
        default: GP_FAIL("gp_kmeans: D = %d outside [1, %d]", D, GP_KMEANS_MAX_D);
    }
#undef KM_CASE_
    GP_LAUNCH_CHECK();
    return 0;
}

static int km_check_sizes(const char* who, int64_t N, int32_t D, int32_t K) {
    if (N < 1 || N > GP_KMEANS_MAX_ROWS) GP_FAIL("%s: N = %lld outside [1, %d]", who, (long long)N, GP_KMEANS_MAX_ROWS);
    if (D < 1 || D > GP_KMEANS_MAX_D) GP_FAIL("%s: D = %d outside [1, %d]", who, D, GP_KMEANS_MAX_D);
    if (K < 1 || K > GP_KMEANS_MAX_K) GP_FAIL("%s: K = %d outside [1, %d]", who, K, GP_KMEANS_MAX_K);
    return 0;
}

// per-cluster mean of `src` [N][dim] by ids, on the row plan `pl` (two launches)
static int km_mean(const KmPlan& pl, int64_t N, int dim, const float* src, const int32_t* ids, int K, float* mean, int32_t* counts,
                   const KmScratch& sc, hipStream_t s) {
    if (km_launch_rows<false, true>(pl, N, dim, src, K, nullptr, const_cast<int32_t*>(ids), nullptr, sc.psum, sc.pcnt, nullptr, 0, s)) return 1;
    hipLaunchKernelGGL(km_finish_kernel<0>, dim3(K), dim3(GP_WAVE), 0, s, K, dim, pl.nb, (const double*)sc.psum, (const int32_t*)sc.pcnt, mean,
                       counts, (double*)nullptr, (const uint32_t*)nullptr, 0);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_kmeans_abi_version(void) { return GP_KMEANS_ABI_VERSION; }

extern "C" int64_t gp_kmeans_scratch_bytes(int64_t N, int32_t D, int32_t K) {
    if (km_check_sizes("gp_kmeans_scratch_bytes", N, D, K)) return -1;
    return (int64_t)KmScratch(nullptr, N, D, K).bytes;
}

extern "C" int gp_kmeans_assign(int64_t N, int32_t D, const float* X, int32_t K, const float* centres, int32_t* ids, float* d2,
                                gp_stream_t stream_) {
    if (km_check_sizes("gp_kmeans_assign", N, D, K)) return 1;
    if (!X || !centres || !ids) GP_FAIL("gp_kmeans_assign: null argument");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("kmeans_assign", s);
    KmPlan pl;                                                   // no partial sums: every batch a workgroup of its own
    pl.rows = KM_BLOCK;
    pl.nb = gp_blocks((size_t)N, KM_BLOCK);
    return km_launch_rows<true, false>(pl, N, D, X, K, centres, ids, d2, nullptr, nullptr, nullptr, 0, s);
}

extern "C" int gp_cluster_mean(int64_t N, int32_t D, const float* X, const int32_t* ids, int32_t K, float* mean, int32_t* counts,
                               void* scratch, gp_stream_t stream_) {
    if (km_check_sizes("gp_cluster_mean", N, D, K)) return 1;
    if (!X || !ids || !mean || !counts || !scratch) GP_FAIL("gp_cluster_mean: null argument");
    if ((uintptr_t)scratch & 255) GP_FAIL("gp_cluster_mean: scratch must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("cluster_mean", s);
    return km_mean(km_plan(N, D, K), N, D, X, ids, K, mean, counts, KmScratch(scratch, N, D, K), s);
}

extern "C" int gp_kmeans_run(int64_t N, int32_t D, const float* X, int32_t K, float* centres, int32_t max_iters, double tol, int32_t* ids,
                             int32_t* counts, const float* aux, int32_t aux_dim, float* aux_mean, uint32_t* status, void* scratch,
                             gp_stream_t stream_) {
    if (km_check_sizes("gp_kmeans_run", N, D, K)) return 1;
    if (max_iters < 1 || max_iters > GP_KMEANS_MAX_ITERS) GP_FAIL("gp_kmeans_run: max_iters = %d outside [1, %d]", max_iters, GP_KMEANS_MAX_ITERS);
    if (!(tol >= 0.0)) GP_FAIL("gp_kmeans_run: tol = %g must be >= 0", tol);
    if (!X || !centres || !ids || !counts || !status || !scratch) GP_FAIL("gp_kmeans_run: null argument");
    if (aux && (aux_dim < 1 || aux_dim > D)) GP_FAIL("gp_kmeans_run: aux_dim = %d outside [1, D = %d]", aux_dim, D);
    if (aux && !aux_mean) GP_FAIL("gp_kmeans_run: aux without aux_mean");
    if ((uintptr_t)scratch & 255) GP_FAIL("gp_kmeans_run: scratch must be 256-byte aligned");
    if ((uintptr_t)status & 7) GP_FAIL("gp_kmeans_run: status must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("kmeans_run", s);
    const KmPlan pl = km_plan(N, D, K);
    const KmScratch sc(scratch, N, D, K);
    GP_HIP_CHECK(hipMemsetAsync(status, 0, GP_KMEANS_STATUS_WORDS * sizeof(uint32_t), s));
    for (int it = 0; it < max_iters; ++it) {
        if (km_launch_rows<true, true>(pl, N, D, X, K, centres, ids, nullptr, sc.psum, sc.pcnt, status, 1, s)) return 1;
        hipLaunchKernelGGL(km_finish_kernel<1>, dim3(K), dim3(GP_WAVE), 0, s, K, D, pl.nb, (const double*)sc.psum, (const int32_t*)sc.pcnt, centres,
                           (int32_t*)nullptr, sc.shift, (const uint32_t*)status, 1);
        GP_LAUNCH_CHECK();
        hipLaunchKernelGGL(km_total_kernel, dim3(1), dim3(KM_BLOCK), 0, s, K, (const double*)sc.shift, tol, status);
        GP_LAUNCH_CHECK();
    }
    // ids, counts and aux_mean describe the centres returned
    KmPlan one;
    one.rows = KM_BLOCK;
    one.nb = gp_blocks((size_t)N, KM_BLOCK);
    if (km_launch_rows<true, false>(one, N, D, X, K, centres, ids, nullptr, nullptr, nullptr, nullptr, 0, s)) return 1;
    if (aux) return km_mean(pl, N, aux_dim, aux, ids, K, aux_mean, counts, sc, s);
    return km_mean(pl, N, D, X, ids, K, sc.mean, counts, sc, s);
}
