// meanshift_kernels.hip -- flat-kernel mean-shift clustering on the device (csrc/gp_meanshift.h, which states the definition in full).
// The per-element programs that a CPU can run are csrc/meanshift_core.h (tests/meanshift_emulate.cpp runs them).
//   ms_select_kernel          one launch per 8-bit pass of the radix select.  A workgroup owns 16 query rows, four per wave; the rows of X
//                             go through LDS in tiles (row stride D | 1: the lanes' rows fall on different banks), a lane takes a point
//                             and adds its squared distance to the wave's four queries (their coordinates are LDS broadcasts), then
//                             counts the next 8 bits of each in the query's 256-bin LDS histogram (integer atomics).  The distances
//                             are recomputed each pass: nothing of size N^2 is stored
//   ms_bandwidth_sum_kernel   one workgroup: the N k-th distances through LDS, added by one lane in ascending order in float64
//   ms_run_init_kernel        the seeds' state (m, count, it, finished) and the status block
//   ms_step_kernel<DP>        ONE step for all unfinished seeds.  A lane owns a seed -- m in DP registers, the float64 sums in 2 * DP
//                             -- and is its only accumulation chain; the points stream through LDS in ascending row order and every
//                             lane reads the same point (a broadcast), so the sums are in ascending row order whatever the grid.  A
//                             workgroup whose seeds are all finished returns at once
//   ms_merge_init_kernel, ms_merge_scan_kernel, ms_merge_pick_kernel   pick and suppress: scan kills every live centre within the radius
//                             of the last winner and reduces the comparator over the rest (per lane, then per workgroup), pick
//                             reduces the workgroups' candidates, appends the winner and counts it
// Every store is an ordinary vector store; the only atomics are on integers.
#include "gp_common.h"

#include "meanshift_core.h"

#define MS_BLOCK 256
#define MS_BW_QPW 4                              // query rows of a wave
#define MS_BW_Q (MS_BW_QPW * MS_BLOCK / 64)      // query rows of a workgroup
#define MS_STEP_WIDE_S 65536                     // from this many seeds a workgroup is 256 lanes, below it one wave: more workgroups
#define MS_MERGE_MAX_BLOCKS 1024
#define MS_DONE (-2)                             // the winner word once the walk is over

// ---- bandwidth --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MS_BLOCK) ms_select_kernel(const float* __restrict__ X, int N, int D, int pass, uint32_t rank0,
                                                             MsTarget* __restrict__ state, float* __restrict__ kth) {
    __shared__ float tile[MS_TILE_FLOATS];
    __shared__ float qs[MS_BW_Q][GP_MEANSHIFT_MAX_D];
    __shared__ uint32_t hist[MS_BW_Q][256];
    __shared__ MsTarget target[MS_BW_Q];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, LD = D | 1;
    const int q0 = blockIdx.x * MS_BW_Q;
    for (int e = t; e < MS_BW_Q * D; e += MS_BLOCK) {
        const int u = e / D, j = e - u * D;
        qs[u][j] = q0 + u < N ? X[(int64_t)(q0 + u) * D + j] : 0.0f;
    }
    for (int e = t; e < MS_BW_Q * 256; e += MS_BLOCK) hist[e >> 8][e & 255] = 0u;
    if (t < MS_BW_Q) {
        MsTarget g = {0u, rank0};
        if (pass > 0 && q0 + t < N) g = state[q0 + t];
        target[t] = g;
    }
    const int tile_rows = MS_TILE_FLOATS / LD, shift = 24 - 8 * pass;
    for (int r0 = 0; r0 < N; r0 += tile_rows) {
        const int rows = N - r0 < tile_rows ? N - r0 : tile_rows;
        __syncthreads();                                       // (the tile's readers are done; the first time: qs, hist and target are stored)
        const float* src = X + (int64_t)r0 * D;
        for (int e = t; e < rows * D; e += MS_BLOCK) {
            const int r = e / D, j = e - r * D;
            tile[r * LD + j] = src[e];
        }
        __syncthreads();
        for (int p = lane; p < rows; p += 64) {
            const float* x = tile + p * LD;
            float acc[MS_BW_QPW];
#pragma unroll
            for (int u = 0; u < MS_BW_QPW; ++u) acc[u] = 0.0f;
            for (int j = 0; j < D; ++j) {
                const float xj = x[j];
#pragma unroll
                for (int u = 0; u < MS_BW_QPW; ++u) {
                    const float d = qs[wave * MS_BW_QPW + u][j] - xj;
                    acc[u] = acc[u] + d * d;
                }
            }
#pragma unroll
            for (int u = 0; u < MS_BW_QPW; ++u) {
                const int q = wave * MS_BW_QPW + u;
                const uint32_t key = ms_key(acc[u]);
                if (q0 + q < N && ms_key_matches(key, target[q], pass)) atomicAdd(&hist[q][(key >> shift) & 255u], 1u);
            }
        }
    }
    __syncthreads();
    if (t < MS_BW_Q && q0 + t < N) {
        const MsTarget g = ms_select_step(target[t], hist[t], pass);
        state[q0 + t] = g;
        if (pass == 3) kth[q0 + t] = ms_kth_value(g);
    }
}

__global__ void __launch_bounds__(MS_BLOCK) ms_bandwidth_sum_kernel(const float* __restrict__ kth, int N, double* __restrict__ bandwidth) {
    __shared__ float buf[4 * MS_BLOCK];
    const int t = threadIdx.x;
    double sum = 0.0;
    for (int base = 0; base < N; base += 4 * MS_BLOCK) {
        const int n = N - base < 4 * MS_BLOCK ? N - base : 4 * MS_BLOCK;
        __syncthreads();
        for (int e = t; e < n; e += MS_BLOCK) buf[e] = kth[base + e];
        __syncthreads();
        if (t == 0)
            for (int e = 0; e < n; ++e) sum += (double)buf[e];
    }
    if (t == 0) *bandwidth = sum / (double)N;
}

// ---- shift ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MS_BLOCK) ms_run_init_kernel(const float* __restrict__ seeds, int S, int D, const double* __restrict__ bandwidth,
                                                               float* __restrict__ m, int32_t* __restrict__ counts, int32_t* __restrict__ its,
                                                               int32_t* __restrict__ finished, int32_t* __restrict__ status) {
    const int64_t e = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (e < (int64_t)S * D) m[e] = seeds[e];
    if (e < S) {
        counts[e] = 0;
        its[e] = 0;
        finished[e] = 0;
    }
    if (e < GP_MEANSHIFT_STATUS_WORDS)
        status[e] = e == GP_MEANSHIFT_ST_UNFINISHED ? S : e == GP_MEANSHIFT_ST_BAD_BANDWIDTH ? (ms_bandwidth_ok(*bandwidth) ? 0 : 1) : 0;
}

template <int DP>
__global__ void __launch_bounds__(MS_BLOCK) ms_step_kernel(const float* __restrict__ X, int N, int D, int S, const double* __restrict__ bandwidth,
                                                           int max_iter, float* __restrict__ m, int32_t* __restrict__ counts,
                                                           int32_t* __restrict__ its, int32_t* __restrict__ finished, int32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) float tile[MS_TILE_FLOATS];
    const int t = threadIdx.x, block = blockDim.x;
    const int64_t s = (int64_t)blockIdx.x * block + t;
    const bool mine = s < S && !finished[s];
    if (!__syncthreads_or(mine ? 1 : 0)) return;
    const double bw = *bandwidth;
    if (!ms_bandwidth_ok(bw)) return;                            // (the same for every lane; the status block says so since the init)
    const float radius2 = ms_radius2(bw);
    MsSeed<DP> seed;
    ms_seed_begin(seed);
#pragma unroll
    for (int j = 0; j < DP; ++j) seed.m[j] = (mine && j < D) ? m[s * D + j] : 0.0f;
    constexpr int TILE_ROWS = MS_TILE_FLOATS / DP;
    for (int r0 = 0; r0 < N; r0 += TILE_ROWS) {
        const int rows = N - r0 < TILE_ROWS ? N - r0 : TILE_ROWS;
        __syncthreads();
        for (int e = t; e < rows * DP; e += block) {
            const int r = e / DP, j = e % DP;
            tile[e] = j < D ? X[(int64_t)(r0 + r) * D + j] : 0.0f;
        }
        __syncthreads();
        if (mine)
            for (int p = 0; p < rows; ++p) ms_seed_point(seed, tile + p * DP, radius2);
    }
    if (!mine) return;
    int it = its[s], count;
    const bool done = ms_seed_end(seed, bw, max_iter, &it, &count);
    counts[s] = count;
    its[s] = it;
    if (count > 0) {
#pragma unroll
        for (int j = 0; j < DP; ++j)
            if (j < D) m[s * D + j] = seed.m[j];
    }
    if (done) {
        finished[s] = 1;
        atomicSub(&status[GP_MEANSHIFT_ST_UNFINISHED], 1);
        atomicMax(&status[GP_MEANSHIFT_ST_N_ITER], it);
        if (count == 0) atomicAdd(&status[GP_MEANSHIFT_ST_EMPTY], 1);
    }
}

// ---- merge ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MS_BLOCK) ms_merge_init_kernel(const int32_t* __restrict__ counts, int S, const double* __restrict__ bandwidth,
                                                                 int32_t* __restrict__ alive, int32_t* __restrict__ winner, int32_t* __restrict__ status) {
    const int64_t s = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (s < S) alive[s] = counts[s] > 0 ? 1 : 0;
    if (s == 0) {
        const bool ok = ms_bandwidth_ok(*bandwidth);
        *winner = ok ? -1 : MS_DONE;
        status[GP_MEANSHIFT_ST_KEPT] = 0;
        status[GP_MEANSHIFT_ST_OVERFLOW] = 0;
        status[GP_MEANSHIFT_ST_LIVE] = 0;
        status[GP_MEANSHIFT_ST_BAD_BANDWIDTH] = ok ? 0 : 1;
    }
}

// the better of two candidates (-1: none)
__device__ __forceinline__ int ms_better(int a, int b, const float* __restrict__ C, const int32_t* __restrict__ counts, int D) {
    if (a < 0) return b;
    if (b < 0) return a;
    return ms_precedes(counts[a], C + (int64_t)a * D, a, counts[b], C + (int64_t)b * D, b, D) ? a : b;
}

__device__ __forceinline__ int ms_block_best(int mine, int* best, const float* __restrict__ C, const int32_t* __restrict__ counts, int D) {
    const int t = threadIdx.x;
    best[t] = mine;
    __syncthreads();
    for (int off = MS_BLOCK / 2; off > 0; off >>= 1) {
        if (t < off) best[t] = ms_better(best[t], best[t + off], C, counts, D);
        __syncthreads();
    }
    return best[0];
}

__global__ void __launch_bounds__(MS_BLOCK) ms_merge_scan_kernel(const float* __restrict__ C, const int32_t* __restrict__ counts, int S, int D,
                                                                 const double* __restrict__ bandwidth, int32_t* __restrict__ alive,
                                                                 const int32_t* __restrict__ winner, int32_t* __restrict__ partial) {
    __shared__ float wc[GP_MEANSHIFT_MAX_D];
    __shared__ int best[MS_BLOCK];
    const int t = threadIdx.x, w = *winner;
    if (w == MS_DONE) return;
    const float radius2 = ms_radius2(*bandwidth);
    if (w >= 0 && t < D) wc[t] = C[(int64_t)w * D + t];
    __syncthreads();
    int b = -1;
    for (int64_t s = (int64_t)blockIdx.x * MS_BLOCK + t; s < S; s += (int64_t)gridDim.x * MS_BLOCK) {
        if (!alive[s]) continue;
        if (w >= 0 && (s == w || ms_dist2(C + s * D, wc, D) <= radius2)) {
            alive[s] = 0;
            continue;
        }
        b = ms_better(b, (int)s, C, counts, D);
    }
    b = ms_block_best(b, best, C, counts, D);
    if (t == 0) partial[blockIdx.x] = b;
}

__global__ void __launch_bounds__(MS_BLOCK) ms_merge_pick_kernel(const float* __restrict__ C, const int32_t* __restrict__ counts, int D,
                                                                 const int32_t* __restrict__ partial, int parts, int32_t* __restrict__ winner,
                                                                 float* __restrict__ centres, int32_t* __restrict__ kept_counts,
                                                                 int32_t* __restrict__ status) {
    __shared__ int best[MS_BLOCK];
    __shared__ int slot;
    const int t = threadIdx.x;
    if (*winner == MS_DONE) return;
    int b = -1;
    for (int e = t; e < parts; e += MS_BLOCK) b = ms_better(b, partial[e], C, counts, D);
    b = ms_block_best(b, best, C, counts, D);                   // (every lane has read *winner before lane 0 stores it below)
    if (t == 0) {
        int k = -1;
        if (b >= 0) {
            k = status[GP_MEANSHIFT_ST_KEPT];
            if (k >= GP_MEANSHIFT_MAX_CENTRES) {
                status[GP_MEANSHIFT_ST_OVERFLOW] = 1;
                k = -1;
            } else {
                kept_counts[k] = counts[b];
                status[GP_MEANSHIFT_ST_KEPT] = k + 1;
            }
        }
        *winner = k >= 0 ? b : MS_DONE;
        status[GP_MEANSHIFT_ST_LIVE] = k >= 0 ? 1 : 0;
        slot = k;
    }
    __syncthreads();
    if (slot >= 0 && t < D) centres[(int64_t)slot * D + t] = C[(int64_t)b * D + t];
}

// ---- the entry points ------------------------------------------------------------------------------------------------------------
struct MsBandwidthScratch {
    MsTarget* state;
    float* kth;
    size_t bytes;
    MsBandwidthScratch(void* p, int64_t N) {
        GpCarver c(p);
        state = c.take<MsTarget>((size_t)N);
        kth = c.take<float>((size_t)N);
        bytes = c.bytes();
    }
};

struct MsRunScratch {
    int32_t* finished;
    size_t bytes;
    MsRunScratch(void* p, int64_t S) {
        GpCarver c(p);
        finished = c.take<int32_t>((size_t)S);
        bytes = c.bytes();
    }
};

struct MsMergeScratch {
    int32_t *alive, *partial, *winner;
    size_t bytes;
    MsMergeScratch(void* p, int64_t S) {
        GpCarver c(p);
        alive = c.take<int32_t>((size_t)S);
        partial = c.take<int32_t>(MS_MERGE_MAX_BLOCKS);
        winner = c.take<int32_t>(1);
        bytes = c.bytes();
    }
};

static int ms_check_scratch(const char* fn, const void* scratch, int64_t have, size_t need) {
    if (!scratch) GP_FAIL("%s: null argument", fn);
    if (have < (int64_t)need) GP_FAIL("%s: scratch holds %lld bytes, %lld are needed", fn, (long long)have, (long long)need);
    if ((uintptr_t)scratch % 256) GP_FAIL("%s: scratch must be 256-byte aligned", fn);
    return 0;
}

extern "C" int gp_meanshift_abi_version(void) { return GP_MEANSHIFT_ABI_VERSION; }

extern "C" int64_t gp_meanshift_scratch_size(int64_t N, int64_t S, int64_t D) {
    const char* why = ms_size_refusal(N, S, D);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_meanshift_scratch_size: %s (N = %lld, S = %lld, D = %lld)", why, (long long)N, (long long)S,
                 (long long)D);
        return -1;
    }
    size_t need = MsBandwidthScratch(nullptr, N).bytes;
    const size_t run = MsRunScratch(nullptr, S).bytes, merge = MsMergeScratch(nullptr, S).bytes;
    if (run > need) need = run;
    if (merge > need) need = merge;
    return (int64_t)need;
}

extern "C" int gp_meanshift_bandwidth(const float* X, int64_t N, int64_t D, double quantile, double* bandwidth, float* kth, void* scratch,
                                      int64_t scratch_bytes, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = ms_size_refusal(N, 1, D);
    if (!why) why = ms_quantile_refusal(quantile);
    if (why) GP_FAIL("gp_meanshift_bandwidth: %s (N = %lld, D = %lld, quantile = %g)", why, (long long)N, (long long)D, quantile);
    if (!X || !bandwidth) GP_FAIL("gp_meanshift_bandwidth: null argument");
    MsBandwidthScratch s(scratch, N);
    if (ms_check_scratch("gp_meanshift_bandwidth", scratch, scratch_bytes, s.bytes)) return 1;
    const uint32_t rank = (uint32_t)ms_kth_rank(N, quantile);
    float* out = kth ? kth : s.kth;
    GpProfScope _p("meanshift_bandwidth", st);
    for (int pass = 0; pass < 4; ++pass)
        hipLaunchKernelGGL(ms_select_kernel, dim3(gp_blocks((size_t)N, MS_BW_Q)), dim3(MS_BLOCK), 0, st, X, (int)N, (int)D, pass, rank, s.state, out);
    hipLaunchKernelGGL(ms_bandwidth_sum_kernel, dim3(1), dim3(MS_BLOCK), 0, st, out, (int)N, bandwidth);
    GP_LAUNCH_CHECK();
    return 0;
}

template <int DP>
static void ms_launch_steps(int steps, unsigned blocks, unsigned block, hipStream_t st, const float* X, int N, int D, int S, const double* bandwidth,
                            int max_iter, float* m, int32_t* counts, int32_t* its, int32_t* finished, int32_t* status) {
    for (int k = 0; k < steps; ++k)
        hipLaunchKernelGGL(ms_step_kernel<DP>, dim3(blocks), dim3(block), 0, st, X, N, D, S, bandwidth, max_iter, m, counts, its, finished, status);
}

extern "C" int gp_meanshift_run(const float* X, int64_t N, int64_t D, const float* seeds, int64_t S, const double* bandwidth, int32_t max_iter,
                                float* seed_centers, int32_t* seed_counts, int32_t* seed_iterations, int32_t* status, void* scratch,
                                int64_t scratch_bytes, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = ms_size_refusal(N, S, D);
    if (!why) why = ms_max_iter_refusal(max_iter);
    if (why) GP_FAIL("gp_meanshift_run: %s (N = %lld, S = %lld, D = %lld, max_iter = %d)", why, (long long)N, (long long)S, (long long)D, max_iter);
    if (!X || !seeds || !bandwidth || !seed_centers || !seed_counts || !seed_iterations || !status) GP_FAIL("gp_meanshift_run: null argument");
    MsRunScratch s(scratch, S);
    if (ms_check_scratch("gp_meanshift_run", scratch, scratch_bytes, s.bytes)) return 1;
    const int n = (int)N, d = (int)D, ns = (int)S, steps = max_iter + 1;
    const unsigned block = S >= MS_STEP_WIDE_S ? MS_BLOCK : 64, blocks = gp_blocks((size_t)S, block);
    size_t init = (size_t)S * D;
    if (init < GP_MEANSHIFT_STATUS_WORDS) init = GP_MEANSHIFT_STATUS_WORDS;
    GpProfScope _p("meanshift_run", st);
    hipLaunchKernelGGL(ms_run_init_kernel, dim3(gp_blocks(init, MS_BLOCK)), dim3(MS_BLOCK), 0, st, seeds, ns, d, bandwidth, seed_centers, seed_counts,
                       seed_iterations, s.finished, status);
#define MS_STEPS(DP) ms_launch_steps<DP>(steps, blocks, block, st, X, n, d, ns, bandwidth, max_iter, seed_centers, seed_counts, seed_iterations, s.finished, status)
    switch (ms_dp(d)) {
        case 4: MS_STEPS(4); break;
        case 8: MS_STEPS(8); break;
        case 16: MS_STEPS(16); break;
        case 32: MS_STEPS(32); break;
        default: MS_STEPS(64); break;
    }
#undef MS_STEPS
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_meanshift_merge(const float* seed_centers, const int32_t* seed_counts, int64_t S, int64_t D, const double* bandwidth,
                                  int32_t first, int32_t rounds, float* centres, int32_t* counts, int32_t* status, void* scratch,
                                  int64_t scratch_bytes, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = ms_size_refusal(1, S, D);
    if (!why) why = ms_rounds_refusal(rounds);
    if (why) GP_FAIL("gp_meanshift_merge: %s (S = %lld, D = %lld, rounds = %d)", why, (long long)S, (long long)D, rounds);
    if (!seed_centers || !seed_counts || !bandwidth || !centres || !counts || !status) GP_FAIL("gp_meanshift_merge: null argument");
    MsMergeScratch s(scratch, S);
    if (ms_check_scratch("gp_meanshift_merge", scratch, scratch_bytes, s.bytes)) return 1;
    const int ns = (int)S, d = (int)D;
    unsigned parts = gp_blocks((size_t)S, MS_BLOCK);
    if (parts > MS_MERGE_MAX_BLOCKS) parts = MS_MERGE_MAX_BLOCKS;
    GpProfScope _p("meanshift_merge", st);
    if (first) hipLaunchKernelGGL(ms_merge_init_kernel, dim3(gp_blocks((size_t)S, MS_BLOCK)), dim3(MS_BLOCK), 0, st, seed_counts, ns, bandwidth, s.alive, s.winner, status);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(ms_merge_scan_kernel, dim3(parts), dim3(MS_BLOCK), 0, st, seed_centers, seed_counts, ns, d, bandwidth, s.alive, s.winner, s.partial);
        hipLaunchKernelGGL(ms_merge_pick_kernel, dim3(1), dim3(MS_BLOCK), 0, st, seed_centers, seed_counts, d, s.partial, (int)parts, s.winner, centres, counts, status);
    }
    GP_LAUNCH_CHECK();
    return 0;
}
