// knn_kernels.hip -- general k-nearest-neighbour search (pytorch3d's knn_points, frnn's frnn_grid_points, pointops' knnquery) and
// batched furthest-point sampling (pointops' furthestsampling_cuda) [REF scene/gaussian_model.py:28-30, 113-117, 208;
// utils/loss_utils.py:36, 43; utils/fps.py:71-88].  DESIGN.md section "General kNN".
//
// gp_knn_points: queries p1[B,P1,D] against candidates p2[B,P2,D], exact brute force, the K nearest sorted by (distance, index).
//   * One query per lane; its top-K list lives in registers.  The list size KB is a compile-time bucket (1, 2, 4, 8, 16, 32 >= K): a
//     run-time `best_d[K - 1]` would put the list in scratch memory.  Candidates are offered in ascending index order and enter only if
//     STRICTLY nearer than the current KB-th, at the first place whose distance they beat, so equal distances keep the lower index
//     first: the list is the KB smallest (distance, index) pairs in lexicographic order.
//   * Candidates stream through LDS in tiles, stored dimension-major: every lane of the workgroup reads the same candidate (broadcast).
//   * Distances: sum over the dimensions IN ORDER of (x - y)^2 (norm 2) or |x - y| (norm 1), no inner-product expansion (coincident
//     points stay at exactly 0).  The build compiles with -ffp-contract=off, so no fused multiply-add changes the rounding.
//   * Two regimes, chosen on the host by the number of workgroups the queries alone fill.  Many queries (1e6 x 512): one workgroup per
//     256 queries walks all candidates and writes the result.  Few queries against many candidates (300 x 1e6): the candidate range is
//     cut into `splits` contiguous pieces, one workgroup per (256 queries, piece); each writes its sorted partial top-K to scratch and
//     gp_knnp_merge_kernel combines the pieces of a query with the same lexicographic rule.  The top-K of a union is the top-K of the
//     pieces' top-Ks, and every distance is computed by the same instructions whichever piece holds it, so the result is bit-identical
//     for every split count.
#include <math.h>

#include <algorithm>

#include "gp_common.h"

#define KNNP_MAX_K 32
#define KNNP_MAX_D 64
#define KNNP_EMPTY 0x7fffffff          // index of an empty slot in the scratch lists (sorts after every real candidate)

// candidates staged per tile: 16 KB of LDS at most
template <int DMAX>
struct KnnpTile { static constexpr int value = DMAX <= 16 ? 256 : 4096 / DMAX; };

// (da, ia) before (db, ib) in the result order
__device__ __forceinline__ bool knnp_before(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

template <int DMAX, int KB, int NORM>
__global__ __launch_bounds__(256) void gp_knnp_kernel(long P1, long P2, int D, const float* __restrict__ p1, const float* __restrict__ p2,
                                                     const int64_t* __restrict__ len1, const int64_t* __restrict__ len2, int K,
                                                     long chunk, float r2_max, int64_t pad_idx, float pad_dist,
                                                     float* __restrict__ dists, int64_t* __restrict__ idx, float* __restrict__ part_d,
                                                     int32_t* __restrict__ part_i) {
    constexpr int TILE = KnnpTile<DMAX>::value;
    __shared__ float s_c[DMAX][TILE];
    const int tid = threadIdx.x;
    const long b = blockIdx.z, split = blockIdx.y, splits = gridDim.y;
    const long q = (long)blockIdx.x * 256 + tid;
    const long n1 = len1 ? min(max(len1[b], (int64_t)0), (int64_t)P1) : P1;
    const long n2 = len2 ? min(max(len2[b], (int64_t)0), (int64_t)P2) : P2;
    const bool live = q < n1;
    const long c0 = split * chunk;
    // a workgroup whose queries are all padding rows skips the candidates (uniform: every thread takes the same branch)
    const long c1 = (long)blockIdx.x * 256 < n1 ? min(c0 + chunk, n2) : c0;
    const int Dn = DMAX == 3 ? 3 : D;

    float x[DMAX];
    const float* qrow = p1 + ((size_t)b * P1 + (live ? q : 0)) * Dn;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) x[d] = (d < Dn && live) ? qrow[d] : 0.f;

    float best_d[KB];
    int best_i[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) { best_d[k] = INFINITY; best_i[k] = KNNP_EMPTY; }

    const float* cand = p2 + (size_t)b * P2 * Dn;
    for (long t0 = c0; t0 < c1; t0 += TILE) {
        const int cnt = (int)min((long)TILE, c1 - t0);
        __syncthreads();
        for (int e = tid; e < TILE * Dn; e += 256) {                     // coalesced rows -> dimension-major tile
            const int j = e / Dn, d = e - j * Dn;
            s_c[d][j] = j < cnt ? cand[(size_t)(t0 + j) * Dn + d] : 0.f;
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < DMAX; ++d) {
                if (DMAX == 3 || d < Dn) {                               // (uniform: D is a kernel argument)
                    const float df = x[d] - s_c[d][j];
                    s = NORM == 2 ? s + df * df : s + fabsf(df);
                }
            }
            if (s < best_d[KB - 1]) {
                // insert at the first place it beats; everything behind moves down one (ties keep the earlier, lower index first)
                float cd = s;
                int ci = (int)(t0 + j);
                bool take = false;
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    take = take || cd < best_d[k];
                    const float td = best_d[k];
                    const int ti = best_i[k];
                    if (take) { best_d[k] = cd; best_i[k] = ci; cd = td; ci = ti; }
                }
            }
        }
    }

    if (splits == 1) {
        if (q < P1) {
            float* od = dists + ((size_t)b * P1 + q) * K;
            int64_t* oi = idx + ((size_t)b * P1 + q) * K;
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                if (k < K) {
                    const bool real = live && best_i[k] != KNNP_EMPTY && best_d[k] <= r2_max;
                    od[k] = real ? best_d[k] : pad_dist;
                    oi[k] = real ? (int64_t)best_i[k] : pad_idx;
                }
            }
        }
    } else if (live) {
        const size_t base = (((size_t)b * P1 + q) * splits + split) * K;
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            if (k < K) { part_d[base + k] = best_d[k]; part_i[base + k] = best_i[k]; }
        }
    }
}

// merge two sorted K-lists (a: LDS or global, b: LDS or global) into registers, then store into o (LDS)
template <int KB>
__device__ __forceinline__ void knnp_merge2(const float* ad, const int* ai, const float* bd, const int* bi, int K, float* od, int* oi) {
    float rd[KB];
    int ri[KB];
    int ia = 0, ib = 0;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        if (k < K) {
            const float da = ia < K ? ad[ia] : INFINITY, db = ib < K ? bd[ib] : INFINITY;
            const int xa = ia < K ? ai[ia] : KNNP_EMPTY, xb = ib < K ? bi[ib] : KNNP_EMPTY;
            const bool ta = !knnp_before(db, xb, da, xa);               // (a real entry never equals another in both keys)
            rd[k] = ta ? da : db;
            ri[k] = ta ? xa : xb;
            ia += ta ? 1 : 0;
            ib += ta ? 0 : 1;
        }
    }
#pragma unroll
    for (int k = 0; k < KB; ++k)
        if (k < K) { od[k] = rd[k]; oi[k] = ri[k]; }
}

// one wave per query: lane l folds the pieces l, l + 64, ... into row l of LDS, then a pairwise tree over the rows
template <int KB>
__global__ __launch_bounds__(64) void gp_knnp_merge_kernel(long P1, const int64_t* __restrict__ len1, int K, int splits,
                                                           const float* __restrict__ part_d, const int32_t* __restrict__ part_i,
                                                           float r2_max, int64_t pad_idx, float pad_dist, float* __restrict__ dists,
                                                           int64_t* __restrict__ idx) {
    __shared__ float s_d[64][KB];
    __shared__ int s_i[64][KB];
    const int lane = threadIdx.x;
    const long row = blockIdx.x;                                         // b * P1 + q
    const long b = row / P1, q = row - b * P1;
    const long n1 = len1 ? min(max(len1[b], (int64_t)0), (int64_t)P1) : P1;
    float* od = dists + (size_t)row * K;
    int64_t* oi = idx + (size_t)row * K;
    if (q >= n1) {                                                       // padding row: its pieces were never written
        for (int k = lane; k < K; k += 64) { od[k] = pad_dist; oi[k] = pad_idx; }
        return;
    }
    for (int k = 0; k < K; ++k) { s_d[lane][k] = INFINITY; s_i[lane][k] = KNNP_EMPTY; }
    const size_t base = (size_t)row * splits * K;
    for (int s = lane; s < splits; s += 64)
        knnp_merge2<KB>(s_d[lane], s_i[lane], part_d + base + (size_t)s * K, part_i + base + (size_t)s * K, K, s_d[lane], s_i[lane]);
    for (int w = 1; w < 64 && w < splits; w *= 2) {
        __syncthreads();
        if ((lane & (2 * w - 1)) == 0 && lane + w < 64)
            knnp_merge2<KB>(s_d[lane], s_i[lane], s_d[lane + w], s_i[lane + w], K, s_d[lane], s_i[lane]);
    }
    __syncthreads();
    for (int k = lane; k < K; k += 64) {
        const float d = s_d[0][k];
        const int i = s_i[0][k];
        const bool real = i != KNNP_EMPTY && d <= r2_max;
        od[k] = real ? d : pad_dist;
        oi[k] = real ? (int64_t)i : pad_idx;
    }
}

template <int DMAX, int KB>
static void launch_knnp(int norm, dim3 grid, hipStream_t s, long P1, long P2, int D, const float* p1, const float* p2, const int64_t* l1,
                        const int64_t* l2, int K, long chunk, float r2_max, int64_t pad_idx, float pad_dist, float* dists, int64_t* idx,
                        float* part_d, int32_t* part_i) {
    if (norm == 2)
        hipLaunchKernelGGL((gp_knnp_kernel<DMAX, KB, 2>), grid, dim3(256), 0, s, P1, P2, D, p1, p2, l1, l2, K, chunk, r2_max, pad_idx,
                           pad_dist, dists, idx, part_d, part_i);
    else
        hipLaunchKernelGGL((gp_knnp_kernel<DMAX, KB, 1>), grid, dim3(256), 0, s, P1, P2, D, p1, p2, l1, l2, K, chunk, r2_max, pad_idx,
                           pad_dist, dists, idx, part_d, part_i);
}

template <int DMAX>
static void launch_knnp_k(int kb, int norm, dim3 grid, hipStream_t s, long P1, long P2, int D, const float* p1, const float* p2,
                          const int64_t* l1, const int64_t* l2, int K, long chunk, float r2_max, int64_t pad_idx, float pad_dist,
                          float* dists, int64_t* idx, float* part_d, int32_t* part_i) {
#define KNNP_CASE(KBV) case KBV: launch_knnp<DMAX, KBV>(norm, grid, s, P1, P2, D, p1, p2, l1, l2, K, chunk, r2_max, pad_idx, pad_dist, \
                                                        dists, idx, part_d, part_i); break;
    switch (kb) { KNNP_CASE(1) KNNP_CASE(2) KNNP_CASE(4) KNNP_CASE(8) KNNP_CASE(16) KNNP_CASE(32) }
#undef KNNP_CASE
}

static int knnp_bucket(int K) { int kb = 1; while (kb < K) kb *= 2; return kb; }

// automatic split count: enough workgroups to cover the chip ~4 times, pieces of at least 512 candidates, scratch <= 256 MB
static long knnp_auto_splits(long B, long P1, long P2, int K) {
    const long qblocks = B * ((P1 + 255) / 256);
    const long target = 1024;
    if (qblocks >= target / 2) return 1;
    long s = (target + qblocks - 1) / qblocks;
    s = std::min(s, std::max(1L, P2 / 512));
    const long cap = (256L << 20) / std::max(1L, B * P1 * K * 8);
    return std::max(1L, std::min(s, cap));
}

extern "C" int gp_knn_points(int64_t B, int64_t P1, int64_t P2, int32_t D, const float* p1, const float* p2, const int64_t* lengths1,
                             const int64_t* lengths2, int32_t K, int32_t norm, float r2_max, int32_t splits, int64_t pad_idx, float pad_dist,
                             float* dists, int64_t* idx, gp_alloc_fn alloc, void* alloc_ctx, gp_stream_t stream_) {
    if (B < 0 || P1 < 0 || P2 < 0) GP_FAIL("gp_knn_points: negative size");
    if (B > 65535 || P1 > 0x7FFFFFF0LL || P2 > 0x7FFFFFF0LL) GP_FAIL("gp_knn_points: need B <= 65535 and P1, P2 < 2^31");
    if (K < 1 || K > KNNP_MAX_K) GP_FAIL("gp_knn_points: K = %d unsupported (1..%d)", K, KNNP_MAX_K);
    if (D < 1 || D > KNNP_MAX_D) GP_FAIL("gp_knn_points: D = %d unsupported (1..%d)", D, KNNP_MAX_D);
    if (norm != 1 && norm != 2) GP_FAIL("gp_knn_points: norm must be 1 or 2, got %d", norm);
    if (splits < 0 || splits > 65535) GP_FAIL("gp_knn_points: splits must be 0 (automatic) .. 65535, got %d", splits);
    if (B == 0 || P1 == 0) return 0;
    if (!p1 || !dists || !idx || (P2 > 0 && !p2)) GP_FAIL("gp_knn_points: null argument");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope _p("knn_points", s);
    const long ns = P2 == 0 ? 1 : (splits > 0 ? splits : knnp_auto_splits(B, P1, P2, K));
    const long chunk = ns == 1 ? P2 : (P2 + ns - 1) / ns;
    float* part_d = nullptr;
    int32_t* part_i = nullptr;
    if (ns > 1) {
        if (!alloc) GP_FAIL("gp_knn_points: split search needs the allocator");
        GpCarver c(nullptr);
        c.take<float>((size_t)B * P1 * ns * K);
        c.take<int32_t>((size_t)B * P1 * ns * K);
        void* mem = alloc(alloc_ctx, GP_BUF_TEMP, c.bytes());
        if (!mem) GP_FAIL("allocator returned NULL for TEMP");
        GpCarver c2(mem);
        part_d = c2.take<float>((size_t)B * P1 * ns * K);
        part_i = c2.take<int32_t>((size_t)B * P1 * ns * K);
    }
    const int kb = knnp_bucket(K);
    const dim3 grid(gp_blocks((size_t)P1, 256), (unsigned)ns, (unsigned)B);
    const int dmax = D == 3 ? 3 : D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64;
    switch (dmax) {
    case 3: launch_knnp_k<3>(kb, norm, grid, s, P1, P2, D, p1, p2, lengths1, lengths2, K, chunk, r2_max, pad_idx, pad_dist, dists, idx, part_d, part_i); break;
    case 8: launch_knnp_k<8>(kb, norm, grid, s, P1, P2, D, p1, p2, lengths1, lengths2, K, chunk, r2_max, pad_idx, pad_dist, dists, idx, part_d, part_i); break;
    case 16: launch_knnp_k<16>(kb, norm, grid, s, P1, P2, D, p1, p2, lengths1, lengths2, K, chunk, r2_max, pad_idx, pad_dist, dists, idx, part_d, part_i); break;
    case 32: launch_knnp_k<32>(kb, norm, grid, s, P1, P2, D, p1, p2, lengths1, lengths2, K, chunk, r2_max, pad_idx, pad_dist, dists, idx, part_d, part_i); break;
    default: launch_knnp_k<64>(kb, norm, grid, s, P1, P2, D, p1, p2, lengths1, lengths2, K, chunk, r2_max, pad_idx, pad_dist, dists, idx, part_d, part_i); break;
    }
    GP_LAUNCH_CHECK();
    if (ns > 1) {
        const unsigned rows = (unsigned)(B * P1);
#define KNNP_MERGE(KBV) case KBV: hipLaunchKernelGGL((gp_knnp_merge_kernel<KBV>), dim3(rows), dim3(64), 0, s, (long)P1, lengths1, (int)K, \
                                                     (int)ns, (const float*)part_d, (const int32_t*)part_i, r2_max, pad_idx, pad_dist, dists, idx); break;
        switch (kb) { KNNP_MERGE(1) KNNP_MERGE(2) KNNP_MERGE(4) KNNP_MERGE(8) KNNP_MERGE(16) KNNP_MERGE(32) }
#undef KNNP_MERGE
        GP_LAUNCH_CHECK();
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Backward of the distances: one thread per query row.  grad_p1 is owned by the row (plain adds), grad_p2 is shared (atomics).
// d dist / d p1 = 2 (p1 - p2) (norm 2), sign(p1 - p2) (norm 1); d dist / d p2 = its negative.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gp_knnp_bwd_kernel(long B, long P1, long P2, int D, const float* __restrict__ p1,
                                                         const float* __restrict__ p2, const int64_t* __restrict__ len1,
                                                         const int64_t* __restrict__ len2, const int64_t* __restrict__ idx, int K, int norm,
                                                         const float* __restrict__ grad_dists, float* __restrict__ grad_p1,
                                                         float* __restrict__ grad_p2) {
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= B * P1) return;
    const long b = row / P1, q = row - b * P1;
    const long n1 = len1 ? min(max(len1[b], (int64_t)0), (int64_t)P1) : P1;
    const long n2 = len2 ? min(max(len2[b], (int64_t)0), (int64_t)P2) : P2;
    if (q >= n1) return;
    const float* x = p1 + (size_t)row * D;
    const int64_t* ri = idx + (size_t)row * K;
    const float* g = grad_dists + (size_t)row * K;
    for (int d = 0; d < D; ++d) {
        float acc = 0.f;
        for (int k = 0; k < K; ++k) {
            const int64_t j = ri[k];
            if (j < 0 || j >= n2) continue;                             // padding
            const float df = x[d] - p2[((size_t)b * P2 + j) * D + d];
            const float gd = norm == 2 ? 2.f * df * g[k] : (df > 0.f ? g[k] : df < 0.f ? -g[k] : 0.f);
            acc += gd;
            if (grad_p2) atomicAdd(grad_p2 + ((size_t)b * P2 + j) * D + d, -gd);
        }
        if (grad_p1) grad_p1[(size_t)row * D + d] += acc;
    }
}

extern "C" int gp_knn_points_backward(int64_t B, int64_t P1, int64_t P2, int32_t D, const float* p1, const float* p2, const int64_t* lengths1,
                                      const int64_t* lengths2, const int64_t* idx, int32_t K, int32_t norm, const float* grad_dists,
                                      float* grad_p1, float* grad_p2, gp_stream_t stream_) {
    if (B < 0 || P1 < 0 || P2 < 0) GP_FAIL("gp_knn_points_backward: negative size");
    if (K < 1 || K > KNNP_MAX_K || D < 1 || D > KNNP_MAX_D || (norm != 1 && norm != 2))
        GP_FAIL("gp_knn_points_backward: K 1..%d, D 1..%d, norm 1 or 2", KNNP_MAX_K, KNNP_MAX_D);
    if (B * P1 == 0 || (!grad_p1 && !grad_p2)) return 0;
    if (!p1 || !p2 || !idx || !grad_dists) GP_FAIL("gp_knn_points_backward: null argument");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope _p("knn_points_bwd", s);
    hipLaunchKernelGGL(gp_knnp_bwd_kernel, dim3(gp_blocks((size_t)(B * P1), 256)), dim3(256), 0, s, (long)B, (long)P1, (long)P2, (int)D, p1, p2,
                       lengths1, lengths2, idx, (int)K, (int)norm, grad_dists, grad_p1, grad_p2);
    GP_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Batched furthest-point sampling (pointops' furthestsampling_cuda semantics): batch i holds the points [offset[i-1], offset[i]) and
// receives the samples [new_offset[i-1], new_offset[i]); every batch starts at its own first point; indices are global.  One workgroup
// per batch runs exactly the selection of gp_fps_kernel (csrc/weights_kernels.hip): the same distance arithmetic, the first maximum
// on ties, so batch 0 of a one-batch call is bit-identical to gp_furthest_point_sampling.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void gp_fps_batched_kernel(const int32_t* __restrict__ offset, const int32_t* __restrict__ new_offset,
                                                               long n_total, long m_total, const float* __restrict__ xyz,
                                                               float* __restrict__ dist, int32_t* __restrict__ idx) {
    __shared__ float s_far_d2[16];
    __shared__ int s_far_id[16];
    __shared__ int s_sel;
    const int bid = blockIdx.x;
    const long start_n = bid ? offset[bid - 1] : 0, end_n = offset[bid];
    const long start_m = bid ? new_offset[bid - 1] : 0, end_m = new_offset[bid];
    // malformed offsets (decreasing, or beyond the buffers the host sized): the batch is skipped, nothing is read or written out of range
    if (start_n < 0 || end_n <= start_n || end_n > n_total || start_m < 0 || end_m <= start_m || end_m > m_total) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long k = start_n + tid; k < end_n; k += 1024) dist[k] = 1e10f;
    if (tid == 0) { idx[start_m] = (int32_t)start_n; s_sel = (int)start_n; }
    __syncthreads();
    for (long j = start_m + 1; j < end_m; ++j) {
        const int cur = s_sel;
        const float cx = xyz[3 * (size_t)cur], cy = xyz[3 * (size_t)cur + 1], cz = xyz[3 * (size_t)cur + 2];
        float far_d2 = -1.f;
        int far_id = 0x7fffffff;
        for (long k = start_n + tid; k < end_n; k += 1024) {
            const float dx = xyz[3 * k] - cx, dy = xyz[3 * k + 1] - cy, dz = xyz[3 * k + 2] - cz;
            const float d = fminf(dx * dx + dy * dy + dz * dz, dist[k]);
            dist[k] = d;
            if (d > far_d2) { far_d2 = d; far_id = (int)k; }
        }
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {
            const float o_d2 = __shfl_xor(far_d2, dd);
            const int o_id = __shfl_xor(far_id, dd);
            if (o_d2 > far_d2 || (o_d2 == far_d2 && o_id < far_id)) { far_d2 = o_d2; far_id = o_id; }
        }
        __syncthreads();
        if (lane == 0) { s_far_d2[wave] = far_d2; s_far_id[wave] = far_id; }
        __syncthreads();
        if (tid == 0) {
            float bd = s_far_d2[0];
            int bi = s_far_id[0];
            for (int w = 1; w < 16; ++w)
                if (s_far_d2[w] > bd || (s_far_d2[w] == bd && s_far_id[w] < bi)) { bd = s_far_d2[w]; bi = s_far_id[w]; }
            if (bi < start_n || bi >= end_n) bi = (int)start_n;       // (only if every distance is NaN: never read outside the batch)
            idx[j] = bi;
            s_sel = bi;
        }
        __syncthreads();
    }
}

extern "C" int gp_furthest_point_sampling_batched(int32_t b, const int32_t* offset, const int32_t* new_offset, int64_t n_total,
                                                  int64_t m_total, const float* xyz, float* tmp, int32_t* idx, gp_stream_t stream_) {
    if (b < 0 || n_total < 0 || n_total > 0x7FFFFFF0LL || m_total < 0) GP_FAIL("gp_furthest_point_sampling_batched: need b >= 0, 0 <= n_total < 2^31, m_total >= 0");
    if (b == 0 || m_total == 0) return 0;
    if (!offset || !new_offset || !xyz || !tmp || !idx) GP_FAIL("gp_furthest_point_sampling_batched: null argument");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope _p("fps_batched", s);
    hipLaunchKernelGGL(gp_fps_batched_kernel, dim3((unsigned)b), dim3(1024), 0, s, offset, new_offset, (long)n_total, (long)m_total, xyz, tmp, idx);
    GP_LAUNCH_CHECK();
    return 0;
}
