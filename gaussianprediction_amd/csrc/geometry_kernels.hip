// geometry_kernels.hip -- surface samples, an exact nearest neighbour on a uniform grid and the distance table of two clouds on the
// device (csrc/gp_geometry.h).  The programs of a lane are csrc/geometry_core.h, which also runs on a CPU (tests/geometry_emulate.cpp).
//   gm_area_kernel         a lane per face by grid stride: its class and float64 area; the classes tallied by wave ballots, the largest
//                          area by a 64-bit integer maximum of its bits, both once per workgroup and word
//   gm_weight_kernel       a workgroup per 1024 faces: the integer weights and their sum
//   gm_scan_sums_kernel    ONE workgroup: the exclusive scan of the tile sums (uint64 for the faces, uint32 for the cells), the total,
//                          and for the faces T, q and the refusal
//   gm_prefix_kernel       a workgroup per tile: the scan inside the tile plus the tile's offset (inclusive for the faces, exclusive
//                          for the cells, which also leaves a copy for the scatter's cursors)
//   gm_sample_kernel, gm_interpolate_kernel      a lane per sample: a binary search over the prefix, then 24-bit barycentrics
//   gm_bounds_kernel       a lane per point by grid stride: integer minima and maxima of order-preserving bits, once per workgroup
//   gm_derive_kernel       one lane: the grid record, so the host reads nothing
//   gm_count_kernel, gm_scatter_kernel           a lane per point: one integer atomic add on its cell each; 16-byte records out
//   gm_query_kernel        a lane per query by grid stride: the rings are a divergent per-lane loop on purpose (neighbouring queries
//                          are not neighbouring lanes; sorting them is DESIGN section 30's follow-up); a candidate is one dwordx4
//   gm_metric_kernel, gm_metric_final_kernel     gp_depth_metrics' reduction in float64: a fixed tree, plain slots, one workgroup last
// No float atomics, no spinning, no fence: everything crosses launch boundaries, and nothing is read by the host in between.
#include "gp_common.h"

#include "geometry_core.h"

static_assert(GM_BLOCK == 4 * GP_WAVE, "four waves a workgroup");

// ---- workgroup helpers ----
template <typename T>
__device__ __forceinline__ T gm_wave_sum(T v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}
// the sum over the workgroup, in every lane; s: [GM_BLOCK / GP_WAVE]
template <typename T>
__device__ __forceinline__ T gm_block_sum(T v, T* s) {
    v = gm_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s[0] + s[1]) + (s[2] + s[3]);
}
// the exclusive scan over the workgroup's lanes; s: [GM_BLOCK]; *total: the sum
template <typename T>
__device__ __forceinline__ T gm_block_scan(T v, T* s, T* total) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < GM_BLOCK; d <<= 1) {
        const T add = tid >= d ? s[tid - d] : (T)0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    *total = s[GM_BLOCK - 1];
    return s[tid] - v;
}

// ---- samples ----
__global__ void __launch_bounds__(GM_BLOCK) gm_area_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                           double* __restrict__ areas, unsigned long long* max_bits, int32_t* counts) {
    __shared__ unsigned long long s_max[GM_BLOCK / GP_WAVE];
    __shared__ int32_t s_tally[GM_BLOCK / GP_WAVE][2];
    int32_t bad = 0, nonfinite = 0;                  // of this wave
    unsigned long long best = 0ull;
    const uint32_t stride = gridDim.x * GM_BLOCK;    // (nf < 2^26: no wrap)
    for (uint32_t first = blockIdx.x * GM_BLOCK; first < nf; first += stride) {
        const uint32_t f = first + threadIdx.x;
        int what = -1;
        if (f < nf) {
            double a;
            what = gm_face_area(vertices, faces, f, nv, &a);
            areas[f] = what == GM_FACE_OK ? a : -1.0;
            if (what == GM_FACE_OK && gm_double_bits(a) > best) best = gm_double_bits(a);
        }
        bad += (int32_t)__popcll(__ballot(what == GM_FACE_BAD_INDEX));
        nonfinite += (int32_t)__popcll(__ballot(what == GM_FACE_NON_FINITE));
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { const unsigned long long o = __shfl_xor(best, s); best = o > best ? o : best; }
    if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = best; s_tally[threadIdx.x >> 6][0] = bad; s_tally[threadIdx.x >> 6][1] = nonfinite; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = s_max[0];
        for (int w = 1; w < GM_BLOCK / GP_WAVE; ++w) m = s_max[w] > m ? s_max[w] : m;
        if (m != 0ull) atomicMax(max_bits, m);
    }
    if (threadIdx.x >= 1 && threadIdx.x <= 2) {
        int32_t sum = 0;
        for (int w = 0; w < GM_BLOCK / GP_WAVE; ++w) sum += s_tally[w][threadIdx.x - 1];
        if (sum != 0) atomicAdd(counts + (threadIdx.x == 1 ? GP_GEOMETRY_BAD_INDEX : GP_GEOMETRY_NON_FINITE), sum);
    }
}

// areas and weights share one array: a workgroup reads its tile's areas and leaves its weights
__global__ void __launch_bounds__(GM_BLOCK) gm_weight_kernel(uint64_t* __restrict__ prefix, uint32_t nf, const unsigned long long* __restrict__ max_bits,
                                                             uint64_t* __restrict__ sums, int32_t* counts) {
    __shared__ uint64_t s_sum[GM_BLOCK / GP_WAVE];
    __shared__ uint64_t s_zero[GM_BLOCK / GP_WAVE];
    const double scale = gm_scale(*max_bits);
    uint64_t sum = 0, zero = 0;
#pragma unroll
    for (int u = 0; u < GM_PER_LANE; ++u) {
        const uint32_t f = blockIdx.x * GM_TILE + threadIdx.x * GM_PER_LANE + u;
        if (f < nf) {
            const double a = gm_bits_double(prefix[f]);
            const uint64_t w = a > 0.0 ? gm_weight(a, scale) : 0;
            prefix[f] = w;
            sum += w;
            zero += (a >= 0.0 && w == 0) ? 1 : 0;
        }
    }
    sum = gm_block_sum(sum, s_sum);
    zero = gm_block_sum(zero, s_zero);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = sum;
        if (zero != 0) atomicAdd(counts + GP_GEOMETRY_ZERO_WEIGHT, (int32_t)zero);
    }
}

template <typename T>
__device__ __forceinline__ T gm_scan_sums(T* sums, uint32_t tiles, T* s) {
    T carry = 0;
    for (uint32_t first = 0; first < tiles; first += GM_BLOCK) {          // (the same trips for the whole workgroup)
        const uint32_t k = first + threadIdx.x;
        const T v = k < tiles ? sums[k] : (T)0;
        T total;
        const T before = gm_block_scan(v, s, &total);
        if (k < tiles) sums[k] = carry + before;
        carry += total;
    }
    return carry;
}

__global__ void __launch_bounds__(GM_BLOCK) gm_scan_sums_u64_kernel(uint64_t* sums, uint32_t tiles, int64_t n, GmSampleHead* head, int32_t* counts) {
    __shared__ uint64_t s[GM_BLOCK];
    const uint64_t total = gm_scan_sums(sums, tiles, s);
    if (threadIdx.x == 0) {
        const GmSampleHead h = gm_sample_head(total, n);
        *head = h;
        counts[GP_GEOMETRY_STATUS] = h.status;
    }
}

__global__ void __launch_bounds__(GM_BLOCK) gm_scan_sums_u32_kernel(uint32_t* sums, uint32_t tiles) {
    __shared__ uint32_t s[GM_BLOCK];
    gm_scan_sums(sums, tiles, s);
}

__global__ void __launch_bounds__(GM_BLOCK) gm_tile_sum_u32_kernel(const uint32_t* __restrict__ data, uint32_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_sum[GM_BLOCK / GP_WAVE];
    uint32_t sum = 0;
#pragma unroll
    for (int u = 0; u < GM_PER_LANE; ++u) {
        const uint32_t k = blockIdx.x * GM_TILE + threadIdx.x * GM_PER_LANE + u;
        if (k < n) sum += data[k];
    }
    sum = gm_block_sum(sum, s_sum);
    if (threadIdx.x == 0) sums[blockIdx.x] = sum;
}

// data[k] = the tile's offset + the scan inside the tile: inclusive, or exclusive with a copy to `copy`
template <typename T, bool INCLUSIVE>
__global__ void __launch_bounds__(GM_BLOCK) gm_prefix_kernel(T* __restrict__ data, uint32_t n, const T* __restrict__ sums, T* __restrict__ copy) {
    __shared__ T s[GM_BLOCK];
    const uint32_t base = blockIdx.x * GM_TILE + threadIdx.x * GM_PER_LANE;
    T v[GM_PER_LANE], mine = 0;
#pragma unroll
    for (int u = 0; u < GM_PER_LANE; ++u) { v[u] = base + u < n ? data[base + u] : (T)0; mine += v[u]; }
    T total;
    T run = sums[blockIdx.x] + gm_block_scan(mine, s, &total);
#pragma unroll
    for (int u = 0; u < GM_PER_LANE; ++u) {
        const T out = INCLUSIVE ? run + v[u] : run;
        run += v[u];
        if (base + u < n) {
            data[base + u] = out;
            if (copy) copy[base + u] = out;
        }
    }
}

__global__ void __launch_bounds__(GM_BLOCK) gm_sample_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                             const uint64_t* __restrict__ prefix, const GmSampleHead* __restrict__ head, uint64_t seed, uint32_t n,
                                                             float* __restrict__ points, int32_t* __restrict__ face, float* __restrict__ bary) {
    const uint32_t i = blockIdx.x * GM_BLOCK + threadIdx.x;
    if (i >= n) return;
    gm_sample(vertices, faces, nv, nf, prefix, *head, seed, i, points, face, bary);
}

__global__ void __launch_bounds__(GM_BLOCK) gm_interpolate_kernel(const float* __restrict__ attributes, int32_t C, const int32_t* __restrict__ faces, uint32_t nv,
                                                                  uint32_t nf, const int32_t* __restrict__ face, const float* __restrict__ bary, uint32_t n,
                                                                  float* __restrict__ out) {
    const uint32_t i = blockIdx.x * GM_BLOCK + threadIdx.x;
    if (i >= n) return;
    gm_interpolate(attributes, C, faces, nv, nf, face, bary, i, out);
}

// ---- the grid ----
// words: lo[3] (start at all ones), hi[3], usable (start at 0)
__global__ void __launch_bounds__(GM_BLOCK) gm_bounds_kernel(const float* __restrict__ points, uint32_t np, uint32_t* words) {
    __shared__ uint32_t s_red[GM_BLOCK / GP_WAVE][7];
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u}, usable = 0;
    const uint32_t stride = gridDim.x * GM_BLOCK;
    for (uint32_t first = blockIdx.x * GM_BLOCK; first < np; first += stride) {          // (np < 2^31, stride <= 2^19: no wrap)
        const uint32_t j = first + threadIdx.x;
        bool ok = false;
        if (j < np) {
            const float p[3] = {points[3 * (size_t)j], points[3 * (size_t)j + 1], points[3 * (size_t)j + 2]};
            ok = gm_usable(p);
            if (ok)
                for (int a = 0; a < 3; ++a) {
                    const uint32_t o = gm_ordered(p[a] + 0.f);
                    lo[a] = o < lo[a] ? o : lo[a];
                    hi[a] = o > hi[a] ? o : hi[a];
                }
        }
        usable += (uint32_t)__popcll(__ballot(ok));          // (of this wave)
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
        for (int a = 0; a < 3; ++a) {
            const uint32_t l = __shfl_xor(lo[a], s), h = __shfl_xor(hi[a], s);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) { s_red[threadIdx.x >> 6][a] = lo[a]; s_red[threadIdx.x >> 6][3 + a] = hi[a]; }
        s_red[threadIdx.x >> 6][6] = usable;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int k = threadIdx.x;
        uint32_t v = s_red[0][k];
        for (int w = 1; w < GM_BLOCK / GP_WAVE; ++w) {
            const uint32_t o = s_red[w][k];
            v = k < 3 ? (o < v ? o : v) : (k < 6 ? (o > v ? o : v) : v + o);
        }
        if (k < 3) atomicMin(words + k, v);
        else if (k < 6) atomicMax(words + k, v);
        else if (v != 0) atomicAdd(words + k, v);
    }
}

__global__ void gm_derive_kernel(const uint32_t* __restrict__ words, int64_t np, float cell, int64_t cap, GmGrid* grid) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    GmGrid g;
    gm_derive(words, (int64_t)words[6], np, cell, &g);
    if ((int64_t)g.cells > cap) {                      // (cannot be: the capacity is what gm_derive can choose)
        g.dims[0] = g.dims[1] = g.dims[2] = 1; g.cells = 1; g.inv = 0.f; g.size = (double)INFINITY;
    }
    *grid = g;
}

__global__ void __launch_bounds__(GM_BLOCK) gm_count_kernel(const float* __restrict__ points, uint32_t np, const GmGrid* __restrict__ grid, uint32_t* start) {
    const uint32_t j = blockIdx.x * GM_BLOCK + threadIdx.x;
    if (j >= np) return;
    const float p[3] = {points[3 * (size_t)j], points[3 * (size_t)j + 1], points[3 * (size_t)j + 2]};
    if (!gm_usable(p)) return;
    const GmGrid g = *grid;
    atomicAdd(start + gm_key(g, p), 1u);              // (a key is below g.cells <= the capacity)
}

__global__ void __launch_bounds__(GM_BLOCK) gm_scatter_kernel(const float* __restrict__ points, uint32_t np, const GmGrid* __restrict__ grid, uint32_t* cursor,
                                                              GmRecord* __restrict__ records) {
    const uint32_t j = blockIdx.x * GM_BLOCK + threadIdx.x;
    if (j >= np) return;
    const float p[3] = {points[3 * (size_t)j], points[3 * (size_t)j + 1], points[3 * (size_t)j + 2]};
    if (!gm_usable(p)) return;
    const GmGrid g = *grid;
    const uint32_t at = atomicAdd(cursor + gm_key(g, p), 1u);
    if (at >= np) return;                              // (cannot be: the cursors start at the scan of these same counts)
    GmRecord r;
    r.x = p[0]; r.y = p[1]; r.z = p[2]; r.index = (int32_t)j;
    records[at] = r;
}

__global__ void __launch_bounds__(GM_BLOCK) gm_query_kernel(const float* __restrict__ queries, uint32_t nq, const GmGrid* __restrict__ grid,
                                                            const uint32_t* __restrict__ start, const GmRecord* __restrict__ records, float* __restrict__ dist2,
                                                            int32_t* __restrict__ index, unsigned long long* stats) {
    __shared__ unsigned long long s_seen[GM_BLOCK / GP_WAVE];
    __shared__ int32_t s_red[GM_BLOCK / GP_WAVE][3];
    const GmGrid g = *grid;
    unsigned long long seen = 0;                     // of this lane
    int32_t ring = 0, excluded = 0, swept = 0;       // ring: of this lane; the others: of this wave
    const uint32_t stride = gridDim.x * GM_BLOCK;
    for (uint32_t first = blockIdx.x * GM_BLOCK; first < nq; first += stride) {
        const uint32_t i = first + threadIdx.x;
        bool bad = false, sw = false;
        if (i < nq) {
            const float q[3] = {queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2]};
            uint64_t v;
            int32_t r, s;
            float d;
            int32_t j;
            gm_query(g, start, records, q, &d, &j, &v, &r, &s);
            dist2[i] = d; index[i] = j;
            seen += v;
            ring = r > ring ? r : ring;
            bad = !gm_usable(q);
            sw = s != 0;
        }
        excluded += (int32_t)__popcll(__ballot(bad));
        swept += (int32_t)__popcll(__ballot(sw));
    }
    seen = gm_wave_sum(seen);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { const int32_t o = __shfl_xor(ring, s); ring = o > ring ? o : ring; }
    if ((threadIdx.x & 63) == 0) {
        s_seen[threadIdx.x >> 6] = seen;
        s_red[threadIdx.x >> 6][0] = ring; s_red[threadIdx.x >> 6][1] = excluded; s_red[threadIdx.x >> 6][2] = swept;
    }
    __syncthreads();
    if (threadIdx.x == 0) {          // one atomic per workgroup and word
        unsigned long long total = 0, r = 0, e = 0, w = 0;
        for (int k = 0; k < GM_BLOCK / GP_WAVE; ++k) {
            total += s_seen[k];
            r = (unsigned long long)s_red[k][0] > r ? (unsigned long long)s_red[k][0] : r;
            e += (unsigned long long)s_red[k][1];
            w += (unsigned long long)s_red[k][2];
        }
        if (total) atomicAdd(stats + GP_GEOMETRY_CANDIDATES, total);
        if (r) atomicMax(stats + GP_GEOMETRY_MAX_RING, r);
        if (e) atomicAdd(stats + GP_GEOMETRY_EXCLUDED_QUERIES, e);
        if (w) atomicAdd(stats + GP_GEOMETRY_SWEPT, w);
        if (blockIdx.x == 0) {       // (words nobody else writes)
            stats[GP_GEOMETRY_EXCLUDED_POINTS] = (unsigned long long)g.excluded;
            stats[GP_GEOMETRY_DIM_X] = (unsigned long long)g.dims[0];
            stats[GP_GEOMETRY_DIM_Y] = (unsigned long long)g.dims[1];
            stats[GP_GEOMETRY_DIM_Z] = (unsigned long long)g.dims[2];
        }
    }
}

// ---- metrics ----
__global__ void __launch_bounds__(GM_BLOCK) gm_metric_kernel(const float* __restrict__ d2, uint32_t n, GmThresholds th, double* __restrict__ slots) {
    __shared__ double s_red[GM_TERMS][GM_BLOCK / GP_WAVE];
    double t[GM_TERMS];
#pragma unroll
    for (int q = 0; q < GM_TERMS; ++q) t[q] = 0.0;
#pragma unroll
    for (int u = 0; u < GM_PER_LANE; ++u) {
        const uint32_t k = blockIdx.x * GM_TILE + u * GM_BLOCK + threadIdx.x;
        if (k < n) {
            double e[GM_TERMS];
            gm_terms(d2[k], th, e);
#pragma unroll
            for (int q = 0; q < GM_TERMS; ++q) t[q] = gm_join(q, t[q], e[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < GM_TERMS; ++q) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) t[q] = gm_join(q, t[q], __shfl_xor(t[q], s));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < GM_TERMS; ++q) s_red[q][threadIdx.x >> 6] = t[q];
    }
    __syncthreads();
    if (threadIdx.x < GM_TERMS) {
        const int q = threadIdx.x;
        slots[(size_t)blockIdx.x * GM_TERMS + q] = gm_join(q, gm_join(q, s_red[q][0], s_red[q][1]), gm_join(q, s_red[q][2], s_red[q][3]));
    }
}

__global__ void __launch_bounds__(GM_BLOCK) gm_metric_final_kernel(const double* __restrict__ slots, uint32_t tiles_ab, uint32_t tiles_ba, int32_t nt,
                                                                   double* __restrict__ table) {
    __shared__ double s_sum[GM_TERMS][GM_BLOCK];
    __shared__ double s_total[2 * GM_TERMS];
    const uint32_t tid = threadIdx.x;
    for (int dir = 0; dir < 2; ++dir) {
        const double* base = slots + (dir ? (size_t)tiles_ab * GM_TERMS : 0);
        const uint32_t tiles = dir ? tiles_ba : tiles_ab;
        double a[GM_TERMS];
#pragma unroll
        for (int q = 0; q < GM_TERMS; ++q) a[q] = 0.0;
        for (uint32_t k = tid; k < tiles; k += GM_BLOCK) {
#pragma unroll
            for (int q = 0; q < GM_TERMS; ++q) a[q] = gm_join(q, a[q], base[(size_t)k * GM_TERMS + q]);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < GM_TERMS; ++q) s_sum[q][tid] = a[q];
        __syncthreads();
        for (uint32_t stride = GM_BLOCK / 2; stride >= 1; stride >>= 1) {
            if (tid < stride) {
#pragma unroll
                for (int q = 0; q < GM_TERMS; ++q) s_sum[q][tid] = gm_join(q, s_sum[q][tid], s_sum[q][tid + stride]);
            }
            __syncthreads();
        }
        if (tid < GM_TERMS) s_total[dir * GM_TERMS + tid] = s_sum[tid][0];
    }
    __syncthreads();
    if (tid == 0) {
        double row[GP_GEOMETRY_COLUMNS];
        gm_row(s_total, nt, row);
        for (int q = 0; q < GP_GEOMETRY_COLUMNS; ++q) table[q] = row[q];
    }
}

// ---- the C entries ----
#define GM_REFUSE(name, why_)                                   \
    do {                                                        \
        const char* w_ = (why_);                                \
        if (w_) GP_FAIL(name ": %s", w_);                       \
    } while (0)

#define GM_REFUSE_SCRATCH(name)                                                                     \
    do {                                                                                            \
        if (!scratch) GP_FAIL(name ": null argument (scratch)");                                    \
        if (((uintptr_t)scratch & 15u) != 0) GP_FAIL(name ": scratch must be 16-byte aligned");     \
    } while (0)

static unsigned gm_capped(size_t n) {
    const unsigned b = gp_blocks(n, GM_BLOCK);
    return b < GM_MAX_BLOCKS ? b : GM_MAX_BLOCKS;
}

extern "C" int gp_geometry_abi_version(void) { return GP_GEOMETRY_ABI_VERSION; }

static int64_t gm_refused_bytes(const char* name, const char* why) {
    snprintf(gp_err_buf, sizeof(gp_err_buf), "%s: %s", name, why);
    return -1;
}

extern "C" int64_t gp_geometry_sample_scratch_bytes(int64_t nf) {
    const char* why = gm_refuse_mesh(0, nf);
    return why ? gm_refused_bytes("gp_geometry_sample_scratch_bytes", why) : gm_sample_layout(nf).bytes;
}

extern "C" int64_t gp_geometry_grid_scratch_bytes(int64_t np, float cell) {
    const char* why = gm_refuse_cloud(np, cell);
    return why ? gm_refused_bytes("gp_geometry_grid_scratch_bytes", why) : gm_grid_layout(np, cell).bytes;
}

extern "C" int64_t gp_geometry_metrics_scratch_bytes(int64_t n_ab, int64_t n_ba) {
    const char* why = gm_refuse_count(n_ab);
    if (!why) why = gm_refuse_count(n_ba);
    return why ? gm_refused_bytes("gp_geometry_metrics_scratch_bytes", why) : gm_metrics_bytes(n_ab, n_ba);
}

extern "C" int gp_geometry_sample(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, int64_t n, uint64_t seed, void* scratch, float* points,
                                  int32_t* face, float* bary, int32_t* counts, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    GM_REFUSE("gp_geometry_sample", gm_refuse_mesh(nv, nf));
    GM_REFUSE("gp_geometry_sample", gm_refuse_count(n));
    if (n < 1) GP_FAIL("gp_geometry_sample: n must be >= 1 (n = %lld)", (long long)n);
    GM_REFUSE_SCRATCH("gp_geometry_sample");
    if (!points || !face || !bary || !counts || (nv > 0 && !vertices) || (nf > 0 && !faces)) GP_FAIL("gp_geometry_sample: null argument");
    const GmSampleScratch s = gm_sample_layout(nf);
    char* base = (char*)scratch;
    unsigned long long* max_bits = (unsigned long long*)(base + s.head);
    GmSampleHead* head = (GmSampleHead*)(base + s.head + 16);
    uint64_t* prefix = (uint64_t*)(base + s.prefix);
    uint64_t* sums = (uint64_t*)(base + s.sums);
    const uint32_t NV = (uint32_t)nv, NF = (uint32_t)nf, tiles = (uint32_t)gm_tiles(nf);
    GpProfScope _p("geometry_sample", st);
    GP_HIP_CHECK(hipMemsetAsync(counts, 0, GP_GEOMETRY_COUNT_WORDS * sizeof(int32_t), st));
    GP_HIP_CHECK(hipMemsetAsync(base + s.head, 0, 64, st));
    if (NF > 0) {
        hipLaunchKernelGGL(gm_area_kernel, dim3(gm_capped(NF)), dim3(GM_BLOCK), 0, st, vertices, faces, NV, NF, (double*)prefix, max_bits, counts);
        GP_LAUNCH_CHECK();
        hipLaunchKernelGGL(gm_weight_kernel, dim3(tiles), dim3(GM_BLOCK), 0, st, prefix, NF, (const unsigned long long*)max_bits, sums, counts);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gm_scan_sums_u64_kernel, dim3(1), dim3(GM_BLOCK), 0, st, sums, tiles, n, head, counts);
    GP_LAUNCH_CHECK();
    if (NF > 0) {
        hipLaunchKernelGGL((gm_prefix_kernel<uint64_t, true>), dim3(tiles), dim3(GM_BLOCK), 0, st, prefix, NF, (const uint64_t*)sums, (uint64_t*)nullptr);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gm_sample_kernel, dim3(gp_blocks((size_t)n, GM_BLOCK)), dim3(GM_BLOCK), 0, st, vertices, faces, NV, NF, (const uint64_t*)prefix,
                       (const GmSampleHead*)head, seed, (uint32_t)n, points, face, bary);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_geometry_interpolate(const float* attributes, int32_t C, const int32_t* faces, int64_t nv, int64_t nf, const int32_t* face, const float* bary,
                                       int64_t n, float* out, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    GM_REFUSE("gp_geometry_interpolate", gm_refuse_mesh(nv, nf));
    GM_REFUSE("gp_geometry_interpolate", gm_refuse_count(n));
    if (C < 1 || C > GP_GEOMETRY_MAX_CHANNELS) GP_FAIL("gp_geometry_interpolate: C must be 1 .. %d (C = %d)", GP_GEOMETRY_MAX_CHANNELS, C);
    if (n == 0) return 0;
    if (!face || !bary || !out || (nv > 0 && !attributes) || (nf > 0 && !faces)) GP_FAIL("gp_geometry_interpolate: null argument");
    GpProfScope _p("geometry_interpolate", st);
    hipLaunchKernelGGL(gm_interpolate_kernel, dim3(gp_blocks((size_t)n, GM_BLOCK)), dim3(GM_BLOCK), 0, st, attributes, C, faces, (uint32_t)nv, (uint32_t)nf, face, bary,
                       (uint32_t)n, out);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_geometry_grid_build(const float* points, int64_t np, float cell, void* scratch, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    GM_REFUSE("gp_geometry_grid_build", gm_refuse_cloud(np, cell));
    GM_REFUSE_SCRATCH("gp_geometry_grid_build");
    if (np > 0 && !points) GP_FAIL("gp_geometry_grid_build: null argument");
    const GmGridScratch s = gm_grid_layout(np, cell);
    char* base = (char*)scratch;
    uint32_t* words = (uint32_t*)(base + s.bounds);
    GmGrid* grid = (GmGrid*)(base + s.grid);
    uint32_t* start = (uint32_t*)(base + s.start);
    uint32_t* cursor = (uint32_t*)(base + s.cursor);
    uint32_t* sums = (uint32_t*)(base + s.sums);
    GmRecord* records = (GmRecord*)(base + s.records);
    const uint32_t NP = (uint32_t)np, entries = (uint32_t)(s.cap + 1), tiles = (uint32_t)gm_tiles(s.cap + 1);
    GpProfScope _p("geometry_grid_build", st);
    GP_HIP_CHECK(hipMemsetAsync(words, 0xFF, 3 * sizeof(uint32_t), st));
    GP_HIP_CHECK(hipMemsetAsync(words + 3, 0, 4 * sizeof(uint32_t), st));
    GP_HIP_CHECK(hipMemsetAsync(start, 0, (size_t)entries * sizeof(uint32_t), st));
    if (NP > 0) {
        hipLaunchKernelGGL(gm_bounds_kernel, dim3(gm_capped(NP)), dim3(GM_BLOCK), 0, st, points, NP, words);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gm_derive_kernel, dim3(1), dim3(GP_WAVE), 0, st, (const uint32_t*)words, np, cell, s.cap, grid);
    GP_LAUNCH_CHECK();
    if (NP > 0) {
        hipLaunchKernelGGL(gm_count_kernel, dim3(gp_blocks(NP, GM_BLOCK)), dim3(GM_BLOCK), 0, st, points, NP, (const GmGrid*)grid, start);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gm_tile_sum_u32_kernel, dim3(tiles), dim3(GM_BLOCK), 0, st, (const uint32_t*)start, entries, sums);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(gm_scan_sums_u32_kernel, dim3(1), dim3(GM_BLOCK), 0, st, sums, tiles);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL((gm_prefix_kernel<uint32_t, false>), dim3(tiles), dim3(GM_BLOCK), 0, st, start, entries, (const uint32_t*)sums, cursor);
    GP_LAUNCH_CHECK();
    if (NP > 0) {
        hipLaunchKernelGGL(gm_scatter_kernel, dim3(gp_blocks(NP, GM_BLOCK)), dim3(GM_BLOCK), 0, st, points, NP, (const GmGrid*)grid, cursor, records);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gp_geometry_grid_query(const float* queries, int64_t nq, const void* scratch, int64_t np, float cell, float* dist2, int32_t* index, int64_t* stats,
                                      gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    GM_REFUSE("gp_geometry_grid_query", gm_refuse_cloud(np, cell));
    GM_REFUSE("gp_geometry_grid_query", gm_refuse_count(nq));
    GM_REFUSE_SCRATCH("gp_geometry_grid_query");
    if (!stats || (nq > 0 && (!queries || !dist2 || !index))) GP_FAIL("gp_geometry_grid_query: null argument");
    const GmGridScratch s = gm_grid_layout(np, cell);
    const char* base = (const char*)scratch;
    GpProfScope _p("geometry_grid_query", st);
    GP_HIP_CHECK(hipMemsetAsync(stats, 0, GP_GEOMETRY_STAT_WORDS * sizeof(int64_t), st));
    // (nq == 0 still launches one workgroup: it writes the words of the grid)
    hipLaunchKernelGGL(gm_query_kernel, dim3(nq > 0 ? gm_capped((size_t)nq) : 1), dim3(GM_BLOCK), 0, st, queries, (uint32_t)nq, (const GmGrid*)(base + s.grid),
                       (const uint32_t*)(base + s.start), (const GmRecord*)(base + s.records), dist2, index, (unsigned long long*)stats);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_geometry_metrics(const float* dist2_ab, int64_t n_ab, const float* dist2_ba, int64_t n_ba, const float* thresholds, int32_t nt, void* scratch,
                                   double* table, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    GM_REFUSE("gp_geometry_metrics", gm_refuse_count(n_ab));
    GM_REFUSE("gp_geometry_metrics", gm_refuse_count(n_ba));
    if (nt < 0 || nt > GP_GEOMETRY_MAX_THRESHOLDS) GP_FAIL("gp_geometry_metrics: nt must be 0 .. %d (nt = %d)", GP_GEOMETRY_MAX_THRESHOLDS, nt);
    GM_REFUSE_SCRATCH("gp_geometry_metrics");
    if (!table || (n_ab > 0 && !dist2_ab) || (n_ba > 0 && !dist2_ba) || (nt > 0 && !thresholds)) GP_FAIL("gp_geometry_metrics: null argument");
    GmThresholds th;
    th.nt = nt;
    for (int k = 0; k < GP_GEOMETRY_MAX_THRESHOLDS; ++k) {
        th.v[k] = k < nt ? thresholds[k] : 0.f;
        if (th.v[k] != th.v[k]) GP_FAIL("gp_geometry_metrics: a threshold is NaN");
    }
    const uint32_t tiles_ab = (uint32_t)gm_tiles(n_ab), tiles_ba = (uint32_t)gm_tiles(n_ba);
    double* slots = (double*)scratch;
    GpProfScope _p("geometry_metrics", st);
    if (tiles_ab > 0) {
        hipLaunchKernelGGL(gm_metric_kernel, dim3(tiles_ab), dim3(GM_BLOCK), 0, st, dist2_ab, (uint32_t)n_ab, th, slots);
        GP_LAUNCH_CHECK();
    }
    if (tiles_ba > 0) {
        hipLaunchKernelGGL(gm_metric_kernel, dim3(tiles_ba), dim3(GM_BLOCK), 0, st, dist2_ba, (uint32_t)n_ba, th, slots + (size_t)tiles_ab * GM_TERMS);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gm_metric_final_kernel, dim3(1), dim3(GM_BLOCK), 0, st, (const double*)slots, tiles_ab, tiles_ba, nt, table);
    GP_LAUNCH_CHECK();
    return 0;
}
