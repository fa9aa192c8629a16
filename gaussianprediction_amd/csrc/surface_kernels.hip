// surface_kernels.hip -- the exact distance from a point to a mesh surface on the device, on a uniform grid over the triangles
// (csrc/gp_surface.h).  The programs of a lane are csrc/surface_core.h, which also runs on a CPU (tests/surface_emulate.cpp).
//   sf_prepare_kernel      a lane per face by grid stride: its 48-byte record; the bounds of the usable corners by integer minima and
//                          maxima of order-preserving bits and the usable count, once per workgroup and word
//   sf_derive_kernel       one lane: the grid record, so the host reads nothing but the two sizes
//   sf_count_kernel        a lane per face: one integer atomic add per cell of its box, or one on the wide list's length
//   sf_tile_sum_kernel, sf_scan_sums_kernel, sf_prefix_kernel      the exclusive scan of the per-cell counts (geometry_kernels.hip's scheme)
//   sf_sizes_kernel        one lane: the pairs and the wide faces, for the caller's 16-byte read
//   sf_status_kernel       one lane: the refusal of a capacity below the pairs
//   sf_fill_kernel         a lane per face: its number to every cell of its box, through the cursors
//   sf_query_kernel        a lane per query by grid stride: the wide list, then the rings -- a divergent per-lane loop on purpose, as
//                          geometry_kernels.hip's; a candidate is one index and three dwordx4 of one record, then float64 arithmetic
// No float atomics, no spinning, no fence: everything crosses launch boundaries.
#include "gp_common.h"

#include "surface_core.h"

static_assert(SF_BLOCK == 4 * GP_WAVE, "four waves a workgroup");

// ---- workgroup helpers ----
__device__ __forceinline__ uint32_t sf_block_sum(uint32_t v, uint32_t* s) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s[0] + s[1]) + (s[2] + s[3]);
}
// the exclusive scan over the workgroup's lanes; s: [SF_BLOCK]; *total: the sum
__device__ __forceinline__ uint32_t sf_block_scan(uint32_t v, uint32_t* s, uint32_t* total) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < SF_BLOCK; d <<= 1) {
        const uint32_t add = tid >= d ? s[tid - d] : 0u;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    *total = s[SF_BLOCK - 1];
    return s[tid] - v;
}

// ---- the build ----
// words: lo[3] (start at all ones), hi[3], usable (start at 0)
__global__ void __launch_bounds__(SF_BLOCK) sf_prepare_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                              SfFace* __restrict__ records, uint32_t* words) {
    __shared__ uint32_t s_red[SF_BLOCK / GP_WAVE][7];
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u}, usable = 0;
    const uint32_t stride = gridDim.x * SF_BLOCK;                // (nf < 2^26: no wrap)
    for (uint32_t first = blockIdx.x * SF_BLOCK; first < nf; first += stride) {
        const uint32_t f = first + threadIdx.x;
        bool ok = false;
        if (f < nf) {
            SfFace r;
            ok = sf_record(vertices, faces, f, nv, &r);
            records[f] = r;
            if (ok)
                for (int a = 0; a < 3; ++a) {
                    const uint32_t o[3] = {gm_ordered(r.a[a] + 0.f), gm_ordered(r.b[a] + 0.f), gm_ordered(r.c[a] + 0.f)};
                    for (int k = 0; k < 3; ++k) {
                        lo[a] = o[k] < lo[a] ? o[k] : lo[a];
                        hi[a] = o[k] > hi[a] ? o[k] : hi[a];
                    }
                }
        }
        usable += (uint32_t)__popcll(__ballot(ok));              // (of this wave)
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
        for (int w = 1; w < SF_BLOCK / GP_WAVE; ++w) {
            const uint32_t o = s_red[w][k];
            v = k < 3 ? (o < v ? o : v) : (k < 6 ? (o > v ? o : v) : v + o);
        }
        if (k < 3) atomicMin(words + k, v);
        else if (k < 6) atomicMax(words + k, v);
        else if (v != 0) atomicAdd(words + k, v);
    }
}

__global__ void sf_derive_kernel(const uint32_t* __restrict__ words, int64_t nf, float cell, int64_t cap, GmGrid* grid) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    GmGrid g;
    sf_derive(words, (int64_t)words[SF_WORD_USABLE], nf, cell, &g);
    if ((int64_t)g.cells > cap) {                      // (cannot be: the capacity is what sf_derive can choose)
        g.dims[0] = g.dims[1] = g.dims[2] = 1; g.cells = 1; g.inv = 0.f; g.size = (double)INFINITY;
    }
    *grid = g;
}

__global__ void __launch_bounds__(SF_BLOCK) sf_count_kernel(const SfFace* __restrict__ records, uint32_t nf, const GmGrid* __restrict__ grid, int32_t wide_cells,
                                                            uint32_t* start, int32_t* __restrict__ wide, uint32_t* words) {
    const uint32_t f = blockIdx.x * SF_BLOCK + threadIdx.x;
    if (f >= nf) return;
    const SfFace r = records[f];
    if (r.face < 0) return;
    const GmGrid g = *grid;
    int32_t lo[3], hi[3];
    sf_box(g, r, lo, hi);
    if (sf_box_cells(lo, hi) > (int64_t)wide_cells) {
        const uint32_t at = atomicAdd(words + SF_WORD_WIDE, 1u);
        if (at < nf) wide[at] = (int32_t)f;            // (always: a face is appended once)
        return;
    }
    for (int32_t z = lo[2]; z <= hi[2]; ++z)
        for (int32_t y = lo[1]; y <= hi[1]; ++y)
            for (int32_t x = lo[0]; x <= hi[0]; ++x) atomicAdd(start + sf_key(g, x, y, z), 1u);          // (a key is below g.cells <= the capacity)
}

__global__ void __launch_bounds__(SF_BLOCK) sf_tile_sum_kernel(const uint32_t* __restrict__ data, uint32_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_sum[SF_BLOCK / GP_WAVE];
    uint32_t sum = 0;
#pragma unroll
    for (int u = 0; u < SF_PER_LANE; ++u) {
        const uint32_t k = blockIdx.x * SF_TILE + threadIdx.x * SF_PER_LANE + u;
        if (k < n) sum += data[k];
    }
    sum = sf_block_sum(sum, s_sum);
    if (threadIdx.x == 0) sums[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(SF_BLOCK) sf_scan_sums_kernel(uint32_t* sums, uint32_t tiles) {
    __shared__ uint32_t s[SF_BLOCK];
    uint32_t carry = 0;
    for (uint32_t first = 0; first < tiles; first += SF_BLOCK) {          // (the same trips for the whole workgroup)
        const uint32_t k = first + threadIdx.x;
        const uint32_t v = k < tiles ? sums[k] : 0u;
        uint32_t total;
        const uint32_t before = sf_block_scan(v, s, &total);
        if (k < tiles) sums[k] = carry + before;
        carry += total;
    }
}

// data[k] = the tile's offset + the exclusive scan inside the tile
__global__ void __launch_bounds__(SF_BLOCK) sf_prefix_kernel(uint32_t* __restrict__ data, uint32_t n, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t s[SF_BLOCK];
    const uint32_t base = blockIdx.x * SF_TILE + threadIdx.x * SF_PER_LANE;
    uint32_t v[SF_PER_LANE], mine = 0;
#pragma unroll
    for (int u = 0; u < SF_PER_LANE; ++u) { v[u] = base + u < n ? data[base + u] : 0u; mine += v[u]; }
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + sf_block_scan(mine, s, &total);
#pragma unroll
    for (int u = 0; u < SF_PER_LANE; ++u) {
        if (base + u < n) data[base + u] = run;
        run += v[u];
    }
}

__global__ void sf_sizes_kernel(const uint32_t* __restrict__ start, const GmGrid* __restrict__ grid, uint32_t* words, int64_t* sizes) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t pairs = start[grid->cells];
    words[SF_WORD_PAIRS] = pairs;
    sizes[0] = (int64_t)pairs;
    sizes[1] = (int64_t)words[SF_WORD_WIDE];
}

__global__ void sf_status_kernel(uint32_t* words, int64_t pair_capacity) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    words[SF_WORD_STATUS] = (int64_t)words[SF_WORD_PAIRS] > pair_capacity ? GP_SURFACE_REFUSED_CAPACITY : 0;
}

__global__ void __launch_bounds__(SF_BLOCK) sf_fill_kernel(const SfFace* __restrict__ records, uint32_t nf, const GmGrid* __restrict__ grid, int32_t wide_cells,
                                                           const uint32_t* __restrict__ words, uint32_t* cursor, int32_t* __restrict__ pairs, int64_t pair_capacity) {
    const uint32_t f = blockIdx.x * SF_BLOCK + threadIdx.x;
    if (f >= nf || words[SF_WORD_STATUS] != 0) return;           // a refused capacity writes nothing
    const SfFace r = records[f];
    if (r.face < 0) return;
    const GmGrid g = *grid;
    int32_t lo[3], hi[3];
    sf_box(g, r, lo, hi);
    if (sf_box_cells(lo, hi) > (int64_t)wide_cells) return;
    for (int32_t z = lo[2]; z <= hi[2]; ++z)
        for (int32_t y = lo[1]; y <= hi[1]; ++y)
            for (int32_t x = lo[0]; x <= hi[0]; ++x) {
                const uint32_t at = atomicAdd(cursor + sf_key(g, x, y, z), 1u);
                if ((int64_t)at < pair_capacity) pairs[at] = (int32_t)f;          // (always: the cursors start at the scan of these same counts)
            }
}

// ---- the query ----
__global__ void __launch_bounds__(SF_BLOCK) sf_query_kernel(const float* __restrict__ queries, uint32_t nq, uint32_t nf, const uint32_t* __restrict__ words,
                                                            const GmGrid* __restrict__ grid, const uint32_t* __restrict__ start, const int32_t* __restrict__ pairs,
                                                            const SfFace* __restrict__ records, const int32_t* __restrict__ wide, float* __restrict__ dist2,
                                                            int32_t* __restrict__ face, int32_t* __restrict__ region, float* __restrict__ closest,
                                                            float* __restrict__ bary, unsigned long long* stats) {
    __shared__ unsigned long long s_seen[SF_BLOCK / GP_WAVE];
    __shared__ int32_t s_red[SF_BLOCK / GP_WAVE][3];
    const GmGrid g = *grid;
    const bool refused = words[SF_WORD_STATUS] != 0 || (pairs == nullptr && words[SF_WORD_PAIRS] != 0);
    uint32_t nwide = words[SF_WORD_WIDE];
    nwide = nwide < nf ? nwide : nf;
    unsigned long long seen = 0;                     // of this lane
    int32_t ring = 0, excluded = 0, swept = 0;       // ring: of this lane; the others: of this wave
    const uint32_t stride = gridDim.x * SF_BLOCK;
    for (uint32_t first = blockIdx.x * SF_BLOCK; first < nq; first += stride) {
        const uint32_t i = first + threadIdx.x;
        bool bad = false, sw = false;
        if (i < nq) {
            const float q[3] = {queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2]};
            uint64_t v;
            int32_t r, s, f, k;
            float d, p[3], u[2];
            sf_query(g, (int64_t)nf, refused, start, pairs, records, wide, nwide, q, &d, &f, &k, p, u, &v, &r, &s);
            dist2[i] = d; face[i] = f; region[i] = k;
            closest[3 * (size_t)i] = p[0]; closest[3 * (size_t)i + 1] = p[1]; closest[3 * (size_t)i + 2] = p[2];
            bary[2 * (size_t)i] = u[0]; bary[2 * (size_t)i + 1] = u[1];
            seen += v;
            ring = r > ring ? r : ring;
            bad = !gm_usable(q);
            sw = s != 0;
        }
        excluded += (int32_t)__popcll(__ballot(bad));
        swept += (int32_t)__popcll(__ballot(sw));
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        seen += __shfl_xor(seen, s);
        const int32_t o = __shfl_xor(ring, s);
        ring = o > ring ? o : ring;
    }
    if ((threadIdx.x & 63) == 0) {
        s_seen[threadIdx.x >> 6] = seen;
        s_red[threadIdx.x >> 6][0] = ring; s_red[threadIdx.x >> 6][1] = excluded; s_red[threadIdx.x >> 6][2] = swept;
    }
    __syncthreads();
    if (threadIdx.x == 0) {          // one atomic per workgroup and word
        unsigned long long total = 0, r = 0, e = 0, w = 0;
        for (int k = 0; k < SF_BLOCK / GP_WAVE; ++k) {
            total += s_seen[k];
            r = (unsigned long long)s_red[k][0] > r ? (unsigned long long)s_red[k][0] : r;
            e += (unsigned long long)s_red[k][1];
            w += (unsigned long long)s_red[k][2];
        }
        if (total) atomicAdd(stats + GP_SURFACE_CANDIDATES, total);
        if (r) atomicMax(stats + GP_SURFACE_MAX_RING, r);
        if (e) atomicAdd(stats + GP_SURFACE_EXCLUDED_QUERIES, e);
        if (w) atomicAdd(stats + GP_SURFACE_SWEPT, w);
        if (blockIdx.x == 0) {       // (words nobody else writes)
            stats[GP_SURFACE_EXCLUDED_FACES] = (unsigned long long)g.excluded;
            stats[GP_SURFACE_DIM_X] = (unsigned long long)g.dims[0];
            stats[GP_SURFACE_DIM_Y] = (unsigned long long)g.dims[1];
            stats[GP_SURFACE_DIM_Z] = (unsigned long long)g.dims[2];
            stats[GP_SURFACE_PAIRS] = (unsigned long long)words[SF_WORD_PAIRS];
            stats[GP_SURFACE_WIDE] = (unsigned long long)words[SF_WORD_WIDE];
            stats[GP_SURFACE_STATUS] = (unsigned long long)words[SF_WORD_STATUS];
        }
    }
}

// ---- the C entries ----
#define SF_REFUSE(name, why_)                                   \
    do {                                                        \
        const char* w_ = (why_);                                \
        if (w_) GP_FAIL(name ": %s", w_);                       \
    } while (0)

#define SF_REFUSE_SCRATCH(name)                                                                     \
    do {                                                                                            \
        if (!scratch) GP_FAIL(name ": null argument (scratch)");                                    \
        if (((uintptr_t)scratch & 15u) != 0) GP_FAIL(name ": scratch must be 16-byte aligned");     \
    } while (0)

static unsigned sf_capped(size_t n) {
    const unsigned b = gp_blocks(n, SF_BLOCK);
    return b < GM_MAX_BLOCKS ? b : GM_MAX_BLOCKS;
}

extern "C" int gp_surface_abi_version(void) { return GP_SURFACE_ABI_VERSION; }

extern "C" int64_t gp_surface_scratch_bytes(int64_t nf, float cell) {
    const char* why = sf_refuse_grid(nf, cell);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_surface_scratch_bytes: %s", why);
        return -1;
    }
    return sf_layout(nf, cell).bytes;
}

extern "C" int gp_surface_grid_count(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, float cell, int32_t wide_cells, void* scratch,
                                     int64_t* sizes, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    SF_REFUSE("gp_surface_grid_count", gm_refuse_mesh(nv, nf));
    SF_REFUSE("gp_surface_grid_count", sf_refuse_grid(nf, cell));
    SF_REFUSE("gp_surface_grid_count", sf_refuse_wide(wide_cells));
    SF_REFUSE_SCRATCH("gp_surface_grid_count");
    if (!sizes || (nf > 0 && (!faces || (nv > 0 && !vertices)))) GP_FAIL("gp_surface_grid_count: null argument");
    const SfScratch s = sf_layout(nf, cell);
    char* base = (char*)scratch;
    uint32_t* words = (uint32_t*)(base + s.words);
    GmGrid* grid = (GmGrid*)(base + s.grid);
    uint32_t* start = (uint32_t*)(base + s.start);
    uint32_t* sums = (uint32_t*)(base + s.sums);
    SfFace* records = (SfFace*)(base + s.records);
    int32_t* wide = (int32_t*)(base + s.wide);
    const uint32_t NF = (uint32_t)nf, entries = (uint32_t)(s.cap + 1), tiles = (uint32_t)gm_tiles(s.cap + 1);
    GpProfScope _p("surface_grid_count", st);
    GP_HIP_CHECK(hipMemsetAsync(words, 0xFF, 3 * sizeof(uint32_t), st));
    GP_HIP_CHECK(hipMemsetAsync(words + 3, 0, (SF_WORDS - 3) * sizeof(uint32_t), st));
    GP_HIP_CHECK(hipMemsetAsync(start, 0, (size_t)entries * sizeof(uint32_t), st));
    if (NF > 0) {
        hipLaunchKernelGGL(sf_prepare_kernel, dim3(sf_capped(NF)), dim3(SF_BLOCK), 0, st, vertices, faces, (uint32_t)nv, NF, records, words);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sf_derive_kernel, dim3(1), dim3(GP_WAVE), 0, st, (const uint32_t*)words, nf, cell, s.cap, grid);
    GP_LAUNCH_CHECK();
    if (NF > 0) {
        hipLaunchKernelGGL(sf_count_kernel, dim3(gp_blocks(NF, SF_BLOCK)), dim3(SF_BLOCK), 0, st, (const SfFace*)records, NF, (const GmGrid*)grid, wide_cells, start, wide,
                           words);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sf_tile_sum_kernel, dim3(tiles), dim3(SF_BLOCK), 0, st, (const uint32_t*)start, entries, sums);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(sf_scan_sums_kernel, dim3(1), dim3(SF_BLOCK), 0, st, sums, tiles);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(sf_prefix_kernel, dim3(tiles), dim3(SF_BLOCK), 0, st, start, entries, (const uint32_t*)sums);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(sf_sizes_kernel, dim3(1), dim3(GP_WAVE), 0, st, (const uint32_t*)start, (const GmGrid*)grid, words, sizes);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_surface_grid_fill(int64_t nf, float cell, int32_t wide_cells, void* scratch, int32_t* pairs, int64_t pair_capacity, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    SF_REFUSE("gp_surface_grid_fill", sf_refuse_grid(nf, cell));
    SF_REFUSE("gp_surface_grid_fill", sf_refuse_wide(wide_cells));
    if (pair_capacity < 0 || pair_capacity >= 0x100000000LL) GP_FAIL("gp_surface_grid_fill: pair_capacity must be 0 .. 2^32 - 1");
    SF_REFUSE_SCRATCH("gp_surface_grid_fill");
    if (pair_capacity > 0 && !pairs) GP_FAIL("gp_surface_grid_fill: null argument");
    const SfScratch s = sf_layout(nf, cell);
    char* base = (char*)scratch;
    uint32_t* words = (uint32_t*)(base + s.words);
    const uint32_t NF = (uint32_t)nf;
    GpProfScope _p("surface_grid_fill", st);
    GP_HIP_CHECK(hipMemcpyAsync(base + s.cursor, base + s.start, (size_t)(s.cap + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(sf_status_kernel, dim3(1), dim3(GP_WAVE), 0, st, words, pair_capacity);
    GP_LAUNCH_CHECK();
    if (NF > 0) {
        hipLaunchKernelGGL(sf_fill_kernel, dim3(gp_blocks(NF, SF_BLOCK)), dim3(SF_BLOCK), 0, st, (const SfFace*)(base + s.records), NF, (const GmGrid*)(base + s.grid),
                           wide_cells, (const uint32_t*)words, (uint32_t*)(base + s.cursor), pairs, pair_capacity);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gp_surface_grid_query(const float* queries, int64_t nq, const void* scratch, const int32_t* pairs, int64_t nf, float cell, float* dist2,
                                     int32_t* face, int32_t* region, float* closest, float* bary, int64_t* stats, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    SF_REFUSE("gp_surface_grid_query", sf_refuse_grid(nf, cell));
    SF_REFUSE("gp_surface_grid_query", gm_refuse_count(nq));
    SF_REFUSE_SCRATCH("gp_surface_grid_query");
    if (!stats || (nq > 0 && (!queries || !dist2 || !face || !region || !closest || !bary))) GP_FAIL("gp_surface_grid_query: null argument");
    const SfScratch s = sf_layout(nf, cell);
    const char* base = (const char*)scratch;
    GpProfScope _p("surface_grid_query", st);
    GP_HIP_CHECK(hipMemsetAsync(stats, 0, GP_SURFACE_STAT_WORDS * sizeof(int64_t), st));
    // (nq == 0 still launches one workgroup: it writes the words of the grid)
    hipLaunchKernelGGL(sf_query_kernel, dim3(nq > 0 ? sf_capped((size_t)nq) : 1), dim3(SF_BLOCK), 0, st, queries, (uint32_t)nq, (uint32_t)nf,
                       (const uint32_t*)(base + s.words), (const GmGrid*)(base + s.grid), (const uint32_t*)(base + s.start), pairs,
                       (const SfFace*)(base + s.records), (const int32_t*)(base + s.wide), dist2, face, region, closest, bary, (unsigned long long*)stats);
    GP_LAUNCH_CHECK();
    return 0;
}
