// volume_kernels.hip -- signed-distance volumes on the device: a bounding-volume tree over the triangles, the signed distance of a mesh
// on a lattice, the counts of a volumetric IoU (csrc/gp_volume.h).  The programs of a lane are csrc/volume_core.h, csrc/sdf_core.h and
// csrc/surface_core.h, which also run on a CPU (tests/volume_emulate.cpp).
//   vl_prepare_kernel      a lane per face by grid stride: its 48-byte record; the bounds of the usable corners, the largest |coordinate|
//                          and the usable count by integer atomics of order-preserving bits, once per workgroup and word
//   vl_key_kernel          a lane per face: its Morton key on those bounds (2^30 where it is not usable)
//   vl_gather_kernel       a lane per sorted position: the record copied into sorted order, so that a leaf is contiguous memory
//   vl_leaf_kernel, vl_level_kernel      a lane per box: a leaf's box; the union of two boxes of the level below -- one launch a level
//   vl_query_kernel        a lane per query by grid stride: the stack walk, nearer child first -- a divergent per-lane loop on purpose;
//                          a box is two dwordx4, a candidate three dwordx4 of one record, then float64 arithmetic
//   vl_lattice_kernel      a lane per lattice point, x fastest: the point by fmaf, the walk, sdf_core.h's sign, 4 bytes written
//   vl_compare_kernel      a lane per pair of values: ballots, integers only
// around gp_radix_sort_pairs (stable).  No float atomics, no spinning, no fence: everything crosses launch boundaries.
#include "gp_common.h"

#include "volume_core.h"

static_assert(VL_BLOCK == 4 * GP_WAVE, "four waves a workgroup");
#define VL_WAVES (VL_BLOCK / GP_WAVE)

// ---- the build ----
// words: lo[3] (start at all ones), hi[3], usable, M (start at 0)
__global__ void __launch_bounds__(VL_BLOCK) vl_prepare_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                              SfFace* __restrict__ records, uint32_t* words) {
    __shared__ uint32_t s_red[VL_WAVES][8];
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u}, usable = 0, m = 0;
    const uint32_t stride = gridDim.x * VL_BLOCK;                // (nf < 2^26: no wrap)
    for (uint32_t first = blockIdx.x * VL_BLOCK; first < nf; first += stride) {
        const uint32_t f = first + threadIdx.x;
        bool ok = false;
        if (f < nf) {
            SfFace r;
            ok = sf_record(vertices, faces, f, nv, &r);
            records[f] = r;
            if (ok)
                for (int a = 0; a < 3; ++a) {
                    const float c[3] = {r.a[a] + 0.f, r.b[a] + 0.f, r.c[a] + 0.f};
                    for (int k = 0; k < 3; ++k) {
                        const uint32_t o = gm_ordered(c[k]), bits = __float_as_uint(fabsf(c[k]));
                        lo[a] = o < lo[a] ? o : lo[a];
                        hi[a] = o > hi[a] ? o : hi[a];
                        m = bits > m ? bits : m;
                    }
                }
        }
        usable += (uint32_t)__popcll(__ballot(ok));              // (of this wave)
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        for (int a = 0; a < 3; ++a) {
            const uint32_t l = __shfl_xor(lo[a], s), h = __shfl_xor(hi[a], s);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
        const uint32_t o = __shfl_xor(m, s);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) { s_red[threadIdx.x >> 6][a] = lo[a]; s_red[threadIdx.x >> 6][3 + a] = hi[a]; }
        s_red[threadIdx.x >> 6][VL_WORD_USABLE] = usable;
        s_red[threadIdx.x >> 6][VL_WORD_M] = m;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const int k = threadIdx.x;
        uint32_t v = s_red[0][k];
        for (int w = 1; w < VL_WAVES; ++w) {
            const uint32_t o = s_red[w][k];
            v = k < 3 ? (o < v ? o : v) : (k == VL_WORD_USABLE ? v + o : (o > v ? o : v));
        }
        if (k < 3) atomicMin(words + k, v);
        else if (k == VL_WORD_USABLE) { if (v != 0) atomicAdd(words + k, v); }
        else atomicMax(words + k, v);
    }
}

__global__ void __launch_bounds__(VL_BLOCK) vl_key_kernel(const SfFace* __restrict__ records, uint32_t nf, const uint32_t* __restrict__ words, uint32_t* __restrict__ keys) {
    const uint32_t f = blockIdx.x * VL_BLOCK + threadIdx.x;
    if (f < nf) keys[f] = vl_key(records[f], words);
}

__global__ void __launch_bounds__(VL_BLOCK) vl_gather_kernel(const SfFace* __restrict__ records, const uint32_t* __restrict__ order, uint32_t nf, SfFace* __restrict__ sorted) {
    const uint32_t i = blockIdx.x * VL_BLOCK + threadIdx.x;
    if (i >= nf) return;
    const uint32_t f = order[i] < nf ? order[i] : 0u;            // (a permutation of 0 .. nf - 1: the values the sort was handed)
    sorted[i] = records[f];
}

__global__ void __launch_bounds__(VL_BLOCK) vl_leaf_kernel(const SfFace* __restrict__ sorted, VlTree t, VlBox* __restrict__ boxes) {
    const uint32_t i = blockIdx.x * VL_BLOCK + threadIdx.x;
    if (i >= t.count[0]) return;
    VlBox b;
    vl_leaf_box(sorted, t, i, &b);
    boxes[t.offset[0] + i] = b;
}

__global__ void __launch_bounds__(VL_BLOCK) vl_level_kernel(VlTree t, uint32_t level, VlBox* boxes) {
    const uint32_t i = blockIdx.x * VL_BLOCK + threadIdx.x;
    if (i >= t.count[level]) return;
    VlBox b;
    vl_union(boxes, t, level, i, &b);
    boxes[t.offset[level] + i] = b;
}

// ---- the tallies of a workgroup: every lane calls it once, after its last query ----
// nodes, candidates, stack, overflow: of this lane; excluded: of this wave (from ballots)
__device__ __forceinline__ void vl_flush(unsigned long long nodes, unsigned long long candidates, int32_t stack, int32_t overflow, uint32_t excluded, const VlTree& t,
                                         uint32_t usable, unsigned long long* stats) {
    __shared__ unsigned long long s_sum[VL_WAVES][2];
    __shared__ int32_t s_red[VL_WAVES][3];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        nodes += __shfl_xor(nodes, s);
        candidates += __shfl_xor(candidates, s);
        const int32_t o = __shfl_xor(stack, s);
        stack = o > stack ? o : stack;
        overflow |= __shfl_xor(overflow, s);
    }
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6][0] = nodes; s_sum[threadIdx.x >> 6][1] = candidates;
        s_red[threadIdx.x >> 6][0] = stack; s_red[threadIdx.x >> 6][1] = overflow; s_red[threadIdx.x >> 6][2] = (int32_t)excluded;
    }
    __syncthreads();
    if (threadIdx.x == 0) {          // one atomic per workgroup and word
        unsigned long long n = 0, c = 0, d = 0, o = 0, e = 0;
        for (int k = 0; k < VL_WAVES; ++k) {
            n += s_sum[k][0]; c += s_sum[k][1];
            d = (unsigned long long)s_red[k][0] > d ? (unsigned long long)s_red[k][0] : d;
            o |= (unsigned long long)s_red[k][1];
            e += (unsigned long long)s_red[k][2];
        }
        if (n) atomicAdd(stats + GP_VOLUME_NODES, n);
        if (c) atomicAdd(stats + GP_VOLUME_CANDIDATES, c);
        if (d) atomicMax(stats + GP_VOLUME_MAX_STACK, d);
        if (o) atomicOr(stats + GP_VOLUME_STATUS, 1ull);
        if (e) atomicAdd(stats + GP_VOLUME_EXCLUDED_QUERIES, e);
        if (blockIdx.x == 0) {       // (words nobody else writes)
            stats[GP_VOLUME_EXCLUDED_FACES] = (unsigned long long)(t.nf - usable);
            stats[GP_VOLUME_LEVELS] = (unsigned long long)t.levels;
            stats[GP_VOLUME_LEAVES] = (unsigned long long)t.count[0];
        }
    }
}

// ---- the query ----
__global__ void __launch_bounds__(VL_BLOCK) vl_query_kernel(const float* __restrict__ queries, uint32_t nq, VlTree t, const uint32_t* __restrict__ words,
                                                            const VlBox* __restrict__ boxes, const SfFace* __restrict__ sorted, float* __restrict__ dist2,
                                                            int32_t* __restrict__ face, int32_t* __restrict__ region, float* __restrict__ closest,
                                                            float* __restrict__ bary, unsigned long long* stats) {
    uint32_t usable = words[VL_WORD_USABLE];
    usable = usable < t.nf ? usable : t.nf;
    const float M = __uint_as_float(words[VL_WORD_M]);
    unsigned long long nodes = 0, candidates = 0;    // of this lane
    int32_t stack = 0, overflow = 0;
    uint32_t excluded = 0;                           // of this wave
    const uint32_t stride = gridDim.x * VL_BLOCK;
    for (uint32_t first = blockIdx.x * VL_BLOCK; first < nq; first += stride) {
        const uint32_t i = first + threadIdx.x;
        bool bad = false;
        if (i < nq) {
            const float q[3] = {queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2]};
            VlTally tally;
            int32_t f, k;
            float d, p[3], u[2];
            vl_query(t, boxes, sorted, usable, M, q, &d, &f, &k, p, u, &tally);
            dist2[i] = d; face[i] = f; region[i] = k;
            closest[3 * (size_t)i] = p[0]; closest[3 * (size_t)i + 1] = p[1]; closest[3 * (size_t)i + 2] = p[2];
            bary[2 * (size_t)i] = u[0]; bary[2 * (size_t)i + 1] = u[1];
            nodes += tally.nodes; candidates += tally.candidates;
            stack = tally.stack > stack ? tally.stack : stack;
            overflow |= tally.overflow;
            bad = !gm_usable(q);
        }
        excluded += (uint32_t)__popcll(__ballot(bad));
    }
    vl_flush(nodes, candidates, stack, overflow, excluded, t, usable, stats);
}

// ---- the lattice ----
__global__ void __launch_bounds__(VL_BLOCK) vl_lattice_kernel(VlTree t, const uint32_t* __restrict__ words, const VlBox* __restrict__ boxes, const SfFace* __restrict__ sorted,
                                                              const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t nv,
                                                              const int32_t* __restrict__ face_edges, const double* __restrict__ edge_normal, uint32_t n_edges,
                                                              const double* __restrict__ vertex_normal, float ox, float oy, float oz, float voxel, int32_t nx, int32_t ny,
                                                              uint32_t n, float* __restrict__ sdf, unsigned long long* stats) {
    __shared__ uint32_t s_tally[VL_WAVES][GP_SDF_STAT_WORDS];
    uint32_t usable = words[VL_WORD_USABLE];
    usable = usable < t.nf ? usable : t.nf;
    const float M = __uint_as_float(words[VL_WORD_M]);
    unsigned long long nodes = 0, candidates = 0;    // of this lane
    int32_t stack = 0, overflow = 0;
    uint32_t excluded = 0, tally_sign[GP_SDF_STAT_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};      // of this wave
    const uint32_t stride = gridDim.x * VL_BLOCK;
    for (uint32_t first = blockIdx.x * VL_BLOCK; first < n; first += stride) {           // (n < 2^31 and the stride is a multiple of the block: no wrap below 2^32)
        const uint32_t i = first + threadIdx.x;
        bool bad = false;
        int row = -1;
        int8_t sg = 0;
        int32_t kd = -1;
        if (i < n) {
            float p[3], d;
            VlTally tally;
            vl_point((int64_t)i, nx, ny, ox, oy, oz, voxel, p);
            row = vl_lattice_point(t, boxes, sorted, usable, M, p, vertices, faces, nv, t.nf, face_edges, edge_normal, n_edges, vertex_normal, &d, &sg, &kd, &tally);
            sdf[i] = d;
            nodes += tally.nodes; candidates += tally.candidates;
            stack = tally.stack > stack ? tally.stack : stack;
            overflow |= tally.overflow;
            bad = !gm_usable(p);
        }
        excluded += (uint32_t)__popcll(__ballot(bad));
        const bool is[GP_SDF_STAT_WORDS] = {row == SD_ROW_SIGNED && kd == GP_SDF_KIND_FACE, row == SD_ROW_SIGNED && kd == GP_SDF_KIND_EDGE,
                                            row == SD_ROW_SIGNED && kd == GP_SDF_KIND_VERTEX, row == SD_ROW_SIGNED && sg < 0, row == SD_ROW_SIGNED && sg > 0,
                                            row == SD_ROW_FOREIGN || (row == SD_ROW_SIGNED && sg == 0), row == SD_ROW_EXCLUDED, row == SD_ROW_FOREIGN};
#pragma unroll
        for (int w = 0; w < GP_SDF_STAT_WORDS; ++w) tally_sign[w] += (uint32_t)__popcll(__ballot(is[w]));
    }
    if ((threadIdx.x & 63) == 0)
        for (int w = 0; w < GP_SDF_STAT_WORDS; ++w) s_tally[threadIdx.x >> 6][w] = tally_sign[w];
    vl_flush(nodes, candidates, stack, overflow, excluded, t, usable, stats);          // (its barrier orders s_tally too)
    if (threadIdx.x < GP_SDF_STAT_WORDS) {           // one atomic per workgroup and word
        unsigned long long total = 0;
        for (int k = 0; k < VL_WAVES; ++k) total += s_tally[k][threadIdx.x];
        unsigned long long* out = stats + GP_VOLUME_STAT_WORDS;
        if (threadIdx.x == GP_SDF_STATUS) { if (total) atomicOr(out + GP_SDF_STATUS, 1ull); }
        else if (total) atomicAdd(out + threadIdx.x, total);
    }
}

// ---- the comparison ----
__global__ void __launch_bounds__(VL_BLOCK) vl_compare_kernel(const float* __restrict__ a, const float* __restrict__ b, uint32_t n, unsigned long long* counts) {
    __shared__ uint32_t s_tally[VL_WAVES][GP_VOLUME_POINTS];
    uint32_t tally[GP_VOLUME_POINTS] = {0, 0, 0, 0, 0};          // of this wave
    const uint32_t stride = gridDim.x * VL_BLOCK;
    for (uint32_t first = blockIdx.x * VL_BLOCK; first < n; first += stride) {
        const uint32_t i = first + threadIdx.x;
        const uint32_t bits = i < n ? vl_compare(a[i], b[i]) : 0u;
#pragma unroll
        for (int w = 0; w < GP_VOLUME_POINTS; ++w) tally[w] += (uint32_t)__popcll(__ballot((bits >> w) & 1u));
    }
    if ((threadIdx.x & 63) == 0)
        for (int w = 0; w < GP_VOLUME_POINTS; ++w) s_tally[threadIdx.x >> 6][w] = tally[w];
    __syncthreads();
    if (threadIdx.x < GP_VOLUME_POINTS) {            // one atomic per workgroup and word
        unsigned long long total = 0;
        for (int k = 0; k < VL_WAVES; ++k) total += s_tally[k][threadIdx.x];
        if (total) atomicAdd(counts + threadIdx.x, total);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[GP_VOLUME_POINTS] = (unsigned long long)n;
}

// ---- the C entries ----
#define VL_REFUSE(name, why_)                                   \
    do {                                                        \
        const char* w_ = (why_);                                \
        if (w_) GP_FAIL(name ": %s", w_);                       \
    } while (0)

#define VL_REFUSE_SCRATCH(name)                                                                     \
    do {                                                                                            \
        if (!scratch) GP_FAIL(name ": null argument (scratch)");                                    \
        if (((uintptr_t)scratch & 15u) != 0) GP_FAIL(name ": scratch must be 16-byte aligned");     \
    } while (0)

static VlScratch vl_scratch(int64_t nf) {
    const int64_t blocks = (nf + 1023) / 1024;                   // (the sort's smallest tile: enough for a sort of nf pairs)
    return vl_layout(nf, GP_VOLUME_LEAF, 256 * blocks + 64, (int64_t)gp_scan_tmp_elems((size_t)(256 * (blocks > 0 ? blocks : 1))));
}

static unsigned vl_capped(size_t n) {
    const unsigned b = gp_blocks(n, VL_BLOCK);
    return b < GM_MAX_BLOCKS ? (b > 0 ? b : 1) : GM_MAX_BLOCKS;
}

extern "C" int gp_volume_abi_version(void) { return GP_VOLUME_ABI_VERSION; }

extern "C" int64_t gp_volume_tree_scratch_bytes(int64_t nf) {
    const char* why = gm_refuse_mesh(0, nf);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_volume_tree_scratch_bytes: %s (nf = %lld)", why, (long long)nf);
        return -1;
    }
    return vl_scratch(nf).bytes;
}

extern "C" int gp_volume_tree(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, void* scratch, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    VL_REFUSE("gp_volume_tree", gm_refuse_mesh(nv, nf));
    VL_REFUSE_SCRATCH("gp_volume_tree");
    if (nf > 0 && (!faces || (nv > 0 && !vertices))) GP_FAIL("gp_volume_tree: null argument");
    const VlScratch s = vl_scratch(nf);
    const VlTree t = vl_tree(nf, GP_VOLUME_LEAF);
    char* base = (char*)scratch;
    uint32_t* words = (uint32_t*)(base + s.words);
    SfFace* records = (SfFace*)(base + s.records);
    SfFace* sorted = (SfFace*)(base + s.sorted);
    VlBox* boxes = (VlBox*)(base + s.boxes);
    GpSortBufs sb;
    for (int k = 0; k < 2; ++k) { sb.k[k] = (uint32_t*)(base + s.sort_k[k]); sb.v[k] = (uint32_t*)(base + s.sort_v[k]); }
    sb.hist = (uint32_t*)(base + s.sort_hist);
    sb.scan_tmp = (uint32_t*)(base + s.sort_tmp);
    sb.scan_tmp_elems = (size_t)s.sort_tmp_elems;
    const uint32_t NF = (uint32_t)nf;
    GpProfScope _p("volume_tree", st);
    GP_HIP_CHECK(hipMemsetAsync(words, 0xFF, 3 * sizeof(uint32_t), st));
    GP_HIP_CHECK(hipMemsetAsync(words + 3, 0, (VL_WORDS - 3) * sizeof(uint32_t), st));
    if (NF > 0) {
        const unsigned g_f = gp_blocks(NF, VL_BLOCK);
        hipLaunchKernelGGL(vl_prepare_kernel, dim3(vl_capped(NF)), dim3(VL_BLOCK), 0, st, vertices, faces, (uint32_t)nv, NF, records, words);
        GP_LAUNCH_CHECK();
        hipLaunchKernelGGL(vl_key_kernel, dim3(g_f), dim3(VL_BLOCK), 0, st, (const SfFace*)records, NF, (const uint32_t*)words, sb.k[0]);
        GP_LAUNCH_CHECK();
        const int r = gp_radix_sort_pairs(sb, NF, VL_KEY_BITS, st, true);
        if (r < 0) return 1;
        hipLaunchKernelGGL(vl_gather_kernel, dim3(g_f), dim3(VL_BLOCK), 0, st, (const SfFace*)records, (const uint32_t*)sb.v[r], NF, sorted);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(vl_leaf_kernel, dim3(gp_blocks(t.count[0], VL_BLOCK)), dim3(VL_BLOCK), 0, st, (const SfFace*)sorted, t, boxes);
    GP_LAUNCH_CHECK();
    for (uint32_t level = 1; level < t.levels; ++level) {
        hipLaunchKernelGGL(vl_level_kernel, dim3(gp_blocks(t.count[level], VL_BLOCK)), dim3(VL_BLOCK), 0, st, t, level, boxes);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gp_volume_query(const float* queries, int64_t nq, const void* scratch, int64_t nf, float* dist2, int32_t* face, int32_t* region, float* closest,
                               float* bary, int64_t* stats, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    VL_REFUSE("gp_volume_query", gm_refuse_mesh(0, nf));
    VL_REFUSE("gp_volume_query", gm_refuse_count(nq));
    VL_REFUSE_SCRATCH("gp_volume_query");
    if (!stats || (nq > 0 && (!queries || !dist2 || !face || !region || !closest || !bary))) GP_FAIL("gp_volume_query: null argument");
    const VlScratch s = vl_scratch(nf);
    const char* base = (const char*)scratch;
    GpProfScope _p("volume_query", st);
    GP_HIP_CHECK(hipMemsetAsync(stats, 0, GP_VOLUME_STAT_WORDS * sizeof(int64_t), st));
    // (nq == 0 still launches one workgroup: it writes the words of the tree)
    hipLaunchKernelGGL(vl_query_kernel, dim3(vl_capped((size_t)nq)), dim3(VL_BLOCK), 0, st, queries, (uint32_t)nq, vl_tree(nf, GP_VOLUME_LEAF),
                       (const uint32_t*)(base + s.words), (const VlBox*)(base + s.boxes), (const SfFace*)(base + s.sorted), dist2, face, region, closest, bary,
                       (unsigned long long*)stats);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_volume_lattice(const void* scratch, const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const int32_t* face_edges,
                                 const double* edge_normal, int64_t n_edges, const double* vertex_normal, float ox, float oy, float oz, float voxel, int32_t nx, int32_t ny,
                                 int32_t nz, float* sdf, int64_t* stats, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    VL_REFUSE("gp_volume_lattice", sd_refuse_tables(nv, nf, n_edges));
    VL_REFUSE("gp_volume_lattice", vl_refuse_lattice(ox, oy, oz, voxel, nx, ny, nz));
    VL_REFUSE_SCRATCH("gp_volume_lattice");
    if (!sdf || !stats || (nf > 0 && (!faces || !face_edges)) || (nv > 0 && (!vertices || !vertex_normal)) || (n_edges > 0 && !edge_normal))
        GP_FAIL("gp_volume_lattice: null argument");
    const VlScratch s = vl_scratch(nf);
    const char* base = (const char*)scratch;
    const uint32_t n = (uint32_t)((int64_t)nx * ny * nz);
    GpProfScope _p("volume_lattice", st);
    GP_HIP_CHECK(hipMemsetAsync(stats, 0, GP_VOLUME_LATTICE_WORDS * sizeof(int64_t), st));
    hipLaunchKernelGGL(vl_lattice_kernel, dim3(vl_capped((size_t)n)), dim3(VL_BLOCK), 0, st, vl_tree(nf, GP_VOLUME_LEAF), (const uint32_t*)(base + s.words),
                       (const VlBox*)(base + s.boxes), (const SfFace*)(base + s.sorted), vertices, faces, (uint32_t)nv, face_edges, edge_normal, (uint32_t)n_edges,
                       vertex_normal, ox, oy, oz, voxel, nx, ny, n, sdf, (unsigned long long*)stats);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_volume_compare(const float* sdf_a, const float* sdf_b, int64_t n, int64_t* counts, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    VL_REFUSE("gp_volume_compare", gm_refuse_count(n));
    if (!counts || (n > 0 && (!sdf_a || !sdf_b))) GP_FAIL("gp_volume_compare: null argument");
    GpProfScope _p("volume_compare", st);
    GP_HIP_CHECK(hipMemsetAsync(counts, 0, GP_VOLUME_COUNT_WORDS * sizeof(int64_t), st));
    hipLaunchKernelGGL(vl_compare_kernel, dim3(vl_capped((size_t)n)), dim3(VL_BLOCK), 0, st, sdf_a, sdf_b, (uint32_t)n, (unsigned long long*)counts);
    GP_LAUNCH_CHECK();
    return 0;
}
