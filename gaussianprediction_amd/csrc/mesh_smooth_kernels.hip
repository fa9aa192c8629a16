// mesh_smooth_kernels.hip -- the edges and the vertex adjacency of a triangle mesh, and Laplacian / Taubin smoothing over them, on the
// device (csrc/gp_mesh_smooth.h).  The programs of a lane are csrc/mesh_smooth_core.h and csrc/mesh_core.h, which also run on a CPU
// (tests/mesh_smooth_emulate.cpp).
//   mt_tally_kernel       a lane per face: the status word, kept faces and degenerate half-edges (integer atomicAdd, one per wave)
//   mt_sort_word_kernel   a lane per sorted position: the key word of the next pass of the sort and the entry it belongs to
//   mt_gather_kernel      a lane per sorted position: the two ends of its entry, the direction in the top bit of the second
//   mt_head_kernel        a lane per sorted position: the heads of the runs, those with first < second (the edges); an edge's head
//                         walks its run, marks the ends of boundary and non-manifold edges (plain byte stores of 1) and counts
//   mt_apply_kernel       a lane per sorted position: the heads write neighbours and edges at their ranks, never beyond what the caller
//                         allocated
//   mt_vertex_kernel      a lane per vertex (and one more): offsets by bisection, the flags
//   mt_step_kernel, mt_umbrella_kernel, mt_pinned_kernel       a lane per vertex and column: one list, one order
// around gp_radix_sort_pairs (two passes of one word each, the second end first: stable, so equal pairs stay in ascending entry) and
// the ordered compaction of mesh_kernels.hip.  No float atomics, no spinning, no fence: whatever one launch leaves for another
// crosses a launch boundary.
#include "gp_common.h"

#include "mesh_compact.h"
#include "mesh_smooth_core.h"

static_assert(MS_BLOCK == 4 * GP_WAVE, "four waves a workgroup");

// all 64 lanes of a wave call them
__device__ __forceinline__ void mt_wave_count(int32_t* word, bool mine) {
    const unsigned long long b = __ballot(mine);
    if (b != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) atomicAdd(word, (int32_t)__popcll(b));
}
__device__ __forceinline__ void mt_wave_add(int32_t* word, int32_t mine) {
    int32_t sum = mine;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if (sum != 0 && (threadIdx.x & 63) == 0) atomicAdd(word, sum);
}

// ---- the edges ----
__global__ void __launch_bounds__(MS_BLOCK) mt_tally_kernel(const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf, int32_t* counts) {
    const uint32_t f = blockIdx.x * MS_BLOCK + threadIdx.x;
    int32_t degenerate = 0;
    const bool kept = f < nf && mt_face_tally(faces, f, nv, counts, &degenerate);
    mt_wave_count(counts + GP_MESH_SMOOTH_FACES, kept);
    mt_wave_add(counts + GP_MESH_SMOOTH_DEGENERATE, degenerate);
}

// `before` may be the very array `element_out` (a lane reads its own word, then writes it)
__global__ void __launch_bounds__(MS_BLOCK) mt_sort_word_kernel(const int32_t* __restrict__ faces, const uint32_t* before, uint32_t n, int word, uint32_t nv,
                                                                uint32_t* __restrict__ key_out, uint32_t* element_out) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t e;
    key_out[i] = mt_sort_word(faces, before, i, word, nv, &e);
    element_out[i] = e;
}

__global__ void __launch_bounds__(MS_BLOCK) mt_gather_kernel(const int32_t* __restrict__ faces, const uint32_t* __restrict__ order, uint32_t n, uint32_t nv,
                                                             uint32_t* __restrict__ first, uint32_t* __restrict__ second) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = order[i];                     // (a permutation of 0 .. n - 1: the values the sort was handed)
    uint32_t a, b;
    mt_entry(faces, e, nv, &a, &b);
    first[i] = a;
    second[i] = b | ((e & 1u) ? MT_DIRECTION : 0u);
}

__global__ void __launch_bounds__(MS_BLOCK) mt_head_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ second, uint32_t n, uint32_t nv,
                                                           uint8_t* __restrict__ head_adj, uint8_t* __restrict__ head_edge, uint8_t* mark_boundary,
                                                           uint8_t* mark_nonmanifold, int32_t* counts) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    bool starts = false, boundary = false, nonmanifold = false, inconsistent = false;
    if (i < n) {
        const bool head = mt_is_head(first, second, i, nv);
        const uint32_t lo = first[i], hi = mt_end(second[i]);
        const bool edge = head && lo < hi;                       // (hi < nv then: an entry has both ends or neither)
        head_adj[i] = head;
        head_edge[i] = edge;
        starts = mt_starts_vertex(first, i, nv);
        if (edge) {
            int32_t face_count, wind;
            mt_run(first, second, i, n, &face_count, &wind);
            boundary = mt_is_boundary(face_count);
            nonmanifold = mt_is_nonmanifold(face_count);
            inconsistent = mt_is_inconsistent(face_count, wind);
            if (boundary) { mark_boundary[lo] = 1; mark_boundary[hi] = 1; }          // (every writer stores the same byte)
            if (nonmanifold) { mark_nonmanifold[lo] = 1; mark_nonmanifold[hi] = 1; }
        }
    }
    mt_wave_count(counts + GP_MESH_SMOOTH_VERTICES, starts);
    mt_wave_count(counts + GP_MESH_SMOOTH_BOUNDARY, boundary);
    mt_wave_count(counts + GP_MESH_SMOOTH_NONMANIFOLD, nonmanifold);
    mt_wave_count(counts + GP_MESH_SMOOTH_INCONSISTENT, inconsistent);
}

__global__ void __launch_bounds__(MS_BLOCK) mt_apply_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ second, const uint8_t* __restrict__ head_adj,
                                                            const uint8_t* __restrict__ head_edge, const uint32_t* __restrict__ rank_adj,
                                                            const uint32_t* __restrict__ rank_edge, uint32_t n, uint32_t n_edges, uint32_t* __restrict__ adj_src,
                                                            int32_t* __restrict__ neighbors, int32_t* __restrict__ edge, int32_t* __restrict__ face_count,
                                                            int32_t* __restrict__ wind) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= n || !head_adj[i]) return;
    const uint32_t lo = first[i], hi = mt_end(second[i]);
    const uint64_t r = rank_adj[i];
    if (r < 2ull * n_edges) {                        // (always, where n_edges is what the plan counted)
        adj_src[r] = lo;
        neighbors[r] = (int32_t)hi;
    }
    if (!head_edge[i]) return;
    const uint32_t e = rank_edge[i];
    if (e >= n_edges) return;
    int32_t c, w;
    mt_run(first, second, i, n, &c, &w);
    edge[2 * (size_t)e] = (int32_t)lo;
    edge[2 * (size_t)e + 1] = (int32_t)hi;
    face_count[e] = c;
    wind[e] = w;
}

// lanes 0 .. nv: offsets; lanes below nv: the flags
__global__ void __launch_bounds__(MS_BLOCK) mt_vertex_kernel(const uint32_t* __restrict__ adj_src, const int32_t* __restrict__ words, uint32_t n_edges, uint32_t nv,
                                                             const uint8_t* __restrict__ mark_boundary, const uint8_t* __restrict__ mark_nonmanifold,
                                                             int32_t* __restrict__ offsets, uint8_t* __restrict__ vertex_flags) {
    const uint64_t v = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v > nv) return;
    int64_t total = words[MT_WORD_ADJ];
    if (total > 2ll * n_edges) total = 2ll * n_edges;             // (what the caller allocated and mt_apply_kernel wrote)
    const int64_t begin = mt_lower_bound(adj_src, total, (int64_t)v);
    offsets[v] = (int32_t)begin;
    if (v < nv) vertex_flags[v] = mt_flags(mark_boundary[v], mark_nonmanifold[v], mt_lower_bound(adj_src, total, (int64_t)v + 1) - begin);
}

// ---- smoothing ----
__global__ void __launch_bounds__(MS_BLOCK) mt_step_kernel(const float* __restrict__ src, uint32_t total, uint32_t nv, uint32_t k, const int32_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ neighbors, int64_t n_neighbors, const uint8_t* __restrict__ pinned, uint8_t mask,
                                                           double s, float* __restrict__ dst) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= total) return;
    const uint32_t v = i / k;
    mt_step(src, nv, k, v, i - v * k, offsets, neighbors, n_neighbors, pinned, mask, s, dst);
}

__global__ void __launch_bounds__(MS_BLOCK) mt_umbrella_kernel(const float* __restrict__ src, uint32_t total, uint32_t nv, uint32_t k, const int32_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ neighbors, int64_t n_neighbors, float* __restrict__ dst) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= total) return;
    const uint32_t v = i / k;
    mt_umbrella(src, nv, k, v, i - v * k, offsets, neighbors, n_neighbors, dst);
}

__global__ void __launch_bounds__(MS_BLOCK) mt_pinned_kernel(const uint8_t* __restrict__ pinned, uint8_t mask, uint32_t nv, int32_t* count) {
    const uint32_t v = blockIdx.x * MS_BLOCK + threadIdx.x;
    mt_wave_count(count, v < nv && mt_is_pinned(pinned, mask, v));
}

// ---- the C entries ----
static MtScratch mt_layout(int64_t nv, int64_t nf) {
    const int64_t blocks = (6 * nf + 1023) / 1024;              // (the sort's smallest tile: enough for a sort of any n <= 6 nf)
    return mt_scratch_layout(nv, nf, 256 * blocks + 64, (int64_t)gp_scan_tmp_elems((size_t)(256 * (blocks > 0 ? blocks : 1))));
}

#define MT_REFUSE_COMMON(name)                                                                      \
    do {                                                                                            \
        const char* why_ = mt_refuse_sizes(nv, nf);                                                 \
        if (why_) GP_FAIL(name ": %s (nv = %lld, nf = %lld)", why_, (long long)nv, (long long)nf);  \
        if (!scratch) GP_FAIL(name ": null argument (scratch)");                                    \
        if (((uintptr_t)scratch & 7u) != 0) GP_FAIL(name ": scratch must be 8-byte aligned");       \
    } while (0)

#define MT_REFUSE_ROWS(name)                                                                        \
    do {                                                                                            \
        const char* why_ = mt_refuse_rows(nv, k);                                                   \
        if (why_) GP_FAIL(name ": %s (nv = %lld, k = %d)", why_, (long long)nv, k);                 \
        if (n_neighbors < 0 || n_neighbors >= 0x80000000LL) GP_FAIL(name ": n_neighbors must be 0 .. 2^31 - 1 (n_neighbors = %lld)", (long long)n_neighbors); \
    } while (0)

extern "C" int gp_mesh_smooth_abi_version(void) { return GP_MESH_SMOOTH_ABI_VERSION; }

extern "C" int64_t gp_mesh_smooth_scratch_bytes(int64_t nv, int64_t nf) {
    const char* why = mt_refuse_sizes(nv, nf);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_mesh_smooth_scratch_bytes: %s (nv = %lld, nf = %lld)", why, (long long)nv, (long long)nf);
        return -1;
    }
    return mt_layout(nv, nf).bytes;
}

extern "C" int gp_mesh_smooth_edges_plan(const int32_t* faces, int64_t nv, int64_t nf, void* scratch, int32_t* counts, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MT_REFUSE_COMMON("gp_mesh_smooth_edges_plan");
    if (!counts || (nf > 0 && !faces)) GP_FAIL("gp_mesh_smooth_edges_plan: null argument");
    const MtScratch s = mt_layout(nv, nf);
    char* base = (char*)scratch;
    int32_t* words = (int32_t*)(base + s.words);
    uint32_t* first = (uint32_t*)(base + s.first);
    uint32_t* second = (uint32_t*)(base + s.second);
    uint8_t* head_adj = (uint8_t*)(base + s.head_adj);
    uint8_t* head_edge = (uint8_t*)(base + s.head_edge);
    uint8_t* mark_boundary = (uint8_t*)(base + s.mark_boundary);
    uint8_t* mark_nonmanifold = (uint8_t*)(base + s.mark_nonmanifold);
    GpSortBufs sb;
    for (int k = 0; k < 2; ++k) { sb.k[k] = (uint32_t*)(base + s.sort_k[k]); sb.v[k] = (uint32_t*)(base + s.sort_v[k]); }
    sb.hist = (uint32_t*)(base + s.sort_hist);
    sb.scan_tmp = (uint32_t*)(base + s.sort_tmp);
    sb.scan_tmp_elems = (size_t)s.sort_tmp_elems;
    const uint32_t NV = (uint32_t)nv, NF = (uint32_t)nf, N6 = (uint32_t)(6 * nf);
    const unsigned g_f = gp_blocks(NF, MS_BLOCK), g_6 = gp_blocks(N6, MS_BLOCK);
    GpProfScope _p("mesh_smooth_edges_plan", st);
    GP_HIP_CHECK(hipMemsetAsync(counts, 0, GP_MESH_SMOOTH_COUNT_WORDS * sizeof(int32_t), st));
    GP_HIP_CHECK(hipMemsetAsync(words, 0, 8 * sizeof(int32_t), st));
    if (NV > 0) {
        GP_HIP_CHECK(hipMemsetAsync(mark_boundary, 0, (size_t)NV, st));
        GP_HIP_CHECK(hipMemsetAsync(mark_nonmanifold, 0, (size_t)NV, st));
    }
    if (NF > 0) {
        hipLaunchKernelGGL(mt_tally_kernel, dim3(g_f), dim3(MS_BLOCK), 0, st, faces, NV, NF, counts);
        GP_LAUNCH_CHECK();
        const int bits = ms_bits(nv);                             // (the largest key: nv, of what is no entry)
        const uint32_t* order = nullptr;
        for (int word = 1; word >= 0; --word) {
            hipLaunchKernelGGL(mt_sort_word_kernel, dim3(g_6), dim3(MS_BLOCK), 0, st, faces, order, N6, word, NV, sb.k[0], sb.v[0]);
            GP_LAUNCH_CHECK();
            const int r = gp_radix_sort_pairs(sb, N6, bits, st, false);
            if (r < 0) return 1;
            order = sb.v[r];
        }
        hipLaunchKernelGGL(mt_gather_kernel, dim3(g_6), dim3(MS_BLOCK), 0, st, faces, order, N6, NV, first, second);
        GP_LAUNCH_CHECK();
        hipLaunchKernelGGL(mt_head_kernel, dim3(g_6), dim3(MS_BLOCK), 0, st, (const uint32_t*)first, (const uint32_t*)second, N6, NV, head_adj, head_edge, mark_boundary,
                           mark_nonmanifold, counts);
        GP_LAUNCH_CHECK();
    }
    if (ms_compact(head_adj, N6, (uint32_t*)(base + s.tile_adj), (uint32_t*)(base + s.rank_adj), words + MT_WORD_ADJ, st)) return 1;
    if (ms_compact(head_edge, N6, (uint32_t*)(base + s.tile_edge), (uint32_t*)(base + s.rank_edge), counts + GP_MESH_SMOOTH_EDGES, st)) return 1;
    return 0;
}

extern "C" int gp_mesh_smooth_edges_apply(int64_t nv, int64_t nf, int64_t n_edges, const void* scratch, int32_t* edge, int32_t* face_count, int32_t* wind,
                                          int32_t* offsets, int32_t* neighbors, uint8_t* vertex_flags, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MT_REFUSE_COMMON("gp_mesh_smooth_edges_apply");
    if (n_edges < 0 || n_edges > 3 * nf) GP_FAIL("gp_mesh_smooth_edges_apply: n_edges must be 0 .. 3*nf (n_edges = %lld, nf = %lld)", (long long)n_edges, (long long)nf);
    if (!offsets || (nv > 0 && !vertex_flags) || (n_edges > 0 && (!edge || !face_count || !wind || !neighbors))) GP_FAIL("gp_mesh_smooth_edges_apply: null argument");
    const MtScratch s = mt_layout(nv, nf);
    const char* base = (const char*)scratch;
    uint32_t* adj_src = (uint32_t*)((char*)scratch + s.adj_src);          // (the one array of the scratch this entry writes)
    const uint32_t NV = (uint32_t)nv, N6 = (uint32_t)(6 * nf), NE = (uint32_t)n_edges;
    GpProfScope _p("mesh_smooth_edges_apply", st);
    if (N6 > 0 && NE > 0) {
        hipLaunchKernelGGL(mt_apply_kernel, dim3(gp_blocks(N6, MS_BLOCK)), dim3(MS_BLOCK), 0, st, (const uint32_t*)(base + s.first), (const uint32_t*)(base + s.second),
                           (const uint8_t*)(base + s.head_adj), (const uint8_t*)(base + s.head_edge), (const uint32_t*)(base + s.rank_adj),
                           (const uint32_t*)(base + s.rank_edge), N6, NE, adj_src, neighbors, edge, face_count, wind);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(mt_vertex_kernel, dim3(gp_blocks((size_t)NV + 1, MS_BLOCK)), dim3(MS_BLOCK), 0, st, (const uint32_t*)adj_src, (const int32_t*)(base + s.words), NE, NV,
                       (const uint8_t*)(base + s.mark_boundary), (const uint8_t*)(base + s.mark_nonmanifold), offsets, vertex_flags);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gp_mesh_smooth_rows_bytes(int64_t nv, int32_t k) {
    const char* why = mt_refuse_rows(nv, k);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_mesh_smooth_rows_bytes: %s (nv = %lld, k = %d)", why, (long long)nv, k);
        return -1;
    }
    return 2 * ((4 * nv * k + 255) / 256 * 256) + 256;
}

extern "C" int gp_mesh_smooth_steps(const float* src, int64_t nv, int32_t k, const int32_t* offsets, const int32_t* neighbors, int64_t n_neighbors,
                                    const uint8_t* pinned, int32_t method, int32_t boundary, int32_t iterations, double lambda_, double mu, void* scratch, float* dst,
                                    int32_t* pinned_count, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MT_REFUSE_ROWS("gp_mesh_smooth_steps");
    const char* why = mt_refuse_options(method, boundary, iterations, lambda_, mu);
    if (why) GP_FAIL("gp_mesh_smooth_steps: %s (iterations = %d, lambda_ = %g, mu = %g)", why, iterations, lambda_, mu);
    if (!scratch) GP_FAIL("gp_mesh_smooth_steps: null argument (scratch)");
    if (((uintptr_t)scratch & 7u) != 0) GP_FAIL("gp_mesh_smooth_steps: scratch must be 8-byte aligned");
    const uint8_t mask = boundary == GP_MESH_SMOOTH_FIXED ? (GP_MESH_SMOOTH_FLAG_BOUNDARY | GP_MESH_SMOOTH_FLAG_NONMANIFOLD) : 0;
    if (!offsets || (nv > 0 && (!src || !dst || (mask && !pinned))) || (n_neighbors > 0 && !neighbors)) GP_FAIL("gp_mesh_smooth_steps: null argument");
    GpProfScope _p("mesh_smooth_steps", st);
    const uint32_t NV = (uint32_t)nv;
    if (pinned_count) {
        GP_HIP_CHECK(hipMemsetAsync(pinned_count, 0, sizeof(int32_t), st));
        if (NV > 0 && mask) {
            hipLaunchKernelGGL(mt_pinned_kernel, dim3(gp_blocks(NV, MS_BLOCK)), dim3(MS_BLOCK), 0, st, pinned, mask, NV, pinned_count);
            GP_LAUNCH_CHECK();
        }
    }
    if (nv == 0) return 0;
    const uint32_t total = (uint32_t)(nv * k);
    const int64_t steps = mt_steps(method, iterations), stride = (4 * nv * k + 255) / 256 * 256;
    if (steps == 0) {
        GP_HIP_CHECK(hipMemcpyAsync(dst, src, 4 * (size_t)total, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    float* buf[2] = {(float*)scratch, (float*)((char*)scratch + stride)};
    const float* from = src;
    for (int64_t step = 0; step < steps; ++step) {
        float* to = step + 1 == steps ? dst : buf[step & 1];
        hipLaunchKernelGGL(mt_step_kernel, dim3(gp_blocks(total, MS_BLOCK)), dim3(MS_BLOCK), 0, st, from, total, NV, (uint32_t)k, offsets, neighbors, n_neighbors, pinned, mask,
                           mt_factor(method, step, lambda_, mu), to);
        GP_LAUNCH_CHECK();
        from = to;
    }
    return 0;
}

extern "C" int gp_mesh_smooth_umbrella(const float* src, int64_t nv, int32_t k, const int32_t* offsets, const int32_t* neighbors, int64_t n_neighbors, float* dst,
                                       gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MT_REFUSE_ROWS("gp_mesh_smooth_umbrella");
    if (!offsets || (nv > 0 && (!src || !dst)) || (n_neighbors > 0 && !neighbors)) GP_FAIL("gp_mesh_smooth_umbrella: null argument");
    if (nv == 0) return 0;
    const uint32_t total = (uint32_t)(nv * k);
    GpProfScope _p("mesh_smooth_umbrella", st);
    hipLaunchKernelGGL(mt_umbrella_kernel, dim3(gp_blocks(total, MS_BLOCK)), dim3(MS_BLOCK), 0, st, src, total, (uint32_t)nv, (uint32_t)k, offsets, neighbors, n_neighbors, dst);
    GP_LAUNCH_CHECK();
    return 0;
}
