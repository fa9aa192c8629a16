// mesh_simplify_kernels.hip -- welding and vertex clustering of a triangle mesh on the device (csrc/gp_mesh_simplify.h).  The programs
// of a lane are csrc/mesh_simplify_core.h and csrc/mesh_core.h, which also run on a CPU (tests/mesh_simplify_emulate.cpp).
//   mz_bounds_partial_kernel, mz_bounds_final_kernel   min and max of the finite coordinates: a partial result per workgroup, ONE
//                         workgroup folds them (comparisons only: no order to keep, no float atomics)
//   mz_key_kernel         a lane per vertex: its three key words
//   mz_sort_word_kernel   a lane per sorted position: the key word of the next pass of the sort and the element it belongs to
//   mz_head_kernel        a lane per sorted position: the head of a run of equal keys flagged at the position and at its vertex
//   mz_segment_kernel     the heads' runs: where each begins, and its cluster number (the rank of its vertex among the flagged)
//   mz_cluster_kernel     a lane per sorted position: its vertex's cluster; the heads write their cluster's member range
//   mz_contract_kernel    a lane per cluster and column: the contracted positions of ALL clusters (the zero-area test reads them)
//   mz_face_kernel        a lane per face: skipped, collapsed, zero-area or surviving, its rotated triple; the counts by integer
//                         atomicAdd, one per wave
//   mz_duplicate_kernel   a lane per sorted position of the faces: a copy of the face before it is dropped
//   mz_keep_cluster_kernel, mz_mark_kernel             which clusters stay (plain byte stores of 1)
//   mz_apply_vertex_kernel, mz_apply_face_kernel, mz_rows_kernel       the outputs
// around gp_radix_sort_pairs (three passes of one word each, least significant first: stable, so the members of a cluster stay in
// ascending old index) and the ordered compaction of mesh_kernels.hip.  No float atomics, no spinning, no fence: whatever one launch
// leaves for another crosses a launch boundary.
#include "gp_common.h"

#include "mesh_compact.h"
#include "mesh_simplify_core.h"

static_assert(MS_BLOCK == 4 * GP_WAVE, "four waves a workgroup");

// ---- the bounds ----
__device__ __forceinline__ void mz_bounds_block_fold(float* acc, float* s_part /* [MS_BLOCK / GP_WAVE][MZ_BOUNDS_WORDS] */) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        float other[MZ_BOUNDS_WORDS];
#pragma unroll
        for (int a = 0; a < MZ_BOUNDS_WORDS; ++a) other[a] = __shfl_xor(acc[a], d);
        mz_bounds_merge(acc, other);
    }
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < MZ_BOUNDS_WORDS; ++a) s_part[(threadIdx.x >> 6) * MZ_BOUNDS_WORDS + a] = acc[a];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < MS_BLOCK / GP_WAVE; ++w) mz_bounds_merge(acc, s_part + w * MZ_BOUNDS_WORDS);
}

__global__ void __launch_bounds__(MS_BLOCK) mz_bounds_partial_kernel(const float* __restrict__ vertices, uint32_t nv, float* __restrict__ partial) {
    __shared__ float s_part[(MS_BLOCK / GP_WAVE) * MZ_BOUNDS_WORDS];
    float acc[MZ_BOUNDS_WORDS];
    mz_bounds_start(acc);
    for (uint64_t v = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x; v < nv; v += (uint64_t)gridDim.x * MS_BLOCK) mz_bounds_fold(acc, vertices + 3 * v);
    mz_bounds_block_fold(acc, s_part);
    if (threadIdx.x == 0)
        for (int a = 0; a < MZ_BOUNDS_WORDS; ++a) partial[blockIdx.x * MZ_BOUNDS_WORDS + a] = acc[a];
}

// ONE workgroup
__global__ void __launch_bounds__(MS_BLOCK) mz_bounds_final_kernel(const float* __restrict__ partial, uint32_t rows, double* __restrict__ record) {
    __shared__ float s_part[(MS_BLOCK / GP_WAVE) * MZ_BOUNDS_WORDS];
    float acc[MZ_BOUNDS_WORDS];
    mz_bounds_start(acc);
    for (uint32_t r = threadIdx.x; r < rows; r += MS_BLOCK) mz_bounds_merge(acc, partial + r * MZ_BOUNDS_WORDS);
    mz_bounds_block_fold(acc, s_part);
    if (threadIdx.x == 0) mz_bounds_record(acc, record);
}

// ---- clusters ----
__global__ void __launch_bounds__(MS_BLOCK) mz_key_kernel(const float* __restrict__ vertices, uint32_t nv, MzGrid grid, uint32_t* __restrict__ keys, int32_t* counts) {
    const uint32_t v = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= nv) return;
    uint32_t key[3];
    mz_key(grid, vertices + 3 * (size_t)v, key, counts);
    keys[3 * (size_t)v] = key[0]; keys[3 * (size_t)v + 1] = key[1]; keys[3 * (size_t)v + 2] = key[2];
}

// `before` may be the very array `element_out` (a lane reads its own word, then writes it)
__global__ void __launch_bounds__(MS_BLOCK) mz_sort_word_kernel(const uint32_t* __restrict__ keys, const uint32_t* before, uint32_t n, int word,
                                                                uint32_t* __restrict__ key_out, uint32_t* element_out) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t e;
    key_out[i] = mz_sort_word(keys, before, i, word, &e);
    element_out[i] = e;
}

__global__ void __launch_bounds__(MS_BLOCK) mz_head_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order, uint32_t nv,
                                                           uint32_t* __restrict__ members, uint8_t* __restrict__ head_pos, uint8_t* __restrict__ head_vertex) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= nv) return;
    const uint32_t v = order[i];                     // (a permutation of 0 .. nv - 1: the values the sort was handed)
    const uint8_t head = mz_is_head(keys, order, i);
    members[i] = v;
    head_pos[i] = head;
    head_vertex[v] = head;
}

__global__ void __launch_bounds__(MS_BLOCK) mz_segment_kernel(const uint32_t* __restrict__ members, const uint8_t* __restrict__ head_pos,
                                                              const uint32_t* __restrict__ rank_pos, const uint32_t* __restrict__ rank_vertex, uint32_t nv,
                                                              uint32_t* __restrict__ seg_begin, int32_t* __restrict__ seg_cluster) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= nv || !head_pos[i]) return;
    const uint32_t s = mz_segment(rank_pos[i], true);          // (below the heads counted, which are at most nv)
    seg_begin[s] = i;
    seg_cluster[s] = (int32_t)rank_vertex[members[i]];
}

__global__ void __launch_bounds__(MS_BLOCK) mz_cluster_kernel(const uint32_t* __restrict__ members, const uint8_t* __restrict__ head_pos,
                                                              const uint32_t* __restrict__ rank_pos, const uint32_t* __restrict__ seg_begin,
                                                              const int32_t* __restrict__ seg_cluster, const int32_t* __restrict__ words, uint32_t nv,
                                                              int32_t* __restrict__ cluster, uint32_t* __restrict__ begin, uint32_t* __restrict__ end) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= nv) return;
    const bool head = head_pos[i] != 0;
    const uint32_t s = mz_segment(rank_pos[i], head), segments = (uint32_t)words[MZ_WORD_SPARE];
    if (s >= segments) return;                       // (cannot be: position 0 is a head)
    const int32_t c = seg_cluster[s];
    cluster[members[i]] = c;
    if (head) {
        begin[c] = i;
        end[c] = s + 1 < segments ? seg_begin[s + 1] : nv;
    }
}

__global__ void __launch_bounds__(MS_BLOCK) mz_contract_kernel(const float* __restrict__ vertices, const uint32_t* __restrict__ members,
                                                               const uint32_t* __restrict__ begin, const uint32_t* __restrict__ end,
                                                               const int32_t* __restrict__ words, uint64_t total, int32_t contraction, float* __restrict__ positions) {
    const uint64_t i = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;          // (3 nv may pass 2^32)
    if (i >= total) return;
    const uint32_t c = (uint32_t)(i / 3u), j = (uint32_t)(i - 3u * (uint64_t)c);
    if (c >= (uint32_t)words[MZ_WORD_CLUSTERS]) return;
    mz_contract(vertices, 3, j, members, begin[c], end[c], contraction, positions + i);
}

// ---- faces ----
// all 64 lanes of a wave call it
__device__ __forceinline__ void mz_wave_count(int32_t* word, bool mine) {
    const unsigned long long b = __ballot(mine);
    if (b != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) atomicAdd(word, (int32_t)__popcll(b));
}

__global__ void __launch_bounds__(MS_BLOCK) mz_face_kernel(const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf, const int32_t* __restrict__ cluster,
                                                           const float* __restrict__ positions, int32_t drop_zero_area, int32_t* __restrict__ rot,
                                                           uint8_t* __restrict__ keep_face, int32_t* counts) {
    const uint32_t f = blockIdx.x * MS_BLOCK + threadIdx.x;
    int what = MZ_SKIPPED;
    if (f < nf) {
        int32_t r[3];
        what = mz_face_class(faces, f, nv, cluster, positions, drop_zero_area, r, counts);
        rot[3 * (size_t)f] = r[0]; rot[3 * (size_t)f + 1] = r[1]; rot[3 * (size_t)f + 2] = r[2];
        keep_face[f] = what == MZ_KEPT;
    }
    mz_wave_count(counts + GP_MESH_SIMPLIFY_COLLAPSED, what == MZ_COLLAPSED);
    mz_wave_count(counts + GP_MESH_SIMPLIFY_ZERO_AREA, what == MZ_ZERO_AREA);
}

__global__ void __launch_bounds__(MS_BLOCK) mz_duplicate_kernel(const uint32_t* __restrict__ rot, const uint32_t* __restrict__ order, uint32_t nv, uint32_t nf,
                                                                uint8_t* __restrict__ keep_face, int32_t* counts) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    const bool copy = i < nf && mz_is_duplicate(rot, order, i, nv);
    if (copy) keep_face[order[i]] = 0;               // (a permutation of 0 .. nf - 1)
    mz_wave_count(counts + GP_MESH_SIMPLIFY_DUPLICATES, copy);
}

__global__ void __launch_bounds__(MS_BLOCK) mz_keep_cluster_kernel(const int32_t* __restrict__ words, uint32_t nv, int32_t keep_unreferenced,
                                                                   uint8_t* __restrict__ keep_cluster) {
    const uint32_t c = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (c < nv) keep_cluster[c] = keep_unreferenced && c < (uint32_t)words[MZ_WORD_CLUSTERS];
}

__global__ void __launch_bounds__(MS_BLOCK) mz_mark_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep_face, const int32_t* __restrict__ cluster,
                                                           uint32_t nf, uint8_t* keep_cluster) {
    const uint32_t f = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (f >= nf || !keep_face[f]) return;            // (a kept face: its indices were checked)
    for (int c = 0; c < 3; ++c) keep_cluster[cluster[faces[3 * (size_t)f + c]]] = 1;          // (every writer stores the same byte)
}

// ---- the outputs ----
__global__ void __launch_bounds__(MS_BLOCK) mz_apply_vertex_kernel(const int32_t* __restrict__ cluster, const uint8_t* __restrict__ keep_cluster,
                                                                   const uint32_t* __restrict__ rank_cluster, const float* __restrict__ positions,
                                                                   const uint32_t* __restrict__ begin, const uint32_t* __restrict__ end, uint32_t nv,
                                                                   float* __restrict__ vertices_out, int32_t* __restrict__ vertex_map, int32_t* __restrict__ vertex_counts) {
    const uint32_t v = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= nv) return;
    const int32_t c = cluster[v];
    vertex_map[v] = keep_cluster[c] ? (int32_t)rank_cluster[c] : -1;
    if (!keep_cluster[v]) return;                    // lane v as cluster v (0 beyond C)
    const size_t r = rank_cluster[v];                // (below the kept clusters counted)
    for (int a = 0; a < 3; ++a) vertices_out[3 * r + a] = positions[3 * (size_t)v + a];
    vertex_counts[r] = (int32_t)(end[v] - begin[v]);
}

__global__ void __launch_bounds__(MS_BLOCK) mz_apply_face_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep_face,
                                                                 const uint32_t* __restrict__ rank_face, const int32_t* __restrict__ cluster,
                                                                 const uint32_t* __restrict__ rank_cluster, uint32_t nf, int32_t* __restrict__ face_index,
                                                                 int32_t* __restrict__ faces_out) {
    const uint32_t f = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (f >= nf || !keep_face[f]) return;
    const size_t r = rank_face[f];
    face_index[r] = (int32_t)f;
    for (int c = 0; c < 3; ++c) faces_out[3 * r + c] = (int32_t)rank_cluster[cluster[faces[3 * (size_t)f + c]]];
}

__global__ void __launch_bounds__(MS_BLOCK) mz_rows_kernel(const float* __restrict__ src, uint32_t total, uint32_t k, int32_t contraction,
                                                           const uint32_t* __restrict__ members, const uint32_t* __restrict__ begin, const uint32_t* __restrict__ end,
                                                           const uint8_t* __restrict__ keep_cluster, const uint32_t* __restrict__ rank_cluster, float* __restrict__ dst) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= total) return;
    const uint32_t c = i / k, j = i - c * k;
    if (!keep_cluster[c]) return;
    mz_contract(src, k, j, members, begin[c], end[c], contraction, dst + (size_t)rank_cluster[c] * k + j);
}

// ---- the C entries ----
static MzScratch mz_layout(int64_t nv, int64_t nf) {
    const int64_t sort_n = nf > nv ? nf : nv;
    const int64_t blocks = (sort_n + 1023) / 1024;              // (the sort's smallest tile: enough for a sort of any n <= sort_n)
    return mz_scratch_layout(nv, nf, 256 * blocks + 64, (int64_t)gp_scan_tmp_elems((size_t)(256 * (blocks > 0 ? blocks : 1))));
}

static GpSortBufs mz_sort_bufs(char* base, const MzScratch& s) {
    GpSortBufs sb;
    for (int k = 0; k < 2; ++k) { sb.k[k] = (uint32_t*)(base + s.sort_k[k]); sb.v[k] = (uint32_t*)(base + s.sort_v[k]); }
    sb.hist = (uint32_t*)(base + s.sort_hist);
    sb.scan_tmp = (uint32_t*)(base + s.sort_tmp);
    sb.scan_tmp_elems = (size_t)s.sort_tmp_elems;
    return sb;
}

// the stable sort of 0 .. n - 1 under the three words keys[e][0 .. 3), word 0 the most significant: the sorted elements, or null
static const uint32_t* mz_sort3(GpSortBufs& sb, const uint32_t* keys, uint32_t n, const int* bits, hipStream_t st) {
    const uint32_t* order = nullptr;
    for (int word = 2; word >= 0; --word) {
        hipLaunchKernelGGL(mz_sort_word_kernel, dim3(gp_blocks(n, MS_BLOCK)), dim3(MS_BLOCK), 0, st, keys, order, n, word, sb.k[0], sb.v[0]);
        if (hipGetLastError() != hipSuccess) { snprintf(gp_err_buf, sizeof(gp_err_buf), "mz_sort_word_kernel: launch failed"); return nullptr; }
        const int r = gp_radix_sort_pairs(sb, n, bits[word], st, false);
        if (r < 0) return nullptr;
        order = sb.v[r];
    }
    return order;
}

#define MZ_REFUSE_COMMON(name)                                                                      \
    do {                                                                                            \
        const char* why_ = ms_refuse_sizes(nv, nf);                                                 \
        if (why_) GP_FAIL(name ": %s (nv = %lld, nf = %lld)", why_, (long long)nv, (long long)nf);  \
        if (!scratch) GP_FAIL(name ": null argument (scratch)");                                    \
        if (((uintptr_t)scratch & 7u) != 0) GP_FAIL(name ": scratch must be 8-byte aligned");       \
    } while (0)

extern "C" int gp_mesh_simplify_abi_version(void) { return GP_MESH_SIMPLIFY_ABI_VERSION; }

extern "C" int64_t gp_mesh_simplify_scratch_bytes(int64_t nv, int64_t nf) {
    const char* why = ms_refuse_sizes(nv, nf);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_mesh_simplify_scratch_bytes: %s (nv = %lld, nf = %lld)", why, (long long)nv, (long long)nf);
        return -1;
    }
    return mz_layout(nv, nf).bytes;
}

extern "C" int gp_mesh_simplify_bounds(const float* vertices, int64_t nv, void* scratch, double* record, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const int64_t nf = 0;
    MZ_REFUSE_COMMON("gp_mesh_simplify_bounds");
    if (nv < 1) GP_FAIL("gp_mesh_simplify_bounds: nv must be >= 1 (nv = %lld)", (long long)nv);
    if (!vertices || !record) GP_FAIL("gp_mesh_simplify_bounds: null argument");
    if (((uintptr_t)record & 7u) != 0) GP_FAIL("gp_mesh_simplify_bounds: record must be 8-byte aligned");
    const MzScratch s = mz_scratch_layout(nv, 0, 0, 0);          // (the partial results lie before everything the sizes move)
    float* partial = (float*)((char*)scratch + s.partial);
    const unsigned rows = gp_blocks((size_t)nv, MS_BLOCK) < MZ_BOUNDS_BLOCKS ? gp_blocks((size_t)nv, MS_BLOCK) : MZ_BOUNDS_BLOCKS;
    GpProfScope _p("mesh_simplify_bounds", st);
    hipLaunchKernelGGL(mz_bounds_partial_kernel, dim3(rows), dim3(MS_BLOCK), 0, st, vertices, (uint32_t)nv, partial);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(mz_bounds_final_kernel, dim3(1), dim3(MS_BLOCK), 0, st, (const float*)partial, (uint32_t)rows, record);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_mesh_simplify_plan(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, int32_t mode, double voxel_size, const double* bounds,
                                     int32_t contraction, int32_t drop_zero_area, int32_t drop_duplicates, int32_t keep_unreferenced, void* scratch,
                                     int32_t* counts, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MZ_REFUSE_COMMON("gp_mesh_simplify_plan");
    MzGrid grid;
    const char* why = mz_plan_grid(grid, mode, voxel_size, bounds);
    if (why) GP_FAIL("gp_mesh_simplify_plan: %s (voxel_size = %g)", why, voxel_size);
    if (mode == GP_MESH_SIMPLIFY_WELD) contraction = GP_MESH_SIMPLIFY_FIRST;
    if (contraction != GP_MESH_SIMPLIFY_FIRST && contraction != GP_MESH_SIMPLIFY_AVERAGE)
        GP_FAIL("gp_mesh_simplify_plan: contraction must be GP_MESH_SIMPLIFY_FIRST or GP_MESH_SIMPLIFY_AVERAGE (contraction = %d)", contraction);
    if (!counts || (nv > 0 && !vertices) || (nf > 0 && !faces)) GP_FAIL("gp_mesh_simplify_plan: null argument");
    const MzScratch s = mz_layout(nv, nf);
    char* base = (char*)scratch;
    int32_t* words = (int32_t*)(base + s.words);
    uint32_t* keys = (uint32_t*)(base + s.keys);
    uint32_t* members = (uint32_t*)(base + s.members);
    uint8_t* head_pos = (uint8_t*)(base + s.head_pos);
    uint8_t* head_vertex = (uint8_t*)(base + s.head_vertex);
    uint32_t* rank_pos = (uint32_t*)(base + s.rank_pos);
    uint32_t* rank_vertex = (uint32_t*)(base + s.rank_vertex);
    uint32_t* seg_begin = (uint32_t*)(base + s.seg_begin);
    int32_t* seg_cluster = (int32_t*)(base + s.seg_cluster);
    int32_t* cluster = (int32_t*)(base + s.cluster);
    uint32_t* begin = (uint32_t*)(base + s.begin);
    uint32_t* end = (uint32_t*)(base + s.end);
    float* positions = (float*)(base + s.positions);
    uint8_t* keep_cluster = (uint8_t*)(base + s.keep_cluster);
    uint32_t* rank_cluster = (uint32_t*)(base + s.rank_cluster);
    int32_t* rot = (int32_t*)(base + s.rot);
    uint8_t* keep_face = (uint8_t*)(base + s.keep_face);
    uint32_t* rank_face = (uint32_t*)(base + s.rank_face);
    GpSortBufs sb = mz_sort_bufs(base, s);
    const uint32_t NV = (uint32_t)nv, NF = (uint32_t)nf;
    const unsigned g_v = gp_blocks(NV, MS_BLOCK), g_f = gp_blocks(NF, MS_BLOCK);
    GpProfScope _p("mesh_simplify_plan", st);
    GP_HIP_CHECK(hipMemsetAsync(counts, 0, GP_MESH_SIMPLIFY_COUNT_WORDS * sizeof(int32_t), st));
    GP_HIP_CHECK(hipMemsetAsync(words, 0, 8 * sizeof(int32_t), st));
    if (NV > 0) {
        hipLaunchKernelGGL(mz_key_kernel, dim3(g_v), dim3(MS_BLOCK), 0, st, vertices, NV, grid, keys, counts);
        GP_LAUNCH_CHECK();
        const uint32_t* order = mz_sort3(sb, keys, NV, grid.bits, st);
        if (!order) return 1;
        hipLaunchKernelGGL(mz_head_kernel, dim3(g_v), dim3(MS_BLOCK), 0, st, (const uint32_t*)keys, order, NV, members, head_pos, head_vertex);
        GP_LAUNCH_CHECK();
    }
    if (ms_compact(head_pos, NV, (uint32_t*)(base + s.tile_a), rank_pos, words + MZ_WORD_SPARE, st)) return 1;
    if (ms_compact(head_vertex, NV, (uint32_t*)(base + s.tile_b), rank_vertex, words + MZ_WORD_CLUSTERS, st)) return 1;
    GP_HIP_CHECK(hipMemcpyAsync(counts + GP_MESH_SIMPLIFY_CLUSTERS, words + MZ_WORD_CLUSTERS, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (NV > 0) {
        hipLaunchKernelGGL(mz_segment_kernel, dim3(g_v), dim3(MS_BLOCK), 0, st, (const uint32_t*)members, (const uint8_t*)head_pos, (const uint32_t*)rank_pos,
                           (const uint32_t*)rank_vertex, NV, seg_begin, seg_cluster);
        GP_LAUNCH_CHECK();
        hipLaunchKernelGGL(mz_cluster_kernel, dim3(g_v), dim3(MS_BLOCK), 0, st, (const uint32_t*)members, (const uint8_t*)head_pos, (const uint32_t*)rank_pos,
                           (const uint32_t*)seg_begin, (const int32_t*)seg_cluster, (const int32_t*)words, NV, cluster, begin, end);
        GP_LAUNCH_CHECK();
        hipLaunchKernelGGL(mz_contract_kernel, dim3(gp_blocks(3 * (size_t)NV, MS_BLOCK)), dim3(MS_BLOCK), 0, st, vertices, (const uint32_t*)members, (const uint32_t*)begin,
                           (const uint32_t*)end, (const int32_t*)words, 3 * (uint64_t)NV, contraction, positions);
        GP_LAUNCH_CHECK();
        hipLaunchKernelGGL(mz_keep_cluster_kernel, dim3(g_v), dim3(MS_BLOCK), 0, st, (const int32_t*)words, NV, keep_unreferenced, keep_cluster);
        GP_LAUNCH_CHECK();
    }
    if (NF > 0) {
        hipLaunchKernelGGL(mz_face_kernel, dim3(g_f), dim3(MS_BLOCK), 0, st, faces, NV, NF, (const int32_t*)cluster, (const float*)positions, drop_zero_area, rot, keep_face,
                           counts);
        GP_LAUNCH_CHECK();
        if (drop_duplicates) {
            const int b = ms_bits(nv), bits[3] = {b, b, b};          // (the largest word: nv, of the faces that did not survive)
            const uint32_t* order = mz_sort3(sb, (const uint32_t*)rot, NF, bits, st);
            if (!order) return 1;
            hipLaunchKernelGGL(mz_duplicate_kernel, dim3(g_f), dim3(MS_BLOCK), 0, st, (const uint32_t*)rot, order, NV, NF, keep_face, counts);
            GP_LAUNCH_CHECK();
        }
        if (!keep_unreferenced && NV > 0) {
            hipLaunchKernelGGL(mz_mark_kernel, dim3(g_f), dim3(MS_BLOCK), 0, st, faces, (const uint8_t*)keep_face, (const int32_t*)cluster, NF, keep_cluster);
            GP_LAUNCH_CHECK();
        }
    }
    if (ms_compact(keep_cluster, NV, (uint32_t*)(base + s.tile_a), rank_cluster, counts + GP_MESH_SIMPLIFY_VERTICES, st)) return 1;
    if (ms_compact(keep_face, NF, (uint32_t*)(base + s.tile_face), rank_face, counts + GP_MESH_SIMPLIFY_FACES, st)) return 1;
    return 0;
}

extern "C" int gp_mesh_simplify_apply(const int32_t* faces, int64_t nv, int64_t nf, const void* scratch, float* vertices_out, int32_t* faces_out, int32_t* vertex_map,
                                      int32_t* face_index, int32_t* vertex_counts, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MZ_REFUSE_COMMON("gp_mesh_simplify_apply");
    if ((nf > 0 && (!faces || !face_index || !faces_out)) || (nv > 0 && (!vertices_out || !vertex_map || !vertex_counts))) GP_FAIL("gp_mesh_simplify_apply: null argument");
    const MzScratch s = mz_layout(nv, nf);
    const char* base = (const char*)scratch;
    const uint32_t NV = (uint32_t)nv, NF = (uint32_t)nf;
    GpProfScope _p("mesh_simplify_apply", st);
    if (NV > 0) {
        hipLaunchKernelGGL(mz_apply_vertex_kernel, dim3(gp_blocks(NV, MS_BLOCK)), dim3(MS_BLOCK), 0, st, (const int32_t*)(base + s.cluster),
                           (const uint8_t*)(base + s.keep_cluster), (const uint32_t*)(base + s.rank_cluster), (const float*)(base + s.positions),
                           (const uint32_t*)(base + s.begin), (const uint32_t*)(base + s.end), NV, vertices_out, vertex_map, vertex_counts);
        GP_LAUNCH_CHECK();
    }
    if (NF > 0 && NV > 0) {
        hipLaunchKernelGGL(mz_apply_face_kernel, dim3(gp_blocks(NF, MS_BLOCK)), dim3(MS_BLOCK), 0, st, faces, (const uint8_t*)(base + s.keep_face),
                           (const uint32_t*)(base + s.rank_face), (const int32_t*)(base + s.cluster), (const uint32_t*)(base + s.rank_cluster), NF, face_index, faces_out);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gp_mesh_simplify_rows(const float* src, int64_t nv, int64_t nf, int32_t k, int32_t contraction, const void* scratch, float* dst, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MZ_REFUSE_COMMON("gp_mesh_simplify_rows");
    if (k < 1 || k > 1024) GP_FAIL("gp_mesh_simplify_rows: k must be 1 .. 1024 (k = %d)", k);
    if (nv * k >= 0x80000000LL) GP_FAIL("gp_mesh_simplify_rows: nv*k must be below 2^31 (nv = %lld, k = %d)", (long long)nv, k);
    if (contraction != GP_MESH_SIMPLIFY_FIRST && contraction != GP_MESH_SIMPLIFY_AVERAGE)
        GP_FAIL("gp_mesh_simplify_rows: contraction must be GP_MESH_SIMPLIFY_FIRST or GP_MESH_SIMPLIFY_AVERAGE (contraction = %d)", contraction);
    if (nv > 0 && (!src || !dst)) GP_FAIL("gp_mesh_simplify_rows: null argument");
    if (nv == 0) return 0;
    const MzScratch s = mz_layout(nv, nf);
    const char* base = (const char*)scratch;
    const uint32_t total = (uint32_t)(nv * k);
    GpProfScope _p("mesh_simplify_rows", st);
    hipLaunchKernelGGL(mz_rows_kernel, dim3(gp_blocks(total, MS_BLOCK)), dim3(MS_BLOCK), 0, st, src, total, (uint32_t)k, contraction, (const uint32_t*)(base + s.members),
                       (const uint32_t*)(base + s.begin), (const uint32_t*)(base + s.end), (const uint8_t*)(base + s.keep_cluster),
                       (const uint32_t*)(base + s.rank_cluster), dst);
    GP_LAUNCH_CHECK();
    return 0;
}
