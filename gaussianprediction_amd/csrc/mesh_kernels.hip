// mesh_kernels.hip -- cleanup of a triangle mesh on the device (csrc/gp_mesh.h): components, the filter, vertex normals.  The programs
// of a lane are csrc/mesh_core.h, which also runs on a CPU (tests/mesh_emulate.cpp).
//   ms_init_kernel        parent[v] = v (a first call), the flags of the call's rounds: flags[0] up unless the last call converged
//   ms_hook_kernel        a lane per face (strided): its two edges hooked by integer atomicMin (plain loads: stale costs a round, no more)
//   ms_jump_kernel        a lane per vertex (strided): up to GP_MESH_HOPS pointers up, one plain store to its own word
//   ms_settle_kernel      a lane per face and per vertex (strided): stores nothing but the next round's flag; a launch of its own, so it sees
//                         every atomic and every store of the round
//   ms_count_kernel       the vertices and faces of every root by integer atomicAdd (one per wave where the labels agree), face_label
//   ms_tile_sum_kernel, ms_scan_kernel, ms_rank_kernel     the ordered compaction of a byte array: tile sums, ONE workgroup scans the
//                         tiles, ballot ranks inside a tile (the order of tsdf_kernels.hip); ms_compact launches the three and is
//                         declared in mesh_compact.h, for mesh_simplify_kernels.hip
//   ms_table_kernel       the roots' rows at their ranks
//   ms_count_key_kernel, ms_keep_label_kernel, ms_keep_vertex_kernel, ms_keep_face_kernel, ms_apply_*_kernel, ms_gather_kernel   the filter
//   ms_face_vector_kernel, ms_incidence_key_kernel, ms_bounds_kernel, ms_normal_kernel   the normals, around gp_radix_sort_pairs
// A round's kernels return at once where the round's flag is down.  No float atomics, no spinning, no fence: whatever one launch
// leaves for another crosses a launch boundary.
#include "gp_common.h"

#include "mesh_compact.h"
#include "mesh_core.h"

static_assert(MS_BLOCK == 4 * GP_WAVE && MS_CHUNKS == 16, "the tile order of mesh_core.h: four waves, four steps");

#define MS_ROUND_BLOCKS 2048u            // the workgroups of a round's launches at the most: eight a CU

__global__ void __launch_bounds__(MS_BLOCK) ms_init_kernel(int32_t* __restrict__ parent, uint32_t nv, int32_t* __restrict__ flags, int32_t rounds,
                                                           int32_t* __restrict__ state, int32_t first) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (first && i < nv) parent[i] = (int32_t)i;
    if (i == 0) {
        flags[0] = first ? 1 : (state[GP_MESH_CONVERGED] == 0 ? 1 : 0);
        if (first) { state[GP_MESH_STATUS] = 0; state[GP_MESH_CONVERGED] = 0; state[GP_MESH_COUNT] = 0; state[GP_MESH_ROUNDS] = 0; }
    } else if (i <= (uint32_t)rounds) {
        flags[i] = 0;
    }
}

// The three kernels of a round stride over their elements with at most MS_ROUND_BLOCKS workgroups: a round whose flag is down is
// three launches of a few hundred workgroups that load one word and leave, not of one workgroup per 256 elements.
__global__ void __launch_bounds__(MS_BLOCK) ms_hook_kernel(int32_t* parent, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                           const int32_t* __restrict__ flag, int32_t* state) {
    if (*flag == 0) return;
    for (uint64_t f = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x; f < nf; f += (uint64_t)gridDim.x * MS_BLOCK)
        ms_hook_face(parent, parent, faces, (int64_t)f, nv, state);
}

__global__ void __launch_bounds__(MS_BLOCK) ms_jump_kernel(int32_t* parent, uint32_t nv, const int32_t* __restrict__ flag) {
    if (*flag == 0) return;
    for (uint64_t v = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x; v < nv; v += (uint64_t)gridDim.x * MS_BLOCK) ms_jump(parent, parent, (int64_t)v);
}

__global__ void __launch_bounds__(MS_BLOCK) ms_settle_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                             const int32_t* __restrict__ flag, int32_t* __restrict__ next, int32_t* __restrict__ state) {
    if (*flag == 0) return;
    const uint64_t first = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x, both = nv > nf ? nv : nf;
    bool open = false;
    for (uint64_t i = first; i < both && !open; i += (uint64_t)gridDim.x * MS_BLOCK)
        open = (i < nf && ms_unsettled_face(parent, faces, (int64_t)i, nv)) || (i < nv && ms_unsettled_vertex(parent, (int64_t)i));
    if (open) *next = 1;                             // (every writer stores the same word)
    if (first == 0) state[GP_MESH_ROUNDS] += 1;      // (one lane of the launch, launches in stream order)
}

// all 64 lanes of a wave call it: one atomic for the lanes that share the first active lane's label, one each for the others
__device__ __forceinline__ void ms_wave_add(int32_t* counts, int32_t label, bool active) {
    const unsigned long long act = __ballot(active);
    if (act == 0ull) return;
    const int leader = __ffsll((long long)act) - 1;
    const int32_t first = __shfl(label, leader);
    const unsigned long long same = __ballot(active && label == first);
    if (!active) return;
    if (label != first) atomicAdd(&counts[label], 1);
    else if ((int)(threadIdx.x & 63) == leader) atomicAdd(&counts[first], (int32_t)__popcll(same));
}

__global__ void __launch_bounds__(MS_BLOCK) ms_count_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                            int32_t* vertex_count, int32_t* face_count, int32_t* __restrict__ face_label,
                                                            uint8_t* __restrict__ is_root, const int32_t* __restrict__ last_flag, int32_t* state) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    int32_t lv = 0, lf = -1;
    if (i < nv) {
        lv = parent[i];
        is_root[i] = lv == (int32_t)i;
    }
    if (i < nf) {
        lf = ms_face_label(parent, faces, i, nv, state);
        face_label[i] = lf;
    }
    ms_wave_add(vertex_count, lv, i < nv);
    ms_wave_add(face_count, lf, lf >= 0);
    if (i == 0) state[GP_MESH_CONVERGED] = *last_flag == 0 ? 1 : 0;
}

// ---- the ordered compaction of keep[0 .. n) ----
__global__ void __launch_bounds__(MS_BLOCK) ms_tile_sum_kernel(const uint8_t* __restrict__ keep, uint32_t n, uint32_t* __restrict__ tile_sums) {
    __shared__ uint32_t s_w[MS_BLOCK / GP_WAVE];
    uint32_t sum = 0;
#pragma unroll
    for (int u = 0; u < MS_PER_LANE; ++u) {
        const uint32_t e = (uint32_t)ms_tile_elem(blockIdx.x, u, threadIdx.x);
        if (e < n && keep[e]) ++sum;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// ONE workgroup: the exclusive scan of the tile sums in place, 256 a step with a carry, and the total
__global__ void __launch_bounds__(MS_BLOCK) ms_scan_kernel(uint32_t* __restrict__ tile_sums, uint32_t tiles, int32_t* __restrict__ total) {
    __shared__ uint32_t s_wave[MS_BLOCK / GP_WAVE];
    __shared__ uint32_t s_carry;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < tiles; base += MS_BLOCK) {          // (uniform: every lane walks every step)
        const uint32_t t = base + tid;
        const uint32_t a = t < tiles ? tile_sums[t] : 0u;
        const uint32_t incl = (uint32_t)gp_wave_scan_add((int)a);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = s_carry;
        for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
        if (t < tiles) tile_sums[t] = before + incl - a;
        __syncthreads();                                   // (every lane has read the carry and the waves' sums)
        if (tid == MS_BLOCK - 1) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) *total = (int32_t)s_carry;
}

__global__ void __launch_bounds__(MS_BLOCK) ms_rank_kernel(const uint8_t* __restrict__ keep, uint32_t n, const uint32_t* __restrict__ tile_sums,
                                                           uint32_t* __restrict__ rank) {
    __shared__ uint32_t s_c[MS_CHUNKS];
    const uint32_t lane = threadIdx.x & 63;
    uint32_t below[MS_PER_LANE];                     // the kept elements of the chunk under this lane
#pragma unroll
    for (int u = 0; u < MS_PER_LANE; ++u) {
        const uint32_t e = (uint32_t)ms_tile_elem(blockIdx.x, u, threadIdx.x);
        const unsigned long long b = __ballot(e < n && keep[e] != 0);
        below[u] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_c[ms_chunk(u, threadIdx.x)] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    const uint32_t off = tile_sums[blockIdx.x];
    uint32_t before[MS_PER_LANE] = {0u, 0u, 0u, 0u}, acc = 0;
#pragma unroll
    for (int c = 0; c < MS_CHUNKS; ++c) {
#pragma unroll
        for (int u = 0; u < MS_PER_LANE; ++u)
            if (c == ms_chunk(u, threadIdx.x)) before[u] = acc;
        acc += s_c[c];
    }
#pragma unroll
    for (int u = 0; u < MS_PER_LANE; ++u) {
        const uint32_t e = (uint32_t)ms_tile_elem(blockIdx.x, u, threadIdx.x);
        if (e < n) rank[e] = off + before[u] + below[u];
    }
}

int ms_compact(const uint8_t* keep, uint32_t n, uint32_t* tile_sums, uint32_t* rank, int32_t* total, hipStream_t st) {
    const uint32_t tiles = (uint32_t)ms_tiles(n);
    if (tiles > 0) {
        hipLaunchKernelGGL(ms_tile_sum_kernel, dim3(tiles), dim3(MS_BLOCK), 0, st, keep, n, tile_sums);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ms_scan_kernel, dim3(1), dim3(MS_BLOCK), 0, st, tile_sums, tiles, total);
    GP_LAUNCH_CHECK();
    if (tiles > 0) {
        hipLaunchKernelGGL(ms_rank_kernel, dim3(tiles), dim3(MS_BLOCK), 0, st, keep, n, (const uint32_t*)tile_sums, rank);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

__global__ void __launch_bounds__(MS_BLOCK) ms_table_kernel(const uint8_t* __restrict__ is_root, const uint32_t* __restrict__ rank,
                                                            const int32_t* __restrict__ vertex_count, const int32_t* __restrict__ face_count, uint32_t nv,
                                                            int32_t* __restrict__ table) {
    const uint32_t v = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= nv || !is_root[v]) return;
    const size_t r = rank[v];                        // (< the roots counted: the scan of the same bytes; never beyond nv)
    table[r] = (int32_t)v;
    table[(size_t)nv + r] = vertex_count[v];
    table[2 * (size_t)nv + r] = face_count[v];
}

// ---- the filter ----
__global__ void __launch_bounds__(MS_BLOCK) ms_count_key_kernel(const int32_t* __restrict__ face_counts, uint32_t C, uint32_t* __restrict__ keys) {
    const uint32_t c = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (c >= C) return;
    const int32_t n = face_counts[c];
    keys[c] = 0x7fffffffu - (uint32_t)(n < 0 ? 0 : n);          // most faces first; the sort is stable: ties in ascending label
}

__global__ void __launch_bounds__(MS_BLOCK) ms_keep_label_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ face_counts,
                                                                 const uint32_t* __restrict__ order, uint32_t C, uint32_t nv, int32_t min_triangles,
                                                                 int32_t keep_largest, uint8_t* __restrict__ keep_label, int32_t* state) {
    const uint32_t pos = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (pos >= C) return;
    const uint32_t c = order ? order[pos] : pos;
    if (c >= C) return;
    const int32_t l = labels[c];
    if (!ms_index_ok(l, nv)) { state[GP_MESH_STATUS] = 1; return; }
    keep_label[l] = ms_keep_component(face_counts[c], min_triangles, keep_largest, pos);
}

__global__ void __launch_bounds__(MS_BLOCK) ms_keep_vertex_kernel(const uint8_t* __restrict__ keep_label, const int32_t* __restrict__ vertex_label, uint32_t nv,
                                                                  uint8_t* __restrict__ keep_vertex, int32_t* state) {
    const uint32_t v = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v < nv) keep_vertex[v] = ms_keep_vertex(keep_label, vertex_label, v, nv, state);
}

__global__ void __launch_bounds__(MS_BLOCK) ms_keep_face_kernel(const uint8_t* __restrict__ keep_vertex, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                                uint8_t* __restrict__ keep_face, int32_t* state) {
    const uint32_t f = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (f < nf) keep_face[f] = ms_keep_face(keep_vertex, faces, f, nv, state);
}

__global__ void __launch_bounds__(MS_BLOCK) ms_apply_vertex_kernel(const uint8_t* __restrict__ keep_vertex, const uint32_t* __restrict__ rank_vertex, uint32_t nv,
                                                                   int32_t* __restrict__ vertex_index) {
    const uint32_t v = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v < nv && keep_vertex[v]) vertex_index[rank_vertex[v]] = (int32_t)v;          // (a rank below the counted total)
}

__global__ void __launch_bounds__(MS_BLOCK) ms_apply_face_kernel(const uint8_t* __restrict__ keep_face, const uint32_t* __restrict__ rank_face,
                                                                 const uint32_t* __restrict__ rank_vertex, const int32_t* __restrict__ faces, uint32_t nf,
                                                                 int32_t* __restrict__ face_index, int32_t* __restrict__ faces_out) {
    const uint32_t f = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (f >= nf || !keep_face[f]) return;
    const size_t r = rank_face[f];
    face_index[r] = (int32_t)f;
    ms_remap_face(faces, f, rank_vertex, faces_out + 3 * r);
}

__global__ void __launch_bounds__(MS_BLOCK) ms_gather_kernel(const float* __restrict__ src, uint32_t total, uint32_t k, const uint8_t* __restrict__ keep_vertex,
                                                             const uint32_t* __restrict__ rank_vertex, float* __restrict__ dst) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= total) return;
    const uint32_t v = i / k, j = i - v * k;
    if (keep_vertex[v]) dst[(size_t)rank_vertex[v] * k + j] = src[i];
}

// ---- the normals ----
__global__ void __launch_bounds__(MS_BLOCK) ms_face_vector_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                                  float* __restrict__ face_vectors, int32_t* state) {
    const uint32_t f = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (f >= nf) return;
    float n[3];
    (void)ms_face_vector(vertices, faces, f, nv, n, state);
    face_vectors[3 * (size_t)f] = n[0]; face_vectors[3 * (size_t)f + 1] = n[1]; face_vectors[3 * (size_t)f + 2] = n[2];
}

__global__ void __launch_bounds__(MS_BLOCK) ms_incidence_key_kernel(const int32_t* __restrict__ faces, uint32_t nv, uint32_t n, uint32_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i < n) keys[i] = ms_incidence_key(faces, i, nv);
}

// where each vertex's run of the sorted keys begins and ends; a vertex without a run keeps begin = end = 0
__global__ void __launch_bounds__(MS_BLOCK) ms_bounds_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t nv, uint32_t* __restrict__ begin,
                                                             uint32_t* __restrict__ end) {
    const uint32_t i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    if (k >= nv) return;                             // (the corners of skipped faces)
    if (i == 0 || keys[i - 1] != k) begin[k] = i;
    if (i == n - 1 || keys[i + 1] != k) end[k] = i + 1;
}

__global__ void __launch_bounds__(MS_BLOCK) ms_normal_kernel(const float* __restrict__ face_vectors, const uint32_t* __restrict__ incidences,
                                                             const uint32_t* __restrict__ begin, const uint32_t* __restrict__ end, uint32_t nv, uint32_t n,
                                                             float* __restrict__ normals) {
    const uint32_t v = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= nv) return;
    const uint32_t b = begin[v], e = end[v];
    float out[3];
    ms_vertex_normal(face_vectors, incidences, b, e <= n ? e : n, out);          // (incidences are 0 .. n - 1: their faces exist)
    normals[3 * (size_t)v] = out[0]; normals[3 * (size_t)v + 1] = out[1]; normals[3 * (size_t)v + 2] = out[2];
}

// ---- the C entries ----
static MsScratch ms_layout(int64_t nv, int64_t nf) {
    const int64_t sort_n = 3 * nf > nv ? 3 * nf : nv;
    const int64_t blocks = (sort_n + 1023) / 1024;              // (the sort's smallest tile: enough for a sort of any n <= sort_n)
    return ms_scratch_layout(nv, nf, 256 * blocks + 64, (int64_t)gp_scan_tmp_elems((size_t)(256 * (blocks > 0 ? blocks : 1))));
}

static GpSortBufs ms_sort_bufs(char* base, const MsScratch& s) {
    GpSortBufs sb;
    for (int k = 0; k < 2; ++k) { sb.k[k] = (uint32_t*)(base + s.sort_k[k]); sb.v[k] = (uint32_t*)(base + s.sort_v[k]); }
    sb.hist = (uint32_t*)(base + s.sort_hist);
    sb.scan_tmp = (uint32_t*)(base + s.sort_tmp);
    sb.scan_tmp_elems = (size_t)s.sort_tmp_elems;
    return sb;
}

#define MS_REFUSE_COMMON(name)                                                                      \
    do {                                                                                            \
        const char* why_ = ms_refuse_sizes(nv, nf);                                                 \
        if (why_) GP_FAIL(name ": %s (nv = %lld, nf = %lld)", why_, (long long)nv, (long long)nf);  \
        if (!scratch) GP_FAIL(name ": null argument (scratch)");                                    \
        if (((uintptr_t)scratch & 3u) != 0) GP_FAIL(name ": scratch must be 4-byte aligned");       \
    } while (0)

extern "C" int gp_mesh_abi_version(void) { return GP_MESH_ABI_VERSION; }

extern "C" int64_t gp_mesh_scratch_bytes(int64_t nv, int64_t nf) {
    const char* why = ms_refuse_sizes(nv, nf);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_mesh_scratch_bytes: %s (nv = %lld, nf = %lld)", why, (long long)nv, (long long)nf);
        return -1;
    }
    return ms_layout(nv, nf).bytes;
}

extern "C" int gp_mesh_components(const int32_t* faces, int64_t nv, int64_t nf, int32_t rounds, int32_t first, int32_t* vertex_label, int32_t* face_label,
                                  int32_t* table, void* scratch, int32_t* state, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MS_REFUSE_COMMON("gp_mesh_components");
    if (rounds < 1 || rounds > GP_MESH_MAX_ROUNDS) GP_FAIL("gp_mesh_components: rounds must be 1 .. %d (rounds = %d)", GP_MESH_MAX_ROUNDS, rounds);
    if (!state || (nf > 0 && (!faces || !face_label)) || (nv > 0 && (!vertex_label || !table))) GP_FAIL("gp_mesh_components: null argument");
    const MsScratch s = ms_layout(nv, nf);
    char* base = (char*)scratch;
    int32_t* flags = (int32_t*)(base + s.flags);
    int32_t* vcount = (int32_t*)(base + s.vertex_count);
    int32_t* fcount = (int32_t*)(base + s.face_count);
    uint8_t* is_root = (uint8_t*)(base + s.keep_vertex);
    const uint32_t NV = (uint32_t)nv, NF = (uint32_t)nf, both = NV > NF ? NV : NF;
    const unsigned g_v = gp_blocks(NV > 0 ? NV : 1, MS_BLOCK), g_both = gp_blocks(both > 0 ? both : 1, MS_BLOCK);
    const auto capped = [](unsigned blocks) { return blocks < MS_ROUND_BLOCKS ? blocks : MS_ROUND_BLOCKS; };
    const unsigned r_v = capped(g_v), r_f = capped(gp_blocks(NF > 0 ? NF : 1, MS_BLOCK)), r_both = capped(g_both);
    GpProfScope _p("mesh_components", st);
    hipLaunchKernelGGL(ms_init_kernel, dim3(gp_blocks(NV > (uint32_t)rounds ? NV : (uint32_t)rounds + 1, MS_BLOCK)), dim3(MS_BLOCK), 0, st, vertex_label, NV, flags,
                       rounds, state, first);
    GP_LAUNCH_CHECK();
    for (int32_t r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(ms_hook_kernel, dim3(r_f), dim3(MS_BLOCK), 0, st, vertex_label, faces, NV, NF, (const int32_t*)(flags + r), state);
        GP_LAUNCH_CHECK();
        hipLaunchKernelGGL(ms_jump_kernel, dim3(r_v), dim3(MS_BLOCK), 0, st, vertex_label, NV, (const int32_t*)(flags + r));
        GP_LAUNCH_CHECK();
        hipLaunchKernelGGL(ms_settle_kernel, dim3(r_both), dim3(MS_BLOCK), 0, st, (const int32_t*)vertex_label, faces, NV, NF, (const int32_t*)(flags + r),
                           flags + r + 1, state);
        GP_LAUNCH_CHECK();
    }
    if (NV > 0) {
        GP_HIP_CHECK(hipMemsetAsync(vcount, 0, 4 * (size_t)NV, st));
        GP_HIP_CHECK(hipMemsetAsync(fcount, 0, 4 * (size_t)NV, st));
    }
    hipLaunchKernelGGL(ms_count_kernel, dim3(g_both), dim3(MS_BLOCK), 0, st, (const int32_t*)vertex_label, faces, NV, NF, vcount, fcount, face_label, is_root,
                       (const int32_t*)(flags + rounds), state);
    GP_LAUNCH_CHECK();
    if (ms_compact(is_root, NV, (uint32_t*)(base + s.tile_vertex), (uint32_t*)(base + s.rank_vertex), state + GP_MESH_COUNT, st)) return 1;
    if (NV > 0) {
        hipLaunchKernelGGL(ms_table_kernel, dim3(g_v), dim3(MS_BLOCK), 0, st, (const uint8_t*)is_root, (const uint32_t*)(base + s.rank_vertex), (const int32_t*)vcount,
                           (const int32_t*)fcount, NV, table);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gp_mesh_filter_plan(const int32_t* faces, int64_t nv, int64_t nf, const int32_t* vertex_label, const int32_t* labels, const int32_t* face_counts,
                                   int64_t components, int32_t min_triangles, int32_t keep_largest, void* scratch, int32_t* counts, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MS_REFUSE_COMMON("gp_mesh_filter_plan");
    if (components < 0 || components > nv) GP_FAIL("gp_mesh_filter_plan: components must be 0 .. nv (components = %lld)", (long long)components);
    if (!counts || (nf > 0 && !faces) || (nv > 0 && !vertex_label) || (components > 0 && (!labels || !face_counts))) GP_FAIL("gp_mesh_filter_plan: null argument");
    const MsScratch s = ms_layout(nv, nf);
    char* base = (char*)scratch;
    uint8_t* keep_label = (uint8_t*)(base + s.keep_label);
    uint8_t* keep_vertex = (uint8_t*)(base + s.keep_vertex);
    uint8_t* keep_face = (uint8_t*)(base + s.keep_face);
    const uint32_t NV = (uint32_t)nv, NF = (uint32_t)nf, C = (uint32_t)components;
    GpProfScope _p("mesh_filter_plan", st);
    GP_HIP_CHECK(hipMemsetAsync(counts, 0, 3 * sizeof(int32_t), st));
    if (NV > 0) GP_HIP_CHECK(hipMemsetAsync(keep_label, 0, NV, st));
    if (C > 0) {
        const uint32_t* order = nullptr;
        if (keep_largest >= 0) {
            GpSortBufs sb = ms_sort_bufs(base, s);
            hipLaunchKernelGGL(ms_count_key_kernel, dim3(gp_blocks(C, MS_BLOCK)), dim3(MS_BLOCK), 0, st, face_counts, C, sb.k[0]);
            GP_LAUNCH_CHECK();
            const int r = gp_radix_sort_pairs(sb, C, 31, st, true);
            if (r < 0) return 1;
            order = sb.v[r];
        }
        hipLaunchKernelGGL(ms_keep_label_kernel, dim3(gp_blocks(C, MS_BLOCK)), dim3(MS_BLOCK), 0, st, labels, face_counts, order, C, NV, min_triangles, keep_largest,
                           keep_label, counts);
        GP_LAUNCH_CHECK();
    }
    if (NV > 0) {
        hipLaunchKernelGGL(ms_keep_vertex_kernel, dim3(gp_blocks(NV, MS_BLOCK)), dim3(MS_BLOCK), 0, st, (const uint8_t*)keep_label, vertex_label, NV, keep_vertex, counts);
        GP_LAUNCH_CHECK();
    }
    if (NF > 0) {
        hipLaunchKernelGGL(ms_keep_face_kernel, dim3(gp_blocks(NF, MS_BLOCK)), dim3(MS_BLOCK), 0, st, (const uint8_t*)keep_vertex, faces, NV, NF, keep_face, counts);
        GP_LAUNCH_CHECK();
    }
    if (ms_compact(keep_vertex, NV, (uint32_t*)(base + s.tile_vertex), (uint32_t*)(base + s.rank_vertex), counts + 1, st)) return 1;
    if (ms_compact(keep_face, NF, (uint32_t*)(base + s.tile_face), (uint32_t*)(base + s.rank_face), counts + 2, st)) return 1;
    return 0;
}

extern "C" int gp_mesh_filter_apply(const int32_t* faces, int64_t nv, int64_t nf, const void* scratch, int32_t* vertex_index, int32_t* face_index,
                                    int32_t* faces_out, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MS_REFUSE_COMMON("gp_mesh_filter_apply");
    if ((nf > 0 && (!faces || !face_index || !faces_out)) || (nv > 0 && !vertex_index)) GP_FAIL("gp_mesh_filter_apply: null argument");
    const MsScratch s = ms_layout(nv, nf);
    const char* base = (const char*)scratch;
    const uint32_t NV = (uint32_t)nv, NF = (uint32_t)nf;
    GpProfScope _p("mesh_filter_apply", st);
    if (NV > 0) {
        hipLaunchKernelGGL(ms_apply_vertex_kernel, dim3(gp_blocks(NV, MS_BLOCK)), dim3(MS_BLOCK), 0, st, (const uint8_t*)(base + s.keep_vertex),
                           (const uint32_t*)(base + s.rank_vertex), NV, vertex_index);
        GP_LAUNCH_CHECK();
    }
    if (NF > 0) {
        hipLaunchKernelGGL(ms_apply_face_kernel, dim3(gp_blocks(NF, MS_BLOCK)), dim3(MS_BLOCK), 0, st, (const uint8_t*)(base + s.keep_face),
                           (const uint32_t*)(base + s.rank_face), (const uint32_t*)(base + s.rank_vertex), faces, NF, face_index, faces_out);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gp_mesh_gather_rows(const float* src, int64_t nv, int32_t k, const void* scratch, float* dst, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const int64_t nf = 0;
    MS_REFUSE_COMMON("gp_mesh_gather_rows");
    if (k < 1 || k > 1024) GP_FAIL("gp_mesh_gather_rows: k must be 1 .. 1024 (k = %d)", k);
    if (nv * k >= 0x80000000LL) GP_FAIL("gp_mesh_gather_rows: nv*k must be below 2^31 (nv = %lld, k = %d)", (long long)nv, k);
    if (nv > 0 && (!src || !dst)) GP_FAIL("gp_mesh_gather_rows: null argument");
    if (nv == 0) return 0;
    const MsScratch s = ms_scratch_layout(nv, 0, 0, 0);          // (keep_vertex and rank_vertex lie before everything nf moves)
    const char* base = (const char*)scratch;
    const uint32_t total = (uint32_t)(nv * k);
    GpProfScope _p("mesh_gather_rows", st);
    hipLaunchKernelGGL(ms_gather_kernel, dim3(gp_blocks(total, MS_BLOCK)), dim3(MS_BLOCK), 0, st, src, total, (uint32_t)k, (const uint8_t*)(base + s.keep_vertex),
                       (const uint32_t*)(base + s.rank_vertex), dst);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, void* scratch, float* normals, int32_t* state,
                                      gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MS_REFUSE_COMMON("gp_mesh_vertex_normals");
    if ((nv > 0 && (!vertices || !normals)) || (nf > 0 && !faces)) GP_FAIL("gp_mesh_vertex_normals: null argument");
    if (nv == 0) return 0;
    const MsScratch s = ms_layout(nv, nf);
    char* base = (char*)scratch;
    float* face_vectors = (float*)(base + s.face_vectors);
    uint32_t* begin = (uint32_t*)(base + s.begin);
    uint32_t* end = (uint32_t*)(base + s.end);
    const uint32_t NV = (uint32_t)nv, NF = (uint32_t)nf, n = 3u * NF;
    GpProfScope _p("mesh_vertex_normals", st);
    GP_HIP_CHECK(hipMemsetAsync(begin, 0, 4 * (size_t)NV, st));
    GP_HIP_CHECK(hipMemsetAsync(end, 0, 4 * (size_t)NV, st));
    const uint32_t* incidences = nullptr;
    if (NF > 0) {
        GpSortBufs sb = ms_sort_bufs(base, s);
        hipLaunchKernelGGL(ms_face_vector_kernel, dim3(gp_blocks(NF, MS_BLOCK)), dim3(MS_BLOCK), 0, st, vertices, faces, NV, NF, face_vectors, state);
        GP_LAUNCH_CHECK();
        hipLaunchKernelGGL(ms_incidence_key_kernel, dim3(gp_blocks(n, MS_BLOCK)), dim3(MS_BLOCK), 0, st, faces, NV, n, sb.k[0]);
        GP_LAUNCH_CHECK();
        const int r = gp_radix_sort_pairs(sb, n, ms_bits(nv), st, true);
        if (r < 0) return 1;
        incidences = sb.v[r];
        hipLaunchKernelGGL(ms_bounds_kernel, dim3(gp_blocks(n, MS_BLOCK)), dim3(MS_BLOCK), 0, st, (const uint32_t*)sb.k[r], n, NV, begin, end);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ms_normal_kernel, dim3(gp_blocks(NV, MS_BLOCK)), dim3(MS_BLOCK), 0, st, (const float*)face_vectors, incidences, (const uint32_t*)begin,
                       (const uint32_t*)end, NV, n, normals);
    GP_LAUNCH_CHECK();
    return 0;
}
