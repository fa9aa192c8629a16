// sdf_kernels.hip -- angle-weighted pseudonormals of a triangle mesh and the sign of a point-to-mesh distance, on the device
// (csrc/gp_sdf.h).  The programs of a lane are csrc/sdf_core.h and csrc/surface_core.h, which also run on a CPU (tests/sdf_emulate.cpp).
//   sd_face_kernel        a lane per face: its record, face_edges (a bisection per side), the keys of its six entries, the counts
//                         (integer atomicAdd, one per wave and word) and the workgroup's volume partial (a fixed tree in LDS, a plain store)
//   sd_walk_kernel        a lane per sorted position: the head of a run walks it and stores the run's sum -- one list, one lane, one order
//   sd_total_kernel       one lane: the partials added in ascending block
//   sd_sign_kernel        a lane per query: surface_core.h's candidate again (float64: one face test), ONE gather of 24 bytes from the
//                         table the closest feature names (the three kinds diverge inside a wave: the gather is the only divergent part),
//                         the tallies by ballots, one integer atomic per workgroup and word
//   sd_means_kernel       a lane per entry: four words through the tree, plain stores
// around gp_radix_sort_pairs (stable: entry 3f + k ascends inside every run).  No float atomics, no spinning, no fence: whatever one
// launch leaves for another crosses a launch boundary.
#include "gp_common.h"

#include "sdf_core.h"

static_assert(SD_BLOCK == 4 * GP_WAVE, "four waves a workgroup");

// all 64 lanes of a wave call them
__device__ __forceinline__ void sd_wave_count(int32_t* word, bool mine) {
    const unsigned long long b = __ballot(mine);
    if (b != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) atomicAdd(word, (int32_t)__popcll(b));
}
__device__ __forceinline__ void sd_wave_add(int32_t* word, int32_t mine) {
    int32_t sum = mine;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if (sum != 0 && (threadIdx.x & 63) == 0) atomicAdd(word, sum);
}
// every lane of the workgroup calls it; x: [SD_BLOCK] in LDS, the lane's term already stored and a barrier passed
__device__ __forceinline__ void sd_block_tree(double* x) {
    for (int d = SD_BLOCK / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) x[threadIdx.x] = x[threadIdx.x] + x[threadIdx.x + d];
        __syncthreads();
    }
}

// ---- the tables ----
__global__ void __launch_bounds__(SD_BLOCK) sd_face_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                           const int32_t* __restrict__ edge, uint32_t n_edges, int32_t* __restrict__ face_edges,
                                                           SdFace* __restrict__ records, uint32_t* __restrict__ corner_key, uint32_t* __restrict__ side_key,
                                                           double* __restrict__ partials, int32_t* counts) {
    __shared__ double s_term[SD_BLOCK];
    const uint32_t f = blockIdx.x * SD_BLOCK + threadIdx.x;
    double term = 0.0;
    bool bad = false, skipped = false, zero_area = false;
    int32_t missing = 0;
    if (f < nf) {
        int32_t fe[3];
        uint32_t ck[3], sk[3];
        SdFace rec;
        sd_face_program(vertices, faces, f, nv, edge, n_edges, fe, &rec, ck, sk, &term, &bad, &skipped, &zero_area, &missing);
        records[f] = rec;
        for (int k = 0; k < 3; ++k) {
            face_edges[3 * (size_t)f + k] = fe[k];
            corner_key[3 * (size_t)f + k] = ck[k];
            side_key[3 * (size_t)f + k] = sk[k];
        }
    }
    s_term[threadIdx.x] = term;
    __syncthreads();
    sd_block_tree(s_term);
    if (threadIdx.x == 0) partials[blockIdx.x] = s_term[0];
    sd_wave_count(counts + GP_SDF_COUNT_STATUS, bad);
    sd_wave_count(counts + GP_SDF_COUNT_SKIPPED, skipped);
    sd_wave_count(counts + GP_SDF_COUNT_ZERO_AREA, zero_area);
    sd_wave_add(counts + GP_SDF_COUNT_MISSING, missing);
}

// rows: the table of `limit` rows the runs' sums go to (zeroed before: a row without a run stays +0.0)
template <bool VERTEX>
__global__ void __launch_bounds__(SD_BLOCK) sd_walk_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ entry, uint32_t n, uint32_t limit,
                                                           const SdFace* __restrict__ records, double* __restrict__ rows) {
    const uint32_t i = blockIdx.x * SD_BLOCK + threadIdx.x;
    if (i >= n || !sd_is_head(key, i, limit)) return;
    double sum[3];
    if (VERTEX) sd_walk_vertex(key, entry, i, n, records, sum);
    else sd_walk_edge(key, entry, i, n, records, sum);
    double* out = rows + 3 * (size_t)key[i];                     // (key[i] < limit: inside the table)
    out[0] = sum[0]; out[1] = sum[1]; out[2] = sum[2];
}

// words: how many doubles a block's partial holds; out[w] = the partials of word w in ascending block, from +0.0
__global__ void sd_total_kernel(const double* __restrict__ partials, uint32_t blocks, uint32_t words, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x >= words) return;
    double sum = 0.0;
    for (uint32_t b = 0; b < blocks; ++b) sum = sum + partials[(size_t)b * words + threadIdx.x];
    out[threadIdx.x] = sum;
}

// ---- the sign ----
__global__ void __launch_bounds__(SD_BLOCK) sd_sign_kernel(const float* __restrict__ queries, uint32_t nq, const float* __restrict__ dist2, const int32_t* __restrict__ face,
                                                           const int32_t* __restrict__ region, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                           uint32_t nv, uint32_t nf, const int32_t* __restrict__ face_edges, const double* __restrict__ edge_normal,
                                                           uint32_t n_edges, const double* __restrict__ vertex_normal, float* __restrict__ sdf, int8_t* __restrict__ sign,
                                                           int32_t* __restrict__ kind, int32_t* __restrict__ element, unsigned long long* stats) {
    __shared__ uint32_t s_tally[SD_BLOCK / GP_WAVE][GP_SDF_STAT_WORDS];
    const uint32_t i = blockIdx.x * SD_BLOCK + threadIdx.x;
    int row = -1;
    int8_t sg = 0;
    int32_t kd = -1;
    if (i < nq) {
        const float q[3] = {queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2]};
        float d;
        int32_t el;
        row = sd_sign(q, dist2[i], face[i], region[i], vertices, faces, nv, nf, face_edges, edge_normal, n_edges, vertex_normal, &d, &sg, &kd, &el);
        sdf[i] = d; sign[i] = sg; kind[i] = kd; element[i] = el;
    }
    const bool is[GP_SDF_STAT_WORDS] = {row == SD_ROW_SIGNED && kd == GP_SDF_KIND_FACE, row == SD_ROW_SIGNED && kd == GP_SDF_KIND_EDGE,
                                        row == SD_ROW_SIGNED && kd == GP_SDF_KIND_VERTEX, row == SD_ROW_SIGNED && sg < 0, row == SD_ROW_SIGNED && sg > 0,
                                        row == SD_ROW_FOREIGN || (row == SD_ROW_SIGNED && sg == 0), row == SD_ROW_EXCLUDED, row == SD_ROW_FOREIGN};
#pragma unroll
    for (int w = 0; w < GP_SDF_STAT_WORDS; ++w) {
        const uint32_t c = (uint32_t)__popcll(__ballot(is[w]));
        if ((threadIdx.x & 63) == 0) s_tally[threadIdx.x >> 6][w] = c;
    }
    __syncthreads();
    if (threadIdx.x < GP_SDF_STAT_WORDS) {           // one atomic per workgroup and word
        uint32_t total = 0;
        for (int k = 0; k < SD_BLOCK / GP_WAVE; ++k) total += s_tally[k][threadIdx.x];
        if (threadIdx.x == GP_SDF_STATUS) { if (total) atomicOr(stats + GP_SDF_STATUS, 1ull); }
        else if (total) atomicAdd(stats + threadIdx.x, (unsigned long long)total);
    }
}

// ---- the means ----
__global__ void __launch_bounds__(SD_BLOCK) sd_means_kernel(const float* __restrict__ sdf, const int8_t* __restrict__ sign, uint32_t n, double* __restrict__ partials) {
    __shared__ double s_term[SD_BLOCK];
    const uint32_t i = blockIdx.x * SD_BLOCK + threadIdx.x;
    double term[GP_SDF_MEAN_WORDS] = {0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        const float d = sdf[i];
        if (ms_finite(d)) {
            const int8_t s = sign[i];
            term[0] = 1.0; term[1] = (double)d; term[2] = s > 0 ? 1.0 : 0.0; term[3] = s < 0 ? 1.0 : 0.0;
        }
    }
    for (int w = 0; w < GP_SDF_MEAN_WORDS; ++w) {
        __syncthreads();
        s_term[threadIdx.x] = term[w];
        __syncthreads();
        sd_block_tree(s_term);
        if (threadIdx.x == 0) partials[(size_t)blockIdx.x * GP_SDF_MEAN_WORDS + w] = s_term[0];
    }
}

// ---- the C entries ----
static SdScratch sd_layout(int64_t nf) {
    const int64_t blocks = (3 * nf + 1023) / 1024;               // (the sort's smallest tile: enough for a sort of any n <= 3 nf)
    return sd_scratch_layout(nf, 256 * blocks + 64, (int64_t)gp_scan_tmp_elems((size_t)(256 * (blocks > 0 ? blocks : 1))));
}

#define SD_REFUSE_SCRATCH(name)                                                                     \
    do {                                                                                            \
        if (!scratch) GP_FAIL(name ": null argument (scratch)");                                    \
        if (((uintptr_t)scratch & 7u) != 0) GP_FAIL(name ": scratch must be 8-byte aligned");       \
    } while (0)

extern "C" int gp_sdf_abi_version(void) { return GP_SDF_ABI_VERSION; }

extern "C" int64_t gp_sdf_tables_scratch_bytes(int64_t nv, int64_t nf, int64_t n_edges) {
    const char* why = sd_refuse_tables(nv, nf, n_edges);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_sdf_tables_scratch_bytes: %s (nv = %lld, nf = %lld, n_edges = %lld)", why, (long long)nv, (long long)nf, (long long)n_edges);
        return -1;
    }
    return sd_layout(nf).bytes;
}

extern "C" int gp_sdf_tables(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const int32_t* edge, int64_t n_edges, void* scratch, int32_t* face_edges,
                             double* edge_normal, double* vertex_normal, double* volume, int32_t* counts, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = sd_refuse_tables(nv, nf, n_edges);
    if (why) GP_FAIL("gp_sdf_tables: %s (nv = %lld, nf = %lld, n_edges = %lld)", why, (long long)nv, (long long)nf, (long long)n_edges);
    SD_REFUSE_SCRATCH("gp_sdf_tables");
    if (!volume || !counts || (nf > 0 && (!faces || !face_edges)) || (nv > 0 && (!vertices || !vertex_normal)) || (n_edges > 0 && (!edge || !edge_normal)))
        GP_FAIL("gp_sdf_tables: null argument");
    const SdScratch s = sd_layout(nf);
    char* base = (char*)scratch;
    SdFace* records = (SdFace*)(base + s.records);
    uint32_t* side_key = (uint32_t*)(base + s.side_key);
    double* partials = (double*)(base + s.partials);
    GpSortBufs sb;
    for (int k = 0; k < 2; ++k) { sb.k[k] = (uint32_t*)(base + s.sort_k[k]); sb.v[k] = (uint32_t*)(base + s.sort_v[k]); }
    sb.hist = (uint32_t*)(base + s.sort_hist);
    sb.scan_tmp = (uint32_t*)(base + s.sort_tmp);
    sb.scan_tmp_elems = (size_t)s.sort_tmp_elems;
    const uint32_t NV = (uint32_t)nv, NF = (uint32_t)nf, NE = (uint32_t)n_edges, N3 = (uint32_t)(3 * nf);
    GpProfScope _p("sdf_tables", st);
    GP_HIP_CHECK(hipMemsetAsync(counts, 0, GP_SDF_COUNT_WORDS * sizeof(int32_t), st));
    if (NV > 0) GP_HIP_CHECK(hipMemsetAsync(vertex_normal, 0, 24 * (size_t)NV, st));          // (all bits zero: +0.0)
    if (NE > 0) GP_HIP_CHECK(hipMemsetAsync(edge_normal, 0, 24 * (size_t)NE, st));
    if (NF > 0) {
        const unsigned g_f = gp_blocks(NF, SD_BLOCK), g_3 = gp_blocks(N3, SD_BLOCK);
        hipLaunchKernelGGL(sd_face_kernel, dim3(g_f), dim3(SD_BLOCK), 0, st, vertices, faces, NV, NF, edge, NE, face_edges, records, sb.k[0], side_key, partials, counts);
        GP_LAUNCH_CHECK();
        int r = gp_radix_sort_pairs(sb, N3, ms_bits(nv), st, true);                           // (the largest key: nv, of what is no entry)
        if (r < 0) return 1;
        if (NV > 0) {
            hipLaunchKernelGGL(sd_walk_kernel<true>, dim3(g_3), dim3(SD_BLOCK), 0, st, (const uint32_t*)sb.k[r], (const uint32_t*)sb.v[r], N3, NV, (const SdFace*)records,
                               vertex_normal);
            GP_LAUNCH_CHECK();
        }
        GP_HIP_CHECK(hipMemcpyAsync(sb.k[0], side_key, 4 * (size_t)N3, hipMemcpyDeviceToDevice, st));
        r = gp_radix_sort_pairs(sb, N3, ms_bits(n_edges), st, true);
        if (r < 0) return 1;
        if (NE > 0) {
            hipLaunchKernelGGL(sd_walk_kernel<false>, dim3(g_3), dim3(SD_BLOCK), 0, st, (const uint32_t*)sb.k[r], (const uint32_t*)sb.v[r], N3, NE, (const SdFace*)records,
                               edge_normal);
            GP_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(sd_total_kernel, dim3(1), dim3(GP_WAVE), 0, st, (const double*)partials, (uint32_t)s.blocks, 1u, volume);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_sdf_sign(const float* queries, int64_t nq, const float* dist2, const int32_t* face, const int32_t* region, const float* closest, const float* bary,
                           const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const int32_t* face_edges, const double* edge_normal, int64_t n_edges,
                           const double* vertex_normal, float* sdf, int8_t* sign, int32_t* kind, int32_t* element, int64_t* stats, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    (void)closest; (void)bary;                       // (never read: the candidate is made again in float64)
    const char* why = sd_refuse_sign(nq, nv, nf, n_edges);
    if (why) GP_FAIL("gp_sdf_sign: %s (nq = %lld, nv = %lld, nf = %lld, n_edges = %lld)", why, (long long)nq, (long long)nv, (long long)nf, (long long)n_edges);
    if (!stats || (nq > 0 && (!queries || !dist2 || !face || !region || !sdf || !sign || !kind || !element)) || (nf > 0 && (!faces || !face_edges)) || (nv > 0 && (!vertices || !vertex_normal)) ||
        (n_edges > 0 && !edge_normal))
        GP_FAIL("gp_sdf_sign: null argument");
    GpProfScope _p("sdf_sign", st);
    GP_HIP_CHECK(hipMemsetAsync(stats, 0, GP_SDF_STAT_WORDS * sizeof(int64_t), st));
    if (nq == 0) return 0;
    hipLaunchKernelGGL(sd_sign_kernel, dim3(gp_blocks((size_t)nq, SD_BLOCK)), dim3(SD_BLOCK), 0, st, queries, (uint32_t)nq, dist2, face, region, vertices, faces, (uint32_t)nv,
                       (uint32_t)nf, face_edges, edge_normal, (uint32_t)n_edges, vertex_normal, sdf, sign, kind, element, (unsigned long long*)stats);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gp_sdf_means_scratch_bytes(int64_t n) {
    const char* why = gm_refuse_count(n);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_sdf_means_scratch_bytes: %s (n = %lld)", why, (long long)n);
        return -1;
    }
    return gm_up(8 * GP_SDF_MEAN_WORDS * (sd_blocks(n) > 0 ? sd_blocks(n) : 1));
}

extern "C" int gp_sdf_means(const float* sdf, const int8_t* sign, int64_t n, void* scratch, double* out, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = gm_refuse_count(n);
    if (why) GP_FAIL("gp_sdf_means: %s (n = %lld)", why, (long long)n);
    SD_REFUSE_SCRATCH("gp_sdf_means");
    if (!out || (n > 0 && (!sdf || !sign))) GP_FAIL("gp_sdf_means: null argument");
    GpProfScope _p("sdf_means", st);
    const uint32_t blocks = (uint32_t)sd_blocks(n);
    if (blocks > 0) {
        hipLaunchKernelGGL(sd_means_kernel, dim3(blocks), dim3(SD_BLOCK), 0, st, sdf, sign, (uint32_t)n, (double*)scratch);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sd_total_kernel, dim3(1), dim3(GP_WAVE), 0, st, (const double*)scratch, blocks, (uint32_t)GP_SDF_MEAN_WORDS, out);
    GP_LAUNCH_CHECK();
    return 0;
}
