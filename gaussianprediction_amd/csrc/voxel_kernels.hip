// voxel_kernels.hip -- voxel-grid downsampling of a point cloud on the device (include/gp_voxel.h).  The arithmetic is
// csrc/voxel_core.h, which also runs on a CPU (gp_voxel_downsample_host, tests/voxel_emulate.cpp).
//   vx_bounds_partial_kernel   up to 1024 workgroups stride over the points: per-lane min / max of each axis and the non-finite flag,
//                              reduced through LDS, one row of seven doubles per workgroup
//   vx_bounds_final_kernel     one workgroup reduces those rows into the record the caller reads.  min and max are exact in any
//                              order, so the tree's shape does not matter; nothing is atomic
//   vx_index_kernel            one lane per point: the int32 voxel index [n][3] and the first chunk of the sort key
//   vx_rekey_kernel            the next chunk of the key, gathered through the running permutation (keys wider than 32 bits only)
//   gp_radix_sort_pairs        per chunk, stable, on exactly the chunk's bits; the values are the permutation
//   vx_heads_kernel            1 where a sorted position starts a voxel; gp_scan_blocks_u32 numbers them and counts M
//   vx_starts_kernel           finishes that scan per workgroup: starts[voxel] = sorted position of its head, starts[M] = n, *m_out = M
//   vx_mean_kernel<C>          one lane per (voxel, channel), C = 3, 6 or 9: the lanes of a voxel read neighbouring addresses of a row;
//                              each walks its voxel's rows in sorted order, which is ascending input row (the sort is stable)
// A voxel that holds every point is one lane per channel walking n rows one after the other: correct, and as slow as that sounds
// (one dependent gather per row).  Every store is an ordinary vector store; the only atomic is the integer one inside the scan.
#include "gp_common.h"

#include "voxel_core.h"

#define VX_BLOCK 256
#define VX_BOUNDS_BLOCKS 1024
#define VX_MEAN_BLOCKS 4096
static_assert(GP_SCAN_TILE % VX_BLOCK == 0, "a workgroup of vx_starts_kernel lies inside one block of the scan");

struct VxIo {
    const double* src[3];
    double* dst[3];
};

struct VxScratch {
    double* partial;                 // [VX_BOUNDS_BLOCKS][8]
    int32_t* idx;                    // [n][3]
    GpSortBufs sb;
    uint32_t *scan, *block_sums, *total, *starts;
    size_t bytes;
};

static VxScratch vx_carve(void* base, size_t n) {
    VxScratch x;
    GpCarver c(base);
    x.partial = c.take<double>((size_t)VX_BOUNDS_BLOCKS * 8);
    x.idx = c.take<int32_t>(n * 3);
    for (int k = 0; k < 2; ++k) { x.sb.k[k] = c.take<uint32_t>(n); x.sb.v[k] = c.take<uint32_t>(n); }
    x.sb.hist = c.take<uint32_t>(gp_sort_hist_elems(n));
    x.sb.scan_tmp_elems = gp_scan_tmp_elems(256 * ((n + 1023) / 1024));
    x.sb.scan_tmp = c.take<uint32_t>(x.sb.scan_tmp_elems);
    x.scan = c.take<uint32_t>(n);
    x.block_sums = c.take<uint32_t>((n + GP_SCAN_TILE - 1) / GP_SCAN_TILE + 64);
    x.total = c.take<uint32_t>(GP_TOTAL_SLOTS);
    x.starts = c.take<uint32_t>(n + 1);
    x.bytes = c.bytes();
    return x;
}

// seven values per lane -> seven per workgroup, in LDS; s: [7][VX_BLOCK]
__device__ __forceinline__ void vx_block_reduce(double (*s)[VX_BLOCK], double* lo, double* hi, double& bad, int tid) {
    for (int a = 0; a < 3; ++a) { s[a][tid] = lo[a]; s[3 + a][tid] = hi[a]; }
    s[6][tid] = bad;
    __syncthreads();
    for (int step = VX_BLOCK / 2; step > 0; step >>= 1) {
        if (tid < step) {
            for (int a = 0; a < 3; ++a) {
                s[a][tid] = fmin(s[a][tid], s[a][tid + step]);
                s[3 + a][tid] = fmax(s[3 + a][tid], s[3 + a][tid + step]);
            }
            s[6][tid] = fmax(s[6][tid], s[6][tid + step]);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(VX_BLOCK) vx_bounds_partial_kernel(const double* __restrict__ points, uint32_t n, double* __restrict__ partial) {
    __shared__ double s[7][VX_BLOCK];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, bad = 0.0;
    for (size_t i = (size_t)blockIdx.x * VX_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * VX_BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double v = points[i * 3 + a];
            if (vx_finite(v)) { lo[a] = fmin(lo[a], v); hi[a] = fmax(hi[a], v); }
            else bad = 1.0;
        }
    }
    vx_block_reduce(s, lo, hi, bad, (int)threadIdx.x);
    if (threadIdx.x < 7) partial[(size_t)blockIdx.x * 8 + threadIdx.x] = s[threadIdx.x][0];
}

__global__ void __launch_bounds__(VX_BLOCK) vx_bounds_final_kernel(const double* __restrict__ partial, uint32_t rows, double* __restrict__ record) {
    __shared__ double s[7][VX_BLOCK];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, bad = 0.0;
    for (uint32_t r = threadIdx.x; r < rows; r += VX_BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], partial[(size_t)r * 8 + a]);
            hi[a] = fmax(hi[a], partial[(size_t)r * 8 + 3 + a]);
        }
        bad = fmax(bad, partial[(size_t)r * 8 + 6]);
    }
    vx_block_reduce(s, lo, hi, bad, (int)threadIdx.x);
    if (threadIdx.x < GP_VOXEL_RECORD_DOUBLES) record[threadIdx.x] = threadIdx.x < 7 ? s[threadIdx.x][0] : 0.0;
}

__global__ void __launch_bounds__(VX_BLOCK) vx_index_kernel(VxGrid g, const double* __restrict__ points, uint32_t n, int32_t* __restrict__ idx,
                                                            uint32_t* __restrict__ key) {
    const size_t i = (size_t)blockIdx.x * VX_BLOCK + threadIdx.x;
    if (i >= n) return;
    int32_t c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a] = vx_index(points[i * 3 + a], g.min_bound[a], g.voxel_size);
        idx[i * 3 + a] = c[a];
    }
    key[i] = vx_chunk_key(g, c, 0);
}

__global__ void __launch_bounds__(VX_BLOCK) vx_rekey_kernel(VxGrid g, int chunk, const int32_t* __restrict__ idx, const uint32_t* __restrict__ perm,
                                                            uint32_t n, uint32_t* __restrict__ key) {
    const size_t i = (size_t)blockIdx.x * VX_BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t p = perm[i];
    const int32_t c[3] = {idx[p * 3], idx[p * 3 + 1], idx[p * 3 + 2]};
    key[i] = vx_chunk_key(g, c, chunk);
}

__global__ void __launch_bounds__(VX_BLOCK) vx_heads_kernel(const int32_t* __restrict__ idx, const uint32_t* __restrict__ perm, uint32_t n,
                                                            uint32_t* __restrict__ heads) {
    const size_t i = (size_t)blockIdx.x * VX_BLOCK + threadIdx.x;
    if (i >= n) return;
    heads[i] = (i == 0 || !vx_same_voxel(idx + (size_t)perm[i] * 3, idx + (size_t)perm[i - 1] * 3)) ? 1u : 0u;
}

// scan: the heads, scanned exclusively inside blocks of GP_SCAN_TILE; block_sums: the blocks' totals.  A position is a head where the
// scan steps up behind it (the block's total stands in behind the block's last position).
__global__ void __launch_bounds__(VX_BLOCK) vx_starts_kernel(const uint32_t* __restrict__ scan, const uint32_t* __restrict__ block_sums,
                                                             const uint32_t* __restrict__ total, uint32_t n, uint32_t* __restrict__ starts,
                                                             int32_t* __restrict__ m_out) {
    __shared__ uint32_t s[VX_BLOCK];
    const int tid = (int)threadIdx.x;
    const size_t i = (size_t)blockIdx.x * VX_BLOCK + tid;
    const uint32_t b = (uint32_t)(((size_t)blockIdx.x * VX_BLOCK) / GP_SCAN_TILE);
    uint32_t part = 0;
    for (uint32_t j = tid; j < b; j += VX_BLOCK) part += block_sums[j];
    s[tid] = part;
    __syncthreads();
    for (int step = VX_BLOCK / 2; step > 0; step >>= 1) {
        if (tid < step) s[tid] += s[tid + step];
        __syncthreads();
    }
    const uint32_t prefix = s[0];
    if (i < n) {
        const uint32_t e = scan[i];
        const bool last = i + 1 == n || (i + 1) % GP_SCAN_TILE == 0;
        const uint32_t next = last ? block_sums[b] : scan[i + 1];
        if (next != e) starts[prefix + e] = (uint32_t)i;
        if (i + 1 == n) starts[prefix + next] = n;
    }
    if (blockIdx.x == 0 && tid == 0) m_out[0] = (int32_t)gp_total_of(total);
}

template <int C>
__global__ void __launch_bounds__(VX_BLOCK) vx_mean_kernel(VxIo io, const int32_t* __restrict__ idx, const uint32_t* __restrict__ perm,
                                                           const uint32_t* __restrict__ starts, const int32_t* __restrict__ m_ptr,
                                                           int32_t* __restrict__ out_index) {
    const size_t lanes = (size_t)(uint32_t)m_ptr[0] * C;
    for (size_t l = (size_t)blockIdx.x * VX_BLOCK + threadIdx.x; l < lanes; l += (size_t)gridDim.x * VX_BLOCK) {
        const size_t v = l / C;
        const int ch = (int)(l % C), arr = ch / 3, col = ch % 3;
        const uint32_t start = starts[v], end = starts[v + 1];
        const double* src = arr == 0 ? io.src[0] : (arr == 1 ? io.src[1] : io.src[2]);      // (selects: no indexing of the argument struct)
        double* dst = arr == 0 ? io.dst[0] : (arr == 1 ? io.dst[1] : io.dst[2]);
        dst[v * 3 + col] = vx_segment_mean(src, perm, start, end, col);
        if (ch < 3) out_index[v * 3 + ch] = idx[(size_t)perm[start] * 3 + ch];
    }
}

extern "C" int gp_voxel_abi_version(void) { return GP_VOXEL_ABI_VERSION; }

extern "C" int64_t gp_voxel_scratch_bytes(int64_t n) {
    if (n < 0 || n >= VX_MAX_N) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_voxel_scratch_bytes: n = %lld: %s", (long long)n, vx_refusal(2));
        return -1;
    }
    return (int64_t)vx_carve(nullptr, (size_t)n).bytes;
}

extern "C" int gp_voxel_bounds(int64_t n, const double* points, void* scratch, double* record, gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (n < 1 || n >= VX_MAX_N) GP_FAIL("gp_voxel_bounds: n = %lld must be in [1, 2^31)", (long long)n);
    if (!points || !scratch || !record) GP_FAIL("gp_voxel_bounds: null argument");
    const VxScratch x = vx_carve(scratch, (size_t)n);
    const unsigned rows = gp_blocks((size_t)n, VX_BLOCK) < VX_BOUNDS_BLOCKS ? gp_blocks((size_t)n, VX_BLOCK) : VX_BOUNDS_BLOCKS;
    GpProfScope _p("voxel_bounds", s);
    hipLaunchKernelGGL(vx_bounds_partial_kernel, dim3(rows), dim3(VX_BLOCK), 0, s, points, (uint32_t)n, x.partial);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(vx_bounds_final_kernel, dim3(1), dim3(VX_BLOCK), 0, s, x.partial, rows, record);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_voxel_downsample(int64_t n, const double* points, const double* colors, const double* normals, double voxel_size,
                                   const double* bounds, double* out_points, double* out_colors, double* out_normals, int32_t* out_index,
                                   int32_t* m_out, void* scratch, gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (!(voxel_size > 0.0)) GP_FAIL("gp_voxel_downsample: voxel_size = %g: %s", voxel_size, vx_refusal(1));
    if (n < 0 || n >= VX_MAX_N) GP_FAIL("gp_voxel_downsample: n = %lld: %s", (long long)n, vx_refusal(2));
    if (!m_out) GP_FAIL("gp_voxel_downsample: null argument");
    if (n == 0) {
        GP_HIP_CHECK(hipMemsetAsync(m_out, 0, sizeof(int32_t), s));
        return 0;
    }
    if (!points || !bounds || !out_points || !out_index || !scratch) GP_FAIL("gp_voxel_downsample: null argument");
    if ((colors != nullptr) != (out_colors != nullptr) || (normals != nullptr) != (out_normals != nullptr))
        GP_FAIL("gp_voxel_downsample: colors / normals and their outputs come together");
    if (bounds[6] != 0.0) GP_FAIL("gp_voxel_downsample: %s", vx_refusal(3));
    for (int a = 0; a < 3; ++a)
        if (!vx_finite(bounds[a]) || !vx_finite(bounds[3 + a]) || bounds[a] > bounds[3 + a]) GP_FAIL("gp_voxel_downsample: bounds are not those of gp_voxel_bounds");
    VxGrid g;
    if (vx_plan(g, bounds, bounds + 3, voxel_size)) GP_FAIL("gp_voxel_downsample: %s (voxel_size = %g)", vx_refusal(4), voxel_size);
    VxScratch x = vx_carve(scratch, (size_t)n);
    const uint32_t N = (uint32_t)n;
    const unsigned grid = gp_blocks((size_t)n, VX_BLOCK);
    {
        GpProfScope _p("voxel_index", s);
        hipLaunchKernelGGL(vx_index_kernel, dim3(grid), dim3(VX_BLOCK), 0, s, g, points, N, x.idx, x.sb.k[0]);
        GP_LAUNCH_CHECK();
    }
    GpSortBufs sb = x.sb;
    int r = 0;
    for (int c = 0; c < g.chunks; ++c) {
        GpProfScope _p("voxel_sort", s);
        if (c > 0) {               // the sorted pairs are in buffer r: they become buffer 0 of the next sort, its keys re-made from the permutation
            if (r == 1) { std::swap(sb.k[0], sb.k[1]); std::swap(sb.v[0], sb.v[1]); }
            hipLaunchKernelGGL(vx_rekey_kernel, dim3(grid), dim3(VX_BLOCK), 0, s, g, c, x.idx, sb.v[0], N, sb.k[0]);
            GP_LAUNCH_CHECK();
        }
        r = gp_radix_sort_pairs(sb, (size_t)n, vx_chunk_width(g, c), s, c == 0);
        if (r < 0) return 1;
    }
    const uint32_t* perm = sb.v[r];
    {
        GpProfScope _p("voxel_heads_scan", s);
        hipLaunchKernelGGL(vx_heads_kernel, dim3(grid), dim3(VX_BLOCK), 0, s, x.idx, perm, N, x.scan);
        GP_LAUNCH_CHECK();
        GP_HIP_CHECK(hipMemsetAsync(x.total, 0, GP_TOTAL_SLOTS * sizeof(uint32_t), s));
        if (gp_scan_blocks_u32(x.scan, (size_t)n, x.block_sums, x.total, s)) return 1;
        hipLaunchKernelGGL(vx_starts_kernel, dim3(grid), dim3(VX_BLOCK), 0, s, x.scan, x.block_sums, x.total, N, x.starts, m_out);
        GP_LAUNCH_CHECK();
    }
    {
        GpProfScope _p("voxel_mean", s);
        const int C = 3 + (colors ? 3 : 0) + (normals ? 3 : 0);
        VxIo io;                   // the arrays present, packed to the front: lane channel 3 .. 5 is the colours, or the normals where there are none
        int k = 0;
        const double* srcs[3] = {points, colors, normals};
        double* dsts[3] = {out_points, out_colors, out_normals};
        for (int a = 0; a < 3; ++a) { io.src[a] = nullptr; io.dst[a] = nullptr; }
        for (int a = 0; a < 3; ++a)
            if (srcs[a]) { io.src[k] = srcs[a]; io.dst[k] = dsts[a]; ++k; }
        const unsigned mgrid = gp_blocks((size_t)n * C, VX_BLOCK) < VX_MEAN_BLOCKS ? gp_blocks((size_t)n * C, VX_BLOCK) : VX_MEAN_BLOCKS;
        if (C == 3) hipLaunchKernelGGL((vx_mean_kernel<3>), dim3(mgrid), dim3(VX_BLOCK), 0, s, io, x.idx, perm, x.starts, m_out, out_index);
        else if (C == 6) hipLaunchKernelGGL((vx_mean_kernel<6>), dim3(mgrid), dim3(VX_BLOCK), 0, s, io, x.idx, perm, x.starts, m_out, out_index);
        else hipLaunchKernelGGL((vx_mean_kernel<9>), dim3(mgrid), dim3(VX_BLOCK), 0, s, io, x.idx, perm, x.starts, m_out, out_index);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gp_voxel_downsample_host(int64_t n, const double* points, const double* colors, const double* normals, double voxel_size,
                                        double* out_points, double* out_colors, double* out_normals, int32_t* out_index, int64_t* m_out) {
    if (!m_out) GP_FAIL("gp_voxel_downsample_host: null argument");
    if (n > 0 && n < VX_MAX_N && (!points || !out_points || !out_index)) GP_FAIL("gp_voxel_downsample_host: null argument");
    if ((colors != nullptr) != (out_colors != nullptr) || (normals != nullptr) != (out_normals != nullptr))
        GP_FAIL("gp_voxel_downsample_host: colors / normals and their outputs come together");
    const int rc = vx_downsample_host(n, points, colors, normals, voxel_size, out_points, out_colors, out_normals, out_index, m_out);
    if (rc) GP_FAIL("gp_voxel_downsample_host: %s", vx_refusal(rc));
    return 0;
}
