// tsdf_kernels.hip -- TSDF fusion and mesh extraction on the device (csrc/gp_tsdf.h).  The arithmetic, the sixteen cases and the tile
// order are csrc/tsdf_core.h, which also runs on a CPU (tests/tsdf_emulate.cpp).  Every kernel is a stream over the grid points, x
// fastest across lanes:
//   ts_integrate_kernel   one lane per point: tsdf, weight and colour loaded once, up to 16 views folded in from registers (the views'
//                         matrices come through uniform loads, the depth gathers of a wave are near-coherent), stored once
//   ts_active_kernel      one lane per point: the eight corners of its cell -> one byte
//   ts_mark_kernel        1024 points per workgroup (GP_TSDF_TILE), four per lane: the seven crossing bits of the point's own edges and
//                         the triangles of its cell as two bytes, and the tile's two sums (integers: butterflies, four waves through LDS)
//   ts_scan_kernel        ONE workgroup: the exclusive scans of the two tile arrays in place, 256 a round with a carry, and the totals
//   ts_rank_kernel        the same tiles again: a point's first vertex and first triangle are its tile's offset + the chunks before its
//                         own + the wave scan below its lane: ascending order by construction
//   ts_vertex_kernel      one lane per point: up to seven vertices at its first vertex onward
//   ts_face_kernel        one lane per point: up to twelve triangles of its cell at its first triangle onward; a vertex number is the
//                         owner's first vertex + its crossing bits below the edge
// No atomics anywhere; every store is an ordinary vector store.
#include "gp_common.h"

#include "tsdf_core.h"

static_assert(TS_BLOCK == 4 * GP_WAVE && TS_CHUNKS == 16, "the tile order of tsdf_core.h: four waves, four steps");

struct TsViews {
    const float* m[GP_TSDF_MAX_VIEWS];
    float tanfovx[GP_TSDF_MAX_VIEWS], tanfovy[GP_TSDF_MAX_VIEWS];
};

__device__ __forceinline__ void ts_ijk(const TsGrid& g, uint32_t n, int32_t* i, int32_t* j, int32_t* k) {
    const uint32_t row = n / (uint32_t)g.nx;
    *i = (int32_t)(n - row * (uint32_t)g.nx);
    *k = (int32_t)(row / (uint32_t)g.ny);
    *j = (int32_t)(row - (uint32_t)*k * (uint32_t)g.ny);
}

__global__ void __launch_bounds__(TS_BLOCK) ts_integrate_kernel(float* tsdf, float* weight, float* color, TsGrid g, uint32_t points,
                                                                const float* __restrict__ depth, const uint8_t* __restrict__ valid,
                                                                const float* __restrict__ image, TsViews views, int32_t V, int32_t H, int32_t W,
                                                                float trunc, float z_min, float view_weight, float weight_max) {
    const uint32_t n = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (n >= points) return;
    int32_t i, j, k;
    ts_ijk(g, n, &i, &j, &k);
    const float x = ts_coord(i, g.voxel, g.ox), y = ts_coord(j, g.voxel, g.oy), z = ts_coord(k, g.voxel, g.oz);
    TsVoxel p;
    p.tsdf = tsdf[n];
    p.w = weight[n];
    p.c[0] = p.c[1] = p.c[2] = 0.f;
    if (color) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.c[c] = color[(size_t)c * points + n];
    }
    const size_t plane = (size_t)H * W;
    for (int32_t v = 0; v < V; ++v)                        // (uniform: the matrix and the tangents are the wave's)
        ts_integrate_view(p, x, y, z, views.m[v], views.tanfovx[v], views.tanfovy[v], depth + (size_t)v * plane,
                          valid ? valid + (size_t)v * plane : nullptr, image ? image + (size_t)v * 3 * plane : nullptr, H, W, trunc, z_min,
                          view_weight, weight_max);
    tsdf[n] = p.tsdf;
    weight[n] = p.w;
    if (color) {
#pragma unroll
        for (int c = 0; c < 3; ++c) color[(size_t)c * points + n] = p.c[c];
    }
}

__global__ void __launch_bounds__(TS_BLOCK) ts_active_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, TsGrid g, uint32_t points,
                                                             float min_weight, uint8_t* __restrict__ active) {
    const uint32_t n = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (n >= points) return;
    int32_t i, j, k;
    ts_ijk(g, n, &i, &j, &k);
    active[n] = ts_cell_active(tsdf, weight, g, n, i, j, k, min_weight);      // (reads its corners only where the cell exists)
}

__global__ void __launch_bounds__(TS_BLOCK) ts_mark_kernel(const float* __restrict__ tsdf, const uint8_t* __restrict__ active, TsGrid g, uint32_t points,
                                                           float iso, uint8_t* __restrict__ marks, uint8_t* __restrict__ tris,
                                                           uint32_t* __restrict__ tile_vertices, uint32_t* __restrict__ tile_tris) {
    __shared__ uint32_t s_v[TS_BLOCK / GP_WAVE], s_t[TS_BLOCK / GP_WAVE];
    uint32_t nv = 0, nt = 0;
#pragma unroll
    for (int u = 0; u < TS_PER_LANE; ++u) {
        const uint32_t n = (uint32_t)ts_tile_point(blockIdx.x, u, threadIdx.x);
        if (n < points) {
            int32_t i, j, k;
            ts_ijk(g, n, &i, &j, &k);
            const int corners = ts_corners_inside(tsdf, g, n, i, j, k, iso);
            const uint8_t m = ts_edge_marks(active, g, n, i, j, k, corners);
            const uint8_t t = active[n] ? (uint8_t)ts_cell_triangles(corners) : (uint8_t)0;
            marks[n] = m;
            tris[n] = t;
            nv += (uint32_t)__popc((unsigned)m);
            nt += t;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        nv += (uint32_t)__shfl_xor((int)nv, d);
        nt += (uint32_t)__shfl_xor((int)nt, d);
    }
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = nv; s_t[threadIdx.x >> 6] = nt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_vertices[blockIdx.x] = (s_v[0] + s_v[1]) + (s_v[2] + s_v[3]);
        tile_tris[blockIdx.x] = (s_t[0] + s_t[1]) + (s_t[2] + s_t[3]);
    }
}

// 256 tile counts a round, the rounds chained by a carry in LDS; both arrays in the same rounds
__global__ void __launch_bounds__(TS_BLOCK) ts_scan_kernel(uint32_t* __restrict__ tile_vertices, uint32_t* __restrict__ tile_tris, uint32_t tiles,
                                                           int32_t* __restrict__ counts) {
    __shared__ uint32_t s_wave[2][TS_BLOCK / GP_WAVE];
    __shared__ uint32_t s_carry[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 2) s_carry[tid] = 0;
    __syncthreads();
    for (uint32_t base = 0; base < tiles; base += TS_BLOCK) {          // (uniform: every lane walks every round)
        const uint32_t t = base + tid;
        uint32_t a[2], incl[2], before[2];
        a[0] = t < tiles ? tile_vertices[t] : 0u;
        a[1] = t < tiles ? tile_tris[t] : 0u;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            incl[q] = (uint32_t)gp_wave_scan_add((int)a[q]);
            if (lane == 63) s_wave[q][wave] = incl[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            before[q] = s_carry[q];
            for (uint32_t w = 0; w < wave; ++w) before[q] += s_wave[q][w];
        }
        if (t < tiles) {
            tile_vertices[t] = before[0] + incl[0] - a[0];
            tile_tris[t] = before[1] + incl[1] - a[1];
        }
        __syncthreads();                                   // (every lane has read the carries and the waves' sums)
        if (tid == TS_BLOCK - 1) { s_carry[0] = before[0] + incl[0]; s_carry[1] = before[1] + incl[1]; }
        __syncthreads();
    }
    if (tid < 2) counts[tid] = (int32_t)s_carry[tid];
}

__global__ void __launch_bounds__(TS_BLOCK) ts_rank_kernel(const uint8_t* __restrict__ marks, const uint8_t* __restrict__ tris, uint32_t points,
                                                           const uint32_t* __restrict__ tile_vertices, const uint32_t* __restrict__ tile_tris,
                                                           uint32_t* __restrict__ first_vertex, uint32_t* __restrict__ first_tri) {
    __shared__ uint32_t s_v[TS_CHUNKS], s_t[TS_CHUNKS];
    uint32_t ex_v[TS_PER_LANE], ex_t[TS_PER_LANE];             // the exclusive scans inside the point's wave
#pragma unroll
    for (int u = 0; u < TS_PER_LANE; ++u) {
        const uint32_t n = (uint32_t)ts_tile_point(blockIdx.x, u, threadIdx.x);
        const uint32_t a = n < points ? (uint32_t)__popc((unsigned)marks[n]) : 0u, b = n < points ? (uint32_t)tris[n] : 0u;
        const uint32_t ia = (uint32_t)gp_wave_scan_add((int)a), ib = (uint32_t)gp_wave_scan_add((int)b);
        ex_v[u] = ia - a;
        ex_t[u] = ib - b;
        if ((threadIdx.x & 63) == 63) { s_v[ts_chunk(u, threadIdx.x)] = ia; s_t[ts_chunk(u, threadIdx.x)] = ib; }
    }
    __syncthreads();
    const uint32_t off_v = tile_vertices[blockIdx.x], off_t = tile_tris[blockIdx.x];
    uint32_t before_v[TS_PER_LANE] = {0u, 0u, 0u, 0u}, before_t[TS_PER_LANE] = {0u, 0u, 0u, 0u}, acc_v = 0, acc_t = 0;
#pragma unroll
    for (int c = 0; c < TS_CHUNKS; ++c) {
#pragma unroll
        for (int u = 0; u < TS_PER_LANE; ++u)
            if (c == ts_chunk(u, threadIdx.x)) { before_v[u] = acc_v; before_t[u] = acc_t; }
        acc_v += s_v[c];
        acc_t += s_t[c];
    }
#pragma unroll
    for (int u = 0; u < TS_PER_LANE; ++u) {
        const uint32_t n = (uint32_t)ts_tile_point(blockIdx.x, u, threadIdx.x);
        if (n < points) {
            first_vertex[n] = off_v + before_v[u] + ex_v[u];
            first_tri[n] = off_t + before_t[u] + ex_t[u];
        }
    }
}

__global__ void __launch_bounds__(TS_BLOCK) ts_vertex_kernel(const float* __restrict__ tsdf, const float* __restrict__ color, TsGrid g, uint32_t points,
                                                             float iso, const uint8_t* __restrict__ marks, const uint32_t* __restrict__ first_vertex,
                                                             float* __restrict__ vertices, float* __restrict__ colors) {
    const uint32_t n = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (n >= points) return;
    const uint32_t m = marks[n];
    if (m == 0) return;
    int32_t i, j, k;
    ts_ijk(g, n, &i, &j, &k);
    size_t row = first_vertex[n];                          // (< counts[0]: the scan of the same bytes)
    for (int e = 0; e < GP_TSDF_EDGES; ++e) {
        if (!((m >> e) & 1u)) continue;
        float pos[3], col[3];
        ts_vertex(tsdf, color, g, n, i, j, k, e, iso, pos, col);          // (a crossing edge's other end exists)
        vertices[row * 3] = pos[0]; vertices[row * 3 + 1] = pos[1]; vertices[row * 3 + 2] = pos[2];
        if (color) { colors[row * 3] = col[0]; colors[row * 3 + 1] = col[1]; colors[row * 3 + 2] = col[2]; }
        ++row;
    }
}

__global__ void __launch_bounds__(TS_BLOCK) ts_face_kernel(const float* __restrict__ tsdf, TsGrid g, uint32_t points, float iso,
                                                           const uint8_t* __restrict__ marks, const uint8_t* __restrict__ tris,
                                                           const uint32_t* __restrict__ first_vertex, const uint32_t* __restrict__ first_tri,
                                                           int32_t* __restrict__ faces) {
    const uint32_t n = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (n >= points) return;
    const int count = tris[n];                             // (> 0 in active cells only: all eight corners are grid points)
    if (count == 0) return;
    int32_t i, j, k;
    ts_ijk(g, n, &i, &j, &k);
    const int corners = ts_corners_inside(tsdf, g, n, i, j, k, iso);
    (void)ts_cell_faces(marks, first_vertex, g, n, corners, count, faces + (size_t)first_tri[n] * 3);      // (never beyond the counted ones)
}

// ---- the C entries ----
extern "C" int gp_tsdf_abi_version(void) { return GP_TSDF_ABI_VERSION; }

extern "C" int gp_tsdf_integrate(const gp_tsdf_volume* vol, const float* depth, const uint8_t* valid, const float* image, const gp_tsdf_view* views,
                                 int32_t V, int32_t H, int32_t W, float z_min, float view_weight, float weight_max, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = ts_refuse_volume(vol);
    if (why) GP_FAIL("gp_tsdf_integrate: %s", why);
    if (V < 1 || V > GP_TSDF_MAX_VIEWS) GP_FAIL("gp_tsdf_integrate: V must be 1 .. %d (V = %d)", GP_TSDF_MAX_VIEWS, V);
    if (H <= 0 || W <= 0) GP_FAIL("gp_tsdf_integrate: H and W must be > 0 (H = %d, W = %d)", H, W);
    if ((int64_t)H * W >= 0x80000000LL) GP_FAIL("gp_tsdf_integrate: H*W must be below 2^31 (H = %d, W = %d)", H, W);
    if (!(ts_finite(z_min) && z_min > 0.f && ts_finite(view_weight) && view_weight > 0.f && ts_finite(weight_max) && weight_max > 0.f))
        GP_FAIL("gp_tsdf_integrate: z_min, view_weight and weight_max must be finite and > 0");
    if (!depth || !views) GP_FAIL("gp_tsdf_integrate: null argument");
    if ((image == nullptr) != (vol->color == nullptr)) GP_FAIL("gp_tsdf_integrate: an image and a colour volume go together (both or neither)");
    TsViews vs;
    for (int v = 0; v < GP_TSDF_MAX_VIEWS; ++v) {
        const gp_tsdf_view& src = views[v < V ? v : 0];
        if (!src.world_view) GP_FAIL("gp_tsdf_integrate: null argument (the world_view of view %d)", v);
        if (!(ts_finite(src.tanfovx) && ts_finite(src.tanfovy))) GP_FAIL("gp_tsdf_integrate: tanfovx and tanfovy must be finite (view %d)", v);
        vs.m[v] = src.world_view; vs.tanfovx[v] = src.tanfovx; vs.tanfovy[v] = src.tanfovy;
    }
    const TsGrid g = ts_grid_of(vol);
    const uint32_t points = (uint32_t)ts_points(g);
    GpProfScope _p("tsdf_integrate", st);
    hipLaunchKernelGGL(ts_integrate_kernel, dim3(gp_blocks(points, TS_BLOCK)), dim3(TS_BLOCK), 0, st, vol->tsdf, vol->weight, vol->color, g, points, depth,
                       valid, image, vs, V, H, W, vol->trunc, z_min, view_weight, weight_max);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gp_tsdf_extract_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
    const char* why = ts_refuse_dims(nx, ny, nz);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_tsdf_extract_scratch_bytes: %s (nx = %d, ny = %d, nz = %d)", why, nx, ny, nz);
        return -1;
    }
    return ts_scratch_layout((int64_t)nx * ny * nz).bytes;
}

extern "C" int gp_tsdf_extract_count(const gp_tsdf_volume* vol, float iso, float min_weight, void* scratch, int32_t* counts, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = ts_refuse_volume(vol);
    if (why) GP_FAIL("gp_tsdf_extract_count: %s", why);
    if (!ts_finite(iso)) GP_FAIL("gp_tsdf_extract_count: iso must be finite");
    if (min_weight != min_weight) GP_FAIL("gp_tsdf_extract_count: min_weight must not be NaN");
    if (!scratch || !counts) GP_FAIL("gp_tsdf_extract_count: null argument");
    if (((uintptr_t)scratch & 3u) != 0) GP_FAIL("gp_tsdf_extract_count: scratch must be 4-byte aligned");
    const TsGrid g = ts_grid_of(vol);
    const uint32_t points = (uint32_t)ts_points(g), tiles = (uint32_t)ts_tiles(points);
    const TsScratch s = ts_scratch_layout(points);
    char* base = (char*)scratch;
    uint8_t* active = (uint8_t*)(base + s.active);
    uint8_t* marks = (uint8_t*)(base + s.marks);
    uint8_t* tris = (uint8_t*)(base + s.tris);
    uint32_t* tile_v = (uint32_t*)(base + s.tile_vertices);
    uint32_t* tile_t = (uint32_t*)(base + s.tile_tris);
    GpProfScope _p("tsdf_extract_count", st);
    hipLaunchKernelGGL(ts_active_kernel, dim3(gp_blocks(points, TS_BLOCK)), dim3(TS_BLOCK), 0, st, vol->tsdf, vol->weight, g, points, min_weight, active);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_mark_kernel, dim3(tiles), dim3(TS_BLOCK), 0, st, vol->tsdf, (const uint8_t*)active, g, points, iso, marks, tris, tile_v, tile_t);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_scan_kernel, dim3(1), dim3(TS_BLOCK), 0, st, tile_v, tile_t, tiles, counts);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_rank_kernel, dim3(tiles), dim3(TS_BLOCK), 0, st, (const uint8_t*)marks, (const uint8_t*)tris, points, (const uint32_t*)tile_v,
                       (const uint32_t*)tile_t, (uint32_t*)(base + s.first_vertex), (uint32_t*)(base + s.first_tri));
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_tsdf_extract_fill(const gp_tsdf_volume* vol, float iso, const void* scratch, float* vertices, float* colors, int32_t* faces,
                                    gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = ts_refuse_volume(vol);
    if (why) GP_FAIL("gp_tsdf_extract_fill: %s", why);
    if (!ts_finite(iso)) GP_FAIL("gp_tsdf_extract_fill: iso must be finite");
    if (!scratch || !vertices || !faces) GP_FAIL("gp_tsdf_extract_fill: null argument");
    if ((colors == nullptr) != (vol->color == nullptr)) GP_FAIL("gp_tsdf_extract_fill: colors and a colour volume go together (both or neither)");
    if (((uintptr_t)scratch & 3u) != 0) GP_FAIL("gp_tsdf_extract_fill: scratch must be 4-byte aligned");
    const TsGrid g = ts_grid_of(vol);
    const uint32_t points = (uint32_t)ts_points(g);
    const TsScratch s = ts_scratch_layout(points);
    const char* base = (const char*)scratch;
    const uint8_t* marks = (const uint8_t*)(base + s.marks);
    const uint8_t* tris = (const uint8_t*)(base + s.tris);
    const uint32_t* first_vertex = (const uint32_t*)(base + s.first_vertex);
    const uint32_t* first_tri = (const uint32_t*)(base + s.first_tri);
    GpProfScope _p("tsdf_extract_fill", st);
    hipLaunchKernelGGL(ts_vertex_kernel, dim3(gp_blocks(points, TS_BLOCK)), dim3(TS_BLOCK), 0, st, (const float*)vol->tsdf, (const float*)vol->color, g, points,
                       iso, marks, first_vertex, vertices, colors);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_face_kernel, dim3(gp_blocks(points, TS_BLOCK)), dim3(TS_BLOCK), 0, st, (const float*)vol->tsdf, g, points, iso, marks, tris,
                       first_vertex, first_tri, faces);
    GP_LAUNCH_CHECK();
    return 0;
}
