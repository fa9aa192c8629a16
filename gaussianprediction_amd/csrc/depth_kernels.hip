// depth_kernels.hip -- depth renders on the device (csrc/gp_depth.h).  The arithmetic and the tile orders are csrc/depth_core.h, which
// also runs on a CPU (tests/depth_emulate.cpp).  Every kernel is a stream over its pixels, bound by memory:
//   dp_resolve_kernel        one lane per pixel: two planes in, one plane and a byte out
//   dp_range_kernel          (no given range only) 1024 pixels per workgroup: the bits of the coloured values, a minimum and a maximum
//                            in the wave, in LDS, then ONE 32-bit atomic minimum and ONE maximum per workgroup -- integer, so the
//                            result does not depend on the order
//   dp_range_finish_kernel   one lane: the two words (or the given pair) -> the pair used, as floats, where the caller reads it
//   dp_color_kernel          one lane per pixel: the pair used through uniform loads, one row of the table gathered
//   dp_normals_kernel        one lane per pixel: five depths, five points, one cross product
//   dp_normals_image_kernel  one lane per pixel
//   dp_count_kernel          1024 pixels per workgroup (GP_DEPTH_TILE), four per lane: sixteen ballots, their population counts summed
//   dp_scan_kernel           ONE workgroup: the exclusive scan of the tile counts in place, 1024 a round with a carry, and the total
//   dp_place_kernel          the same ballots again; a pixel's row is its tile's offset + the chunks before its own + the set bits
//                            below its lane: row-major order by construction
//   dp_metric_kernel         1024 pixels per workgroup, four per lane; the twelve float32 sums by the tree gp_depth.h states, out as
//                            float64 with plain stores into the tile's slot
//   dp_metric_finalize       one workgroup per image adds the slots in a fixed order in float64 and forms the row
// No float atomics anywhere; every store is an ordinary vector store.
#include "gp_common.h"

#include "depth_core.h"

static_assert(DP_BLOCK == 4 * GP_WAVE && DP_CHUNKS == 16, "the tile order of depth_core.h: four waves, four steps");

__global__ void __launch_bounds__(DP_BLOCK) dp_resolve_kernel(const float* __restrict__ accum, const float* __restrict__ alpha, float alpha_min,
                                                              float* __restrict__ depth, uint8_t* __restrict__ valid, uint32_t plane) {
    const uint32_t p = blockIdx.x * DP_BLOCK + threadIdx.x;
    if (p >= plane) return;
    const DpResolved r = dp_resolve_pixel(accum[p], alpha[p], alpha_min);
    depth[p] = r.depth;
    valid[p] = r.valid;
}

__global__ void __launch_bounds__(DP_BLOCK) dp_range_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ valid, int32_t mode,
                                                            uint32_t plane, uint32_t* __restrict__ words) {
    __shared__ uint32_t s_lo[DP_BLOCK / GP_WAVE], s_hi[DP_BLOCK / GP_WAVE];
    uint32_t lo = DP_RANGE_LO_INIT, hi = DP_RANGE_HI_INIT;
#pragma unroll
    for (int u = 0; u < DP_PER_LANE; ++u) {
        const uint32_t p = (uint32_t)dp_tile_pixel(blockIdx.x, u, threadIdx.x);
        if (p < plane) {
            float v;
            if (dp_value(depth[p], valid, p, mode, &v)) {
                const uint32_t b = dp_bits(v);
                lo = b < lo ? b : lo;
                hi = b > hi ? b : hi;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t ol = (uint32_t)__shfl_xor((int)lo, d), oh = (uint32_t)__shfl_xor((int)hi, d);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < DP_BLOCK / GP_WAVE; ++w) {
            lo = s_lo[w] < lo ? s_lo[w] : lo;
            hi = s_hi[w] > hi ? s_hi[w] : hi;
        }
        if (hi != DP_RANGE_HI_INIT) {
            (void)__hip_atomic_fetch_min(words, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_max(words + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// words: range itself, holding dp_range_kernel's result where the pair is derived (nothing is read where it is given)
__global__ void __launch_bounds__(GP_WAVE) dp_range_finish_kernel(float lo, float hi, uint32_t* __restrict__ words) {
    if (threadIdx.x != 0) return;
    const bool given = lo < hi;
    float pair[2];
    dp_range_of(lo, hi, given ? 0u : words[0], given ? 0u : words[1], pair);
    words[0] = dp_bits(pair[0]);
    words[1] = dp_bits(pair[1]);
}

__global__ void __launch_bounds__(DP_BLOCK) dp_color_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ valid, int32_t mode,
                                                            const float* __restrict__ range, const float* __restrict__ lut, float bg0, float bg1,
                                                            float bg2, float* __restrict__ out, uint32_t plane) {
    const uint32_t p = blockIdx.x * DP_BLOCK + threadIdx.x;
    if (p >= plane) return;
    const float lo = range[0], hi = range[1];              // (dp_range_finish_kernel's: this launch is behind it)
    float col[3] = {bg0, bg1, bg2};
    float v;
    if (dp_value(depth[p], valid, p, mode, &v)) {
        const int row = dp_lut_row(v, lo, hi);             // (0 .. 255 whatever v is)
        col[0] = lut[row * 3]; col[1] = lut[row * 3 + 1]; col[2] = lut[row * 3 + 2];
    }
    out[p] = col[0];
    out[(size_t)plane + p] = col[1];
    out[2 * (size_t)plane + p] = col[2];
}

__global__ void __launch_bounds__(DP_BLOCK) dp_normals_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ valid, float tanfovx,
                                                              float tanfovy, float* __restrict__ normals, uint8_t* __restrict__ nvalid, int32_t H,
                                                              int32_t W) {
    const uint32_t plane = (uint32_t)H * (uint32_t)W;
    const uint32_t p = blockIdx.x * DP_BLOCK + threadIdx.x;
    if (p >= plane) return;
    const int32_t y = (int32_t)(p / (uint32_t)W), x = (int32_t)(p - (uint32_t)y * (uint32_t)W);
    float n[3];
    const uint8_t ok = dp_normal(depth, valid, x, y, tanfovx, tanfovy, W, H, n);      // (reads its neighbours only where they are inside)
    normals[p] = n[0];
    normals[(size_t)plane + p] = n[1];
    normals[2 * (size_t)plane + p] = n[2];
    nvalid[p] = ok;
}

__global__ void __launch_bounds__(DP_BLOCK) dp_normals_image_kernel(const float* __restrict__ normals, const uint8_t* __restrict__ nvalid, float bg0,
                                                                    float bg1, float bg2, float* __restrict__ out, uint32_t plane) {
    const uint32_t p = blockIdx.x * DP_BLOCK + threadIdx.x;
    if (p >= plane) return;
    const bool ok = nvalid[p] != 0;
    out[p] = ok ? normals[p] * 0.5f + 0.5f : bg0;
    out[(size_t)plane + p] = ok ? normals[(size_t)plane + p] * 0.5f + 0.5f : bg1;
    out[2 * (size_t)plane + p] = ok ? normals[2 * (size_t)plane + p] * 0.5f + 0.5f : bg2;
}

// ---- the ordered compaction ----
__global__ void __launch_bounds__(DP_BLOCK) dp_count_kernel(const uint8_t* __restrict__ valid, uint32_t plane, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_wave[DP_BLOCK / GP_WAVE];
    uint32_t n = 0;
#pragma unroll
    for (int u = 0; u < DP_PER_LANE; ++u) {
        const uint32_t p = (uint32_t)dp_tile_pixel(blockIdx.x, u, threadIdx.x);
        const bool take = p < plane && (!valid || valid[p] != 0);
        n += (uint32_t)__popcll(__ballot(take));
    }
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// 256 tile counts a round (a round covers 262 144 pixels: a few rounds for any picture), the rounds chained by a carry in LDS
__global__ void __launch_bounds__(DP_BLOCK) dp_scan_kernel(uint32_t* __restrict__ counts, uint32_t tiles, int32_t* __restrict__ total) {
    __shared__ uint32_t s_wave[DP_BLOCK / GP_WAVE];
    __shared__ uint32_t s_carry;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < tiles; base += DP_BLOCK) {          // (uniform: every lane walks every round)
        const uint32_t k = base + tid;
        const uint32_t a = k < tiles ? counts[k] : 0u;
        const uint32_t incl = (uint32_t)gp_wave_scan_add((int)a);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = s_carry;
        for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
        if (k < tiles) counts[k] = before + incl - a;
        __syncthreads();                                   // (every lane has read the carry and the waves' sums)
        if (tid == DP_BLOCK - 1) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) total[0] = (int32_t)s_carry;
}

__global__ void __launch_bounds__(DP_BLOCK) dp_place_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ valid, const float* __restrict__ image,
                                                            const float* __restrict__ cam2world, float tanfovx, float tanfovy, int32_t H, int32_t W,
                                                            const uint32_t* __restrict__ offsets, float* __restrict__ points, float* __restrict__ colors,
                                                            int32_t* __restrict__ index) {
    __shared__ uint32_t s_chunk[DP_CHUNKS];
    const uint32_t plane = (uint32_t)H * (uint32_t)W;
    bool take[DP_PER_LANE];
    uint32_t below[DP_PER_LANE];
#pragma unroll
    for (int u = 0; u < DP_PER_LANE; ++u) {
        const uint32_t p = (uint32_t)dp_tile_pixel(blockIdx.x, u, threadIdx.x);
        take[u] = p < plane && (!valid || valid[p] != 0);
        const unsigned long long ballot = __ballot(take[u]);
        below[u] = gp_mbcnt(ballot);                       // the set bits below this lane
        if ((threadIdx.x & 63) == 0) s_chunk[dp_chunk(u, threadIdx.x)] = (uint32_t)__popcll(ballot);
    }
    __syncthreads();
    const uint32_t tile_first = offsets[blockIdx.x];
    uint32_t before[DP_PER_LANE] = {0u, 0u, 0u, 0u}, acc = 0;
#pragma unroll
    for (int c = 0; c < DP_CHUNKS; ++c) {
#pragma unroll
        for (int u = 0; u < DP_PER_LANE; ++u)
            if (c == dp_chunk(u, threadIdx.x)) before[u] = acc;
        acc += s_chunk[c];
    }
#pragma unroll
    for (int u = 0; u < DP_PER_LANE; ++u) {
        if (!take[u]) continue;
        const uint32_t p = (uint32_t)dp_tile_pixel(blockIdx.x, u, threadIdx.x);
        const size_t row = (size_t)tile_first + before[u] + below[u];          // < the count of valid pixels <= plane
        const int32_t y = (int32_t)(p / (uint32_t)W), x = (int32_t)(p - (uint32_t)y * (uint32_t)W);
        const DpVec X = dp_world(cam2world, dp_point(x, y, depth[p], tanfovx, tanfovy, W, H));
        points[row * 3] = X.x; points[row * 3 + 1] = X.y; points[row * 3 + 2] = X.z;
        if (colors) {
            colors[row * 3] = image[p]; colors[row * 3 + 1] = image[(size_t)plane + p]; colors[row * 3 + 2] = image[2 * (size_t)plane + p];
        }
        if (index) index[row] = (int32_t)p;
    }
}

// ---- metrics ----
__global__ void __launch_bounds__(DP_BLOCK) dp_metric_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const uint8_t* __restrict__ mask,
                                                             const float* __restrict__ scale, float gt_min, float gt_max, uint32_t plane,
                                                             double* __restrict__ slots) {
    __shared__ float s_red[GP_DEPTH_SUMS][DP_BLOCK / GP_WAVE];
    const uint32_t img = blockIdx.y;
    const float* d = pred + (size_t)img * plane;
    const float* g = gt + (size_t)img * plane;
    const uint8_t* mk = mask ? mask + (size_t)img * plane : nullptr;
    const float* sc = scale ? scale + img : nullptr;
    float t[GP_DEPTH_SUMS];
#pragma unroll
    for (int q = 0; q < GP_DEPTH_SUMS; ++q) t[q] = 0.f;
#pragma unroll
    for (int u = 0; u < DP_PER_LANE; ++u) {
        const uint32_t p = (uint32_t)dp_tile_pixel(blockIdx.x, u, threadIdx.x);
        if (p < plane) dp_metric_terms(d[p], g[p], !mk || mk[p] != 0, sc, gt_min, gt_max, t);
    }
#pragma unroll
    for (int q = 0; q < GP_DEPTH_SUMS; ++q) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) t[q] += __shfl_xor(t[q], s);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < GP_DEPTH_SUMS; ++q) s_red[q][threadIdx.x >> 6] = t[q];
    }
    __syncthreads();
    if (threadIdx.x < GP_DEPTH_SUMS) {
        const int q = threadIdx.x;
        slots[((size_t)img * gridDim.x + blockIdx.x) * GP_DEPTH_SUMS + q] = (double)((s_red[q][0] + s_red[q][1]) + (s_red[q][2] + s_red[q][3]));
    }
}

__global__ void __launch_bounds__(DP_BLOCK) dp_metric_finalize(const double* __restrict__ slots, uint32_t tiles, double* __restrict__ table) {
    __shared__ double s_sum[GP_DEPTH_SUMS][DP_BLOCK];
    const uint32_t img = blockIdx.x, tid = threadIdx.x;
    const double* base = slots + (size_t)img * tiles * GP_DEPTH_SUMS;
    double a[GP_DEPTH_SUMS];
#pragma unroll
    for (int q = 0; q < GP_DEPTH_SUMS; ++q) a[q] = 0.0;
    for (uint32_t k = tid; k < tiles; k += DP_BLOCK) {
#pragma unroll
        for (int q = 0; q < GP_DEPTH_SUMS; ++q) a[q] += base[(size_t)k * GP_DEPTH_SUMS + q];
    }
#pragma unroll
    for (int q = 0; q < GP_DEPTH_SUMS; ++q) s_sum[q][tid] = a[q];
    __syncthreads();
    for (uint32_t stride = DP_BLOCK / 2; stride >= 1; stride >>= 1) {
        if (tid < stride) {
#pragma unroll
            for (int q = 0; q < GP_DEPTH_SUMS; ++q) s_sum[q][tid] += s_sum[q][tid + stride];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double s[GP_DEPTH_SUMS], row[GP_DEPTH_COLUMNS];
#pragma unroll
        for (int q = 0; q < GP_DEPTH_SUMS; ++q) s[q] = s_sum[q][0];
        dp_metric_row(s, row);
#pragma unroll
        for (int q = 0; q < GP_DEPTH_COLUMNS; ++q) table[(size_t)img * GP_DEPTH_COLUMNS + q] = row[q];
    }
}

// ---- the C entries ----
extern "C" int gp_depth_abi_version(void) { return GP_DEPTH_ABI_VERSION; }

extern "C" int gp_depth_resolve(const float* accum, const float* alpha, float alpha_min, float* depth, uint8_t* valid, int32_t H, int32_t W,
                                gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = dp_refuse_plane(H, W);
    if (why) GP_FAIL("gp_depth_resolve: %s (H = %d, W = %d)", why, H, W);
    if (alpha_min != alpha_min) GP_FAIL("gp_depth_resolve: alpha_min must not be NaN");
    if (!accum || !alpha || !depth || !valid) GP_FAIL("gp_depth_resolve: null argument");
    const uint32_t plane = (uint32_t)((int64_t)H * W);
    GpProfScope _p("depth_resolve", st);
    hipLaunchKernelGGL(dp_resolve_kernel, dim3(gp_blocks(plane, DP_BLOCK)), dim3(DP_BLOCK), 0, st, accum, alpha, alpha_min, depth, valid, plane);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_depth_colorize(const float* depth, const uint8_t* valid, int32_t mode, float lo, float hi, const float* lut, float bg_r, float bg_g,
                                 float bg_b, float* range, float* out, int32_t H, int32_t W, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = dp_refuse_plane(H, W);
    if (why) GP_FAIL("gp_depth_colorize: %s (H = %d, W = %d)", why, H, W);
    if (mode != 0 && mode != 1) GP_FAIL("gp_depth_colorize: mode must be 0 (depth) or 1 (disparity) (mode = %d)", mode);
    if (lo != lo || hi != hi) GP_FAIL("gp_depth_colorize: lo and hi must not be NaN");
    if (!depth || !lut || !range || !out) GP_FAIL("gp_depth_colorize: null argument");
    const uint32_t plane = (uint32_t)((int64_t)H * W);
    GpProfScope _p("depth_colorize", st);
    if (!(lo < hi)) {
        GP_HIP_CHECK(hipMemsetAsync(range, 0xFF, sizeof(uint32_t), st));               // DP_RANGE_LO_INIT
        GP_HIP_CHECK(hipMemsetAsync(range + 1, 0, sizeof(uint32_t), st));              // DP_RANGE_HI_INIT
        hipLaunchKernelGGL(dp_range_kernel, dim3(gp_blocks(plane, GP_DEPTH_TILE)), dim3(DP_BLOCK), 0, st, depth, valid, mode, plane, (uint32_t*)range);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(dp_range_finish_kernel, dim3(1), dim3(GP_WAVE), 0, st, lo, hi, (uint32_t*)range);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(dp_color_kernel, dim3(gp_blocks(plane, DP_BLOCK)), dim3(DP_BLOCK), 0, st, depth, valid, mode, (const float*)range, lut, bg_r, bg_g,
                       bg_b, out, plane);
    GP_LAUNCH_CHECK();
    return 0;
}

static const char* dp_refuse_view(const gp_depth_view* view, int32_t H, int32_t W) {
    if (!view) return "null argument";
    if (view->W != W || view->H != H) return "the view's W and H must be the call's";
    if (view->tanfovx != view->tanfovx || view->tanfovy != view->tanfovy) return "tanfovx and tanfovy must not be NaN";
    return nullptr;
}

extern "C" int gp_depth_normals(const float* depth, const uint8_t* valid, const gp_depth_view* view, float* normals, uint8_t* nvalid, int32_t H,
                                int32_t W, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = dp_refuse_plane(H, W);
    if (why) GP_FAIL("gp_depth_normals: %s (H = %d, W = %d)", why, H, W);
    if ((why = dp_refuse_view(view, H, W))) GP_FAIL("gp_depth_normals: %s (H = %d, W = %d)", why, H, W);
    if (!depth || !normals || !nvalid) GP_FAIL("gp_depth_normals: null argument");
    const uint32_t plane = (uint32_t)((int64_t)H * W);
    GpProfScope _p("depth_normals", st);
    hipLaunchKernelGGL(dp_normals_kernel, dim3(gp_blocks(plane, DP_BLOCK)), dim3(DP_BLOCK), 0, st, depth, valid, view->tanfovx, view->tanfovy, normals,
                       nvalid, H, W);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_depth_normals_image(const float* normals, const uint8_t* nvalid, float bg_r, float bg_g, float bg_b, float* out, int32_t H,
                                      int32_t W, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = dp_refuse_plane(H, W);
    if (why) GP_FAIL("gp_depth_normals_image: %s (H = %d, W = %d)", why, H, W);
    if (!normals || !nvalid || !out) GP_FAIL("gp_depth_normals_image: null argument");
    const uint32_t plane = (uint32_t)((int64_t)H * W);
    GpProfScope _p("depth_normals_image", st);
    hipLaunchKernelGGL(dp_normals_image_kernel, dim3(gp_blocks(plane, DP_BLOCK)), dim3(DP_BLOCK), 0, st, normals, nvalid, bg_r, bg_g, bg_b, out, plane);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t gp_depth_unproject_scratch_bytes(int32_t H, int32_t W) {
    const char* why = dp_refuse_plane(H, W);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_depth_unproject_scratch_bytes: %s (H = %d, W = %d)", why, H, W);
        return -1;
    }
    return dp_tiles(H, W) * (int64_t)sizeof(uint32_t);
}

extern "C" int gp_depth_unproject(const float* depth, const uint8_t* valid, const float* image, const gp_depth_view* view, float* points,
                                  float* colors, int32_t* index, int32_t* count, void* scratch, int32_t H, int32_t W, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = dp_refuse_plane(H, W);
    if (why) GP_FAIL("gp_depth_unproject: %s (H = %d, W = %d)", why, H, W);
    if ((why = dp_refuse_view(view, H, W))) GP_FAIL("gp_depth_unproject: %s (H = %d, W = %d)", why, H, W);
    if (!depth || !view->cam2world || !points || !count || !scratch) GP_FAIL("gp_depth_unproject: null argument");
    if ((image == nullptr) != (colors == nullptr)) GP_FAIL("gp_depth_unproject: image and colors go together (both or neither)");
    if (((uintptr_t)scratch & 3u) != 0) GP_FAIL("gp_depth_unproject: scratch must be 4-byte aligned");
    const uint32_t plane = (uint32_t)((int64_t)H * W), tiles = (uint32_t)dp_tiles(H, W);
    uint32_t* counts = (uint32_t*)scratch;
    GpProfScope _p("depth_unproject", st);
    hipLaunchKernelGGL(dp_count_kernel, dim3(tiles), dim3(DP_BLOCK), 0, st, valid, plane, counts);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(dp_scan_kernel, dim3(1), dim3(DP_BLOCK), 0, st, counts, tiles, count);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(dp_place_kernel, dim3(tiles), dim3(DP_BLOCK), 0, st, depth, valid, image, view->cam2world, view->tanfovx, view->tanfovy, H, W,
                       (const uint32_t*)counts, points, colors, index);
    GP_LAUNCH_CHECK();
    return 0;
}

static const char* dp_refuse_batch(int32_t B, int32_t H, int32_t W) {
    if (B <= 0) return "B must be > 0";
    const char* why = dp_refuse_plane(H, W);
    if (why) return why;
    if (B > 65535) return "B must be at most 65535";
    return nullptr;
}

extern "C" int64_t gp_depth_metrics_scratch_bytes(int32_t B, int32_t H, int32_t W) {
    const char* why = dp_refuse_batch(B, H, W);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_depth_metrics_scratch_bytes: %s (B = %d, H = %d, W = %d)", why, B, H, W);
        return -1;
    }
    return (int64_t)B * dp_tiles(H, W) * GP_DEPTH_SUMS * (int64_t)sizeof(double);
}

extern "C" int gp_depth_metrics(const float* pred, const float* gt, const uint8_t* mask, const float* scale, float gt_min, float gt_max, int32_t B,
                                int32_t H, int32_t W, void* scratch, double* table, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = dp_refuse_batch(B, H, W);
    if (why) GP_FAIL("gp_depth_metrics: %s (B = %d, H = %d, W = %d)", why, B, H, W);
    if (gt_min != gt_min || gt_max != gt_max) GP_FAIL("gp_depth_metrics: gt_min and gt_max must not be NaN");
    if (!pred || !gt || !scratch || !table) GP_FAIL("gp_depth_metrics: null argument");
    if (((uintptr_t)scratch & 7u) != 0) GP_FAIL("gp_depth_metrics: scratch must be 8-byte aligned");
    const uint32_t plane = (uint32_t)((int64_t)H * W), tiles = (uint32_t)dp_tiles(H, W);
    GpProfScope _p("depth_metrics", st);
    hipLaunchKernelGGL(dp_metric_kernel, dim3(tiles, (unsigned)B), dim3(DP_BLOCK), 0, st, pred, gt, mask, scale, gt_min, gt_max, plane, (double*)scratch);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(dp_metric_finalize, dim3((unsigned)B), dim3(DP_BLOCK), 0, st, (const double*)scratch, tiles, table);
    GP_LAUNCH_CHECK();
    return 0;
}
