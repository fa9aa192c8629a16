// flow_kernels.hip -- optical flow rendered on the device (csrc/gp_flow.h).  The arithmetic is csrc/flow_core.h, which also runs on a CPU
// (tests/flow_emulate.cpp).  Every kernel is a stream over its elements, bound by memory:
//   fl_project_kernel    one lane per Gaussian: its rows of xyz0 and xyz1 (12 bytes each), the two views' matrices through uniform
//                        loads, one row of three floats out
//   fl_resolve_kernel    one lane per pixel: three planes in, two planes, alpha and a byte out
//   fl_max_kernel        (max_flow <= 0 only) 1024 pixels per workgroup: the bits of the finite magnitudes, a maximum in the wave, in
//                        LDS, then ONE 32-bit atomic maximum per workgroup -- integer, so the result does not depend on the order
//   fl_color_kernel      one lane per pixel, the 55-row wheel in LDS
//   fl_metric_kernel     1024 pixels per workgroup (GP_FLOW_TILE), four per lane; the seven float32 sums by the tree gp_flow.h states,
//                        out as float64 with plain stores into the tile's slot
//   fl_metric_finalize   one workgroup per image adds the slots in a fixed order in float64 and forms the row
//   fl_warp_kernel       one lane per pixel: the sample position once, four taps per channel
// No float atomics anywhere; every store is an ordinary vector store.
#include "gp_common.h"

#include "flow_core.h"

#define FL_BLOCK 256
#define FL_PER_LANE (GP_FLOW_TILE / FL_BLOCK)

__global__ void __launch_bounds__(FL_BLOCK) fl_project_kernel(const float* __restrict__ v0, const float* __restrict__ p0, int32_t W0, int32_t H0,
                                                              const float* __restrict__ v1, const float* __restrict__ p1, int32_t W1, int32_t H1,
                                                              const float* __restrict__ xyz0, const float* __restrict__ xyz1, uint32_t N,
                                                              float* __restrict__ out) {
    const uint32_t i = blockIdx.x * FL_BLOCK + threadIdx.x;
    if (i >= N) return;
    const size_t o = (size_t)i * 3;
    const float a[3] = {xyz0[o], xyz0[o + 1], xyz0[o + 2]}, b[3] = {xyz1[o], xyz1[o + 1], xyz1[o + 2]};
    float row[3];
    fl_project_row(v0, p0, W0, H0, v1, p1, W1, H1, a, b, row);
    out[o] = row[0]; out[o + 1] = row[1]; out[o + 2] = row[2];
}

__global__ void __launch_bounds__(FL_BLOCK) fl_resolve_kernel(const float* __restrict__ comp, float alpha_min, float* __restrict__ flow,
                                                              float* __restrict__ alpha, uint8_t* __restrict__ valid, uint32_t plane) {
    const uint32_t p = blockIdx.x * FL_BLOCK + threadIdx.x;
    if (p >= plane) return;
    const FlResolved r = fl_resolve_pixel(comp[p], comp[(size_t)plane + p], comp[2 * (size_t)plane + p], alpha_min);
    flow[p] = r.u;
    flow[(size_t)plane + p] = r.v;
    alpha[p] = r.alpha;
    valid[p] = r.valid;
}

__global__ void __launch_bounds__(FL_BLOCK) fl_max_kernel(const float* __restrict__ flow, const uint8_t* __restrict__ valid, uint32_t plane,
                                                          uint32_t* __restrict__ max_bits) {
    __shared__ uint32_t s_max[FL_BLOCK / GP_WAVE];
    uint32_t m = 0u;
#pragma unroll
    for (int u = 0; u < FL_PER_LANE; ++u) {
        const uint32_t p = blockIdx.x * GP_FLOW_TILE + u * FL_BLOCK + threadIdx.x;
        if (p < plane) {
            const float fu = flow[p], fv = flow[(size_t)plane + p];
            if (fl_coloured(fu, fv, valid, p)) {
                const uint32_t b = fl_magnitude_bits(fu, fv);
                m = b > m ? b : m;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, d);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = s_max[0] > s_max[1] ? s_max[0] : s_max[1], b = s_max[2] > s_max[3] ? s_max[2] : s_max[3];
        a = a > b ? a : b;
        if (a != 0u) (void)__hip_atomic_fetch_max(max_bits, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(FL_BLOCK) fl_color_kernel(const float* __restrict__ flow, const uint8_t* __restrict__ valid, float max_flow,
                                                            float bg0, float bg1, float bg2, float* __restrict__ scale, float* __restrict__ out,
                                                            uint32_t plane) {
    __shared__ float s_wheel[GP_FLOW_WHEEL * 3];
    if (threadIdx.x < GP_FLOW_WHEEL * 3) s_wheel[threadIdx.x] = fl_wheel(threadIdx.x / 3, threadIdx.x % 3);
    __syncthreads();
    float s;
    if (max_flow > 0.f) {
        s = max_flow;
        if (blockIdx.x == 0 && threadIdx.x == 0) scale[0] = max_flow;       // (nobody reads it in this mode)
    } else {
        s = fl_scale_of(max_flow, scale[0]);                                // (fl_max_kernel's result: this launch is behind it)
    }
    const uint32_t p = blockIdx.x * FL_BLOCK + threadIdx.x;
    if (p >= plane) return;
    const float fu = flow[p], fv = flow[(size_t)plane + p];
    float col[3] = {bg0, bg1, bg2};
    if (fl_coloured(fu, fv, valid, p)) fl_color(fu, fv, s, s_wheel, col);
    out[p] = col[0];
    out[(size_t)plane + p] = col[1];
    out[2 * (size_t)plane + p] = col[2];
}

__global__ void __launch_bounds__(FL_BLOCK) fl_metric_kernel(const float* __restrict__ flow, const float* __restrict__ gt, const uint8_t* __restrict__ mask,
                                                             uint32_t plane, double* __restrict__ slots) {
    __shared__ float s_red[GP_FLOW_SUMS][FL_BLOCK / GP_WAVE];
    const uint32_t img = blockIdx.y;
    const float* f = flow + (size_t)img * 2 * plane;
    const float* g = gt + (size_t)img * 2 * plane;
    const uint8_t* mk = mask ? mask + (size_t)img * plane : nullptr;
    float t[GP_FLOW_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < FL_PER_LANE; ++u) {
        const uint32_t p = blockIdx.x * GP_FLOW_TILE + u * FL_BLOCK + threadIdx.x;
        if (p < plane) fl_metric_terms(f[p], f[(size_t)plane + p], g[p], g[(size_t)plane + p], !mk || mk[p] != 0, t);
    }
#pragma unroll
    for (int q = 0; q < GP_FLOW_SUMS; ++q) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) t[q] += __shfl_xor(t[q], d);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < GP_FLOW_SUMS; ++q) s_red[q][threadIdx.x >> 6] = t[q];
    }
    __syncthreads();
    if (threadIdx.x < GP_FLOW_SUMS) {
        const int q = threadIdx.x;
        slots[((size_t)img * gridDim.x + blockIdx.x) * GP_FLOW_SUMS + q] = (double)((s_red[q][0] + s_red[q][1]) + (s_red[q][2] + s_red[q][3]));
    }
}

__global__ void __launch_bounds__(FL_BLOCK) fl_metric_finalize(const double* __restrict__ slots, uint32_t tiles, double* __restrict__ table) {
    __shared__ double s_sum[GP_FLOW_SUMS][FL_BLOCK];
    const uint32_t img = blockIdx.x, tid = threadIdx.x;
    const double* base = slots + (size_t)img * tiles * GP_FLOW_SUMS;
    double a[GP_FLOW_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t k = tid; k < tiles; k += FL_BLOCK) {
#pragma unroll
        for (int q = 0; q < GP_FLOW_SUMS; ++q) a[q] += base[(size_t)k * GP_FLOW_SUMS + q];
    }
#pragma unroll
    for (int q = 0; q < GP_FLOW_SUMS; ++q) s_sum[q][tid] = a[q];
    __syncthreads();
    for (uint32_t stride = FL_BLOCK / 2; stride >= 1; stride >>= 1) {
        if (tid < stride) {
#pragma unroll
            for (int q = 0; q < GP_FLOW_SUMS; ++q) s_sum[q][tid] += s_sum[q][tid + stride];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double s[GP_FLOW_SUMS], row[GP_FLOW_COLUMNS];
#pragma unroll
        for (int q = 0; q < GP_FLOW_SUMS; ++q) s[q] = s_sum[q][0];
        fl_metric_row(s, row);
#pragma unroll
        for (int q = 0; q < GP_FLOW_COLUMNS; ++q) table[(size_t)img * GP_FLOW_COLUMNS + q] = row[q];
    }
}

__global__ void __launch_bounds__(FL_BLOCK) fl_warp_kernel(const float* __restrict__ image, const float* __restrict__ flow, float* __restrict__ out,
                                                           int32_t C, int32_t H, int32_t W) {
    const uint32_t plane = (uint32_t)H * (uint32_t)W;
    const uint32_t p = blockIdx.x * FL_BLOCK + threadIdx.x;
    if (p >= plane) return;
    const int32_t y = (int32_t)(p / (uint32_t)W), x = (int32_t)(p - (uint32_t)y * (uint32_t)W);
    const float fu = flow[p], fv = flow[(size_t)plane + p];
    for (int32_t c = 0; c < C; ++c) out[(size_t)c * plane + p] = fl_warp_pixel(image + (size_t)c * plane, H, W, x, y, fu, fv);
}

extern "C" int gp_flow_abi_version(void) { return GP_FLOW_ABI_VERSION; }

extern "C" int gp_flow_project(const gp_flow_view* view0, const gp_flow_view* view1, const float* xyz0, const float* xyz1, int64_t N, float* out,
                               gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (N < 0 || N >= 0x80000000LL) GP_FAIL("gp_flow_project: N must be >= 0 and below 2^31 (N = %lld)", (long long)N);
    if (!view0 || !view1) GP_FAIL("gp_flow_project: null argument");
    if (view0->W <= 0 || view0->H <= 0 || view1->W <= 0 || view1->H <= 0)
        GP_FAIL("gp_flow_project: H and W must be > 0 (view0 %d x %d, view1 %d x %d)", view0->W, view0->H, view1->W, view1->H);
    if (!view0->viewmatrix || !view0->projmatrix || !view1->viewmatrix || !view1->projmatrix) GP_FAIL("gp_flow_project: null argument");
    if (N == 0) return 0;
    if (!xyz0 || !xyz1 || !out) GP_FAIL("gp_flow_project: null argument");
    GpProfScope _p("flow_project", st);
    hipLaunchKernelGGL(fl_project_kernel, dim3(gp_blocks((size_t)N, FL_BLOCK)), dim3(FL_BLOCK), 0, st, view0->viewmatrix, view0->projmatrix, view0->W,
                       view0->H, view1->viewmatrix, view1->projmatrix, view1->W, view1->H, xyz0, xyz1, (uint32_t)N, out);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_flow_resolve(const float* composite, float alpha_min, float* flow, float* alpha, uint8_t* valid, int32_t H, int32_t W,
                               gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = fl_refuse_plane(H, W);
    if (why) GP_FAIL("gp_flow_resolve: %s (H = %d, W = %d)", why, H, W);
    if (alpha_min != alpha_min) GP_FAIL("gp_flow_resolve: alpha_min must not be NaN");
    if (!composite || !flow || !alpha || !valid) GP_FAIL("gp_flow_resolve: null argument");
    const uint32_t plane = (uint32_t)((int64_t)H * W);
    GpProfScope _p("flow_resolve", st);
    hipLaunchKernelGGL(fl_resolve_kernel, dim3(gp_blocks(plane, FL_BLOCK)), dim3(FL_BLOCK), 0, st, composite, alpha_min, flow, alpha, valid, plane);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_flow_colorize(const float* flow, const uint8_t* valid, float max_flow, float bg_r, float bg_g, float bg_b, float* scale, float* out,
                                int32_t H, int32_t W, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = fl_refuse_plane(H, W);
    if (why) GP_FAIL("gp_flow_colorize: %s (H = %d, W = %d)", why, H, W);
    if (max_flow != max_flow) GP_FAIL("gp_flow_colorize: max_flow must not be NaN");
    if (!flow || !scale || !out) GP_FAIL("gp_flow_colorize: null argument");
    const uint32_t plane = (uint32_t)((int64_t)H * W);
    GpProfScope _p("flow_colorize", st);
    if (!(max_flow > 0.f)) {
        GP_HIP_CHECK(hipMemsetAsync(scale, 0, sizeof(float), st));
        hipLaunchKernelGGL(fl_max_kernel, dim3(gp_blocks(plane, GP_FLOW_TILE)), dim3(FL_BLOCK), 0, st, flow, valid, plane, (uint32_t*)scale);
        GP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(fl_color_kernel, dim3(gp_blocks(plane, FL_BLOCK)), dim3(FL_BLOCK), 0, st, flow, valid, max_flow, bg_r, bg_g, bg_b, scale, out, plane);
    GP_LAUNCH_CHECK();
    return 0;
}

static const char* fl_refuse_batch(int32_t B, int32_t H, int32_t W) {
    if (B <= 0) return "B must be > 0";
    const char* why = fl_refuse_plane(H, W);
    if (why) return why;
    if (B > 65535) return "B must be at most 65535";
    return nullptr;
}

extern "C" int64_t gp_flow_metrics_scratch_bytes(int32_t B, int32_t H, int32_t W) {
    const char* why = fl_refuse_batch(B, H, W);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_flow_metrics_scratch_bytes: %s (B = %d, H = %d, W = %d)", why, B, H, W);
        return -1;
    }
    return (int64_t)B * fl_tiles(H, W) * GP_FLOW_SUMS * (int64_t)sizeof(double);
}

extern "C" int gp_flow_metrics(const float* flow, const float* gt, const uint8_t* mask, int32_t B, int32_t H, int32_t W, void* scratch, double* table,
                               gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = fl_refuse_batch(B, H, W);
    if (why) GP_FAIL("gp_flow_metrics: %s (B = %d, H = %d, W = %d)", why, B, H, W);
    if (!flow || !gt || !scratch || !table) GP_FAIL("gp_flow_metrics: null argument");
    if (((uintptr_t)scratch & 7u) != 0) GP_FAIL("gp_flow_metrics: scratch must be 8-byte aligned");
    const uint32_t plane = (uint32_t)((int64_t)H * W), tiles = (uint32_t)fl_tiles(H, W);
    GpProfScope _p("flow_metrics", st);
    hipLaunchKernelGGL(fl_metric_kernel, dim3(tiles, (unsigned)B), dim3(FL_BLOCK), 0, st, flow, gt, mask, plane, (double*)scratch);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(fl_metric_finalize, dim3((unsigned)B), dim3(FL_BLOCK), 0, st, (const double*)scratch, tiles, table);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_flow_warp(const float* image, const float* flow, float* out, int32_t C, int32_t H, int32_t W, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (C <= 0) GP_FAIL("gp_flow_warp: C must be > 0 (C = %d)", C);
    const char* why = fl_refuse_plane(H, W);
    if (why) GP_FAIL("gp_flow_warp: %s (H = %d, W = %d)", why, H, W);
    if ((int64_t)C * H * W >= 0x80000000LL) GP_FAIL("gp_flow_warp: C*H*W must be below 2^31 (C = %d, H = %d, W = %d)", C, H, W);
    if (!image || !flow || !out) GP_FAIL("gp_flow_warp: null argument");
    const uint32_t plane = (uint32_t)((int64_t)H * W);
    GpProfScope _p("flow_warp", st);
    hipLaunchKernelGGL(fl_warp_kernel, dim3(gp_blocks(plane, FL_BLOCK)), dim3(FL_BLOCK), 0, st, image, flow, out, C, H, W);
    GP_LAUNCH_CHECK();
    return 0;
}
