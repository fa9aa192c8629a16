// densify_kernels.hip -- densify (clone + split), opacity reset and prune on the device (include/gp_densify.h), gfx950.
//
//   gp_densify_stats   one launch: the per-view statistics of the visible rows
//   gp_densify_plan    two launches: per-row keep bits + per-block class counts; one workgroup scans the block counts and writes the
//                      status block
//   gp_densify_apply   one launch: workgroup b owns input rows [256 b, 256 b + 256).  The rows it keeps in segment j are a contiguous
//                      run of the output (segment base + the scanned count of the blocks before it), so a lane owns a flat float
//                      index of that run: stores are fully coalesced, loads are coalesced inside every run of consecutive survivors.
//                      Ranks inside the block come from the keep bytes by ballot and popcount.
// No atomics, no host reads; plain (vector) stores only.
#include "gp_common.h"

#include "../../include/gp_densify.h"

#define DN_BLOCK GP_DENSIFY_BLOCK
#define DN_WAVES (DN_BLOCK / GP_WAVE)
#define DN_CLASSES 6       // keep bits of segments 0..3, clone selected, split selected
#define DN_CLONE_BIT 4
#define DN_SPLIT_BIT 5
static_assert(DN_BLOCK == 256, "the apply keeps block-local row numbers in one byte");

// ------------------------------------------------------------------------------------------------
// the arithmetic, stated once (plan and apply must agree on it)
// ------------------------------------------------------------------------------------------------
// torch.max over a row propagates a NaN
__device__ __forceinline__ float dn_max2(float a, float b) { return (a != a) ? a : ((b > a || b != b) ? b : a); }
__device__ __forceinline__ float dn_max3(float a, float b, float c) { return dn_max2(dn_max2(a, b), c); }
__device__ __forceinline__ float dn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
// inverse_sigmoid(min(sigmoid(o), 0.01)); torch.minimum propagates a NaN
__device__ __forceinline__ float dn_reset_opacity(float o) {
    const float s = dn_sigmoid(o);
    const float m = (s < 0.01f || s != s) ? s : 0.01f;
    return logf(m / (1.f - m));
}
// log(exp(s) / 1.6), the division as the multiplication by the rounded reciprocal that torch's device kernel for `tensor / scalar` performs
__device__ __forceinline__ float dn_shrink(float e) { return logf(e * (1.0f / 1.6f)); }

// ------------------------------------------------------------------------------------------------
// per-view statistics
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DN_BLOCK) void gp_densify_stats_kernel(size_t N, const uint8_t* __restrict__ visible, const int32_t* __restrict__ radii,
                                                                   const float* __restrict__ grad, float* __restrict__ max_radii2D,
                                                                   float* __restrict__ accum, float* __restrict__ denom, float* __restrict__ accum_max) {
    const size_t i = (size_t)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (i >= N || !visible[i]) return;
    const float r = (float)radii[i], m = max_radii2D[i];
    max_radii2D[i] = (r > m) ? r : m;
    const float gx = grad[3 * i], gy = grad[3 * i + 1];
    const float s = sqrtf(gx * gx + gy * gy);
    accum[i] += s;
    denom[i] += 1.f;
    const float a = accum_max[i];
    accum_max[i] = (s > a) ? s : a;
}

// ------------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------------
struct DnThresholds {
    float grad, dense, min_opacity, screen, world;
    uint32_t flags;
};

__global__ __launch_bounds__(DN_BLOCK) void gp_densify_plan_kernel(size_t N, const float* __restrict__ accum, const float* __restrict__ denom,
                                                                  const float* __restrict__ max_radii2D, const float* __restrict__ scaling,
                                                                  const float* __restrict__ opacity, DnThresholds t, uint8_t* __restrict__ keep,
                                                                  uint32_t* __restrict__ counts, uint32_t nb) {
    __shared__ uint32_t s_cnt[DN_WAVES][DN_CLASSES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t i = (size_t)blockIdx.x * DN_BLOCK + tid;
    uint32_t bits = 0;
    if (i < N) {
        const bool densify = t.flags & GP_DENSIFY_DENSIFY, reset = t.flags & GP_DENSIFY_RESET, prune = t.flags & GP_DENSIFY_PRUNE;
        const float e0 = expf(scaling[3 * i]), e1 = expf(scaling[3 * i + 1]), e2 = expf(scaling[3 * i + 2]);
        const float smax = dn_max3(e0, e1, e2);
        bool clone = false, split = false;
        if (densify) {
            const float d = denom[i];
            const float g = (d > 0.f) ? accum[i] / fmaxf(d, 1.f) : 0.f;      // _mean_grad
            clone = (fabsf(g) >= t.grad) && (smax <= t.dense);
            split = (g >= t.grad) && (smax > t.dense);
        }
        bool pruned_same = false, pruned_split = false;      // rows with the source's scaling / with the shrunk scaling
        if (prune) {
            float o = opacity[i];
            if (reset) o = dn_reset_opacity(o);
            pruned_same = pruned_split = dn_sigmoid(o) < t.min_opacity;
            if (t.flags & GP_DENSIFY_SCREEN) {
                const float radius = densify ? 0.f : max_radii2D[i];          // densification_postfix zeroes it for every row
                const bool big_vs = radius > t.screen;
                pruned_same |= big_vs || (smax > t.world);
                if (split) {
                    const float shrunk = dn_max3(expf(dn_shrink(e0)), expf(dn_shrink(e1)), expf(dn_shrink(e2)));
                    pruned_split |= big_vs || (shrunk > t.world);
                }
            }
        }
        if (!split && !pruned_same) bits |= 1u;
        if (clone && !pruned_same) bits |= 2u;
        if (split && !pruned_split) bits |= 4u | 8u;
        if (clone) bits |= 1u << DN_CLONE_BIT;
        if (split) bits |= 1u << DN_SPLIT_BIT;
        keep[i] = (uint8_t)bits;
    }
#pragma unroll
    for (int k = 0; k < DN_CLASSES; ++k) {
        const unsigned long long b = __ballot((bits >> k) & 1u);
        if (lane == 0) s_cnt[wave][k] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (tid < DN_CLASSES) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < DN_WAVES; ++w) c += s_cnt[w][tid];
        counts[(size_t)tid * nb + blockIdx.x] = c;
    }
}

// One workgroup: wave k turns the block counts of segment k into exclusive prefixes, in place; waves 0 and 1 also add up the clone /
// split selections; thread 0 writes the status block.
__global__ __launch_bounds__(DN_BLOCK) void gp_densify_scan_kernel(uint32_t N, uint32_t* __restrict__ counts, uint32_t nb, uint32_t* __restrict__ status) {
    __shared__ uint32_t s_total[DN_CLASSES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* c = counts + (size_t)wave * nb;
    uint32_t run = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += GP_WAVE) {
        const uint32_t b = b0 + lane;
        const uint32_t v = (b < nb) ? c[b] : 0u;
        const uint32_t incl = (uint32_t)gp_wave_scan_add((int)v);
        if (b < nb) c[b] = run + incl - v;
        run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (lane == 0) s_total[wave] = run;
    if (wave < 2) {
        const uint32_t* sel = counts + (size_t)(DN_CLONE_BIT + wave) * nb;
        uint32_t sum = 0;
        for (uint32_t b = lane; b < nb; b += GP_WAVE) sum += sel[b];
        sum = (uint32_t)gp_wave_scan_add((int)sum);
        if (lane == 63) s_total[DN_CLONE_BIT + wave] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t k0 = s_total[0], k1 = s_total[1], k2 = s_total[2], k3 = s_total[3];
        const uint32_t cloned = s_total[DN_CLONE_BIT], split = s_total[DN_SPLIT_BIT];
        status[GP_DENSIFY_ST_CLONED] = cloned;
        status[GP_DENSIFY_ST_SPLIT] = split;
        status[GP_DENSIFY_ST_PRUNED] = (N - split - k0) + (cloned - k1) + (split - k2) + (split - k3);
        status[GP_DENSIFY_ST_ROWS] = k0 + k1 + k2 + k3;
        status[GP_DENSIFY_ST_BASE + 0] = 0;
        status[GP_DENSIFY_ST_BASE + 1] = k0;
        status[GP_DENSIFY_ST_BASE + 2] = k0 + k1;
        status[GP_DENSIFY_ST_BASE + 3] = k0 + k1 + k2;
    }
}

// ------------------------------------------------------------------------------------------------
// apply
// ------------------------------------------------------------------------------------------------
struct DnTable {
    gp_densify_tensor t[GP_DENSIFY_MAX_TENSORS];
    const float* stats_in[4];
    float* stats_out[4];
    const float* scaling;      // the inputs of the SCALING / ROTATION entries: a split copy's xyz reads them
    const float* rotation;
    const float* normals;
    int32_t n;
};

enum { DN_COPY, DN_NEW, DN_XYZ, DN_SHRINK, DN_RESET };

// One contiguous run of `cnt` output rows of one tensor: lane f owns floats f, f + 256, ... of it; (row, col) advance without a
// division inside the loop.
template <int MODE>
__device__ __forceinline__ void dn_run(const gp_densify_tensor& e, const DnTable& tab, const uint8_t* __restrict__ src_of, uint32_t cnt,
                                       size_t in_row0, size_t out_row0, size_t out_rows, size_t N, int copy_no) {
    const uint32_t w = (uint32_t)e.width, total = cnt * w;
    const uint32_t dr = DN_BLOCK / w, dc = DN_BLOCK % w;
    uint32_t r = threadIdx.x / w, c = threadIdx.x % w;
    for (uint32_t f = threadIdx.x; f < total; f += DN_BLOCK) {
        const size_t orow = out_row0 + r;
        if (orow < out_rows) {
            const size_t srow = in_row0 + src_of[r];
            const size_t si = srow * w + c, oi = orow * w + c;
            float val = e.in[si];
            if (MODE == DN_SHRINK) val = dn_shrink(expf(val));
            if (MODE == DN_RESET) val = dn_reset_opacity(val);
            if (MODE == DN_XYZ) {
                const float* q = tab.rotation + 4 * srow;
                const float* s = tab.scaling + 3 * srow;
                const float* z = tab.normals + ((size_t)copy_no * N + srow) * 3;
                const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);      // build_rotation
                const float qw = q[0] / n, qx = q[1] / n, qy = q[2] / n, qz = q[3] / n;
                float r0, r1, r2;
                if (c == 0) { r0 = 1.f - 2.f * (qy * qy + qz * qz); r1 = 2.f * (qx * qy - qw * qz); r2 = 2.f * (qx * qz + qw * qy); }
                else if (c == 1) { r0 = 2.f * (qx * qy + qw * qz); r1 = 1.f - 2.f * (qx * qx + qz * qz); r2 = 2.f * (qy * qz - qw * qx); }
                else { r0 = 2.f * (qx * qz - qw * qy); r1 = 2.f * (qy * qz + qw * qx); r2 = 1.f - 2.f * (qx * qx + qy * qy); }
                const float v0 = z[0] * expf(s[0]), v1 = z[1] * expf(s[1]), v2 = z[2] * expf(s[2]);
                val = fmaf(r2, v2, fmaf(r1, v1, r0 * v0)) + val;                                  // a 3-term dot product accumulated by FMA
            }
            e.out[oi] = val;
            if (e.out_exp_avg) {
                e.out_exp_avg[oi] = (MODE == DN_COPY) ? e.in_exp_avg[si] : 0.f;
                e.out_exp_avg_sq[oi] = (MODE == DN_COPY) ? e.in_exp_avg_sq[si] : 0.f;
            }
        }
        r += dr; c += dc;
        if (c >= w) { c -= w; ++r; }
    }
}

__global__ __launch_bounds__(DN_BLOCK) void gp_densify_apply_kernel(size_t N, DnTable tab, size_t out_rows, uint32_t flags,
                                                                   const uint8_t* __restrict__ keep, const uint32_t* __restrict__ prefix, uint32_t nb,
                                                                   const uint32_t* __restrict__ status) {
    __shared__ uint8_t s_src[4][DN_BLOCK];       // segment j: the block-local input row of its r-th kept row
    __shared__ uint32_t s_wcnt[4][DN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row0 = (size_t)blockIdx.x * DN_BLOCK;
    const uint32_t bits = (row0 + tid < N) ? keep[row0 + tid] : 0u;
    uint32_t rank[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long b = __ballot((bits >> j) & 1u);
        rank[j] = gp_mbcnt(b);
        if (lane == 0) s_wcnt[j][wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    uint32_t cnt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < DN_WAVES; ++w) {
            const uint32_t c = s_wcnt[j][w];
            if (w < wave) before += c;
            all += c;
        }
        cnt[j] = all;
        if ((bits >> j) & 1u) s_src[j][before + rank[j]] = (uint8_t)tid;
    }
    __syncthreads();
    const bool densify = flags & GP_DENSIFY_DENSIFY, reset = flags & GP_DENSIFY_RESET;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        if (cnt[j] == 0) continue;
        const size_t out0 = (size_t)status[GP_DENSIFY_ST_BASE + j] + prefix[(size_t)j * nb + blockIdx.x];
        const uint8_t* src_of = s_src[j];
#pragma unroll 1
        for (int k = 0; k < tab.n; ++k) {
            const gp_densify_tensor& e = tab.t[k];
            if (reset && e.role == GP_DENSIFY_ROLE_OPACITY) dn_run<DN_RESET>(e, tab, src_of, cnt[j], row0, out0, out_rows, N, 0);
            else if (j >= 2 && e.role == GP_DENSIFY_ROLE_XYZ) dn_run<DN_XYZ>(e, tab, src_of, cnt[j], row0, out0, out_rows, N, j - 2);
            else if (j >= 2 && e.role == GP_DENSIFY_ROLE_SCALING) dn_run<DN_SHRINK>(e, tab, src_of, cnt[j], row0, out0, out_rows, N, 0);
            else if (j == 0) dn_run<DN_COPY>(e, tab, src_of, cnt[j], row0, out0, out_rows, N, 0);
            else dn_run<DN_NEW>(e, tab, src_of, cnt[j], row0, out0, out_rows, N, 0);
        }
        // the statistics: zero after a densify [REF scene/gaussian_model.py:657-661], else compacted (only segment 0 has rows then)
        for (uint32_t r = tid; r < cnt[j]; r += DN_BLOCK) {
            const size_t orow = out0 + r, srow = row0 + src_of[r];
            if (orow >= out_rows) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) tab.stats_out[k][orow] = densify ? 0.f : tab.stats_in[k][srow];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------------
static inline uint32_t dn_blocks(int64_t N) { return (uint32_t)((N + DN_BLOCK - 1) / DN_BLOCK); }

struct DnScratch {
    uint8_t* keep;
    uint32_t* counts;
    size_t bytes;
    DnScratch(void* p, int64_t N) {
        GpCarver c(p);
        keep = c.take<uint8_t>((size_t)N);
        counts = c.take<uint32_t>((size_t)DN_CLASSES * dn_blocks(N));
        bytes = c.bytes();
    }
};

extern "C" int gp_densify_abi_version(void) { return GP_DENSIFY_ABI_VERSION; }

extern "C" int64_t gp_densify_scratch_bytes(int64_t N) {
    if (N < 1 || N > GP_DENSIFY_MAX_ROWS) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_densify_scratch_bytes: N = %lld outside [1, %d]", (long long)N, GP_DENSIFY_MAX_ROWS);
        return -1;
    }
    return (int64_t)DnScratch(nullptr, N).bytes;
}

extern "C" int gp_densify_stats(int64_t N, const uint8_t* visible, const int32_t* radii, const float* grad, float* max_radii2D, float* accum,
                                float* denom, float* accum_max, gp_stream_t stream_) {
    if (N < 0 || N > GP_DENSIFY_MAX_ROWS) GP_FAIL("gp_densify_stats: N = %lld outside [0, %d]", (long long)N, GP_DENSIFY_MAX_ROWS);
    if (N == 0) return 0;
    if (!visible || !radii || !grad || !max_radii2D || !accum || !denom || !accum_max) GP_FAIL("gp_densify_stats: null argument");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("densify_stats", s);
    hipLaunchKernelGGL(gp_densify_stats_kernel, dim3(dn_blocks(N)), dim3(DN_BLOCK), 0, s, (size_t)N, visible, radii, grad, max_radii2D, accum,
                       denom, accum_max);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_densify_plan(int64_t N, const float* accum, const float* denom, const float* max_radii2D, const float* scaling,
                               const float* opacity, float grad_threshold, float dense_extent, float min_opacity, float max_screen_size,
                               float world_extent, uint32_t flags, void* scratch, uint32_t* status, gp_stream_t stream_) {
    if (N < 1 || N > GP_DENSIFY_MAX_ROWS) GP_FAIL("gp_densify_plan: N = %lld outside [1, %d]", (long long)N, GP_DENSIFY_MAX_ROWS);
    if (!(grad_threshold > 0.f))
        GP_FAIL("gp_densify_plan: grad_threshold = %g must be > 0 (the split pass relies on the zero gradient of cloned rows failing it)",
                (double)grad_threshold);
    if (flags & ~(GP_DENSIFY_DENSIFY | GP_DENSIFY_RESET | GP_DENSIFY_PRUNE | GP_DENSIFY_SCREEN)) GP_FAIL("gp_densify_plan: unknown flags 0x%x", flags);
    if (!accum || !denom || !max_radii2D || !scaling || !opacity || !scratch || !status) GP_FAIL("gp_densify_plan: null argument");
    if ((uintptr_t)scratch & 255) GP_FAIL("gp_densify_plan: scratch must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("densify_plan", s);
    DnScratch sc(scratch, N);
    const uint32_t nb = dn_blocks(N);
    DnThresholds t = {grad_threshold, dense_extent, min_opacity, max_screen_size, world_extent, flags};
    hipLaunchKernelGGL(gp_densify_plan_kernel, dim3(nb), dim3(DN_BLOCK), 0, s, (size_t)N, accum, denom, max_radii2D, scaling, opacity, t, sc.keep,
                       sc.counts, nb);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(gp_densify_scan_kernel, dim3(1), dim3(DN_BLOCK), 0, s, (uint32_t)N, sc.counts, nb, status);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_densify_apply(int64_t N, int32_t num_tensors, const gp_densify_tensor* tensors, const float* normals,
                                const float* const* stats_in, float* const* stats_out, int64_t out_rows, uint32_t flags, const void* scratch,
                                const uint32_t* status, gp_stream_t stream_) {
    if (N < 1 || N > GP_DENSIFY_MAX_ROWS) GP_FAIL("gp_densify_apply: N = %lld outside [1, %d]", (long long)N, GP_DENSIFY_MAX_ROWS);
    if (num_tensors < 1 || num_tensors > GP_DENSIFY_MAX_TENSORS)
        GP_FAIL("gp_densify_apply: num_tensors = %d outside [1, %d]", num_tensors, GP_DENSIFY_MAX_TENSORS);
    if (out_rows < 0 || out_rows > 2 * (int64_t)GP_DENSIFY_MAX_ROWS) GP_FAIL("gp_densify_apply: out_rows = %lld", (long long)out_rows);
    if (flags & ~(GP_DENSIFY_DENSIFY | GP_DENSIFY_RESET | GP_DENSIFY_PRUNE | GP_DENSIFY_SCREEN)) GP_FAIL("gp_densify_apply: unknown flags 0x%x", flags);
    if (!tensors || !stats_in || !stats_out || !scratch || !status) GP_FAIL("gp_densify_apply: null argument");
    if ((uintptr_t)scratch & 255) GP_FAIL("gp_densify_apply: scratch must be 256-byte aligned");
    if (out_rows == 0) return 0;
    DnTable tab;
    memset(&tab, 0, sizeof(tab));
    tab.n = num_tensors;
    tab.normals = normals;
    static const int32_t role_width[5] = {0, 3, 3, 4, 1};
    bool has_opacity = false, has_xyz = false;
    for (int k = 0; k < num_tensors; ++k) {
        const gp_densify_tensor& e = tensors[k];
        if (!e.in || !e.out) GP_FAIL("gp_densify_apply: tensor %d has a null parameter pointer", k);
        if (e.width < 1 || e.width > 65536) GP_FAIL("gp_densify_apply: tensor %d has width %d", k, e.width);
        const int moments = !!e.in_exp_avg + !!e.in_exp_avg_sq + !!e.out_exp_avg + !!e.out_exp_avg_sq;
        if (moments != 0 && moments != 4) GP_FAIL("gp_densify_apply: tensor %d: the four moment pointers are all NULL or all set", k);
        if (e.role < 0 || e.role > GP_DENSIFY_ROLE_OPACITY) GP_FAIL("gp_densify_apply: tensor %d has role %d", k, e.role);
        if (e.role != GP_DENSIFY_ROLE_NONE && e.width != role_width[e.role])
            GP_FAIL("gp_densify_apply: tensor %d with role %d must have width %d (got %d)", k, e.role, role_width[e.role], e.width);
        if (e.role == GP_DENSIFY_ROLE_SCALING) tab.scaling = e.in;
        if (e.role == GP_DENSIFY_ROLE_ROTATION) tab.rotation = e.in;
        has_opacity |= e.role == GP_DENSIFY_ROLE_OPACITY;
        has_xyz |= e.role == GP_DENSIFY_ROLE_XYZ;
        tab.t[k] = e;
    }
    if ((flags & GP_DENSIFY_DENSIFY) && !(has_xyz && tab.scaling && tab.rotation && normals))
        GP_FAIL("gp_densify_apply: GP_DENSIFY_DENSIFY needs the XYZ, SCALING and ROTATION entries and the normals");
    if ((flags & GP_DENSIFY_RESET) && !has_opacity) GP_FAIL("gp_densify_apply: GP_DENSIFY_RESET needs the OPACITY entry");
    for (int k = 0; k < 4; ++k) {
        if (!stats_in[k] || !stats_out[k]) GP_FAIL("gp_densify_apply: statistics pointer %d is null", k);
        tab.stats_in[k] = stats_in[k];
        tab.stats_out[k] = stats_out[k];
    }
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("densify_apply", s);
    DnScratch sc(const_cast<void*>(scratch), N);
    const uint32_t nb = dn_blocks(N);
    hipLaunchKernelGGL(gp_densify_apply_kernel, dim3(nb), dim3(DN_BLOCK), 0, s, (size_t)N, tab, (size_t)out_rows, flags, (const uint8_t*)sc.keep,
                       (const uint32_t*)sc.counts, nb, status);
    GP_LAUNCH_CHECK();
    return 0;
}
