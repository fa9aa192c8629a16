// loss_adam_kernels.h -- the multi-tensor Adam launch's table and chunk body (shared by gp_adam_multi_kernel and by the launches that
// carry the same chunks: the keypoint MLP's data backward, deform_mlp_small.hip, and the keypoint blend's backward, deform_kernels.hip),
// the loss finalize's body (the blend backward's launch carries it too), and the fused step's internal interface: the "rider" structs
// that gp_train_step_run keeps on its stack and the _impl forms of the carrying entry points that take them as arguments (the public
// entry points of include/gp_hip.h are wrappers that pass "no riders").  Everything else of loss_adam_kernels.hip is private to it.
#pragma once
#include "gp_common.h"

#define ADAM_MAX_TENSORS 32
#define ADAM_CHUNK 16384   // elements per workgroup-chunk
struct AdamTable {
    float* p[ADAM_MAX_TENSORS];
    float* g[ADAM_MAX_TENSORS];
    float* m[ADAM_MAX_TENSORS];
    float* v[ADAM_MAX_TENSORS];
    unsigned long long n[ADAM_MAX_TENSORS];
    float step_size[ADAM_MAX_TENSORS];           // lr / (1 - beta1^t) with the TENSOR's step count t
    float bc2_sqrt[ADAM_MAX_TENSORS];            // sqrt(1 - beta2^t)
    unsigned keep_grad_mask;                     // bit k: leave tensor k's gradient as it is
    unsigned chunk_begin[ADAM_MAX_TENSORS + 1];   // prefix of chunk counts
    int count;
};

// One chunk (ADAM_CHUNK elements of one tensor) by a workgroup of THREADS threads: element-wise, so the result does not depend on
// THREADS or on which launch carries the chunk.
template <int THREADS>
__device__ __forceinline__ void adam_chunk_body(const AdamTable& t, unsigned chunk, int tid, float b1, float b2, float eps, int zero_grad,
                                                const uint32_t* __restrict__ skip_flag) {
    const bool skip = skip_flag && *skip_flag != 0;      // the frame that produced these gradients was invalid: no update
    int k = 0;
    while (k + 1 < t.count && chunk >= t.chunk_begin[k + 1]) ++k;
    const size_t base = (size_t)(chunk - t.chunk_begin[k]) * ADAM_CHUNK;
    const size_t n = t.n[k];
    float* __restrict__ p = t.p[k]; float* __restrict__ g = t.g[k]; float* __restrict__ m = t.m[k]; float* __restrict__ v = t.v[k];
    const float step_size = t.step_size[k], bc2_sqrt = t.bc2_sqrt[k];
    if ((t.keep_grad_mask >> k) & 1u) zero_grad = 0;
    const size_t end = base + ADAM_CHUNK < n ? base + ADAM_CHUNK : n;
    auto upd = [&](float4& pv, const float4& gv, float4& mv, float4& vv) {
        float* pp = (float*)&pv; const float* gg = (const float*)&gv; float* mm = (float*)&mv; float* vq = (float*)&vv;
#pragma unroll
        for (int u = 0; u < 4; ++u) gp_adam_update(pp[u], gg[u], mm[u], vq[u], b1, b2, eps, step_size, bc2_sqrt);
    };
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    size_t i = base + (size_t)tid * 4;
    if (skip) {             // discard the gradients (where this pass owns their zeroing), leave p / m / v untouched
        if (zero_grad)
            for (size_t j = base + tid; j < end; j += THREADS) g[j] = 0.f;
        return;
    }
    // two independent 16-byte streams per thread and iteration: 8 loads in flight per lane
    constexpr size_t S = (size_t)THREADS * 4;
    for (; i + S + 3 < end; i += 2 * S) {
        const size_t j = i + S;
        float4 pa = *(float4*)(p + i), ga = *(float4*)(g + i), ma = *(float4*)(m + i), va = *(float4*)(v + i);
        float4 pb = *(float4*)(p + j), gb = *(float4*)(g + j), mb = *(float4*)(m + j), vb = *(float4*)(v + j);
        upd(pa, ga, ma, va);
        upd(pb, gb, mb, vb);
        *(float4*)(p + i) = pa; *(float4*)(m + i) = ma; *(float4*)(v + i) = va;
        *(float4*)(p + j) = pb; *(float4*)(m + j) = mb; *(float4*)(v + j) = vb;
        if (zero_grad) { *(float4*)(g + i) = zero4; *(float4*)(g + j) = zero4; }
    }
    for (; i < end; i += S) {
        if (i + 3 < n) {
            float4 pv = *(float4*)(p + i), gv = *(float4*)(g + i), mv = *(float4*)(m + i), vv = *(float4*)(v + i);
            upd(pv, gv, mv, vv);
            *(float4*)(p + i) = pv; *(float4*)(m + i) = mv; *(float4*)(v + i) = vv;
            if (zero_grad) *(float4*)(g + i) = zero4;
        } else {
            for (size_t j = i; j < n; ++j) {
                gp_adam_update(p[j], g[j], m[j], v[j], b1, b2, eps, step_size, bc2_sqrt);
                if (zero_grad) g[j] = 0.f;
            }
        }
    }
}

// The rider: an optimizer launch whose tensors need nothing the keypoint MLP's backward produces (the per-Gaussian tensors: HBM-bound,
// every CU) travels in the SAME launch as that backward's data kernel (16 workgroups, bound by the rate at which one CU takes the
// weights in) -- gp_train_step_run fills the struct and passes it to gp_mlp_backward_impl, whose small-row path carries it and clears
// `armed`; a rider that comes back armed is launched on its own (gp_adam_rider_launch).  Host-only.
struct GpAdamRider {
    AdamTable t;
    float b1, b2, eps;
    int zero_grad;
    const uint32_t* skip_flag;
    unsigned chunks;
    bool armed;
};
// fills `r` from the optimizer's arrays (the arguments of gp_adam_step_multi_steps); armed unless there is nothing to update
int gp_adam_rider_fill(GpAdamRider* r, int count, float* const* params, float* const* grads, float* const* exp_avgs,
                       float* const* exp_avg_sqs, const int64_t* numels, const float* lrs, const int64_t* steps, float beta1, float beta2,
                       float eps, int zero_grad, uint32_t keep_grad_mask, const uint32_t* skip_flag);
int gp_adam_rider_launch(GpAdamRider* r, hipStream_t s);    // an armed rider as a plain gp_adam_multi_kernel (scope "adam"); disarms it
int gp_mlp_backward_impl(const gp_mlp_params* p, const gp_mlp_input* x, const float* acts, const float* dL_dout, gp_mlp_grads* g,
                         float* dL_dfeature, float* dL_dxyz, gp_alloc_fn alloc, void* alloc_ctx, gp_stream_t stream, GpAdamRider* rider,
                         bool accumulate_dfeature);         // (rider may be NULL; "+=" into dL_dfeature: the feature-split kernel only)
bool gp_mlp_backward_splits(const gp_mlp_params* p, int64_t rows);      // would it take the feature-split data kernel?

// ---- the loss scalar: loss = (1-lam) * sums[0]/n + lam * (1 - sums[1]/n) [+ scale/n * sum|x|], one 256-thread workgroup
__device__ __forceinline__ float block_sum_256(float v, float* s_red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}
// The slot totals in a fixed order: thread k walks slots k, k + 256, ..., xor-butterfly inside the wave, the four wave sums
// through LDS.  (Round 2 let ONE thread walk the slots: 512 dependent double loads, 19 us for a scalar.)
__device__ __forceinline__ void loss_slot_totals(const double* __restrict__ sums, int nslots, double* s_red /*[8]*/, double& s0, double& s1) {
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    // eight slot pairs per trip to memory, added in the same order as one by one (as a rolled loop every pair was a dependent
    // round trip: 16 + 8 of them made this scalar's kernel 9.5 us between the loss forward and its backward)
    const double2* s2 = reinterpret_cast<const double2*>(sums);
    for (int k0 = tid; k0 < nslots; k0 += 256 * 8) {
        double2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int k = k0 + 256 * u; v[u] = s2[k < nslots ? k : nslots - 1]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) if (k0 + 256 * u < nslots) { a += v[u].x; b += v[u].y; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_xor(a, d);
        b += __shfl_xor(b, d);
    }
    if ((tid & 63) == 0) { s_red[2 * (tid >> 6)] = a; s_red[2 * (tid >> 6) + 1] = b; }
    __syncthreads();
    s0 = (s_red[0] + s_red[2]) + (s_red[4] + s_red[6]);
    s1 = (s_red[1] + s_red[3]) + (s_red[5] + s_red[7]);
}
struct LossFinalizeDev {
    const double* sums;         // [nslots][2]: the loss kernel's per-tile sums
    int nslots;
    double n;                   // channels * H * W
    float lambda;
    const float* x;             // the regulariser's input (NULL: no regulariser term)
    long nx;
    float scale_over_n;
    float* loss;
};
// (fixed summation order: the same scalar whichever launch carries the workgroup)
__device__ __forceinline__ void loss_finalize_body(const LossFinalizeDev& f, float* s_red /*[4]*/, double* s_tot /*[8]*/) {
    float tot = 0.f;
    if (f.x) {
        const float* __restrict__ x = f.x;
        const long nx = f.nx;
        float acc = 0.f;
        if ((nx & 3) == 0 && (((uintptr_t)x) & 15) == 0) {          // 16-byte loads, four independent per thread in flight
            const float4* x4 = (const float4*)x;
            const long n4 = nx >> 2;
            for (long i0 = threadIdx.x; i0 < n4; i0 += 256 * 8) {
                float4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const long i = i0 + 256 * u; v[u] = x4[i < n4 ? i : n4 - 1]; }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (i0 + 256 * u < n4) acc += (fabsf(v[u].x) + fabsf(v[u].y)) + (fabsf(v[u].z) + fabsf(v[u].w));
            }
        } else {
            for (long i = threadIdx.x; i < nx; i += 256) acc += fabsf(x[i]);
        }
        tot = block_sum_256(acc, s_red);
    }
    double s0, s1;
    loss_slot_totals(f.sums, f.nslots, s_tot, s0, s1);
    if (threadIdx.x == 0) {
        const float l = (float)((1.0 - (double)f.lambda) * s0 / f.n + (double)f.lambda * (1.0 - s1 / f.n));
        f.loss[0] = f.x ? l + tot * f.scale_over_n : l;
    }
}

// (validated; x may be NULL: no regulariser term)
int gp_loss_finalize_fill(LossFinalizeDev* f, const double* sums, int32_t channels, int32_t H, int32_t W, float lambda_dssim, const float* x,
                          int64_t n, float scale, float* loss);
int gp_loss_finalize_launch(const LossFinalizeDev& f, hipStream_t s);   // one workgroup of its own (gp_loss_finalize_reg_kernel)

// ---- riders of the keypoint blend's backward launch (gp_blend_backward_impl, nn = 6 / 8 kernels; deform_kernels.hip).  That launch is
// bound by its own instruction stream and leaves HBM half idle; gp_train_step_run puts into it, as workgroups IN FRONT of the blend's own:
//   * the loss finalize (one workgroup): nothing on the device reads the scalar, and the launch runs before every optimizer launch
//     that moves the regulariser's input;
//   * the Adam chunks of the tensors whose gradients the projection backward has already finished (_scaling, _opacity).
// gp_blend_backward_impl clears the flags of what it carried; whatever comes back armed its caller launches on its own.
struct BlendRideDev {
    AdamTable t;
    float b1, b2, eps;
    int zero_grad;
    const uint32_t* skip_flag;
    unsigned adam_chunks;       // workgroups [fin_blocks, fin_blocks + adam_chunks): one Adam chunk each
    unsigned fin_blocks;        // 0 / 1: workgroup 0 is the loss finalize
    LossFinalizeDev fin;
};
struct GpBlendRider {           // host-only
    GpAdamRider adam;
    LossFinalizeDev fin;
    bool fin_armed;
};
int gp_blend_backward_impl(const gp_blend_args* a, const float* dL_dxyz_t, const float* dL_dq_t, float* dL_ddelta, float* dL_draw_w,
                           float* dL_dxyz, float* dL_drot, gp_alloc_fn alloc, void* alloc_ctx, gp_stream_t stream, GpBlendRider* riders);

// ---- rider of the fused loss launch (gp_loss_l1_ssim_fused_impl): the composite backward's prologue -- its tile order (needs the
// composite FORWARD's ranges and tile_work only) and the zero fill of its accumulators (needs nothing).  gp_train_step_run obtains the
// backward's TEMP block ahead of the loss (gp_raster_backward_prepare, gp_capi_raster.hip: `pro` describes the prologue, armed = false
// where the stand-alone prologue has to run), hands `pro` to the loss launch and pro.acc to gp_raster_backward_impl as `prepared_acc`.
struct GpLossPrologue {
    const int2* ranges;
    const int32_t* tile_work;
    int T;
    uint32_t* order;
    float* acc;
    size_t acc_floats;
    bool armed;
};
int gp_raster_backward_prepare(const gp_raster_settings* st, const gp_raster_inputs* in, const gp_raster_saved* saved, gp_alloc_fn alloc,
                               void* alloc_ctx, GpLossPrologue* pro);
int gp_loss_l1_ssim_fused_impl(const float* img, const float* gt, int32_t channels, int32_t H, int32_t W, float lambda_dssim,
                               const float* upstream, double* sums, float* dimg, const float* x, int64_t n, float scale, float* gx,
                               gp_stream_t stream, const GpLossPrologue* pro);       // (pro may be NULL)
int gp_raster_backward_impl(const gp_raster_settings* st, const gp_raster_inputs* in, const gp_raster_outputs* fwd,
                            const gp_raster_saved* saved, const float* dL_dcolor, const float* dL_ddepth, gp_raster_grads* g,
                            gp_alloc_fn alloc, void* alloc_ctx, gp_stream_t stream, float* prepared_acc);    // (NULL: obtains its own)
