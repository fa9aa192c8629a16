// trajectory_kernels.hip -- motion trajectories drawn on the device (csrc/gp_trajectory.h).  The arithmetic is csrc/trajectory_core.h,
// which also runs on a CPU (tests/trajectory_emulate.cpp).
//   tj_step_kernel      one lane per point j of one step: idx[j], the previous pixel px[j] and the new one move coalesced over j, the
//                       point's row of xyz is one gather; the lane projects, walks the in-image part of its segment (at most
//                       max(W, H) iterations, one 64-bit division) and claims each pixel with a 32-bit atomic maximum of the key
//                       s*P + j + 1 -- no return value is used, so nothing waits for the atomics
//   tj_resolve_kernel   one lane per pixel: the owner's colour, the base's pixel or zero, three coalesced stores
// Nothing of size S*P exists: a step reads the pixels of the one before and replaces them.  The keys make the result independent of the
// schedule.  Every store is an ordinary vector store.
#include "gp_common.h"

#include "trajectory_core.h"

#define TJ_BLOCK 256

struct TjClaim {
    uint32_t* owner;
    uint32_t key;
    __device__ __forceinline__ void operator()(int64_t offset) const {
        (void)__hip_atomic_fetch_max(owner + offset, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__global__ void __launch_bounds__(TJ_BLOCK) tj_step_kernel(gp_traj_view c, const float* __restrict__ xyz, const int32_t* __restrict__ idx, uint32_t N,
                                                           uint32_t P, uint32_t key_base, int first, int2* __restrict__ px,
                                                           uint32_t* __restrict__ owner, int32_t H, int32_t W, float min_depth) {
    const uint32_t j = blockIdx.x * TJ_BLOCK + threadIdx.x;
    if (j >= P) return;
    const uint32_t row = idx ? (uint32_t)idx[j] : j;          // (a negative index is a large one)
    TjPixel prev;
    prev.x = prev.y = TJ_NONE;
    if (!first) {
        const int2 p = px[j];
        prev.x = p.x;
        prev.y = p.y;
    }
    TjClaim claim;
    claim.owner = owner;
    claim.key = key_base + j + 1u;
    const TjPixel now = tj_point_step(c, row < N ? xyz + (size_t)row * 3 : nullptr, min_depth, first != 0, prev, W, H, claim);
    px[j] = make_int2(now.x, now.y);
}

__global__ void __launch_bounds__(TJ_BLOCK) tj_resolve_kernel(const uint32_t* __restrict__ owner, const float* __restrict__ colors, int64_t P,
                                                              const float* __restrict__ base, float* __restrict__ out, uint32_t plane) {
    const uint32_t p = blockIdx.x * TJ_BLOCK + threadIdx.x;
    if (p >= plane) return;
    const uint32_t key = owner[p];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[(size_t)ch * plane + p] = tj_resolve_pixel(key, colors, P, base, p, plane, ch);
}

extern "C" int gp_traj_abi_version(void) { return GP_TRAJ_ABI_VERSION; }

extern "C" int gp_traj_step(const gp_traj_view* view, const float* xyz, const int32_t* idx, int64_t N, int64_t P, int64_t s, int32_t* px,
                            uint32_t* owner, int32_t H, int32_t W, float min_depth, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = tj_refusal(N, P, s, H, W, idx != nullptr);
    if (why) GP_FAIL("gp_traj_step: %s (N = %lld, P = %lld, s = %lld, H = %d, W = %d)", why, (long long)N, (long long)P, (long long)s, H, W);
    if (P == 0) return 0;
    if (!view || !xyz || !px || !owner) GP_FAIL("gp_traj_step: null argument");
    const uint32_t rows = N > 0xFFFFFFFFLL ? 0xFFFFFFFFu : (uint32_t)N;        // (an index is 32 bits wide: more rows cannot be named)
    GpProfScope _p("traj_step", st);
    hipLaunchKernelGGL(tj_step_kernel, dim3(gp_blocks((size_t)P, TJ_BLOCK)), dim3(TJ_BLOCK), 0, st, *view, xyz, idx, rows, (uint32_t)P,
                       (uint32_t)(s * P), s == 0 ? 1 : 0, (int2*)px, owner, H, W, min_depth);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_traj_resolve(const uint32_t* owner, const float* colors, int64_t P, const float* base, float* out, int32_t H, int32_t W,
                               gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = tj_refusal(P, P, 0, H, W, false);        // (the checks of P, H and W; N and idx are not this entry's)
    if (why) GP_FAIL("gp_traj_resolve: %s (P = %lld, H = %d, W = %d)", why, (long long)P, H, W);
    if (!owner || !out || (P > 0 && !colors)) GP_FAIL("gp_traj_resolve: null argument");
    const uint32_t plane = (uint32_t)((int64_t)H * W);
    GpProfScope _p("traj_resolve", st);
    hipLaunchKernelGGL(tj_resolve_kernel, dim3(gp_blocks(plane, TJ_BLOCK)), dim3(TJ_BLOCK), 0, st, owner, colors, P, base, out, plane);
    GP_LAUNCH_CHECK();
    return 0;
}
