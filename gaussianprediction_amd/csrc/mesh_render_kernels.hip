// mesh_render_kernels.hip -- a triangle rasterizer with a 64-bit visibility buffer on the device (csrc/gp_mesh_render.h).  The programs
// of a lane are csrc/mesh_render_core.h, which also runs on a CPU (tests/mesh_render_emulate.cpp).
//   mr_vertex_kernel      a lane per vertex: its 16-byte record (snapped position, 1 / P_z, flags), once per view
//   mr_face_kernel        a lane per face, by grid stride over at most MR_FACE_BLOCKS workgroups: its class; the counts tallied by wave
//                         ballots and added once per workgroup and word (integer atomicAdd); a drawn face whose box holds at most
//                         GP_MESH_RENDER_NARROW_MAX pixels is drawn by its lane, the others enter the list of wide faces (a wave
//                         ballot, one atomicAdd per wave that has one)
//   mr_wide_kernel        a launch of fixed size: GP_MESH_RENDER_SPLIT waves per entry of the list, by grid stride, each spreading
//                         8 x 8 blocks of the box over its 64 lanes: a triangle that fills the screen is nobody's serial loop
//   mr_resolve_kernel, mr_interpolate_kernel, mr_normals_kernel, mr_shade_kernel      a lane per pixel
// Visibility is one 64-bit unsigned atomic minimum per counting sample (global_atomic_umin_x2), after a plain load that leaves it out
// where the key is not smaller.  No float atomics, no spinning, no fence: the list crosses a launch boundary, and nothing is read by
// the host between the launches.
#include "gp_common.h"

#include "mesh_render_core.h"

static_assert(MR_BLOCK == 4 * GP_WAVE, "four waves a workgroup");

struct MrBackground { float v[GP_MESH_RENDER_MAX_CHANNELS]; };

__global__ void __launch_bounds__(MR_BLOCK) mr_vertex_kernel(const float* __restrict__ vertices, uint32_t nv, const float* __restrict__ world_view, MrView view,
                                                             MrVertex* __restrict__ records) {
    const uint32_t v = blockIdx.x * MR_BLOCK + threadIdx.x;
    if (v >= nv) return;
    records[v] = mr_vertex(world_view, vertices + 3 * (size_t)v, view);
}

__global__ void __launch_bounds__(MR_BLOCK) mr_face_kernel(const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf, const MrVertex* __restrict__ records, MrView view,
                                                           unsigned long long* vis, int32_t* coverage, int32_t* words, uint32_t* __restrict__ wide_list,
                                                           int32_t* counts) {
    __shared__ int32_t s_tally[MR_BLOCK / GP_WAVE][MR_CLASSES];
    int32_t tally[MR_CLASSES] = {0, 0, 0, 0, 0, 0};  // of this wave (the same in its 64 lanes)
    const uint32_t stride = gridDim.x * MR_BLOCK;    // (at most MR_FACE_BLOCKS * MR_BLOCK; nf is below 2^31 / 3: no wrap)
    for (uint32_t first = blockIdx.x * MR_BLOCK; first < nf; first += stride) {          // (the same trips for a whole workgroup)
        const uint32_t f = first + threadIdx.x;
        MrFace t;
        int what = -1;
        int64_t pixels = 0;
        if (f < nf) {
            what = mr_classify(faces, f, nv, records, view, t);
            if (what == MR_DRAW) pixels = mr_box_pixels(t);
        }
#pragma unroll
        for (int c = 0; c < MR_CLASSES; ++c) tally[c] += (int32_t)__popcll(__ballot(what == c));
        const bool wide = pixels > GP_MESH_RENDER_NARROW_MAX;
        const unsigned long long b = __ballot(wide);
        if (b != 0ull) {                             // (wave-uniform)
            const int leader = __ffsll((long long)b) - 1;
            int32_t base = 0;
            if ((int)(threadIdx.x & 63) == leader) {
                base = atomicAdd(words + MR_WORD_WIDE, (int32_t)__popcll(b));
                atomicAdd(counts + GP_MESH_RENDER_WIDE, (int32_t)__popcll(b));
            }
            base = __shfl(base, leader);
            if (wide) wide_list[(uint32_t)base + gp_mbcnt(b)] = f;      // (every face enters once: below nf)
        }
        if (pixels > 0 && !wide) mr_draw_narrow(t, f, view.W, vis, coverage);
    }
    // one atomic add per workgroup and word: tens of thousands of waves adding to one word take longer than the drawing
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < MR_CLASSES; ++c) s_tally[threadIdx.x >> 6][c] = tally[c];
    __syncthreads();
    if (threadIdx.x < MR_CLASSES) {
        int32_t sum = 0;
        for (int w = 0; w < MR_BLOCK / GP_WAVE; ++w) sum += s_tally[w][threadIdx.x];
        if (sum != 0) atomicAdd(counts + mr_count_word((int)threadIdx.x), sum);
    }
}

__global__ void __launch_bounds__(MR_BLOCK) mr_wide_kernel(const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf, const MrVertex* __restrict__ records, MrView view,
                                                           unsigned long long* vis, int32_t* coverage, const int32_t* __restrict__ words,
                                                           const uint32_t* __restrict__ wide_list) {
    const uint32_t listed = (uint32_t)words[MR_WORD_WIDE];
    const uint64_t entries = (uint64_t)(listed < nf ? listed : nf) * GP_MESH_RENDER_SPLIT;
    const uint64_t waves = (uint64_t)gridDim.x * (MR_BLOCK / GP_WAVE);
    const int lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * (MR_BLOCK / GP_WAVE) + (threadIdx.x >> 6); i < entries; i += waves) {
        const uint32_t f = wide_list[i / GP_MESH_RENDER_SPLIT];
        MrFace t;
        if (f >= nf || mr_classify(faces, f, nv, records, view, t) != MR_DRAW) continue;          // (cannot be: the list holds drawn faces)
        mr_draw_wide_lane(t, f, (int)(i % GP_MESH_RENDER_SPLIT), lane, view.W, vis, coverage);
    }
}

__global__ void __launch_bounds__(MR_BLOCK) mr_resolve_kernel(const unsigned long long* __restrict__ vis, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                              const MrVertex* __restrict__ records, MrView view, int32_t* __restrict__ face, float* __restrict__ depth,
                                                              uint8_t* __restrict__ valid, float* __restrict__ bary) {
    const uint32_t p = blockIdx.x * MR_BLOCK + threadIdx.x;
    if (p >= (uint32_t)view.H * (uint32_t)view.W) return;
    mr_resolve_pixel(vis, faces, nv, nf, records, view, (int32_t)(p % (uint32_t)view.W), (int32_t)(p / (uint32_t)view.W), face, depth, valid, bary);
}

__global__ void __launch_bounds__(MR_BLOCK) mr_interpolate_kernel(const float* __restrict__ attributes, int32_t C, const int32_t* __restrict__ faces, uint32_t nv,
                                                                  uint32_t nf, const MrVertex* __restrict__ records, const int32_t* __restrict__ face,
                                                                  const uint8_t* __restrict__ valid, const float* __restrict__ bary, MrBackground background,
                                                                  uint32_t plane, float* __restrict__ out) {
    const uint32_t p = blockIdx.x * MR_BLOCK + threadIdx.x;
    if (p >= plane) return;
    mr_interpolate_pixel(attributes, C, faces, nv, nf, records, face, valid, bary, background.v, p, plane, out);
}

__global__ void __launch_bounds__(MR_BLOCK) mr_normals_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t nv, uint32_t nf,
                                                              const float* __restrict__ world_view, MrView view, const int32_t* __restrict__ face,
                                                              const float* __restrict__ depth, const uint8_t* __restrict__ valid, float* __restrict__ normals,
                                                              uint8_t* __restrict__ nvalid) {
    const uint32_t p = blockIdx.x * MR_BLOCK + threadIdx.x, plane = (uint32_t)view.H * (uint32_t)view.W;
    if (p >= plane) return;
    float n[3];
    nvalid[p] = mr_normal_pixel(vertices, faces, nv, nf, world_view, view, face, depth, valid, (int32_t)(p % (uint32_t)view.W), (int32_t)(p / (uint32_t)view.W), n);
    normals[p] = n[0]; normals[(size_t)plane + p] = n[1]; normals[2 * (size_t)plane + p] = n[2];
}

__global__ void __launch_bounds__(MR_BLOCK) mr_shade_kernel(const float* __restrict__ color, const float* __restrict__ normals, const uint8_t* __restrict__ nvalid,
                                                            const float* __restrict__ depth, MrView view, float ambient, float bg0, float bg1, float bg2,
                                                            float* __restrict__ out) {
    const uint32_t p = blockIdx.x * MR_BLOCK + threadIdx.x;
    if (p >= (uint32_t)view.H * (uint32_t)view.W) return;
    const float bg[3] = {bg0, bg1, bg2};
    mr_shade_pixel(color, normals, nvalid, depth, view, ambient, bg, (int32_t)(p % (uint32_t)view.W), (int32_t)(p / (uint32_t)view.W), out);
}

// ---- the C entries ----
#define MR_REFUSE_SIZES(name)                                                                                                             \
    do {                                                                                                                                  \
        const char* why_ = mr_refuse_sizes(nv, nf, H, W);                                                                                 \
        if (why_) GP_FAIL(name ": %s (nv = %lld, nf = %lld, H = %d, W = %d)", why_, (long long)nv, (long long)nf, (int)H, (int)W);      \
    } while (0)

#define MR_REFUSE_SCRATCH(name)                                                                     \
    do {                                                                                            \
        if (!scratch) GP_FAIL(name ": null argument (scratch)");                                    \
        if (((uintptr_t)scratch & 15u) != 0) GP_FAIL(name ": scratch must be 16-byte aligned");     \
    } while (0)

static MrView mr_view(float tanfovx, float tanfovy, float z_near, int32_t H, int32_t W, int32_t cull) {
    MrView v;
    v.tanfovx = tanfovx; v.tanfovy = tanfovy; v.z_near = z_near; v.W = W; v.H = H; v.cull = cull;
    return v;
}

extern "C" int gp_mesh_render_abi_version(void) { return GP_MESH_RENDER_ABI_VERSION; }

extern "C" int64_t gp_mesh_render_scratch_bytes(int64_t nv, int64_t nf, int32_t H, int32_t W) {
    const char* why = mr_refuse_sizes(nv, nf, H, W);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_mesh_render_scratch_bytes: %s (nv = %lld, nf = %lld, H = %d, W = %d)", why, (long long)nv, (long long)nf, H, W);
        return -1;
    }
    return mr_scratch_layout(nv, nf, H, W).bytes;
}

extern "C" int gp_mesh_render_rasterize(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const float* world_view, float tanfovx, float tanfovy,
                                        int32_t H, int32_t W, float z_near, int32_t cull, void* scratch, int32_t* coverage, int32_t* counts, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MR_REFUSE_SIZES("gp_mesh_render_rasterize");
    MR_REFUSE_SCRATCH("gp_mesh_render_rasterize");
    if (!counts || !world_view || (nv > 0 && !vertices) || (nf > 0 && !faces)) GP_FAIL("gp_mesh_render_rasterize: null argument");
    const char* why = mr_refuse_raster(tanfovx, tanfovy, z_near, cull);
    if (why) GP_FAIL("gp_mesh_render_rasterize: %s (tanfovx = %g, tanfovy = %g, z_near = %g, cull = %d)", why, tanfovx, tanfovy, z_near, cull);
    const MrScratch s = mr_scratch_layout(nv, nf, H, W);
    char* base = (char*)scratch;
    int32_t* words = (int32_t*)(base + s.words);
    MrVertex* records = (MrVertex*)(base + s.records);
    unsigned long long* vis = (unsigned long long*)(base + s.vis);
    uint32_t* wide_list = (uint32_t*)(base + s.wide);
    const MrView view = mr_view(tanfovx, tanfovy, z_near, H, W, cull);
    const uint32_t NV = (uint32_t)nv, NF = (uint32_t)nf;
    const size_t plane = (size_t)H * W;
    GpProfScope _p("mesh_render_rasterize", st);
    GP_HIP_CHECK(hipMemsetAsync(counts, 0, GP_MESH_RENDER_COUNT_WORDS * sizeof(int32_t), st));
    GP_HIP_CHECK(hipMemsetAsync(words, 0, 8 * sizeof(int32_t), st));
    GP_HIP_CHECK(hipMemsetAsync(vis, 0xFF, 8 * plane, st));
    if (coverage) GP_HIP_CHECK(hipMemsetAsync(coverage, 0, 4 * plane, st));
    if (NV > 0) {
        hipLaunchKernelGGL(mr_vertex_kernel, dim3(gp_blocks(NV, MR_BLOCK)), dim3(MR_BLOCK), 0, st, vertices, NV, world_view, view, records);
        GP_LAUNCH_CHECK();
    }
    if (NF > 0) {
        const unsigned face_blocks = gp_blocks(NF, MR_BLOCK);
        hipLaunchKernelGGL(mr_face_kernel, dim3(face_blocks < MR_FACE_BLOCKS ? face_blocks : MR_FACE_BLOCKS), dim3(MR_BLOCK), 0, st, faces, NV, NF,
                           (const MrVertex*)records, view, vis, coverage, words, wide_list, counts);
        GP_LAUNCH_CHECK();
        const unsigned blocks = gp_blocks((size_t)NF * GP_MESH_RENDER_SPLIT, MR_BLOCK / GP_WAVE);
        hipLaunchKernelGGL(mr_wide_kernel, dim3(blocks < MR_WIDE_BLOCKS ? blocks : MR_WIDE_BLOCKS), dim3(MR_BLOCK), 0, st, faces, NV, NF, (const MrVertex*)records, view,
                           vis, coverage, (const int32_t*)words, (const uint32_t*)wide_list);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gp_mesh_render_resolve(const int32_t* faces, int64_t nv, int64_t nf, int32_t H, int32_t W, const void* scratch, int32_t* face, float* depth,
                                      uint8_t* valid, float* bary, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MR_REFUSE_SIZES("gp_mesh_render_resolve");
    MR_REFUSE_SCRATCH("gp_mesh_render_resolve");
    if (!face || !depth || !valid || !bary || (nf > 0 && !faces)) GP_FAIL("gp_mesh_render_resolve: null argument");
    const MrScratch s = mr_scratch_layout(nv, nf, H, W);
    const char* base = (const char*)scratch;
    const size_t plane = (size_t)H * W;
    GpProfScope _p("mesh_render_resolve", st);
    hipLaunchKernelGGL(mr_resolve_kernel, dim3(gp_blocks(plane, MR_BLOCK)), dim3(MR_BLOCK), 0, st, (const unsigned long long*)(base + s.vis), faces, (uint32_t)nv,
                       (uint32_t)nf, (const MrVertex*)(base + s.records), mr_view(1.f, 1.f, 1.f, H, W, GP_MESH_RENDER_CULL_NONE), face, depth, valid, bary);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_mesh_render_interpolate(const float* attributes, int32_t C, const int32_t* faces, int64_t nv, int64_t nf, int32_t H, int32_t W, const void* scratch,
                                          const int32_t* face, const uint8_t* valid, const float* bary, const float* background, float* out, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MR_REFUSE_SIZES("gp_mesh_render_interpolate");
    MR_REFUSE_SCRATCH("gp_mesh_render_interpolate");
    if (C < 1 || C > GP_MESH_RENDER_MAX_CHANNELS) GP_FAIL("gp_mesh_render_interpolate: C must be 1 .. %d (C = %d)", GP_MESH_RENDER_MAX_CHANNELS, C);
    if (!face || !valid || !bary || !background || !out || (nv > 0 && !attributes) || (nf > 0 && !faces)) GP_FAIL("gp_mesh_render_interpolate: null argument");
    const MrScratch s = mr_scratch_layout(nv, nf, H, W);
    const char* base = (const char*)scratch;
    const size_t plane = (size_t)H * W;
    MrBackground bg;
    for (int c = 0; c < GP_MESH_RENDER_MAX_CHANNELS; ++c) bg.v[c] = c < C ? background[c] : 0.f;
    GpProfScope _p("mesh_render_interpolate", st);
    hipLaunchKernelGGL(mr_interpolate_kernel, dim3(gp_blocks(plane, MR_BLOCK)), dim3(MR_BLOCK), 0, st, attributes, C, faces, (uint32_t)nv, (uint32_t)nf,
                       (const MrVertex*)(base + s.records), face, valid, bary, bg, (uint32_t)plane, out);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_mesh_render_normals(const float* vertices, const int32_t* faces, int64_t nv, int64_t nf, const float* world_view, float tanfovx, float tanfovy,
                                      int32_t H, int32_t W, const int32_t* face, const float* depth, const uint8_t* valid, float* normals, uint8_t* nvalid,
                                      gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    MR_REFUSE_SIZES("gp_mesh_render_normals");
    if (!world_view || !face || !depth || !valid || !normals || !nvalid || (nv > 0 && !vertices) || (nf > 0 && !faces)) GP_FAIL("gp_mesh_render_normals: null argument");
    const char* why = mr_refuse_view(tanfovx, tanfovy);
    if (why) GP_FAIL("gp_mesh_render_normals: %s (tanfovx = %g, tanfovy = %g)", why, tanfovx, tanfovy);
    const size_t plane = (size_t)H * W;
    GpProfScope _p("mesh_render_normals", st);
    hipLaunchKernelGGL(mr_normals_kernel, dim3(gp_blocks(plane, MR_BLOCK)), dim3(MR_BLOCK), 0, st, vertices, faces, (uint32_t)nv, (uint32_t)nf, world_view,
                       mr_view(tanfovx, tanfovy, 1.f, H, W, GP_MESH_RENDER_CULL_NONE), face, depth, valid, normals, nvalid);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_mesh_render_shade(const float* color, const float* normals, const uint8_t* nvalid, const float* depth, float tanfovx, float tanfovy, int32_t H,
                                    int32_t W, float ambient, float bg_r, float bg_g, float bg_b, float* out, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const int64_t nv = 0, nf = 0;
    MR_REFUSE_SIZES("gp_mesh_render_shade");
    if (!color || !normals || !nvalid || !depth || !out) GP_FAIL("gp_mesh_render_shade: null argument");
    const char* why = mr_refuse_view(tanfovx, tanfovy);
    if (why) GP_FAIL("gp_mesh_render_shade: %s (tanfovx = %g, tanfovy = %g)", why, tanfovx, tanfovy);
    if (!dp_finite(ambient)) GP_FAIL("gp_mesh_render_shade: ambient must be finite (ambient = %g)", ambient);
    const size_t plane = (size_t)H * W;
    GpProfScope _p("mesh_render_shade", st);
    hipLaunchKernelGGL(mr_shade_kernel, dim3(gp_blocks(plane, MR_BLOCK)), dim3(MR_BLOCK), 0, st, color, normals, nvalid, depth,
                       mr_view(tanfovx, tanfovy, 1.f, H, W, GP_MESH_RENDER_CULL_NONE), ambient, bg_r, bg_g, bg_b, out);
    GP_LAUNCH_CHECK();
    return 0;
}
