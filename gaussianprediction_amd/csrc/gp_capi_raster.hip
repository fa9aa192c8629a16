// gp_capi_raster.hip -- extern "C" entry points of the rasterizer (see include/gp_hip.h).
// Host orchestration only: sizes buffers, asks the caller's allocator for scratch, enqueues the
// kernels of raster_kernels.hip / sort_scan.hip on the caller's stream.
#include "gp_common.h"
#include "raster_kernels.h"
#include "loss_adam_kernels.h"     // GpLossPrologue
#include <stdlib.h>
#include <atomic>
#include <vector>

thread_local char gp_err_buf[512] = "";
static std::atomic<uint32_t> g_key_tag{0};       // numbers the forward calls that check a depth-key promise (never 0)

extern "C" const char* gp_last_error(void) { return gp_err_buf; }
extern "C" const char* gp_version(void) { return "gaussianprediction_amd 0.4 (gfx950)"; }
extern "C" int gp_abi_version(void) { return GP_ABI_VERSION; }

static int tile_bits_for(int T) {
    int b = 1;
    while ((1 << b) < T) ++b;
    return b;
}

static int make_dims(const gp_raster_settings* st, const gp_raster_inputs* in, RasterDims& d) {
    if (!st || !in) GP_FAIL("null settings/inputs");
    if (st->image_width <= 0 || st->image_height <= 0) GP_FAIL("bad image size %dx%d", st->image_width, st->image_height);
    if (in->num_gaussians < 0 || in->num_gaussians > 0x7FFFFFF0LL) GP_FAIL("num_gaussians out of range");
    if (st->sh_degree < 0 || st->sh_degree > 3) GP_FAIL("sh_degree %d unsupported (0..3)", st->sh_degree);
    const bool has_sr = in->scales != nullptr || in->rotations != nullptr;
    if (in->num_gaussians > 0) {  // (an empty tensor has a NULL data pointer: nothing to check then)
        if ((in->shs == nullptr) == (in->colors_precomp == nullptr)) GP_FAIL("Please provide exactly one of either SHs or precomputed colors!");
        if (has_sr == (in->cov3D_precomp != nullptr) || (has_sr && (!in->scales || !in->rotations)))
            GP_FAIL("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    }
    if (in->shs && st->sh_coeffs < (st->sh_degree + 1) * (st->sh_degree + 1)) GP_FAIL("shs has %d coeffs, degree %d needs more", st->sh_coeffs, st->sh_degree);
    if (in->shs && st->sh_coeffs > 16) GP_FAIL("sh_coeffs %d > 16 unsupported", st->sh_coeffs);
    if (in->shs_rest && (!in->shs || st->sh_coeffs != 16)) GP_FAIL("shs_rest needs shs (= features_dc) and sh_coeffs == 16");
    if (!st->bg || !st->viewmatrix || !st->projmatrix || !st->campos) GP_FAIL("null camera pointers");
    if (in->num_gaussians > 0 && (!in->means3D || !in->opacities)) GP_FAIL("null means3D/opacities");
    d.N = (int)in->num_gaussians;
    d.M = in->shs ? st->sh_coeffs : 0;
    d.D = st->sh_degree;
    d.W = st->image_width;
    d.H = st->image_height;
    d.gx = (d.W + GP_TILE - 1) / GP_TILE;
    d.gy = (d.H + GP_TILE - 1) / GP_TILE;
    d.tanfovx = st->tanfovx;
    d.tanfovy = st->tanfovy;
    d.fx = (float)d.W / (2.f * st->tanfovx);
    d.fy = (float)d.H / (2.f * st->tanfovy);
    d.scale_mod = st->scale_modifier;
    d.late_color = (st->sh_ready_event && in->shs) ? 1 : 0;
    d.visible = nullptr; d.zero_words = nullptr; d.n_zero = 0;
    d.key_hi = 0u; d.key_base = 0u; d.key_culled = 0xFFFFFFFFu; d.key_flag = nullptr; d.key_tag = 0u;
    d.sb_side = nullptr;
    d.raw_opacity = nullptr;
    if (st->raw_activations) {
        if (in->cov3D_precomp || !in->scales) GP_FAIL("raw_activations needs scales + rotations (not cov3D_precomp)");
        d.raw_opacity = in->opacities;
    }
    if (st->depth_key_bits != 0 && st->depth_key_bits != 32) {
        if (st->depth_key_bits < 8 || st->depth_key_bits > 31) GP_FAIL("depth_key_bits must be 0, 32 or 8 .. 31 (got %d)", st->depth_key_bits);
        if (!st->binning_status) GP_FAIL("depth_key_bits needs binning_status (the word a broken promise raises)");
        const uint32_t low = (1u << st->depth_key_bits) - 1u;
        d.key_hi = ~low;
        d.key_base = st->depth_key_base;
        d.key_culled = low;                         // behind (or level with) every visible key of the promised range
        d.key_flag = st->binning_status + 2;        // (the status block's scratch word: 3 words are required then)
        do { d.key_tag = ++g_key_tag; } while (d.key_tag == 0u);
    }
    return 0;
}

// saved-state layouts (recomputed identically in forward and backward)
struct GeomLayout {
    float4* rec;
    uint8_t* clamped;
    float2* sb_side;        // (RasterDims.sb_side)
    size_t bytes;
    GeomLayout(void* base, size_t N) {
        GpCarver c(base);
        rec = c.take<float4>(3 * N + 1);
        clamped = c.take<uint8_t>(N + 1);
        sb_side = c.take<float2>(GP_SB_HOIST == 1 ? N + 1 : 0);
        bytes = c.bytes();
    }
};
struct ImageLayout {
    int2* ranges;
    float* final_T;
    int32_t* n_contrib;
    int32_t* tile_work;    // per tile: largest list position consumed by the forward (backward work estimate)
    uint32_t* order;       // heavy-first launch order of the forward
    size_t bytes;
    uint32_t* total;       // R, written by the scan of the per-Gaussian tile counts (zeroed with `ranges`: it sits behind them)
    ImageLayout(void* base, size_t T, size_t P) {
        GpCarver c(base);
        ranges = c.take<int2>(T + GP_TOTAL_SLOTS / 2);
        total = (uint32_t*)(ranges + T);
        final_T = c.take<float>(P);
        n_contrib = c.take<int32_t>(P);
        tile_work = c.take<int32_t>(T);
        order = c.take<uint32_t>(T);
        bytes = c.bytes();
    }
};

// The binning stage of the forward: from the depth-ordered Gaussians (ids, tile rectangles, tile counts) to the per-tile lists and
// their ranges.  One statement of the sequence for gp_raster_forward and for gp_debug_bin_lists (the tests run what ships).
struct GpBinStage {
    RasterDims d;                   // N, gx and key_tag are read
    size_t T;
    const uint32_t* sorted_ids;     // [N] Gaussian ids in depth order
    const uint2* rects;             // [N] tile rectangles in depth order
    uint32_t* tt;                   // [N] tiles per Gaussian in depth order (duplicate path: scanned in place)
    uint32_t* block_sums;           // one word per GP_SCAN_TILE Gaussians (duplicate path)
    bool counting;                  // gp_bin_supported(N, T): binning by counting, else duplicate + radix sort
    GpBinPlan bp;
    uint32_t* binhist;              // bp.hist_elems words (counting path)
    int64_t capacity;               // gp_raster_settings.binning_capacity
    uint32_t* status;               // gp_raster_settings.binning_status
    int2* ranges;                   // [T], zero on entry
    uint32_t* total;                // GP_TOTAL_SLOTS words, zero on entry
    uint32_t* order;                // [T] the composite forward's tile order (written by the counting path: order_done)
};
// R: the instances binned (capacity mode: the capacity).  BINNING is asked from `alloc` (point_list[R], then room for the composite
// forward's sub-block masks: this stage writes the first R words only) and handed back in bin / bin_bytes.
static int gp_binning_stage(const GpBinStage& b, gp_alloc_fn alloc, void* alloc_ctx, hipStream_t s, uint32_t& R, uint32_t*& point_list,
                            void*& bin_out, size_t& bin_bytes_out, bool& order_done) {
    const RasterDims& d = b.d;
    const size_t N = (size_t)d.N, T = b.T;
    const uint32_t* sorted_ids = b.sorted_ids;
    const uint2* rects = b.rects;
    uint32_t* tt = b.tt;
    const bool counting = b.counting;
    const GpBinPlan& bp = b.bp;
    uint32_t* binhist = b.binhist;
    // tile counts -> instance offsets: scanned inside blocks here, finished by the duplicate kernel (one launch, not three)
    uint32_t* block_sums = b.block_sums;
    if (counting) {         // per-(block, tile) instance counts; the blocks' totals go into the R slots
        GpProfScope _p("bin_count", s);
        if (gp_bin_count(bp, N, d.gx, T, rects, binhist, b.total, s)) return 1;
    } else if (gp_scan_blocks_u32(tt, N, block_sums, b.total, s)) return 1;
    const bool capacity_mode = b.capacity > 0;
    if (capacity_mode) {    // no host synchronisation: everything below is sized by the caller's capacity
        if (!b.status) GP_FAIL("binning_capacity needs binning_status (device, 2 words)");
        if (b.capacity > 0x7FFFFF00ll) GP_FAIL("binning_capacity too large");
        R = (uint32_t)b.capacity;          // (the status word and the sentinel keys are written by the duplicate launch)
    } else {
        uint32_t slots[GP_TOTAL_SLOTS];
        GP_HIP_CHECK(hipMemcpyAsync(slots, b.total, sizeof(slots), hipMemcpyDeviceToHost, s));
        GP_HIP_CHECK(hipStreamSynchronize(s));
        uint64_t Rsum = 0;
        for (int k = 0; k < GP_TOTAL_SLOTS; ++k) Rsum += slots[k];
        if (Rsum > 0x7FFFFF00ull) GP_FAIL("too many tile-splat instances (%llu)", (unsigned long long)Rsum);
        R = (uint32_t)Rsum;
        if (R > 0x7FFFFF00u) GP_FAIL("too many tile-splat instances (%u)", R);
        if (b.status && (!counting || R == 0)) {   // exact mode reports R too (a caller sizing its capacity reads it from here; the counting path's scatter writes it)
            hipLaunchKernelGGL(gp_binning_status_kernel, dim3(1), dim3(1), 0, s, b.total, 0xFFFFFFFFu, b.status, d.key_tag);
            GP_LAUNCH_CHECK();
        }
    }

    if (R > 0 && counting) {
        const size_t bin_bytes = gp_align_up((size_t)R * 4, 256) + gp_align_up(2 * (size_t)R + 8, 256);
        void* bin = alloc(alloc_ctx, GP_BUF_BINNING, bin_bytes);
        if (!bin) GP_FAIL("allocator returned NULL for BINNING");
        point_list = (uint32_t*)bin;
        bin_out = bin; bin_bytes_out = bin_bytes;
        if (gp_bin_scatter(bp, N, d.gx, T, sorted_ids, rects, binhist, point_list, R, b.ranges, b.status, b.order, d.key_tag, s)) return 1;
        order_done = true;
    } else if (R > 0) {
        // capacity mode pads the keys with 0xFFFFFFFF: its low `tbits` bits must sort behind every real tile id
        const int tbits = tile_bits_for((int)T + (capacity_mode ? 1 : 0));
        const int passes = (tbits + 7) / 8;
        const int res = passes & 1;  // buffer pair holding the sorted result
        // BINNING = point_list[R] (u32) followed by smask[R] (u16: which 4x4 sub-blocks of its tile an instance can touch)
        const size_t bin_bytes = gp_align_up((size_t)R * 4, 256) + gp_align_up(2 * (size_t)R + 8, 256);
        void* bin = alloc(alloc_ctx, GP_BUF_BINNING, bin_bytes);
        if (!bin) GP_FAIL("allocator returned NULL for BINNING");
        point_list = (uint32_t*)bin;
        bin_out = bin; bin_bytes_out = bin_bytes;
        const size_t bh = gp_sort_hist_elems(R), bs = gp_scan_tmp_elems(256 * (((size_t)R + 4095) / 4096));
        auto carve_bin = [&](GpCarver& c, uint32_t*& bk0, uint32_t*& bk1, uint32_t*& bvo, uint32_t*& bhist, uint32_t*& bscan) {
            bk0 = c.take<uint32_t>(R); bk1 = c.take<uint32_t>(R); bvo = c.take<uint32_t>(R);
            bhist = c.take<uint32_t>(bh); bscan = c.take<uint32_t>(bs);
        };
        uint32_t *bk0, *bk1, *bvo, *bhist, *bscan;
        GpCarver bc0(nullptr);
        carve_bin(bc0, bk0, bk1, bvo, bhist, bscan);
        void* btmp = alloc(alloc_ctx, GP_BUF_TEMP, bc0.bytes());
        if (!btmp) GP_FAIL("allocator returned NULL for TEMP (%zu B)", bc0.bytes());
        GpCarver bc(btmp);
        carve_bin(bc, bk0, bk1, bvo, bhist, bscan);
        GpSortBufs tb;
        tb.k[0] = bk0; tb.k[1] = bk1;
        tb.v[res] = point_list; tb.v[res ^ 1] = bvo;
        tb.hist = bhist; tb.scan_tmp = bscan; tb.scan_tmp_elems = bs;
        { GpProfScope _p("duplicate", s);
        const unsigned ndup = gp_blocks(N, 256);
        hipLaunchKernelGGL(gp_duplicate_kernel, dim3(ndup + (capacity_mode ? gp_blocks(R, 4096) : 0u)), dim3(256), 0, s, d, sorted_ids, tt,
                           (const uint32_t*)block_sums, (const uint32_t*)b.total, rects, tb.k[0], tb.v[0], R, b.status, ndup, d.key_tag);
        GP_LAUNCH_CHECK(); }
        int r2;
        { GpProfScope _p("tile_sort", s); r2 = gp_radix_sort_pairs(tb, R, tbits, s); }
        if (r2 < 0) return 1;
        if (r2 != res) GP_FAIL("internal: sort parity mismatch");
        { GpProfScope _p("tile_ranges", s);
        hipLaunchKernelGGL(gp_tile_ranges_kernel, dim3(gp_blocks(R, 256)), dim3(256), 0, s, tb.k[r2], R, (uint32_t)T, b.ranges);
        GP_LAUNCH_CHECK(); }
    }
    return 0;
}

extern "C" int gp_raster_forward(const gp_raster_settings* st, const gp_raster_inputs* in, gp_raster_outputs* out,
                                 gp_raster_saved* saved, gp_alloc_fn alloc, void* alloc_ctx, gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    RasterDims d;
    if (make_dims(st, in, d)) return 1;
    if (!out || !out->color || !out->depth || !out->tidx || (d.N > 0 && !out->radii)) GP_FAIL("null output pointers");
    if (!saved || !alloc) GP_FAIL("null saved/alloc");
    const size_t N = (size_t)d.N, T = (size_t)d.gx * d.gy, P = (size_t)d.W * d.H;

    ImageLayout il0(nullptr, T, P);
    void* img = alloc(alloc_ctx, GP_BUF_IMAGE, il0.bytes);
    if (!img) GP_FAIL("allocator returned NULL for IMAGE (%zu B)", il0.bytes);
    ImageLayout il(img, T, P);
    GeomLayout gl0(nullptr, N);
    void* geom = alloc(alloc_ctx, GP_BUF_GEOM, gl0.bytes);
    if (!geom) GP_FAIL("allocator returned NULL for GEOM (%zu B)", gl0.bytes);
    GeomLayout gl(geom, N);
    d.sb_side = gl.sb_side;
    saved->geom = geom; saved->geom_bytes = gl.bytes;
    saved->image = img; saved->image_bytes = il.bytes;
    saved->binning = nullptr; saved->binning_bytes = 0; saved->num_rendered = 0;

    {   // tile ranges + the instance counter's slots behind them start from zero: by the preprocess launch when it has enough
        // threads, else by a memset of its own
        const size_t words = (T + GP_TOTAL_SLOTS / 2) * 2;
        if ((size_t)N >= words) { d.zero_words = (uint32_t*)il.ranges; d.n_zero = (int)words; }
        else GP_HIP_CHECK(hipMemsetAsync(il.ranges, 0, words * sizeof(uint32_t), s));
    }
    d.visible = out->visible;
    uint32_t R = 0;
    uint32_t* point_list = nullptr;
    bool order_done = false;            // (the counting path's scatter launch also writes the forward's tile order)
    if (N > 0) {
        // ---- per-Gaussian temporaries -----------------------------------------------------------
        GpCarver tc0(nullptr);
        const size_t hist_elems = gp_sort_hist_elems(N);
        const size_t scan_elems = gp_scan_tmp_elems(256 * ((N + 4095) / 4096) > N + 1 ? 256 * ((N + 4095) / 4096) : N + 1) + (N + GP_SCAN_TILE - 1) / GP_SCAN_TILE + 64;
        // binning by counting (bin_kernels.hip) whenever the per-tile histogram fits a workgroup's LDS; else duplicate + radix sort
        const bool counting = gp_bin_supported(N, T);
        GpBinPlan bp = {0, 0, 0};
        if (counting) bp = gp_bin_plan(N, T);
        const bool dsort3 = gp_dsort_supported(N);          // depth sort in three 11-bit counting passes (else four 8-bit radix passes)
        auto carve_tmp = [&](GpCarver& c, uint32_t*& k0, uint32_t*& k1, uint32_t*& v0, uint32_t*& v1, uint2*& tiles,
                             uint2*& rects, uint32_t*& tt, uint32_t*& hist, uint32_t*& scan_tmp, uint32_t*& binhist, uint32_t*& dshist) {
            k0 = c.take<uint32_t>(N); k1 = c.take<uint32_t>(N); v0 = c.take<uint32_t>(N); v1 = c.take<uint32_t>(N);
            tiles = c.take<uint2>(N); rects = c.take<uint2>(N); tt = c.take<uint32_t>(N + 1);
            hist = c.take<uint32_t>(hist_elems); scan_tmp = c.take<uint32_t>(scan_elems);
            binhist = c.take<uint32_t>(bp.hist_elems);
            dshist = c.take<uint32_t>(dsort3 ? gp_dsort_hist_elems(N) : 0);
        };
        uint32_t *k0, *k1, *v0, *v1, *tt, *hist, *scan_tmp, *binhist, *dshist;
        uint2 *tiles, *rects;      // per-Gaussian tile rectangle by id, and the same in depth order
        carve_tmp(tc0, k0, k1, v0, v1, tiles, rects, tt, hist, scan_tmp, binhist, dshist);
        void* tmp = alloc(alloc_ctx, GP_BUF_TEMP, tc0.bytes());
        if (!tmp) GP_FAIL("allocator returned NULL for TEMP (%zu B)", tc0.bytes());
        GpCarver tc(tmp);
        carve_tmp(tc, k0, k1, v0, v1, tiles, rects, tt, hist, scan_tmp, binhist, dshist);

        {
            GpProfScope _p("preprocess_fwd", s);
            const bool al16 = (((uintptr_t)in->shs | (uintptr_t)in->shs_rest) & 15) == 0;
            auto kern = gp_preprocess_fwd_kernel;
            if (in->shs && in->shs_rest) {
                if (!al16) GP_FAIL("shs/shs_rest must be 16-byte aligned");
                kern = gp_preprocess_fwd_split_kernel;
            } else if (in->shs && d.M == 16 && al16) {
                kern = gp_preprocess_fwd_sh16_kernel;
            }
            hipLaunchKernelGGL(kern, dim3(gp_blocks(N, 256)), dim3(256), 0, s, d, in->means3D, in->scales, in->rotations,
                               in->opacities, in->shs, in->shs_rest, in->colors_precomp, in->cov3D_precomp, st->viewmatrix,
                               st->projmatrix, st->campos, out->radii, gl.rec, k0, tiles, gl.clamped);
            GP_LAUNCH_CHECK();
        }
        GpSortBufs sb;
        sb.k[0] = k0; sb.k[1] = k1; sb.v[0] = v0; sb.v[1] = v1; sb.hist = hist; sb.scan_tmp = scan_tmp; sb.scan_tmp_elems = scan_elems;
        int r1;
        // (values = 0 .. N-1, generated by the first pass)
        // the last pass also carries every Gaussian's tile rectangle + tile count into depth order (was a launch of its own)
        const GpSortEpilogue ep = {tiles, rects, tt};
        const int key_bits = d.key_hi ? st->depth_key_bits : 32;       // (a promised key range: fewer passes, same order)
        if (st->depth_key_range) {      // {min, max} key of the visible Gaussians, for a caller that sizes depth_key_bits from it
            GP_HIP_CHECK(hipMemsetAsync(st->depth_key_range, 0xFF, 4, s));
            GP_HIP_CHECK(hipMemsetAsync(st->depth_key_range + 1, 0, 4, s));
            hipLaunchKernelGGL(gp_key_range_kernel, dim3(gp_blocks(N, 1024)), dim3(256), 0, s, (const uint32_t*)k0, (const int32_t*)out->radii, (int)N,
                               d.key_base, st->depth_key_range);
            GP_LAUNCH_CHECK();
        }
        { GpProfScope _p("depth_sort", s); r1 = (dsort3 && key_bits == 32) ? gp_depth_sort3(sb, N, dshist, s, &ep) : gp_radix_sort_pairs(sb, N, key_bits, s, true, &ep); }
        if (r1 < 0) return 1;
        const uint32_t* sorted_ids = sb.v[r1];
        GpBinStage bs;
        bs.d = d; bs.T = T; bs.sorted_ids = sorted_ids; bs.rects = rects; bs.tt = tt; bs.block_sums = scan_tmp;
        bs.counting = counting; bs.bp = bp; bs.binhist = binhist;
        bs.capacity = st->binning_capacity; bs.status = st->binning_status;
        bs.ranges = il.ranges; bs.total = il.total; bs.order = il.order;
        if (gp_binning_stage(bs, alloc, alloc_ctx, s, R, point_list, saved->binning, saved->binning_bytes, order_done)) return 1;
    }
    if (N == 0 && st->binning_status)      // nothing to bin: {R, overflow} = {0, 0} (a stale overflow word would make Adam skip the step)
        GP_HIP_CHECK(hipMemsetAsync(st->binning_status, 0, 2 * sizeof(uint32_t), s));
    saved->num_rendered = (int64_t)R;
    if (!order_done) {
        hipLaunchKernelGGL(gp_tile_order_kernel, dim3(1), dim3(1024), 0, s, il.ranges, (const int32_t*)nullptr, (int)T, il.order);
        GP_LAUNCH_CHECK();
    }
    if (d.late_color && N > 0) {    // the SH coefficients may still be in flight (parameter all-gather): wait here, not at the top
        GP_HIP_CHECK(hipStreamWaitEvent(s, (hipEvent_t)st->sh_ready_event, 0));
        GpProfScope _p("sh_color", s);
        const bool al16 = (((uintptr_t)in->shs | (uintptr_t)in->shs_rest) & 15) == 0;
        auto kern = gp_sh_color_kernel;
        if (in->shs_rest) kern = gp_sh_color_split_kernel;                 // (alignment was checked for the preprocess launch)
        else if (d.M == 16 && al16) kern = gp_sh_color_sh16_kernel;
        GeomLayout glc(saved->geom, N);
        hipLaunchKernelGGL(kern, dim3(gp_blocks(N, 256)), dim3(256), 0, s, d, in->means3D, in->shs, in->shs_rest, st->campos,
                           (const int32_t*)out->radii, glc.rec, glc.clamped);
        GP_LAUNCH_CHECK();
    }
    { GpProfScope _p("composite_fwd", s, 1);
        hipLaunchKernelGGL((gp_debug_get(0) == 3 ? gp_composite_fwd_count_kernel : gp_debug_get(0) == 2 ? gp_composite_fwd_sbc_kernel : gp_composite_fwd_sb_kernel), dim3((unsigned)T), dim3(256), 0, s, d, il.ranges, point_list, gl.rec, st->bg,
                       out->color, out->depth, out->tidx, il.final_T, il.n_contrib, il.order, il.tile_work,
                       point_list ? (uint16_t*)((uint8_t*)point_list + gp_align_up((size_t)R * 4, 256)) : (uint16_t*)nullptr);
    GP_LAUNCH_CHECK(); }
    return 0;
}

// The backward's TEMP block (accumulators + tile order) handed out BEFORE the backward: gp_train_step_run lets the fused loss launch carry
// the prologue (loss_adam_kernels.h, GpLossPrologue) and passes the block (pro->acc) to gp_raster_backward_impl for the same saved state.
// pro->armed stays false where the stand-alone prologue has to run (nothing rendered, nothing saved)
int gp_raster_backward_prepare(const gp_raster_settings* st, const gp_raster_inputs* in, const gp_raster_saved* saved, gp_alloc_fn alloc,
                               void* alloc_ctx, GpLossPrologue* pro) {
    pro->armed = false;
    RasterDims d;
    if (make_dims(st, in, d)) return 1;
    const size_t N = (size_t)d.N, T = (size_t)d.gx * d.gy, P = (size_t)d.W * d.H;
    if (N == 0 || !saved || !saved->image || saved->num_rendered <= 0 || !alloc) return 0;
    ImageLayout il(saved->image, T, P);
    const size_t acc_floats = (size_t)GP_ACC_STRIDE * N;
    float* acc = (float*)alloc(alloc_ctx, GP_BUF_TEMP, gp_align_up(acc_floats * 4, 256) + gp_align_up(T * 4, 256));
    if (!acc) GP_FAIL("allocator returned NULL for TEMP");
    pro->ranges = il.ranges; pro->tile_work = il.tile_work; pro->T = (int)T;
    pro->order = (uint32_t*)((char*)acc + gp_align_up(acc_floats * 4, 256));
    pro->acc = acc; pro->acc_floats = acc_floats; pro->armed = true;
    return 0;
}

// `prepared_acc` (NULL: none): the block of gp_raster_backward_prepare for the same arguments, its prologue already enqueued
int gp_raster_backward_impl(const gp_raster_settings* st, const gp_raster_inputs* in, const gp_raster_outputs* fwd,
                            const gp_raster_saved* saved, const float* dL_dcolor, const float* dL_ddepth, gp_raster_grads* g,
                            gp_alloc_fn alloc, void* alloc_ctx, gp_stream_t stream_, float* prepared_acc) {
    hipStream_t s = (hipStream_t)stream_;
    RasterDims d;
    if (make_dims(st, in, d)) return 1;
    if (!fwd || !saved || !g || !alloc || !dL_dcolor) GP_FAIL("null argument");
    const size_t N = (size_t)d.N, T = (size_t)d.gx * d.gy, P = (size_t)d.W * d.H;
    if (N == 0) return 0;
    if (!g->dL_dmeans3D || !g->dL_dmeans2D || !g->dL_dopacities) GP_FAIL("null gradient outputs");
    if (in->shs ? (!g->dL_dshs && !g->adam_shs) : !g->dL_dcolors_precomp) GP_FAIL("missing colour gradient output");
    if (in->cov3D_precomp ? !g->dL_dcov3D_precomp : (!g->dL_dscales || !g->dL_drotations)) GP_FAIL("missing covariance gradient output");
    if (!saved->geom || !saved->image) GP_FAIL("saved state missing");
    AdamFuseDev af;
    memset(&af, 0, sizeof(af));
    if (g->adam_shs) {      // the optimizer step of (shs, shs_rest) inside this kernel: validated before anything is written
        const gp_adam_fuse* a = g->adam_shs;
        if (!(in->shs && in->shs_rest) || d.M != 16) GP_FAIL("adam_shs needs the split SH layout (shs [N,1,3] + shs_rest [N,15,3])");
        if (!a->exp_avg_dc || !a->exp_avg_sq_dc || !a->exp_avg_rest || !a->exp_avg_sq_rest) GP_FAIL("adam_shs: null moment pointer");
        if ((((uintptr_t)in->shs_rest | (uintptr_t)a->exp_avg_rest | (uintptr_t)a->exp_avg_sq_rest) & 15) != 0)
            GP_FAIL("adam_shs: shs_rest and its moments must be 16-byte aligned");
        if (a->step < 1) GP_FAIL("adam_shs: bad step");
        const float bc1 = 1.f - powf(a->beta1, (float)a->step);      // as gp_adam_step_multi
        af.p_dc = (float*)in->shs; af.m_dc = a->exp_avg_dc; af.v_dc = a->exp_avg_sq_dc;
        af.p_rest = (float*)in->shs_rest; af.m_rest = a->exp_avg_rest; af.v_rest = a->exp_avg_sq_rest;
        af.step_dc = a->lr_dc / bc1; af.step_rest = a->lr_rest / bc1;
        af.b1 = a->beta1; af.b2 = a->beta2; af.eps = a->eps;
        af.bc2_sqrt = sqrtf(1.f - powf(a->beta2, (float)a->step));
        af.skip = a->skip_flag; af.on = 1;
    }
    GeomLayout gl(saved->geom, N);
    ImageLayout il(saved->image, T, P);
    const uint32_t R = (uint32_t)saved->num_rendered;
    const uint32_t* point_list = (const uint32_t*)saved->binning;
    if (R > 0 && !point_list) GP_FAIL("saved binning state missing");

    const size_t acc_floats = (size_t)GP_ACC_STRIDE * N;
    // (gp_train_step_run: the block was obtained ahead of the loss, and the loss launch carried the prologue -- gp_raster_backward_prepare)
    const bool prepared = prepared_acc && R > 0;
    float* acc = prepared ? prepared_acc : (float*)alloc(alloc_ctx, GP_BUF_TEMP, gp_align_up(acc_floats * 4, 256) + gp_align_up(T * 4, 256));
    if (!acc) GP_FAIL("allocator returned NULL for TEMP");
    uint32_t* order_bwd = (uint32_t*)((char*)acc + gp_align_up(acc_floats * 4, 256));
    if (prepared) {            // (both done inside the loss launch)
    } else if (R > 0) {        // (tile order for the composite backward + the accumulators' fill, one launch)
        const unsigned zb = (unsigned)std::min<size_t>(2048, std::max<size_t>(1, (acc_floats / 4 + 1023) / 1024));
        hipLaunchKernelGGL(gp_bwd_prologue_kernel, dim3(1 + zb), dim3(1024), 0, s, il.ranges, il.tile_work, (int)T, order_bwd, acc, acc_floats);
        GP_LAUNCH_CHECK();
    } else {
        GP_HIP_CHECK(hipMemsetAsync(acc, 0, acc_floats * 4, s));
    }
    float* g_mean2D = acc;   // AoS, stride GP_ACC_STRIDE
    float* g_conic = acc + 2;
    float* g_opacity = acc + 5;
    float* g_color = acc + 6;
    float* g_depth = acc + 9;
    if (R > 0) {
        static thread_local int ablate_set = 0;
        if (gp_debug_get(1) != ablate_set) { ablate_set = gp_debug_get(1); if (gp_bwd_set_ablate(ablate_set)) GP_FAIL("bwd ablate flag"); }
        GpProfScope _p("composite_bwd", s);
        auto kern = dL_ddepth ? gp_composite_bwd_depth_kernel : gp_composite_bwd_kernel;
        hipLaunchKernelGGL(kern, dim3((unsigned)((T + 7) / 8 * 8) * GP_BWD_PARTS),
                           dim3(64), 0, s, d, il.ranges, point_list, (const uint16_t*)((const uint8_t*)point_list + gp_align_up((size_t)R * 4, 256)), gl.rec,
                           st->bg, (const float*)fwd->color, (const float*)fwd->depth, (const float*)il.final_T,
                           (const int32_t*)il.n_contrib, dL_dcolor, dL_ddepth, g_mean2D, g_conic, g_opacity, g_color, g_depth, order_bwd);
        GP_LAUNCH_CHECK();
    }
    {
        GpProfScope _p("preprocess_bwd", s);
        const bool al16 = (((uintptr_t)in->shs | (uintptr_t)in->shs_rest | (uintptr_t)g->dL_dshs | (uintptr_t)g->dL_dshs_rest) & 15) == 0;
        auto kern = gp_preprocess_bwd_kernel;
        if (in->shs && in->shs_rest) {
            if (!al16 || (!g->dL_dshs_rest && !af.on)) GP_FAIL("split SH mode needs 16-byte aligned tensors and dL_dshs_rest");
            kern = af.on ? gp_preprocess_bwd_split_adam_kernel : gp_preprocess_bwd_split_kernel;
        } else if (in->shs && d.M == 16 && al16) {
            kern = gp_preprocess_bwd_sh16_kernel;
        }
        if (g->accumulate_shs && kern == gp_preprocess_bwd_kernel)
            GP_FAIL("accumulate_shs needs the staged SH kernels (16 coeffs, 16-byte aligned)");      // (before anything is written)
        const bool sha = kern == gp_preprocess_bwd_split_adam_kernel;      // (its own workgroup shape)
        hipLaunchKernelGGL(kern, dim3(gp_blocks(N, sha ? GP_PB_ADAM_GAUSSIANS : 256)), dim3(sha ? GP_PB_ADAM_THREADS : 256), 0, s, d,
                           in->means3D, in->scales, in->rotations, in->shs,
                           in->shs_rest, in->cov3D_precomp, st->viewmatrix, st->projmatrix, st->campos, fwd->radii, gl.clamped,
                           g_mean2D, g_conic, g_opacity, g_color, g_depth, g->dL_dmeans3D, g->dL_dmeans2D, g->dL_dshs,
                           g->dL_dshs_rest, in->shs ? nullptr : g->dL_dcolors_precomp, g->dL_dopacities, g->dL_dscales,
                           g->dL_drotations, g->dL_dcov3D_precomp, (kern != gp_preprocess_bwd_kernel) ? g->accumulate_shs : 0, af);
        GP_LAUNCH_CHECK();
    }
    return 0;
}
extern "C" int gp_raster_backward(const gp_raster_settings* st, const gp_raster_inputs* in, const gp_raster_outputs* fwd,
                                  const gp_raster_saved* saved, const float* dL_dcolor, const float* dL_ddepth,
                                  gp_raster_grads* g, gp_alloc_fn alloc, void* alloc_ctx, gp_stream_t stream_) {
    return gp_raster_backward_impl(st, in, fwd, saved, dL_dcolor, dL_ddepth, g, alloc, alloc_ctx, stream_, nullptr);
}

extern "C" int gp_debug_counters(uint64_t* out4) {
    if (!out4) GP_FAIL("null argument");
    unsigned long long v[4];
    if (gp_pair_counters_read(v)) GP_FAIL("gp_debug_counters: device read failed");
    for (int k = 0; k < 4; ++k) out4[k] = v[k];
    return 0;
}

extern "C" int gp_raster_mark_visible(int64_t n, const float* means3D, const float* viewmatrix, uint8_t* present,
                                      gp_stream_t stream_) {
    if (n < 0 || n > 0x7FFFFFF0LL) GP_FAIL("n out of range");
    if (n == 0) return 0;
    if (!means3D || !viewmatrix || !present) GP_FAIL("null argument");
    hipLaunchKernelGGL(gp_mark_visible_kernel, dim3(gp_blocks((size_t)n, 256)), dim3(256), 0, (hipStream_t)stream_, (int)n,
                       means3D, viewmatrix, present);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_raster_debug_binning(const gp_raster_settings* st, const gp_raster_saved* saved, uint32_t* point_list,
                                       int32_t* ranges, gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (!st || !saved || !ranges) GP_FAIL("null argument");
    const int gx = (st->image_width + GP_TILE - 1) / GP_TILE, gy = (st->image_height + GP_TILE - 1) / GP_TILE;
    const size_t T = (size_t)gx * gy, P = (size_t)st->image_width * st->image_height;
    ImageLayout il(saved->image, T, P);
    GP_HIP_CHECK(hipMemcpyAsync(ranges, il.ranges, T * sizeof(int2), hipMemcpyDeviceToDevice, s));
    if (saved->num_rendered > 0) {
        if (!point_list) GP_FAIL("null point_list");
        GP_HIP_CHECK(hipMemcpyAsync(point_list, saved->binning, (size_t)saved->num_rendered * 4, hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

// ---- diagnostic entries over the index primitives (tests/test_gpu_sort_scan.py, tests/test_gpu_binning_direct.py) ------------------
// Scratch of one call: device blocks from hipMalloc, freed when the call returns (hipFree waits for the device).
struct GpDebugScratch {
    std::vector<void*> blocks;
    uint32_t* point_list = nullptr;         // gp_debug_bin_lists: the caller's list stands in for the BINNING block
    ~GpDebugScratch() { for (void* p : blocks) (void)hipFree(p); }
    void* get(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
        blocks.push_back(p);
        return p;
    }
    static void* alloc(void* ctx, int which, size_t bytes) {
        GpDebugScratch* self = (GpDebugScratch*)ctx;
        return which == GP_BUF_BINNING ? (void*)self->point_list : self->get(bytes);
    }
};

extern "C" int gp_debug_sort_pairs(int algo, const uint32_t* keys, const uint32_t* vals, int64_t n, int nbits, const uint32_t* by_value,
                                   uint32_t* keys_out, uint32_t* vals_out, uint32_t* sorted_out, uint32_t* count_out, gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (algo != 0 && algo != 1) GP_FAIL("gp_debug_sort_pairs: algo %d (0 = radix, 1 = three counting passes)", algo);
    if (n < 0 || n > 0x7FFFFFF0LL) GP_FAIL("gp_debug_sort_pairs: n out of range");
    if (nbits < 1 || nbits > 32) GP_FAIL("gp_debug_sort_pairs: nbits %d out of range (1 .. 32)", nbits);
    if (by_value && (vals || !sorted_out || !count_out)) GP_FAIL("gp_debug_sort_pairs: by_value needs iota values (vals == NULL), sorted_out and count_out");
    if (algo == 1 && (nbits != 32 || vals || n > 512LL * 8192LL))
        GP_FAIL("gp_debug_sort_pairs: the counting sort takes 32 key bits, iota values and n <= %lld", 512LL * 8192LL);
    if (n == 0) return 0;
    if (!keys || !keys_out || !vals_out) GP_FAIL("gp_debug_sort_pairs: null argument");
    const size_t N = (size_t)n;
    const size_t hist_elems = gp_sort_hist_elems(N), scan_elems = gp_scan_tmp_elems(256 * ((N + 4095) / 4096));
    const size_t ds_elems = algo == 1 ? gp_dsort_hist_elems(N) : 0;
    GpSortBufs sb;
    uint32_t* dshist;
    auto carve = [&](GpCarver& c) {
        for (int k = 0; k < 2; ++k) { sb.k[k] = c.take<uint32_t>(N); sb.v[k] = c.take<uint32_t>(N); }
        sb.hist = c.take<uint32_t>(hist_elems); sb.scan_tmp = c.take<uint32_t>(scan_elems);
        dshist = c.take<uint32_t>(ds_elems);
    };
    GpCarver c0(nullptr);
    carve(c0);
    GpDebugScratch scratch;
    void* tmp = scratch.get(c0.bytes());
    if (!tmp) GP_FAIL("gp_debug_sort_pairs: hipMalloc of %zu B failed", c0.bytes());
    GpCarver c(tmp);
    carve(c);
    sb.scan_tmp_elems = scan_elems;
    GP_HIP_CHECK(hipMemcpyAsync(sb.k[0], keys, N * 4, hipMemcpyDeviceToDevice, s));
    if (vals) GP_HIP_CHECK(hipMemcpyAsync(sb.v[0], vals, N * 4, hipMemcpyDeviceToDevice, s));
    const GpSortEpilogue ep = {(const uint2*)by_value, (uint2*)sorted_out, count_out};
    const int r = algo == 1 ? gp_depth_sort3(sb, N, dshist, s, by_value ? &ep : nullptr)
                            : gp_radix_sort_pairs(sb, N, nbits, s, vals == nullptr, by_value ? &ep : nullptr);
    if (r < 0) return 1;
    GP_HIP_CHECK(hipMemcpyAsync(keys_out, sb.k[r], N * 4, hipMemcpyDeviceToDevice, s));
    GP_HIP_CHECK(hipMemcpyAsync(vals_out, sb.v[r], N * 4, hipMemcpyDeviceToDevice, s));
    GP_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int gp_debug_scan_blocks(uint32_t* data, int64_t n, uint32_t* block_sums, uint32_t* total_slots, gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (n < 0 || n > 0x7FFFFFF0LL) GP_FAIL("gp_debug_scan_blocks: n out of range");
    if (!total_slots) GP_FAIL("gp_debug_scan_blocks: null argument");
    GP_HIP_CHECK(hipMemsetAsync(total_slots, 0, GP_TOTAL_SLOTS * sizeof(uint32_t), s));
    if (n > 0) {
        if (!data || !block_sums) GP_FAIL("gp_debug_scan_blocks: null argument");
        if (gp_scan_blocks_u32(data, (size_t)n, block_sums, total_slots, s)) return 1;
    }
    GP_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int gp_debug_bin_lists(int path, int64_t n, int gx, int gy, const uint32_t* sorted_ids, const uint32_t* rect_sorted, int64_t capacity,
                                  uint32_t* point_list, int32_t* ranges, uint32_t* status, uint32_t* r_out, gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (path != 0 && path != 1) GP_FAIL("gp_debug_bin_lists: path %d (0 = counting, 1 = duplicate + radix sort)", path);
    if (n < 0 || n > 0x7FFFFFF0LL) GP_FAIL("gp_debug_bin_lists: n out of range");
    if (gx < 1 || gy < 1 || gx > 0xFFFF || gy > 0xFFFF || (int64_t)gx * gy > (1LL << 24)) GP_FAIL("gp_debug_bin_lists: bad tile grid %d x %d", gx, gy);
    if (capacity < 0 || capacity > 0x7FFFFF00LL) GP_FAIL("gp_debug_bin_lists: capacity out of range");
    if (!ranges || !status || !r_out) GP_FAIL("gp_debug_bin_lists: null argument");
    const size_t N = (size_t)n, T = (size_t)gx * gy;
    if (path == 0 && !gp_bin_supported(N, T)) GP_FAIL("gp_debug_bin_lists: binning by counting does not take n = %lld, %zu tiles", (long long)n, T);
    *r_out = 0;
    GP_HIP_CHECK(hipMemsetAsync(ranges, 0, T * sizeof(int2), s));
    if (N == 0) {
        GP_HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(uint32_t), s));
        GP_HIP_CHECK(hipStreamSynchronize(s));
        return 0;
    }
    if (!sorted_ids || !rect_sorted) GP_FAIL("gp_debug_bin_lists: null argument");
    GpBinStage bs;
    memset(&bs.d, 0, sizeof(bs.d));
    bs.d.N = (int)n; bs.d.gx = gx; bs.d.gy = gy;
    bs.T = T; bs.sorted_ids = sorted_ids; bs.rects = (const uint2*)rect_sorted;
    bs.counting = path == 0;
    bs.bp = GpBinPlan{0, 0, 0};
    if (bs.counting) bs.bp = gp_bin_plan(N, T);
    bs.capacity = capacity; bs.status = status; bs.ranges = (int2*)ranges;
    const size_t n_sums = (N + GP_SCAN_TILE - 1) / GP_SCAN_TILE + 64;
    auto carve = [&](GpCarver& c) {
        bs.tt = c.take<uint32_t>(N + 1); bs.block_sums = c.take<uint32_t>(n_sums); bs.binhist = c.take<uint32_t>(bs.bp.hist_elems);
        bs.total = c.take<uint32_t>(GP_TOTAL_SLOTS); bs.order = c.take<uint32_t>(T);
    };
    GpCarver c0(nullptr);
    carve(c0);
    GpDebugScratch scratch;
    scratch.point_list = point_list;
    void* tmp = scratch.get(c0.bytes());
    if (!tmp) GP_FAIL("gp_debug_bin_lists: hipMalloc of %zu B failed", c0.bytes());
    GpCarver c(tmp);
    carve(c);
    GP_HIP_CHECK(hipMemsetAsync(bs.total, 0, GP_TOTAL_SLOTS * sizeof(uint32_t), s));
    if (!bs.counting) {     // tiles per Gaussian (in the forward: the depth sort's epilogue)
        std::vector<uint32_t> h(2 * N);
        GP_HIP_CHECK(hipMemcpyAsync(h.data(), rect_sorted, N * sizeof(uint2), hipMemcpyDeviceToHost, s));
        GP_HIP_CHECK(hipStreamSynchronize(s));
        for (size_t i = 0; i < N; ++i) h[i] = (h[2 * i + 1] & 0xFFFFu) * (h[2 * i + 1] >> 16);
        GP_HIP_CHECK(hipMemcpyAsync(bs.tt, h.data(), N * 4, hipMemcpyHostToDevice, s));
        GP_HIP_CHECK(hipStreamSynchronize(s));
    }
    uint32_t R = 0;
    uint32_t* pl = nullptr;
    void* bin = nullptr;
    size_t bin_bytes = 0;
    bool order_done = false;
    if (gp_binning_stage(bs, GpDebugScratch::alloc, &scratch, s, R, pl, bin, bin_bytes, order_done)) return 1;
    GP_HIP_CHECK(hipStreamSynchronize(s));
    *r_out = R;
    return 0;
}
