// jpeg_kernels.hip -- baseline JPEG encoding on the device (include/gp_jpeg.h): three launches per call whatever the batch is.
//   1. jpeg_segment_kernel  one workgroup per restart interval of GP_JPEG_RESTART_MCUS MCUs: pixels -> Y Cb Cr -> subsample -> DCT ->
//                           quantise, all in LDS; a lane per block counts and then packs its codes at prefix-summed bit offsets; a
//                           second prefix sum over the 0xFF bytes stuffs them; the interval and its length go to scratch
//   2. jpeg_layout_kernel   one workgroup per image: the intervals' offsets, the file's length
//   3. jpeg_copy_kernel     one workgroup per interval: the header, the interval, the RST marker or EOI in place
// The workgroup programs themselves are csrc/jpeg_core.h, which also runs on a CPU.  Quantised coefficients never reach memory.  Every
// store is an ordinary vector store; the only atomics are integer ors on LDS, whose result does not depend on their order.
#include "gp_common.h"

#include "../../include/gp_jpeg.h"
#include "jpeg_core.h"

__global__ void __launch_bounds__(JPG_BLOCK) jpeg_segment_kernel(JpgPlan p) {
    __shared__ JpgSegShared sh;
    jpg_segment_block(sh, p, (int)blockIdx.y, (int)blockIdx.x);
}

__global__ void __launch_bounds__(JPG_BLOCK) jpeg_layout_kernel(JpgPlan p) {
    __shared__ JpgLayoutShared sh;
    jpg_layout_block(sh, p, (int)blockIdx.x);
}

__global__ void __launch_bounds__(JPG_BLOCK) jpeg_copy_kernel(JpgPlan p) {
    jpg_copy_block(p, (int)blockIdx.y, (int)blockIdx.x);
}

static_assert(sizeof(JpgSegShared) <= 65536, "an interval and the workgroup's tables fit the LDS a kernel gets without opting in");
static_assert(JPG_MAX_BLOCKS <= JPG_BLOCK, "a lane per block");

static int jpg_check_sizes(const char* who, int64_t B, int32_t H, int32_t W, int32_t sub) {
    if (B < 1 || B > GP_JPEG_MAX_BATCH) GP_FAIL("%s: B = %lld outside [1, %d]", who, (long long)B, GP_JPEG_MAX_BATCH);
    if (H < 1 || H > GP_JPEG_MAX_SIDE) GP_FAIL("%s: H = %d outside [1, %d]", who, H, GP_JPEG_MAX_SIDE);
    if (W < 1 || W > GP_JPEG_MAX_SIDE) GP_FAIL("%s: W = %d outside [1, %d]", who, W, GP_JPEG_MAX_SIDE);
    if (sub != GP_JPEG_420 && sub != GP_JPEG_444) GP_FAIL("%s: subsampling = %d is neither GP_JPEG_420 nor GP_JPEG_444", who, sub);
    JpgPlan p;
    jpg_plan_sizes(p, 1, H, W, sub);
    if (jpg_bound_of(p) >= ((int64_t)1 << 31))
        GP_FAIL("%s: %d x %d: the largest file, %lld bytes, must stay below 2^31", who, H, W, (long long)jpg_bound_of(p));
    return 0;
}

// the sizes of a plan, and its arrays carved out of `scratch`
static size_t jpg_plan(JpgPlan& p, int B, int H, int W, int sub, void* scratch) {
    jpg_plan_sizes(p, B, H, W, sub);
    GpCarver c(scratch);
    p.seg = c.take<uint8_t>((size_t)B * p.nseg * p.seg_stride);
    p.seg_len = c.take<uint32_t>((size_t)B * p.nseg);
    p.seg_off = c.take<uint32_t>((size_t)B * p.nseg);
    return c.bytes();
}

extern "C" int gp_jpeg_abi_version(void) { return GP_JPEG_ABI_VERSION; }

extern "C" int gp_jpeg_quant_tables(int32_t quality, uint8_t* lum, uint8_t* chr) {
    if (quality < 1 || quality > 100) GP_FAIL("gp_jpeg_quant_tables: quality = %d outside [1, 100]", quality);
    if (!lum || !chr) GP_FAIL("gp_jpeg_quant_tables: null argument");
    jpg_quant_tables(quality, lum, chr);
    return 0;
}

extern "C" int64_t gp_jpeg_bound(int32_t H, int32_t W, int32_t subsampling) {
    if (jpg_check_sizes("gp_jpeg_bound", 1, H, W, subsampling)) return -1;
    JpgPlan p;
    jpg_plan_sizes(p, 1, H, W, subsampling);
    return jpg_bound_of(p);
}

extern "C" int64_t gp_jpeg_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t subsampling) {
    if (jpg_check_sizes("gp_jpeg_scratch_bytes", B, H, W, subsampling)) return -1;
    JpgPlan p;
    return (int64_t)jpg_plan(p, B, H, W, subsampling, nullptr);
}

extern "C" int gp_jpeg_encode(int32_t B, int32_t H, int32_t W, const void* src, int32_t src_kind, const uint8_t* lum, const uint8_t* chr,
                              int32_t subsampling, uint8_t* out, int64_t out_stride, uint32_t* sizes, void* scratch, gp_stream_t stream_) {
    if (jpg_check_sizes("gp_jpeg_encode", B, H, W, subsampling)) return 1;
    if (src_kind != GP_PNG_SRC_F32 && src_kind != GP_PNG_SRC_U8) GP_FAIL("gp_jpeg_encode: src_kind = %d is neither GP_PNG_SRC_F32 nor GP_PNG_SRC_U8", src_kind);
    if (out_stride < gp_jpeg_bound(H, W, subsampling))
        GP_FAIL("gp_jpeg_encode: out_stride = %lld below gp_jpeg_bound(%d, %d, %d) = %lld", (long long)out_stride, H, W, subsampling, (long long)gp_jpeg_bound(H, W, subsampling));
    if (!src || !lum || !chr || !out || !sizes || !scratch) GP_FAIL("gp_jpeg_encode: null argument");
    for (int i = 0; i < 64; ++i)
        if (!lum[i] || !chr[i]) GP_FAIL("gp_jpeg_encode: quantisation entry %d is 0 (every entry must be >= 1)", i);
    if ((uintptr_t)scratch & 255) GP_FAIL("gp_jpeg_encode: scratch must be 256-byte aligned");
    if (src_kind == GP_PNG_SRC_F32 && ((uintptr_t)src & 3)) GP_FAIL("gp_jpeg_encode: a float32 src must be 4-byte aligned");
    if ((uintptr_t)sizes & 3) GP_FAIL("gp_jpeg_encode: sizes must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("jpeg_encode", s);
    JpgPlan p;
    jpg_plan(p, B, H, W, subsampling, scratch);
    p.src_kind = src_kind; p.src = src;
    p.out = out; p.out_stride = out_stride; p.sizes = sizes;
    for (int i = 0; i < 64; ++i) { p.qt[0][i] = lum[i]; p.qt[1][i] = chr[i]; }
    if (jpg_build_header(p) != JPG_HEAD) GP_FAIL("gp_jpeg_encode: the header is not GP_JPEG_HEAD_BYTES long");
    hipLaunchKernelGGL(jpeg_segment_kernel, dim3(p.nseg, B), dim3(JPG_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_layout_kernel, dim3(B), dim3(JPG_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_copy_kernel, dim3(p.nseg, B), dim3(JPG_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    return 0;
}
