// png_decode_kernels.hip -- PNG decoding on the device (include/gp_png_decode.h): four launches per call whatever the batch is.
//   1. pngd_inflate_kernel   one workgroup per segment: lane 0 reads the bits into literals and tokens, all lanes resolve a batch of
//                            bytes against the 32 K window in LDS and flush it, with the segment's Adler sums
//   2. pngd_status_kernel    one workgroup per image: status[b], mode[b], the Adler-32 from the segments' sums
//   3. pngd_unfilter_kernel  one workgroup per image: the five row filters undone in place, rows skewed by one chunk per lane
//   4. pngd_convert_kernel   one lane per pixel: planar uint8 / float32 (byte / 255), the composite over a background
// The workgroup programs themselves are csrc/png_decode_core.h, which also runs on a CPU.  Every store is an ordinary vector store; the
// only atomics are integer adds / ors on LDS, whose result does not depend on their order.  No workgroup waits for another.
#include "gp_common.h"

#include "../../include/gp_png_decode.h"
#include "png_decode_core.h"

__global__ void __launch_bounds__(PNG_BLOCK) pngd_inflate_kernel(PngdPlan p) {
    __shared__ PngdInflateShared sh;
    pngd_inflate_block(sh, p, (int)blockIdx.x);
}

__global__ void __launch_bounds__(PNG_BLOCK) pngd_status_kernel(PngdPlan p) {
    __shared__ PngdStatusShared sh;
    pngd_status_block(sh, p, (int)blockIdx.x);
}

__global__ void __launch_bounds__(PNG_BLOCK) pngd_unfilter_kernel(PngdPlan p) {
    __shared__ PngdUnfilterShared sh;
    pngd_unfilter_block(sh, p, (int)blockIdx.x);
}

__global__ void __launch_bounds__(PNG_BLOCK) pngd_convert_kernel(PngdPlan p) {
    const int x = (int)(blockIdx.x * PNG_BLOCK + threadIdx.x);
    if (x < p.W) pngd_convert_pixel(p, (int)blockIdx.z, (int)blockIdx.y, x);
}

static_assert(sizeof(PngdInflateShared) <= 160 * 1024 / 3, "three inflate workgroups per CU");
static_assert((PNGD_WINDOW & (PNGD_WINDOW - 1)) == 0 && PNGD_BATCH + 258 <= PNGD_WINDOW && PNGD_BATCH >= 2 * 258, "the window is a ring; a batch fits it");

static int pngd_check_sizes(const char* who, int64_t B, int32_t H, int32_t W, int32_t C, int64_t nseg) {
    if (B < 1 || B > GP_PNG_DECODE_MAX_BATCH) GP_FAIL("%s: B = %lld outside [1, %d]", who, (long long)B, GP_PNG_DECODE_MAX_BATCH);
    if (H < 1) GP_FAIL("%s: H = %d must be >= 1", who, H);
    if (W < 1) GP_FAIL("%s: W = %d must be >= 1", who, W);
    if (H > 65535) GP_FAIL("%s: H = %d above 65535 (the rows are one grid dimension)", who, H);
    if (C < 1 || C > 4) GP_FAIL("%s: C = %d outside [1, 4]", who, C);
    // (positions in the filtered stream are 32-bit ints)
    const int64_t S = (int64_t)H * ((int64_t)C * W + 1);
    if (S >= ((int64_t)1 << 31)) GP_FAIL("%s: H * (C W + 1) = %lld must stay below 2^31", who, (long long)S);
    if (nseg < B) GP_FAIL("%s: nseg = %lld below B = %lld (every image has a segment)", who, (long long)nseg, (long long)B);
    return 0;
}

// the sizes of a plan, and its arrays carved out of `scratch`
static size_t pngd_plan(PngdPlan& p, int B, int H, int W, int C, int nseg, void* scratch) {
    p.B = B; p.H = H; p.W = W; p.C = C; p.nseg = nseg;
    p.row = 1 + C * W;
    p.S = (int64_t)H * p.row;
    p.S_pad = (int64_t)gp_align_up((size_t)p.S, 16);
    GpCarver c(scratch);
    p.filt = c.take<uint8_t>((size_t)B * p.S_pad);
    p.info = c.take<uint32_t>((size_t)nseg * PNGD_INFO_WORDS);
    return c.bytes();
}

extern "C" int gp_png_decode_abi_version(void) { return GP_PNG_DECODE_ABI_VERSION; }

extern "C" int64_t gp_png_decode_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t nseg) {
    if (pngd_check_sizes("gp_png_decode_scratch_bytes", B, H, W, C, nseg)) return -1;
    PngdPlan p;
    return (int64_t)pngd_plan(p, B, H, W, C, nseg, nullptr);
}

extern "C" int gp_png_decode(int32_t B, int32_t H, int32_t W, int32_t C, int32_t C_out, int32_t dst_kind, const uint8_t* payload,
                             int64_t payload_bytes, const int64_t* segments, int32_t nseg, const int32_t* image_seg,
                             const float* background, void* dst, int64_t dst_stride, uint32_t* status, uint32_t* mode, void* scratch,
                             gp_stream_t stream_) {
    if (pngd_check_sizes("gp_png_decode", B, H, W, C, nseg)) return 1;
    if (C_out < 1 || C_out > C) GP_FAIL("gp_png_decode: C_out = %d outside [1, C = %d]", C_out, C);
    if (dst_kind != GP_PNG_DECODE_DST_U8 && dst_kind != GP_PNG_DECODE_DST_F32) GP_FAIL("gp_png_decode: dst_kind = %d is neither GP_PNG_DECODE_DST_U8 nor GP_PNG_DECODE_DST_F32", dst_kind);
    if (background && (C != 4 || C_out != 3)) GP_FAIL("gp_png_decode: a background needs C = 4 and C_out = 3 (got C = %d, C_out = %d)", C, C_out);
    if (payload_bytes < 0 || payload_bytes >= ((int64_t)1 << 40)) GP_FAIL("gp_png_decode: payload_bytes = %lld outside [0, 2^40)", (long long)payload_bytes);
    if (dst_stride < (int64_t)C_out * H * W) GP_FAIL("gp_png_decode: dst_stride = %lld below C_out * H * W = %lld", (long long)dst_stride, (long long)C_out * H * W);
    if (!payload || !segments || !image_seg || !dst || !status || !mode || !scratch) GP_FAIL("gp_png_decode: null argument");
    if ((uintptr_t)scratch & 255) GP_FAIL("gp_png_decode: scratch must be 256-byte aligned");
    if ((uintptr_t)segments & 7) GP_FAIL("gp_png_decode: segments must be 8-byte aligned");
    if (((uintptr_t)image_seg | (uintptr_t)status | (uintptr_t)mode | (uintptr_t)background) & 3) GP_FAIL("gp_png_decode: image_seg, status, mode and background must be 4-byte aligned");
    if (dst_kind == GP_PNG_DECODE_DST_F32 && ((uintptr_t)dst & 3)) GP_FAIL("gp_png_decode: a float32 dst must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("png_decode", s);
    PngdPlan p;
    pngd_plan(p, B, H, W, C, nseg, scratch);
    p.C_out = C_out; p.dst_kind = dst_kind;
    p.payload = payload; p.payload_bytes = payload_bytes; p.seg = segments; p.image_seg = image_seg; p.bg = background;
    p.dst = dst; p.dst_stride = dst_stride; p.status = status; p.mode = mode;
    hipLaunchKernelGGL(pngd_inflate_kernel, dim3(nseg), dim3(PNG_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(pngd_status_kernel, dim3(B), dim3(PNG_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(pngd_unfilter_kernel, dim3(B), dim3(PNG_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(pngd_convert_kernel, dim3(gp_blocks((size_t)W, PNG_BLOCK), H, B), dim3(PNG_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    return 0;
}
