// jpeg_decode_kernels.hip -- baseline JPEG decoding on the device (include/gp_jpeg_decode.h): four launches per call whatever the batch is.
//   1. jpgd_entropy_kernel  one wave per 64 restart intervals of one image: the image's decoding tables built in LDS, then a lane per
//                           interval reads its own bytes and writes whole blocks of int16 coefficients
//   2. jpgd_status_kernel   one workgroup per image: the segment table checked, status[b]
//   3. jpgd_idct_kernel     one workgroup per 32 blocks, eight lanes per block: dequantise, columns, rows, 8-bit planes
//   4. jpgd_pixel_kernel    one lane per pixel: chroma upsampling, colour, planar uint8 / float32 (byte / 255)
// The workgroup programs themselves are csrc/jpeg_decode_core.h, which also runs on a CPU.  Every store is an ordinary vector store and
// there is no atomic at all.  No workgroup waits for another.  The entropy kernel's workgroups share nothing but their image's 1.2 KB of
// tables -- every lane streams its own bytes once and writes its own blocks once -- so which XCD a workgroup lands on changes nothing
// an L2 could keep, and the grid is left in its natural order.
#include "gp_common.h"

#include "../../include/gp_jpeg_decode.h"
#include "jpeg_decode_core.h"

__global__ void __launch_bounds__(JPD_ENT_LANES) jpgd_entropy_kernel(JpdPlan p) {
    __shared__ JpdEntropyShared sh;
    jpd_entropy_block(sh, p, (int)blockIdx.y, (int)blockIdx.x);
}

__global__ void __launch_bounds__(JPD_BLOCK) jpgd_status_kernel(JpdPlan p) {
    __shared__ JpdStatusShared sh;
    jpd_status_block(sh, p, (int)blockIdx.x);
}

__global__ void __launch_bounds__(JPD_BLOCK) jpgd_idct_kernel(JpdPlan p) {
    __shared__ JpdIdctShared sh;
    jpd_idct_block(sh, p, (int)blockIdx.y, (int)blockIdx.x);
}

__global__ void __launch_bounds__(JPD_BLOCK) jpgd_pixel_kernel(JpdPlan p) {
    const int x = (int)(blockIdx.x * JPD_BLOCK + threadIdx.x);
    if (x < p.W) jpd_pixel(p, (int)blockIdx.z, (int)blockIdx.y, x);
}

static_assert(GP_JPEG_DECODE_TABLE_BYTES == JPD_TAB_HUFF + 4 * JPD_HUFF_BYTES, "the layout of an image's tables");
static_assert(sizeof(JpdEntropyShared) <= 8192, "the entropy kernel's LDS never bounds its occupancy");

static int jpgd_check_sizes(const char* who, int64_t B, int32_t H, int32_t W, int32_t sub, int64_t nseg) {
    if (B < 1 || B > GP_JPEG_DECODE_MAX_BATCH) GP_FAIL("%s: B = %lld outside [1, %d]", who, (long long)B, GP_JPEG_DECODE_MAX_BATCH);
    if (H < 1 || H > GP_JPEG_MAX_SIDE) GP_FAIL("%s: H = %d outside [1, %d]", who, H, GP_JPEG_MAX_SIDE);
    if (W < 1 || W > GP_JPEG_MAX_SIDE) GP_FAIL("%s: W = %d outside [1, %d]", who, W, GP_JPEG_MAX_SIDE);
    if (sub != GP_JPEG_420 && sub != GP_JPEG_444) GP_FAIL("%s: subsampling = %d is neither GP_JPEG_420 nor GP_JPEG_444", who, sub);
    // (block and byte positions inside an image are 32-bit ints)
    const int64_t ms = sub == GP_JPEG_420 ? 16 : 8, area = ((H + ms - 1) / ms * ms) * ((W + ms - 1) / ms * ms);
    if (3 * area >= ((int64_t)1 << 31)) GP_FAIL("%s: %d x %d: the MCU-padded planes, %lld bytes, must stay below 2^31", who, H, W, (long long)(3 * area));
    if (nseg < B) GP_FAIL("%s: nseg = %lld below B = %lld (every image has a segment)", who, (long long)nseg, (long long)B);
    return 0;
}

// the sizes of a plan, and its arrays carved out of `scratch`
static size_t jpgd_plan(JpdPlan& p, int B, int H, int W, int sub, int nseg, void* scratch) {
    jpd_plan_sizes(p, B, H, W, sub, nseg);
    GpCarver c(scratch);
    p.coef = c.take<int16_t>((size_t)B * p.nblk * 64);
    p.planes = c.take<uint8_t>((size_t)B * p.plane_bytes);
    p.info = c.take<uint32_t>((size_t)nseg);
    return c.bytes();
}

extern "C" int gp_jpeg_decode_abi_version(void) { return GP_JPEG_DECODE_ABI_VERSION; }

extern "C" int64_t gp_jpeg_decode_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t subsampling, int32_t nseg) {
    if (jpgd_check_sizes("gp_jpeg_decode_scratch_bytes", B, H, W, subsampling, nseg)) return -1;
    JpdPlan p;
    return (int64_t)jpgd_plan(p, B, H, W, subsampling, nseg, nullptr);
}

extern "C" int gp_jpeg_decode(int32_t B, int32_t H, int32_t W, int32_t subsampling, int32_t dst_kind, const uint8_t* payload,
                              int64_t payload_bytes, const int64_t* segments, int32_t nseg, const int32_t* image_seg, int32_t max_image_seg,
                              const uint8_t* tables, void* dst, int64_t dst_stride, uint32_t* status, void* scratch, gp_stream_t stream_) {
    if (jpgd_check_sizes("gp_jpeg_decode", B, H, W, subsampling, nseg)) return 1;
    if (dst_kind != GP_JPEG_DECODE_DST_U8 && dst_kind != GP_JPEG_DECODE_DST_F32) GP_FAIL("gp_jpeg_decode: dst_kind = %d is neither GP_JPEG_DECODE_DST_U8 nor GP_JPEG_DECODE_DST_F32", dst_kind);
    if (payload_bytes < 0 || payload_bytes >= ((int64_t)1 << 40)) GP_FAIL("gp_jpeg_decode: payload_bytes = %lld outside [0, 2^40)", (long long)payload_bytes);
    if (max_image_seg < 1 || max_image_seg > nseg) GP_FAIL("gp_jpeg_decode: max_image_seg = %d outside [1, nseg = %d]", max_image_seg, nseg);
    if (dst_stride < (int64_t)3 * H * W) GP_FAIL("gp_jpeg_decode: dst_stride = %lld below 3 * H * W = %lld", (long long)dst_stride, (long long)3 * H * W);
    if (!payload || !segments || !image_seg || !tables || !dst || !status || !scratch) GP_FAIL("gp_jpeg_decode: null argument");
    if ((uintptr_t)scratch & 255) GP_FAIL("gp_jpeg_decode: scratch must be 256-byte aligned");
    if ((uintptr_t)segments & 7) GP_FAIL("gp_jpeg_decode: segments must be 8-byte aligned");
    if (((uintptr_t)image_seg | (uintptr_t)status) & 3) GP_FAIL("gp_jpeg_decode: image_seg and status must be 4-byte aligned");
    if (dst_kind == GP_JPEG_DECODE_DST_F32 && ((uintptr_t)dst & 3)) GP_FAIL("gp_jpeg_decode: a float32 dst must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("jpeg_decode", s);
    JpdPlan p;
    jpgd_plan(p, B, H, W, subsampling, nseg, scratch);
    p.dst_kind = dst_kind; p.max_image_seg = max_image_seg;
    p.payload = payload; p.payload_bytes = payload_bytes; p.seg = segments; p.image_seg = image_seg; p.tables = tables;
    p.dst = dst; p.dst_stride = dst_stride; p.status = status;
    hipLaunchKernelGGL(jpgd_entropy_kernel, dim3(gp_blocks((size_t)max_image_seg, JPD_ENT_LANES), B), dim3(JPD_ENT_LANES), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpgd_status_kernel, dim3(B), dim3(JPD_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpgd_idct_kernel, dim3(gp_blocks((size_t)p.nblk, JPD_IDCT_BLOCKS), B), dim3(JPD_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpgd_pixel_kernel, dim3(gp_blocks((size_t)W, JPD_BLOCK), H, B), dim3(JPD_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    return 0;
}
