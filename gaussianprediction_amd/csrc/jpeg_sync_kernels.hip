// jpeg_sync_kernels.hip -- baseline JPEG files without restart markers decoded on many lanes (include/gp_jpeg_sync.h): the
// self-synchronising entropy stage in front of jpeg_decode_kernels.hip's transform and pixel stage.  Ten launches per call whatever the
// batch is:
//   0. a memset               the coefficient blocks zeroed (a block that straddles a cut is written by two lanes)
//   1. jpgs_plan_kernel       one workgroup: the segment rows checked, every image's subsequences and its first slot
//   2. jpgs_chunk_kernel      one workgroup of 256 lanes per 256 subsequences of one image: the speculative pass and the rounds to the
//                             chunk's fixpoint, states in LDS
//   3. jpgs_cross_kernel      one workgroup per image, a lane per chunk: the chunks repaired from their left neighbours, to a fixpoint
//   4. jpgs_count_kernel      a lane per subsequence: blocks begun, DC sums
//   5. jpgs_scan_kernel       one workgroup per image: first blocks, DC predictions
//   6. jpgs_write_kernel      a lane per subsequence: the coefficients
//   7. jpgs_status_kernel     one workgroup per image: status[b], info[b]
//   8. 9.                     the transform and the pixels of csrc/jpeg_decode_core.h, unchanged
// The workgroup programs are csrc/jpeg_sync_core.h, which also runs on a CPU.  Every store is an ordinary vector store, there is no
// atomic, and no workgroup waits for another: the stages communicate across launches only.  A lane per subsequence is divergent by
// nature, as jpgd_entropy_kernel is; what the lanes share is the image's tables in LDS.
#include "gp_common.h"

#include "../../include/gp_jpeg_sync.h"
#include "jpeg_sync_core.h"

__global__ void __launch_bounds__(JPS_C) jpgs_plan_kernel(JpsPlan p) {
    __shared__ JpsPlanShared sh;
    jps_plan_block(sh, p);
}

__global__ void __launch_bounds__(JPS_C) jpgs_chunk_kernel(JpsPlan p) {
    __shared__ JpsChunkShared sh;
    jps_chunk_block(sh, p, (int)blockIdx.y, (int)blockIdx.x);
}

__global__ void __launch_bounds__(JPS_C) jpgs_cross_kernel(JpsPlan p) {
    __shared__ JpsChunkShared sh;
    jps_cross_block(sh, p, (int)blockIdx.x);
}

__global__ void __launch_bounds__(JPS_C) jpgs_count_kernel(JpsPlan p) {
    __shared__ JpdEntropyShared sh;
    jps_pass_block(sh, p, (int)blockIdx.y, (int)blockIdx.x, 1);
}

__global__ void __launch_bounds__(JPS_C) jpgs_scan_kernel(JpsPlan p) {
    __shared__ JpsScanShared sh;
    jps_scan_block(sh, p, (int)blockIdx.x);
}

__global__ void __launch_bounds__(JPS_C) jpgs_write_kernel(JpsPlan p) {
    __shared__ JpdEntropyShared sh;
    jps_pass_block(sh, p, (int)blockIdx.y, (int)blockIdx.x, 2);
}

__global__ void __launch_bounds__(JPS_C) jpgs_status_kernel(JpsPlan p) {
    __shared__ JpsStatusShared sh;
    jps_status_block(sh, p, (int)blockIdx.x);
}

__global__ void __launch_bounds__(JPD_BLOCK) jpgs_idct_kernel(JpdPlan p) {
    __shared__ JpdIdctShared sh;
    jpd_idct_block(sh, p, (int)blockIdx.y, (int)blockIdx.x);
}

__global__ void __launch_bounds__(JPD_BLOCK) jpgs_pixel_kernel(JpdPlan p) {
    const int x = (int)(blockIdx.x * JPD_BLOCK + threadIdx.x);
    if (x < p.W) jpd_pixel(p, (int)blockIdx.z, (int)blockIdx.y, x);
}

static_assert(sizeof(JpsChunkShared) <= 16384, "the chunk kernel's LDS never bounds its occupancy");

static int jpgs_check_sizes(const char* who, int64_t B, int32_t H, int32_t W, int32_t sub, int64_t payload_bytes) {
    if (B < 1 || B > GP_JPEG_DECODE_MAX_BATCH) GP_FAIL("%s: B = %lld outside [1, %d]", who, (long long)B, GP_JPEG_DECODE_MAX_BATCH);
    if (H < 1 || H > GP_JPEG_MAX_SIDE) GP_FAIL("%s: H = %d outside [1, %d]", who, H, GP_JPEG_MAX_SIDE);
    if (W < 1 || W > GP_JPEG_MAX_SIDE) GP_FAIL("%s: W = %d outside [1, %d]", who, W, GP_JPEG_MAX_SIDE);
    if (sub != GP_JPEG_420 && sub != GP_JPEG_444) GP_FAIL("%s: subsampling = %d is neither GP_JPEG_420 nor GP_JPEG_444", who, sub);
    const int64_t ms = sub == GP_JPEG_420 ? 16 : 8, area = ((H + ms - 1) / ms * ms) * ((W + ms - 1) / ms * ms);
    if (3 * area >= ((int64_t)1 << 31)) GP_FAIL("%s: %d x %d: the MCU-padded planes, %lld bytes, must stay below 2^31", who, H, W, (long long)(3 * area));
    if (payload_bytes < 0 || payload_bytes >= ((int64_t)1 << 37)) GP_FAIL("%s: payload_bytes = %lld outside [0, 2^37)", who, (long long)payload_bytes);
    return 0;
}

// the sizes of a plan, and its arrays carved out of `scratch`
static size_t jpgs_plan(JpsPlan& p, int B, int H, int W, int sub, int64_t payload_bytes, void* scratch) {
    jpd_plan_sizes(p.d, B, H, W, sub, B);
    p.slots = jps_slots(B, payload_bytes);
    GpCarver c(scratch);
    p.d.coef = c.take<int16_t>((size_t)B * p.d.nblk * 64);
    p.d.planes = c.take<uint8_t>((size_t)B * p.d.plane_bytes);
    p.d.info = nullptr;
    p.img = c.take<uint32_t>((size_t)B * 4);
    p.ex = c.take<uint64_t>((size_t)p.slots);
    p.used = c.take<uint64_t>((size_t)p.slots);
    p.dc = c.take<uint64_t>((size_t)p.slots);
    p.nb = c.take<uint32_t>((size_t)p.slots);
    p.flag = c.take<uint32_t>((size_t)p.slots);
    p.rnd = c.take<uint32_t>((size_t)p.slots);
    return c.bytes();
}

extern "C" int gp_jpeg_sync_abi_version(void) { return GP_JPEG_SYNC_ABI_VERSION; }

extern "C" int64_t gp_jpeg_sync_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t subsampling, int64_t payload_bytes) {
    if (jpgs_check_sizes("gp_jpeg_sync_scratch_bytes", B, H, W, subsampling, payload_bytes)) return -1;
    JpsPlan p;
    return (int64_t)jpgs_plan(p, B, H, W, subsampling, payload_bytes, nullptr);
}

extern "C" int gp_jpeg_sync_decode(int32_t B, int32_t H, int32_t W, int32_t subsampling, int32_t dst_kind, const uint8_t* payload,
                                   int64_t payload_bytes, const int64_t* segments, int32_t nseg, const int32_t* image_seg, int32_t max_image_seg,
                                   const uint8_t* tables, void* dst, int64_t dst_stride, uint32_t* status, uint32_t* info, void* scratch,
                                   gp_stream_t stream_) {
    if (jpgs_check_sizes("gp_jpeg_sync_decode", B, H, W, subsampling, payload_bytes)) return 1;
    if (dst_kind != GP_JPEG_DECODE_DST_U8 && dst_kind != GP_JPEG_DECODE_DST_F32) GP_FAIL("gp_jpeg_sync_decode: dst_kind = %d is neither GP_JPEG_DECODE_DST_U8 nor GP_JPEG_DECODE_DST_F32", dst_kind);
    if (nseg != B) GP_FAIL("gp_jpeg_sync_decode: nseg = %d is not B = %d (every image is exactly one segment)", nseg, B);
    if (max_image_seg != 1) GP_FAIL("gp_jpeg_sync_decode: max_image_seg = %d is not 1 (every image is exactly one segment)", max_image_seg);
    if (dst_stride < (int64_t)3 * H * W) GP_FAIL("gp_jpeg_sync_decode: dst_stride = %lld below 3 * H * W = %lld", (long long)dst_stride, (long long)3 * H * W);
    if (!payload || !segments || !image_seg || !tables || !dst || !status || !info || !scratch) GP_FAIL("gp_jpeg_sync_decode: null argument");
    if ((uintptr_t)scratch & 255) GP_FAIL("gp_jpeg_sync_decode: scratch must be 256-byte aligned");
    if ((uintptr_t)segments & 7) GP_FAIL("gp_jpeg_sync_decode: segments must be 8-byte aligned");
    if (((uintptr_t)image_seg | (uintptr_t)status | (uintptr_t)info) & 3) GP_FAIL("gp_jpeg_sync_decode: image_seg, status and info must be 4-byte aligned");
    if (dst_kind == GP_JPEG_DECODE_DST_F32 && ((uintptr_t)dst & 3)) GP_FAIL("gp_jpeg_sync_decode: a float32 dst must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("jpeg_sync_decode", s);
    JpsPlan p;
    jpgs_plan(p, B, H, W, subsampling, payload_bytes, scratch);
    p.d.dst_kind = dst_kind; p.d.max_image_seg = 1;
    p.d.payload = payload; p.d.payload_bytes = payload_bytes; p.d.seg = segments; p.d.image_seg = image_seg; p.d.tables = tables;
    p.d.dst = dst; p.d.dst_stride = dst_stride; p.d.status = status; p.info = info;
    const unsigned chunks = gp_blocks((size_t)(payload_bytes / JPS_S + 1), JPS_C);          // of the longest scan the payload can hold
    GP_HIP_CHECK(hipMemsetAsync(p.d.coef, 0, (size_t)B * p.d.nblk * 64 * sizeof(int16_t), s));
    hipLaunchKernelGGL(jpgs_plan_kernel, dim3(1), dim3(JPS_C), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpgs_chunk_kernel, dim3(chunks, B), dim3(JPS_C), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpgs_cross_kernel, dim3(B), dim3(JPS_C), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpgs_count_kernel, dim3(chunks, B), dim3(JPS_C), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpgs_scan_kernel, dim3(B), dim3(JPS_C), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpgs_write_kernel, dim3(chunks, B), dim3(JPS_C), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpgs_status_kernel, dim3(B), dim3(JPS_C), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpgs_idct_kernel, dim3(gp_blocks((size_t)p.d.nblk, JPD_IDCT_BLOCKS), B), dim3(JPD_BLOCK), 0, s, p.d);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpgs_pixel_kernel, dim3(gp_blocks((size_t)W, JPD_BLOCK), H, B), dim3(JPD_BLOCK), 0, s, p.d);
    GP_LAUNCH_CHECK();
    return 0;
}
