// png_kernels.hip -- PNG encoding on the device (include/gp_png.h): four launches per call whatever the batch is.
//   1. png_filter_kernel   one workgroup per row: quantise, choose the row's filter, write the filtered stream
//   2. png_band_kernel     one workgroup per band of GP_PNG_BAND_BYTES: run tokens, histogram in LDS, the length-limited Huffman code
//                          and the block header by lane 0, the bits packed into LDS at prefix-summed offsets, the band's Adler sums
//   3. png_layout_kernel   one workgroup per image: the chunk offsets, the Adler-32, the file's length
//   4. png_chunk_kernel    one workgroup per band: the chunk in place, its CRC-32 from the lanes' slices (x^(8n) mod P)
// The workgroup programs themselves are csrc/png_core.h, which also runs on a CPU.  Every store is an ordinary vector store; the only
// atomics are integer adds / ors / xors on LDS, whose result does not depend on their order.
#include "gp_common.h"

#include "../../include/gp_png.h"
#include "png_core.h"

__global__ void __launch_bounds__(PNG_BLOCK) png_filter_kernel(PngPlan p) {
    __shared__ PngFilterShared sh;
    png_filter_block(sh, p, (int)blockIdx.y, (int)blockIdx.x);
}

__global__ void __launch_bounds__(PNG_BLOCK) png_band_kernel(PngPlan p) {
    __shared__ PngBandShared sh;
    png_band_block(sh, p, (int)blockIdx.y, (int)blockIdx.x);
}

__global__ void __launch_bounds__(PNG_BLOCK) png_layout_kernel(PngPlan p) {
    __shared__ PngLayoutShared sh;
    png_layout_block(sh, p, (int)blockIdx.x);
}

__global__ void __launch_bounds__(PNG_BLOCK) png_chunk_kernel(PngPlan p) {
    __shared__ PngChunkShared sh;
    png_chunk_block(sh, p, (int)blockIdx.y, (int)blockIdx.x);
}

static_assert(GP_PNG_BAND_BYTES >= 8192 && GP_PNG_BAND_BYTES % 256 == 0 && GP_PNG_BAND_BYTES < 65536, "a band is one stored block at worst");

// the stream itself, per band 5 bytes of stored-block header and 12 of chunk framing, the zlib header (2), the final block and the
// Adler-32 (9), signature and IHDR (33), IEND (12); a multiple of 8
static int64_t png_bound_of(int64_t S) {
    const int64_t nb = (S + PNG_BAND - 1) / PNG_BAND;
    return (S + 17 * nb + 2 + 9 + PNG_HEAD_BYTES + 12 + 7) / 8 * 8;
}

static int png_check_sizes(const char* who, int64_t B, int32_t H, int32_t W) {
    if (B < 1 || B > GP_PNG_MAX_BATCH) GP_FAIL("%s: B = %lld outside [1, %d]", who, (long long)B, GP_PNG_MAX_BATCH);
    if (H < 1) GP_FAIL("%s: H = %d must be >= 1", who, H);
    if (W < 1) GP_FAIL("%s: W = %d must be >= 1", who, W);
    // (the file's length is a 32-bit word that the host reads as an int32, and stream positions are ints)
    const int64_t S = (int64_t)H * (3 * (int64_t)W + 1);
    if (png_bound_of(S) >= ((int64_t)1 << 31))
        GP_FAIL("%s: H * (3 W + 1) = %lld: the largest file, %lld bytes, must stay below 2^31", who, (long long)S, (long long)png_bound_of(S));
    return 0;
}

// the sizes of a plan, and its arrays carved out of `scratch`
static size_t png_plan(PngPlan& p, int B, int H, int W, void* scratch) {
    p.B = B; p.H = H; p.W = W;
    p.row = 1 + 3 * W;
    p.S = (int64_t)H * p.row;
    p.S_pad = (int64_t)gp_align_up((size_t)p.S, 16);
    p.NB = (int)((p.S + PNG_BAND - 1) / PNG_BAND);
    GpCarver c(scratch);
    p.filt = c.take<uint8_t>((size_t)B * p.S_pad);
    p.comp = c.take<uint8_t>((size_t)B * p.NB * PNG_COMP_STRIDE);
    p.info = c.take<uint32_t>((size_t)B * p.NB * 4);
    p.chunk_off = c.take<uint32_t>((size_t)B * p.NB);
    p.adler = c.take<uint32_t>((size_t)B);
    return c.bytes();
}

extern "C" int gp_png_abi_version(void) { return GP_PNG_ABI_VERSION; }

extern "C" int64_t gp_png_bound(int32_t H, int32_t W) {
    if (png_check_sizes("gp_png_bound", 1, H, W)) return -1;
    return png_bound_of((int64_t)H * (3 * (int64_t)W + 1));
}

extern "C" int64_t gp_png_scratch_bytes(int32_t B, int32_t H, int32_t W) {
    if (png_check_sizes("gp_png_scratch_bytes", B, H, W)) return -1;
    PngPlan p;
    return (int64_t)png_plan(p, B, H, W, nullptr);
}

extern "C" int gp_png_encode(int32_t B, int32_t H, int32_t W, const void* src, int32_t src_kind, uint32_t flags, uint8_t* out,
                             int64_t out_stride, uint32_t* sizes, void* scratch, gp_stream_t stream_) {
    if (png_check_sizes("gp_png_encode", B, H, W)) return 1;
    if (src_kind != GP_PNG_SRC_F32 && src_kind != GP_PNG_SRC_U8) GP_FAIL("gp_png_encode: src_kind = %d is neither GP_PNG_SRC_F32 nor GP_PNG_SRC_U8", src_kind);
    if (flags & ~GP_PNG_FILTER_NONE) GP_FAIL("gp_png_encode: unknown flag bits 0x%x", flags);
    if (out_stride < gp_png_bound(H, W)) GP_FAIL("gp_png_encode: out_stride = %lld below gp_png_bound(%d, %d) = %lld", (long long)out_stride, H, W, (long long)gp_png_bound(H, W));
    if (!src || !out || !sizes || !scratch) GP_FAIL("gp_png_encode: null argument");
    if ((uintptr_t)scratch & 255) GP_FAIL("gp_png_encode: scratch must be 256-byte aligned");
    if (src_kind == GP_PNG_SRC_F32 && ((uintptr_t)src & 3)) GP_FAIL("gp_png_encode: a float32 src must be 4-byte aligned");
    if ((uintptr_t)sizes & 3) GP_FAIL("gp_png_encode: sizes must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("png_encode", s);
    PngPlan p;
    png_plan(p, B, H, W, scratch);
    p.flags = flags; p.src_kind = src_kind; p.src = src;
    p.out = out; p.out_stride = out_stride; p.sizes = sizes;
    hipLaunchKernelGGL(png_filter_kernel, dim3(H, B), dim3(PNG_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_band_kernel, dim3(p.NB, B), dim3(PNG_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_layout_kernel, dim3(B), dim3(PNG_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_chunk_kernel, dim3(p.NB, B), dim3(PNG_BLOCK), 0, s, p);
    GP_LAUNCH_CHECK();
    return 0;
}
