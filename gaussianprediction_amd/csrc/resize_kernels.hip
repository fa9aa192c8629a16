// resize_kernels.hip -- Pillow-exact 8-bit resizing on the device (include/gp_resize.h).  The arithmetic is csrc/resize_core.h.
//   rs_fused_kernel        one workgroup of 256 lanes per tile of 64 x 32 output pixels of one plane (of all four planes with
//                          alpha_mode, alpha first): the tile's coefficients go to LDS, the horizontal pass of the source rows the tile
//                          needs goes to LDS as bytes, the vertical pass reads them there; the intermediate never reaches memory
//   rs_horizontal_kernel   one lane per output sample of a row: the only pass where the height stays, else the first of the two-launch
//                          path, writing the 8-bit intermediate to `scratch`
//   rs_vertical_kernel     one lane per output sample, consecutive lanes on consecutive columns: the only pass where the width stays,
//                          else the second of the two-launch path
//   rs_copy_kernel         equal sizes
// The programs themselves are csrc/resize_core.h, which also runs on a CPU (tests/resize_emulate.cpp).
// Every store is an ordinary vector store; nothing is atomic; no workgroup waits for another.
#include "gp_common.h"

#include "resize_core.h"

static_assert(RS_BLOCK % GP_RESIZE_TILE_W == 0, "a lane of the fused workgroup keeps its column");

__global__ void __launch_bounds__(RS_BLOCK) rs_copy_kernel(RsPlan p) {
    rs_copy_sample(p, (int)(blockIdx.x * RS_BLOCK + threadIdx.x), (int)blockIdx.y, (int)blockIdx.z);
}

__global__ void __launch_bounds__(RS_BLOCK) rs_horizontal_kernel(RsPlan p) {
    rs_horizontal_sample(p, (int)(blockIdx.x * RS_BLOCK + threadIdx.x), (int)blockIdx.y, (int)blockIdx.z);
}

__global__ void __launch_bounds__(RS_BLOCK) rs_vertical_kernel(RsPlan p) {
    rs_vertical_sample(p, (int)(blockIdx.x * RS_BLOCK + threadIdx.x), (int)blockIdx.y, (int)blockIdx.z);
}

__global__ void __launch_bounds__(RS_BLOCK) rs_fused_kernel(RsPlan p) {
    extern __shared__ int32_t rs_lds[];
    rs_fused_block(rs_lds, p, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
}

static int rs_check_sizes(const char* who, int64_t B, int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t filter, RsAxis& ax, RsAxis& ay) {
    if (B < 1) GP_FAIL("%s: B = %lld must be >= 1", who, (long long)B);
    if (C != 1 && C != 3 && C != 4) GP_FAIL("%s: C = %d is not 1, 3 or 4", who, C);
    if (B * C > 65535) GP_FAIL("%s: B * C = %lld above 65535 (the planes are one grid dimension)", who, (long long)B * C);
    if (H < 1 || W < 1 || Ho < 1 || Wo < 1) GP_FAIL("%s: sizes %d x %d -> %d x %d must all be >= 1", who, W, H, Wo, Ho);
    if (H > 65535 || W > 65535 || Ho > 65535 || Wo > 65535) GP_FAIL("%s: sizes %d x %d -> %d x %d must all be <= 65535", who, W, H, Wo, Ho);
    if (rs_support(filter) < 0.0) GP_FAIL("%s: filter = %d is not one of GP_RESIZE_LANCZOS .. GP_RESIZE_HAMMING", who, filter);
    if (rs_axis(ax, W, Wo, filter) || rs_axis(ay, H, Ho, filter)) GP_FAIL("%s: more than 2^24 taps per sample", who);
    return 0;
}

extern "C" int gp_resize_abi_version(void) { return GP_RESIZE_ABI_VERSION; }

static int rs_ksize_checked(int32_t in, int32_t out, int32_t filter, RsAxis& a) {
    if (in < 1 || out < 1) GP_FAIL("gp_resize: sizes in = %d, out = %d must be >= 1", in, out);
    if (rs_support(filter) < 0.0) GP_FAIL("gp_resize: filter = %d is not one of GP_RESIZE_LANCZOS .. GP_RESIZE_HAMMING", filter);
    if (rs_axis(a, in, out, filter)) GP_FAIL("gp_resize: %d -> %d has more than 2^24 taps per sample", in, out);
    return 0;
}

extern "C" int gp_resize_ksize(int32_t in, int32_t out, int32_t filter) {
    RsAxis a;
    return rs_ksize_checked(in, out, filter, a) ? -1 : a.ksize;
}

extern "C" int gp_resize_coeffs(int32_t in, int32_t out, int32_t filter, int32_t* bounds, int32_t* coeffs) {
    RsAxis a;
    if (rs_ksize_checked(in, out, filter, a)) return 1;
    if (!bounds || !coeffs) GP_FAIL("gp_resize_coeffs: null argument");
    double* w = (double*)malloc(sizeof(double) * (size_t)a.ksize);
    if (!w) GP_FAIL("gp_resize_coeffs: out of memory");
    rs_coeffs(a, bounds, coeffs, w);
    free(w);
    return 0;
}

extern "C" int gp_resize_path(int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t filter) {
    RsAxis ax, ay;
    if (rs_check_sizes("gp_resize_path", 1, 1, H, W, Ho, Wo, filter, ax, ay)) return -1;
    int rows;
    return rs_path(ax, ay, &rows);
}

extern "C" int64_t gp_resize_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t filter) {
    RsAxis ax, ay;
    if (rs_check_sizes("gp_resize_scratch_bytes", B, C, H, W, Ho, Wo, filter, ax, ay)) return -1;
    int rows;
    return rs_path(ax, ay, &rows) == GP_RESIZE_PATH_TWO_LAUNCH ? (int64_t)gp_align_up((size_t)B * C * H * Wo, 256) : 0;
}

extern "C" int gp_resize_u8(int32_t B, int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo, int32_t filter, const uint8_t* src,
                            int64_t src_stride, const int32_t* xbounds, const int32_t* xcoeffs, int32_t xtaps, const int32_t* ybounds,
                            const int32_t* ycoeffs, int32_t ytaps, int32_t alpha_mode, int32_t dst_kind, void* dst, int64_t dst_stride,
                            void* scratch, gp_stream_t stream_) {
    RsAxis ax, ay;
    if (rs_check_sizes("gp_resize_u8", B, C, H, W, Ho, Wo, filter, ax, ay)) return 1;
    if (alpha_mode != 0 && alpha_mode != 1) GP_FAIL("gp_resize_u8: alpha_mode = %d is neither 0 nor 1", alpha_mode);
    if (alpha_mode && C != 4) GP_FAIL("gp_resize_u8: alpha_mode needs C = 4 (got C = %d)", C);
    if (dst_kind != GP_RESIZE_DST_U8 && dst_kind != GP_RESIZE_DST_F32) GP_FAIL("gp_resize_u8: dst_kind = %d is neither GP_RESIZE_DST_U8 nor GP_RESIZE_DST_F32", dst_kind);
    const int64_t elem = dst_kind == GP_RESIZE_DST_F32 ? 4 : 1;
    if (src_stride < (int64_t)C * H * W) GP_FAIL("gp_resize_u8: src_stride = %lld below C * H * W = %lld", (long long)src_stride, (long long)C * H * W);
    if (dst_stride < elem * C * Ho * Wo) GP_FAIL("gp_resize_u8: dst_stride = %lld bytes below C * Ho * Wo = %lld elements", (long long)dst_stride, (long long)C * Ho * Wo);
    if (dst_kind == GP_RESIZE_DST_F32 && (dst_stride & 3)) GP_FAIL("gp_resize_u8: dst_stride = %lld bytes of a float32 dst must be a multiple of 4", (long long)dst_stride);
    int rows;
    const int path = rs_path(ax, ay, &rows);
    const bool horiz = W != Wo, vert = H != Ho;
    if (horiz && xtaps != ax.ksize) GP_FAIL("gp_resize_u8: xtaps = %d, but %d -> %d with this filter has %d", xtaps, W, Wo, ax.ksize);
    if (vert && ytaps != ay.ksize) GP_FAIL("gp_resize_u8: ytaps = %d, but %d -> %d with this filter has %d", ytaps, H, Ho, ay.ksize);
    if (!src || !dst || (horiz && (!xbounds || !xcoeffs)) || (vert && (!ybounds || !ycoeffs))) GP_FAIL("gp_resize_u8: null argument");
    if (path == GP_RESIZE_PATH_TWO_LAUNCH && !scratch) GP_FAIL("gp_resize_u8: null scratch on the two-launch path");
    if (((uintptr_t)xbounds | (uintptr_t)xcoeffs | (uintptr_t)ybounds | (uintptr_t)ycoeffs) & 3) GP_FAIL("gp_resize_u8: the tables must be 4-byte aligned");
    if (dst_kind == GP_RESIZE_DST_F32 && ((uintptr_t)dst & 3)) GP_FAIL("gp_resize_u8: a float32 dst must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream_;
    GpProfScope prof("resize", s);
    RsPlan p;
    p.B = B; p.C = C; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo;
    p.xtaps = horiz ? xtaps : 0; p.ytaps = vert ? ytaps : 0;
    p.alpha_mode = alpha_mode; p.dst_kind = dst_kind; p.path = path; p.rows = rows;
    p.src = src; p.src_stride = src_stride; p.xb = xbounds; p.xk = xcoeffs; p.yb = ybounds; p.yk = ycoeffs;
    p.dst = dst; p.dst_stride = dst_stride; p.mid = (uint8_t*)scratch;
    const unsigned planes = (unsigned)(B * C);
    switch (path) {
        case GP_RESIZE_PATH_COPY:
            hipLaunchKernelGGL(rs_copy_kernel, dim3(gp_blocks((size_t)W, RS_BLOCK), H, planes), dim3(RS_BLOCK), 0, s, p);
            break;
        case GP_RESIZE_PATH_FUSED:
            hipLaunchKernelGGL(rs_fused_kernel, dim3(gp_blocks((size_t)Wo, GP_RESIZE_TILE_W), gp_blocks((size_t)Ho, GP_RESIZE_TILE_H), alpha_mode ? (unsigned)B : planes),
                               dim3(RS_BLOCK), (size_t)rs_fused_lds(ax, ay, &rows), s, p);
            break;
        case GP_RESIZE_PATH_HORIZONTAL:
            hipLaunchKernelGGL(rs_horizontal_kernel, dim3(gp_blocks((size_t)Wo, RS_BLOCK), H, planes), dim3(RS_BLOCK), 0, s, p);
            break;
        case GP_RESIZE_PATH_TWO_LAUNCH:
            hipLaunchKernelGGL(rs_horizontal_kernel, dim3(gp_blocks((size_t)Wo, RS_BLOCK), H, planes), dim3(RS_BLOCK), 0, s, p);
            GP_LAUNCH_CHECK();
            hipLaunchKernelGGL(rs_vertical_kernel, dim3(gp_blocks((size_t)Wo, RS_BLOCK), Ho, planes), dim3(RS_BLOCK), 0, s, p);
            break;
        default:
            hipLaunchKernelGGL(rs_vertical_kernel, dim3(gp_blocks((size_t)Wo, RS_BLOCK), Ho, planes), dim3(RS_BLOCK), 0, s, p);
            break;
    }
    GP_LAUNCH_CHECK();
    return 0;
}
