// lpips_kernels.hip -- LPIPS v0.1 with the AlexNet / VGG16 backbones (include/gp_lpips.h) [REF lpipsPyTorch/modules/*.py].
//   * prepare: both [3][H][W] images -> one NHWC buffer [2][H][W][3], z-scored (the first one quantised to 8 bits on request);
//   * ONE implicit-GEMM convolution kernel (+ bias + ReLU) on v_mfma_f32_32x32x2_f32 (exact float32: a k-ordered fmaf chain):
//     M = output pixels of render and gt together, N = Cout, K = k * k * Cin with Cin innermost (NHWC keeps it contiguous).
//     A BM x BN x 32 block (BM = 128, or 64 for layers of few output pixels; BN = 64 / 128), four waves in 2 x 2, each
//     (BM / 64) x (BN / 64) tiles of 32 x 32; the A tile is gathered (image borders, M and K tails zero-filled) and the weight tile
//     read while the previous tile's MFMAs run, both staged [row][k] in LDS (a second LDS buffer was measured: no gain at
//     128 x 128, and the 128 x 64 layers -- VGG's two largest -- lost a quarter to the halved occupancy) with a
//     36-float row so that a lane's 16 consecutive k (lane half h takes k = 16 h .. 16 h + 15 of the tile: the SAME permutation
//     of k for A and B) come in four ds_read_b128 free of bank conflicts;
//   * max-pool 3/2 and 2/2, floor mode, NHWC;
//   * distance: 16 / 32 / 64 lanes per pixel, both feature vectors in registers, the per-pixel value in float32, per-workgroup sums as
//     doubles in slots of their own; finalize adds the slots in a fixed order in double.  No atomics anywhere.
// The pairs of a batch are processed in turn with the geometry of one pair, so row b of a batched call is bit-identical to the
// call on pair b alone; every output element's sum runs in the same k order wherever its tile lies, so an identical pair gives
// identical features and a distance of exactly 0.
#include <math.h>

#include "../../include/gp_lpips.h"
#include "gp_common.h"

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

#define LP_BM 128
#define LP_BK 32
#define LP_SMALL_GRID 512            // at most this many 128-row workgroups (two per CU of a 256-CU device): take 64-row tiles
#define LP_LDK 36                // padded LDS row (floats): 16 rows x 144 B start in 16 different 16-B bank groups
#define LP_MAX_LAYERS 32
#define LP_MAX_CONVS 13
#define LP_DIST_REGS 2           // float4s per lane held in registers: C <= 512 on 64 lanes
#define LP_DIST_MAX_BLOCKS 2048

// ---- network tables ----------------------------------------------------------------------------
struct LpLayer { int kind, cin, cout, k, stride, pad, tap, conv; };
struct LpNet { int n; LpLayer l[LP_MAX_LAYERS]; int convs; };

static void lp_push(LpNet& t, int kind, int cin, int cout, int k, int stride, int pad, int tap) {
    LpLayer& e = t.l[t.n++];
    e.kind = kind; e.cin = cin; e.cout = cout; e.k = k; e.stride = stride; e.pad = pad; e.tap = tap;
    e.conv = kind == GP_LPIPS_CONV ? t.convs++ : -1;
}

static const LpNet* lp_net(int32_t net) {
    static LpNet alex, vgg;
    static bool built = [] {
        // torchvision alexnet().features; the five ReLU outputs are tapped, the last pool is never run
        const int a[5][5] = {{3, 64, 11, 4, 2}, {64, 192, 5, 1, 2}, {192, 384, 3, 1, 1}, {384, 256, 3, 1, 1}, {256, 256, 3, 1, 1}};
        alex.n = alex.convs = 0;
        for (int i = 0; i < 5; ++i) {
            lp_push(alex, GP_LPIPS_CONV, a[i][0], a[i][1], a[i][2], a[i][3], a[i][4], 0);
            lp_push(alex, GP_LPIPS_RELU, a[i][1], a[i][1], 0, 0, 0, 1);
            if (i == 0 || i == 1 || i == 4) lp_push(alex, GP_LPIPS_POOL, a[i][1], a[i][1], 3, 2, 0, 0);
        }
        // torchvision vgg16().features (configuration D); taps: the last ReLU of each of the five blocks
        const int d[5][2] = {{64, 2}, {128, 2}, {256, 3}, {512, 3}, {512, 3}};
        vgg.n = vgg.convs = 0;
        int c = 3;
        for (int b = 0; b < 5; ++b) {
            for (int i = 0; i < d[b][1]; ++i) {
                lp_push(vgg, GP_LPIPS_CONV, c, d[b][0], 3, 1, 1, 0);
                c = d[b][0];
                lp_push(vgg, GP_LPIPS_RELU, c, c, 0, 0, 0, i == d[b][1] - 1);
            }
            lp_push(vgg, GP_LPIPS_POOL, c, c, 2, 2, 0, 0);
        }
        return true;
    }();
    (void)built;
    return net == GP_LPIPS_ALEX ? &alex : net == GP_LPIPS_VGG ? &vgg : nullptr;
}

static int lp_check_net(const char* who, int32_t net) {
    if (net == GP_LPIPS_SQUEEZE) GP_FAIL("%s: net 'squeeze' is not provided (alex and vgg are)", who);
    if (!lp_net(net)) GP_FAIL("%s: unknown net %d (GP_LPIPS_ALEX = 0, GP_LPIPS_VGG = 1)", who, net);
    return 0;
}

// packed weights: per convolution [Cout][k][k][Cin] then [Cout] bias, then the five lin vectors; every array 256-B aligned
struct LpPacked { size_t w[LP_MAX_CONVS], b[LP_MAX_CONVS], lin[GP_LPIPS_TAPS]; int linc[GP_LPIPS_TAPS]; size_t floats; };

static void lp_packed_plan(const LpNet& t, LpPacked& p) {
    size_t off = 0;
    int taps = 0;
    for (int i = 0; i < t.n; ++i) {
        const LpLayer& e = t.l[i];
        if (e.kind == GP_LPIPS_CONV) {
            p.w[e.conv] = off; off = gp_align_up(off + (size_t)e.cout * e.k * e.k * e.cin, 64);
            p.b[e.conv] = off; off = gp_align_up(off + (size_t)e.cout, 64);
        }
        if (e.tap) p.linc[taps++] = e.cout;
    }
    for (int k = 0; k < GP_LPIPS_TAPS; ++k) { p.lin[k] = off; off = gp_align_up(off + (size_t)p.linc[k], 64); }
    p.floats = off;
}

// ---- prepare -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gp_lpips_prepare_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t HW,
                                                               int quantize, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * HW) return;
    const int img = i >= HW;
    const int64_t p = img ? i - HW : i;
    const float* src = img ? b : a;
    // the float32 values of the reference's buffers [REF networks.py:41-44]
    const float mean[3] = {-.030f, -.088f, -.188f}, sd[3] = {.458f, .448f, .450f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = src[c * HW + p];
        if (quantize && img == 0) {
            const float q = fminf(fmaxf(floorf(__fadd_rn(__fmul_rn(v, 255.f), 0.5f)), 0.f), 255.f);
            v = __fdiv_rn(q, 255.f);
        }
        out[i * 3 + c] = __fdiv_rn(__fsub_rn(v, mean[c]), sd[c]);
    }
}

// ---- weight repack: [Cout][Cin][k][k] -> [Cout][k][k][Cin] ------------------------------------------
__global__ __launch_bounds__(256) void gp_lpips_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int cin, int kk, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ci = (int)(i % cin);
    const int64_t r = i / cin;
    const int s = (int)(r % kk);
    const int64_t n = r / kk;
    out[i] = w[(n * cin + ci) * kk + s];
}

__global__ __launch_bounds__(256) void gp_lpips_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- convolution -----------------------------------------------------------------------------------
struct LpConv {
    const float* x; const float* w; const float* bias; float* y;
    int H, W, Cin, Cout, ks, stride, pad, Ho, Wo, M, K;
};

// VEC: Cin % 4 == 0 -- four consecutive k are four consecutive channels of one tap, 16-B aligned in x and in w.
template <int BM, int BN, bool VEC>
__global__ __launch_bounds__(256) void gp_lpips_conv_kernel(LpConv p) {
    constexpr int WM = BM / 2, TM = WM / 32, WN = BN / 2, TN = WN / 32, AU = BM / 32, BU = BN / 32;
    __shared__ __attribute__((aligned(16))) float As[BM * LP_LDK];
    __shared__ __attribute__((aligned(16))) float Bs[BN * LP_LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int m_blk = blockIdx.x * BM, n_blk = blockIdx.y * BN;
    const int kq = tid & 7, r0 = tid >> 3;      // this thread stages k = 4 kq .. 4 kq + 3 of rows r0, r0 + 32, ...
    const int HoWo = p.Ho * p.Wo;
    int iy0[AU], ix0[AU];
    int64_t xb[AU];
#pragma unroll
    for (int i = 0; i < AU; ++i) {
        const int m = m_blk + r0 + 32 * i;
        const bool mv = m < p.M;
        const int mm = mv ? m : 0;
        const int n = mm / HoWo, rem = mm - n * HoWo, oy = rem / p.Wo, ox = rem - oy * p.Wo;
        iy0[i] = mv ? oy * p.stride - p.pad : -(1 << 20);       // (a row past M fails every bounds test: zeros)
        ix0[i] = ox * p.stride - p.pad;
        xb[i] = (int64_t)n * p.H * p.W * p.Cin;
    }
    float4 ra[AU], rb[BU];

    auto load_tile = [&](int kt) {
        const int k = kt * LP_BK + 4 * kq;
        if (VEC) {
            const int tap = k / p.Cin, ci = k - tap * p.Cin, ky = tap / p.ks, kx = tap - ky * p.ks;
            const bool kv = k < p.K;
#pragma unroll
            for (int i = 0; i < AU; ++i) {
                const int iy = iy0[i] + ky, ix = ix0[i] + kx;
                const bool ok = kv && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
                const int64_t o = ok ? xb[i] + ((int64_t)iy * p.W + ix) * p.Cin + ci : 0;
                const float4 v = *reinterpret_cast<const float4*>(p.x + o);
                ra[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < BU; ++j) {
                const int n = n_blk + r0 + 32 * j;
                const bool ok = kv && n < p.Cout;
                const int64_t o = ok ? (int64_t)n * p.K + k : 0;
                const float4 v = *reinterpret_cast<const float4*>(p.w + o);
                rb[j] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
            float va[AU][4], vb[BU][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ke = k + e;
                const int tap = ke / p.Cin, ci = ke - tap * p.Cin, ky = tap / p.ks, kx = tap - ky * p.ks;
                const bool kv = ke < p.K;
#pragma unroll
                for (int i = 0; i < AU; ++i) {
                    const int iy = iy0[i] + ky, ix = ix0[i] + kx;
                    const bool ok = kv && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
                    const int64_t o = ok ? xb[i] + ((int64_t)iy * p.W + ix) * p.Cin + ci : 0;
                    const float v = p.x[o];
                    va[i][e] = ok ? v : 0.f;
                }
#pragma unroll
                for (int j = 0; j < BU; ++j) {
                    const int n = n_blk + r0 + 32 * j;
                    const bool ok = kv && n < p.Cout;
                    const int64_t o = ok ? (int64_t)n * p.K + ke : 0;
                    const float v = p.w[o];
                    vb[j][e] = ok ? v : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < AU; ++i) ra[i] = make_float4(va[i][0], va[i][1], va[i][2], va[i][3]);
#pragma unroll
            for (int j = 0; j < BU; ++j) rb[j] = make_float4(vb[j][0], vb[j][1], vb[j][2], vb[j][3]);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < AU; ++i) *reinterpret_cast<float4*>(&As[(r0 + 32 * i) * LP_LDK + 4 * kq]) = ra[i];
#pragma unroll
        for (int j = 0; j < BU; ++j) *reinterpret_cast<float4*>(&Bs[(r0 + 32 * j) * LP_LDK + 4 * kq]) = rb[j];
    };

    lp_f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        }
    }
    const int nk = (p.K + LP_BK - 1) / LP_BK;
    load_tile(0);
    store_tile();
    __syncthreads();
    const int l31 = lane & 31, h16 = (lane >> 5) * 16;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) load_tile(kt + 1);         // (in flight under this tile's MFMAs)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const float4*>(&As[(wm * WM + i * 32 + l31) * LP_LDK + h16 + 4 * q]);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const float4*>(&Bs[(wn * WN + j * 32 + l31) * LP_LDK + h16 + 4 * q]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const float a = e == 0 ? af[i].x : e == 1 ? af[i].y : e == 2 ? af[i].z : af[i].w;
                        const float b = e == 0 ? bf[j].x : e == 1 ? bf[j].y : e == 2 ? bf[j].z : bf[j].w;
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i][j], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
        if (kt + 1 < nk) {
            store_tile();
            __syncthreads();
        }
    }
    // C/D map of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n_blk + wn * WN + j * 32 + l31;
        if (n >= p.Cout) continue;
        const float bias = p.bias[n];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m_blk + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m < p.M) p.y[(int64_t)m * p.Cout + n] = fmaxf(acc[i][j][r] + bias, 0.f);
            }
        }
    }
}

// ---- max-pool ----------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T lp_max(T a, T b);
template <>
__device__ __forceinline__ float lp_max<float>(float a, float b) { return fmaxf(a, b); }
template <>
__device__ __forceinline__ float4 lp_max<float4>(float4 a, float4 b) {
    return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

// T = float4: C % 4 == 0, `C` counts float4s
template <typename T>
__global__ __launch_bounds__(256) void gp_lpips_pool_kernel(const T* __restrict__ x, T* __restrict__ y, int H, int W, int C, int Ho, int Wo,
                                                            int ks, int stride, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    int64_t r = i / C;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int64_t n = r / Ho;
    const T* src = x + ((n * H + (int64_t)oy * stride) * W + (int64_t)ox * stride) * C + c;
    T v = src[0];
    for (int ky = 0; ky < ks; ++ky)
        for (int kx = 0; kx < ks; ++kx) v = lp_max<T>(v, src[((int64_t)ky * W + kx) * C]);
    y[i] = v;
}

// ---- distance of one tapped layer ----------------------------------------------------------------------
// f: [2][P][C] (render's features, then gt's), C % 4 == 0.  LPP lanes per pixel (16 for C <= 64, 32 for C <= 128, else 64), each
// holding up to two float4 of both feature vectors in registers: a wave works on 64 / LPP pixels at a time.  Workgroup g owns pixels
// [g * per, (g + 1) * per), per a multiple of 16.  slots[g] = the workgroup's sum as a double.
template <int LPP>
__global__ __launch_bounds__(256) void gp_lpips_dist_kernel(const float* __restrict__ f, int64_t P, int C, const float* __restrict__ lw,
                                                            int64_t per, double* __restrict__ slots) {
    constexpr int PPW = 64 / LPP;
    __shared__ double s_w[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / LPP, sl = lane % LPP;
    const int C4 = C >> 2;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* lw4 = reinterpret_cast<const float4*>(lw);
    float4 w[LP_DIST_REGS];
#pragma unroll
    for (int r = 0; r < LP_DIST_REGS; ++r) w[r] = sl + LPP * r < C4 ? lw4[sl + LPP * r] : zero;
    const int64_t p0 = (int64_t)blockIdx.x * per, p1 = p0 + per < P ? p0 + per : P;
    double sum = 0.0;
    for (int64_t base = p0 + wave * PPW; base < p1; base += 4 * PPW) {
        const int64_t px = base + sub;
        const bool live = px < p1;
        const float4* fx = reinterpret_cast<const float4*>(f + (live ? px : p0) * C);
        const float4* fy = reinterpret_cast<const float4*>(f + (P + (live ? px : p0)) * C);
        float4 x[LP_DIST_REGS], y[LP_DIST_REGS];
#pragma unroll
        for (int r = 0; r < LP_DIST_REGS; ++r) {
            const int c = sl + LPP * r;
            const bool in = c < C4;
            x[r] = fx[in ? c : 0]; y[r] = fy[in ? c : 0];
            if (!in) { x[r] = zero; y[r] = zero; }
        }
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int r = 0; r < LP_DIST_REGS; ++r) {
            sx += (x[r].x * x[r].x + x[r].y * x[r].y) + (x[r].z * x[r].z + x[r].w * x[r].w);
            sy += (y[r].x * y[r].x + y[r].y * y[r].y) + (y[r].z * y[r].z + y[r].w * y[r].w);
        }
#pragma unroll
        for (int d = LPP / 2; d >= 1; d >>= 1) { sx += __shfl_xor(sx, d); sy += __shfl_xor(sy, d); }
        const float nx = sqrtf(sx) + 1e-10f, ny = sqrtf(sy) + 1e-10f;       // [REF utils.py:6-8]
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < LP_DIST_REGS; ++r) {
            const float d0 = x[r].x / nx - y[r].x / ny, d1 = x[r].y / nx - y[r].y / ny;
            const float d2 = x[r].z / nx - y[r].z / ny, d3 = x[r].w / nx - y[r].w / ny;
            s += (w[r].x * (d0 * d0) + w[r].y * (d1 * d1)) + (w[r].z * (d2 * d2) + w[r].w * (d3 * d3));
        }
#pragma unroll
        for (int d = LPP / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        sum += live ? (double)s : 0.0;        // (every lane of a pixel's group holds that pixel's value)
    }
#pragma unroll
    for (int d = 32; d >= LPP; d >>= 1) sum += __shfl_xor(sum, d);      // the wave's 64 / LPP pixel groups, a fixed tree
    if (lane == 0) s_w[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) slots[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// ---- finalize: one workgroup per pair ---------------------------------------------------------------------
struct LpFinalize {
    const double* slots[GP_LPIPS_TAPS];
    int n[GP_LPIPS_TAPS];
    double pixels[GP_LPIPS_TAPS];
    const uint32_t* invalid;        // this pair's word (or NULL)
    double* out;                    // this pair's row
};

__global__ __launch_bounds__(256) void gp_lpips_finalize_kernel(LpFinalize f) {
    __shared__ double s_t[GP_LPIPS_TAPS][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int l = 0; l < GP_LPIPS_TAPS; ++l) {
        double a = 0.0;
        for (int k = tid; k < f.n[l]; k += 256) a += f.slots[l][k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor(a, d);
        if (lane == 0) s_t[l][wave] = a;
    }
    __syncthreads();
    if (tid != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const bool bad = f.invalid && f.invalid[0] != 0u;
    double total = 0.0;
#pragma unroll
    for (int l = 0; l < GP_LPIPS_TAPS; ++l) {
        const double t = ((s_t[l][0] + s_t[l][1]) + (s_t[l][2] + s_t[l][3])) / f.pixels[l];
        total += t;
        f.out[1 + l] = bad ? nan : t;
    }
    f.out[0] = bad ? nan : total;
    f.out[6] = bad ? nan : 0.0;
    f.out[7] = bad ? nan : 0.0;
}

// ------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------
static inline int lp_out(int n, int k, int stride, int pad) { return (n + 2 * pad - k) / stride + 1; }

static int lp_launch_conv(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int ks,
                          int stride, int pad, hipStream_t s) {
    LpConv p;
    p.x = x; p.w = w_packed; p.bias = bias; p.y = y;
    p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.ks = ks; p.stride = stride; p.pad = pad;
    p.Ho = lp_out(H, ks, stride, pad); p.Wo = lp_out(W, ks, stride, pad);
    const int64_t M = (int64_t)N * p.Ho * p.Wo, K = (int64_t)ks * ks * Cin;
    if (p.Ho <= 0 || p.Wo <= 0) GP_FAIL("gp_lpips conv: empty output (H=%d W=%d k=%d stride=%d pad=%d)", H, W, ks, stride, pad);
    if (M > INT32_MAX - LP_BM || K > INT32_MAX - LP_BK) GP_FAIL("gp_lpips conv: more than 2^31 output pixels or k * k * Cin");
    p.M = (int)M; p.K = (int)K;
    const bool vec = Cin % 4 == 0;
    const int bn = Cout <= 64 ? 64 : 128;
    const int64_t ntiles = (Cout + bn - 1) / bn;
    // 64-row tiles where 128-row ones would leave CUs idle (the deep, small layers: a few thousand output pixels).  A shape decides,
    // never the device, and the k order of every output element is the same in all variants: the results do not depend on it.
    const int bm = ((M + LP_BM - 1) / LP_BM) * ntiles <= LP_SMALL_GRID ? 64 : LP_BM;
    const dim3 grid((unsigned)((M + bm - 1) / bm), (unsigned)ntiles);
    if (grid.y > 65535) GP_FAIL("gp_lpips conv: Cout %d too large", Cout);
    GpProfScope _p("lpips_conv", s);
#define LP_CONV_LAUNCH(BM_, BN_)                                                                                   \
    do {                                                                                                           \
        if (vec) hipLaunchKernelGGL((gp_lpips_conv_kernel<BM_, BN_, true>), grid, dim3(256), 0, s, p);             \
        else hipLaunchKernelGGL((gp_lpips_conv_kernel<BM_, BN_, false>), grid, dim3(256), 0, s, p);                \
    } while (0)
    if (bm == 64 && bn == 64) LP_CONV_LAUNCH(64, 64);
    else if (bm == 64) LP_CONV_LAUNCH(64, 128);
    else if (bn == 64) LP_CONV_LAUNCH(128, 64);
    else LP_CONV_LAUNCH(128, 128);
#undef LP_CONV_LAUNCH
    GP_LAUNCH_CHECK();
    return 0;
}

static int lp_launch_pool(const float* x, float* y, int N, int H, int W, int C, int ks, int stride, hipStream_t s) {
    const int Ho = lp_out(H, ks, stride, 0), Wo = lp_out(W, ks, stride, 0);
    if (H < ks || W < ks) GP_FAIL("gp_lpips pool: empty output (H=%d W=%d k=%d)", H, W, ks);
    GpProfScope _p("lpips_pool", s);
    if (C % 4 == 0) {
        const int64_t total = (int64_t)N * Ho * Wo * (C / 4);
        if ((total + 255) / 256 > INT32_MAX) GP_FAIL("gp_lpips pool: too many elements");
        hipLaunchKernelGGL(gp_lpips_pool_kernel<float4>, dim3(gp_blocks((size_t)total, 256)), dim3(256), 0, s, (const float4*)x, (float4*)y, H, W,
                           C / 4, Ho, Wo, ks, stride, total);
    } else {
        const int64_t total = (int64_t)N * Ho * Wo * C;
        if ((total + 255) / 256 > INT32_MAX) GP_FAIL("gp_lpips pool: too many elements");
        hipLaunchKernelGGL(gp_lpips_pool_kernel<float>, dim3(gp_blocks((size_t)total, 256)), dim3(256), 0, s, x, y, H, W, C, Ho, Wo, ks, stride, total);
    }
    GP_LAUNCH_CHECK();
    return 0;
}

static int lp_launch_pack(const float* w, float* out, int Cin, int Cout, int ks, hipStream_t s) {
    const int64_t total = (int64_t)Cout * ks * ks * Cin;
    hipLaunchKernelGGL(gp_lpips_pack_kernel, dim3(gp_blocks((size_t)total, 256)), dim3(256), 0, s, w, out, Cin, ks * ks, total);
    GP_LAUNCH_CHECK();
    return 0;
}

// the walk over one net at one size: activation sizes, the largest one, the slots per tap
struct LpPlan {
    size_t act_floats;                      // each of the two activation buffers
    int dist_blocks[GP_LPIPS_TAPS];
    int64_t dist_per[GP_LPIPS_TAPS], pixels[GP_LPIPS_TAPS];
    size_t bytes;
    float* act[2];
    double* slots[GP_LPIPS_TAPS];
};

static int lp_plan(const LpNet& t, int32_t net, int32_t B, int32_t H, int32_t W, void* scratch, LpPlan& pl) {
    if (B <= 0 || H <= 0 || W <= 0) GP_FAIL("gp_lpips: B, H, W must be positive (got B=%d H=%d W=%d)", B, H, W);
    const int lim = net == GP_LPIPS_ALEX ? 31 : 16;
    if ((H < W ? H : W) < lim)
        GP_FAIL("gp_lpips: the %s feature maps are empty below min(H, W) = %d (got H=%d W=%d)", net == GP_LPIPS_ALEX ? "alex" : "vgg", lim, H, W);
    int h = H, w = W, taps = 0;
    size_t big = (size_t)2 * H * W * 3;
    for (int i = 0; i < t.n && taps < GP_LPIPS_TAPS; ++i) {
        const LpLayer& e = t.l[i];
        if (e.kind == GP_LPIPS_CONV || e.kind == GP_LPIPS_POOL) {
            h = lp_out(h, e.k, e.stride, e.pad); w = lp_out(w, e.k, e.stride, e.pad);
            if (h <= 0 || w <= 0) GP_FAIL("gp_lpips: an empty feature map at layer %d (H=%d W=%d)", i, H, W);
            const size_t n = (size_t)2 * h * w * e.cout;
            if (n > big) big = n;
            if ((int64_t)2 * h * w > INT32_MAX - LP_BM) GP_FAIL("gp_lpips: H=%d W=%d is too large", H, W);
        } else if (e.tap) {
            if (e.cout > 256 * LP_DIST_REGS || e.cout % 4) GP_FAIL("gp_lpips: a tapped layer of %d channels (a multiple of 4, at most %d)", e.cout, 256 * LP_DIST_REGS);
            const int64_t P = (int64_t)h * w;
            int64_t per = (P + LP_DIST_MAX_BLOCKS - 1) / LP_DIST_MAX_BLOCKS;
            per = (per + 15) / 16 * 16;             // (whole rounds of the four waves at up to four pixels each)
            pl.pixels[taps] = P; pl.dist_per[taps] = per; pl.dist_blocks[taps] = (int)((P + per - 1) / per);
            ++taps;
        }
    }
    pl.act_floats = big;
    GpCarver c(scratch);
    pl.act[0] = c.take<float>(big);
    pl.act[1] = c.take<float>(big);
    for (int k = 0; k < GP_LPIPS_TAPS; ++k) pl.slots[k] = c.take<double>(pl.dist_blocks[k]);
    pl.bytes = c.bytes();
    return 0;
}

extern "C" int gp_lpips_abi_version(void) { return GP_LPIPS_ABI_VERSION; }

extern "C" int gp_lpips_num_layers(int32_t net) {
    if (lp_check_net("gp_lpips_num_layers", net)) return -1;
    return lp_net(net)->n;
}

extern "C" int gp_lpips_layer(int32_t net, int32_t index, int32_t* desc) {
    if (lp_check_net("gp_lpips_layer", net)) return 1;
    const LpNet& t = *lp_net(net);
    if (!desc || index < 0 || index >= t.n) GP_FAIL("gp_lpips_layer: index %d outside [0, %d) or a null desc", index, t.n);
    const LpLayer& e = t.l[index];
    const int32_t d[8] = {e.kind, e.cin, e.cout, e.k, e.stride, e.pad, e.tap, e.conv};
    memcpy(desc, d, sizeof(d));
    return 0;
}

extern "C" int64_t gp_lpips_weight_floats(int32_t net) {
    if (lp_check_net("gp_lpips_weight_floats", net)) return -1;
    LpPacked p;
    lp_packed_plan(*lp_net(net), p);
    return (int64_t)p.floats;
}

extern "C" int gp_lpips_pack_weights(int32_t net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, float* packed,
                                     gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (lp_check_net("gp_lpips_pack_weights", net)) return 1;
    if (!conv_w || !conv_b || !lin_w || !packed) GP_FAIL("gp_lpips_pack_weights: null argument");
    const LpNet& t = *lp_net(net);
    LpPacked p;
    lp_packed_plan(t, p);
    for (int i = 0; i < t.n; ++i) {
        const LpLayer& e = t.l[i];
        if (e.kind != GP_LPIPS_CONV) continue;
        if (!conv_w[e.conv] || !conv_b[e.conv]) GP_FAIL("gp_lpips_pack_weights: convolution %d has a null weight or bias", e.conv);
        if (lp_launch_pack(conv_w[e.conv], packed + p.w[e.conv], e.cin, e.cout, e.k, s)) return 1;
        hipLaunchKernelGGL(gp_lpips_copy_kernel, dim3(gp_blocks(e.cout, 256)), dim3(256), 0, s, conv_b[e.conv], packed + p.b[e.conv], e.cout);
        GP_LAUNCH_CHECK();
    }
    for (int k = 0; k < GP_LPIPS_TAPS; ++k) {
        if (!lin_w[k]) GP_FAIL("gp_lpips_pack_weights: lin %d is null", k);
        hipLaunchKernelGGL(gp_lpips_copy_kernel, dim3(gp_blocks(p.linc[k], 256)), dim3(256), 0, s, lin_w[k], packed + p.lin[k], p.linc[k]);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int64_t gp_lpips_scratch_bytes(int32_t net, int32_t B, int32_t H, int32_t W) {
    if (lp_check_net("gp_lpips_scratch_bytes", net)) return -1;
    LpPlan pl;
    if (lp_plan(*lp_net(net), net, B, H, W, nullptr, pl)) return -1;
    return (int64_t)pl.bytes;
}

extern "C" int gp_lpips(int32_t net, const float* packed, const float* a, const float* b, int32_t B, int32_t H, int32_t W, uint32_t flags,
                        void* scratch, const uint32_t* invalid_flag, double* out, gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (lp_check_net("gp_lpips", net)) return 1;
    if (!packed || !a || !b || !scratch || !out) GP_FAIL("gp_lpips: null argument");
    if (flags & ~GP_LPIPS_QUANTIZE8) GP_FAIL("gp_lpips: unknown flag bits 0x%x", flags);
    if (((uintptr_t)scratch & 255) != 0) GP_FAIL("gp_lpips: scratch must be 256-byte aligned");
    const LpNet& t = *lp_net(net);
    LpPlan pl;
    if (lp_plan(t, net, B, H, W, scratch, pl)) return 1;
    LpPacked pk;
    lp_packed_plan(t, pk);
    const int64_t HW = (int64_t)H * W;
    for (int32_t img = 0; img < B; ++img) {
        int cur = 0, h = H, w = W, taps = 0;
        {
            GpProfScope _p("lpips_prepare", s);
            hipLaunchKernelGGL(gp_lpips_prepare_kernel, dim3(gp_blocks((size_t)(2 * HW), 256)), dim3(256), 0, s, a + (size_t)img * 3 * HW,
                               b + (size_t)img * 3 * HW, HW, (int)(flags & GP_LPIPS_QUANTIZE8), pl.act[0]);
            GP_LAUNCH_CHECK();
        }
        LpFinalize f;
        memset(&f, 0, sizeof(f));
        for (int i = 0; i < t.n && taps < GP_LPIPS_TAPS; ++i) {
            const LpLayer& e = t.l[i];
            if (e.kind == GP_LPIPS_CONV) {      // (+ the ReLU that follows every convolution of both nets)
                if (lp_launch_conv(pl.act[cur], packed + pk.w[e.conv], packed + pk.b[e.conv], pl.act[cur ^ 1], 2, h, w, e.cin, e.cout, e.k, e.stride,
                                   e.pad, s))
                    return 1;
                h = lp_out(h, e.k, e.stride, e.pad); w = lp_out(w, e.k, e.stride, e.pad);
                cur ^= 1;
            } else if (e.kind == GP_LPIPS_POOL) {
                if (lp_launch_pool(pl.act[cur], pl.act[cur ^ 1], 2, h, w, e.cout, e.k, e.stride, s)) return 1;
                h = lp_out(h, e.k, e.stride, 0); w = lp_out(w, e.k, e.stride, 0);
                cur ^= 1;
            } else if (e.tap) {
                GpProfScope _p("lpips_dist", s);
                auto kernel = e.cout <= 64 ? gp_lpips_dist_kernel<16> : e.cout <= 128 ? gp_lpips_dist_kernel<32> : gp_lpips_dist_kernel<64>;
                hipLaunchKernelGGL(kernel, dim3(pl.dist_blocks[taps]), dim3(256), 0, s, pl.act[cur], pl.pixels[taps], e.cout,
                                   packed + pk.lin[taps], pl.dist_per[taps], pl.slots[taps]);
                GP_LAUNCH_CHECK();
                f.slots[taps] = pl.slots[taps]; f.n[taps] = pl.dist_blocks[taps]; f.pixels[taps] = (double)pl.pixels[taps];
                ++taps;
            }
        }
        f.invalid = invalid_flag ? invalid_flag + img : nullptr;
        f.out = out + (size_t)img * GP_LPIPS_COLUMNS;
        GpProfScope _p("lpips_finalize", s);
        hipLaunchKernelGGL(gp_lpips_finalize_kernel, dim3(1), dim3(256), 0, s, f);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gp_lpips_conv2d_relu(const float* x, const float* w, const float* bias, float* w_packed, float* y, int32_t N, int32_t H, int32_t W,
                                    int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride, int32_t pad, gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (!x || !w || !bias || !w_packed || !y) GP_FAIL("gp_lpips_conv2d_relu: null argument");
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || ksize <= 0 || stride <= 0 || pad < 0)
        GP_FAIL("gp_lpips_conv2d_relu: N, H, W, Cin, Cout, ksize, stride must be positive and pad >= 0");
    if ((int64_t)N * H * W * Cin > ((int64_t)1 << 40)) GP_FAIL("gp_lpips_conv2d_relu: input too large");
    if (lp_out(H, ksize, stride, pad) <= 0 || lp_out(W, ksize, stride, pad) <= 0)       // (before the repack writes anything)
        GP_FAIL("gp_lpips_conv2d_relu: empty output (H=%d W=%d k=%d stride=%d pad=%d)", H, W, ksize, stride, pad);
    if ((int64_t)N * lp_out(H, ksize, stride, pad) * lp_out(W, ksize, stride, pad) > INT32_MAX - LP_BM || (int64_t)ksize * ksize * Cin > INT32_MAX - LP_BK)
        GP_FAIL("gp_lpips_conv2d_relu: more than 2^31 output pixels or k * k * Cin");
    if (lp_launch_pack(w, w_packed, Cin, Cout, ksize, s)) return 1;
    return lp_launch_conv(x, w_packed, bias, y, N, H, W, Cin, Cout, ksize, stride, pad, s);
}

extern "C" int gp_lpips_maxpool(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ksize, int32_t stride,
                                gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (!x || !y) GP_FAIL("gp_lpips_maxpool: null argument");
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || ksize <= 0 || stride <= 0) GP_FAIL("gp_lpips_maxpool: N, H, W, C, ksize, stride must be positive");
    return lp_launch_pool(x, y, N, H, W, C, ksize, stride, s);
}
