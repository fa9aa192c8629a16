// metric_kernels.hip -- the evaluation metrics of a rendered view against its ground truth, on the device and in one call:
// L1, MSE, PSNR in both call shapes of the reference, SSIM [REF utils/loss_utils.py:54-98, utils/image_utils.py:18-20,
// metrics.py:138-147, train.py:107,252-282] and the five-scale MS-SSIM of pytorch_msssim (absent here: parity is unpinned, the
// definition is restated in include/gp_hip.h and tests/metrics_ref.py).
//   * one launch per pyramid level; a workgroup = one 32x32 tile of one (image, channel): the tile and its 5-pixel zero halo staged
//     in LDS once, the separable 11-tap filter over the four maps a, b, a^2 + b^2, a b (the loss kernel's form,
//     loss_adam_kernels.hip), and the 2x2 average-pooled next level of both images written from the same staging;
//   * the valid-convolution maps of MS-SSIM are the interior (5 <= y < h-5, 5 <= x < w-5) of the zero-padded maps, so level 0
//     yields the sums of |d|, d^2, SSIM over all pixels (the reference's SSIM) and of cs, ssim over the interior in one pass;
//   * per-workgroup sums leave as doubles with plain stores into slots of their own; one finalize workgroup per image adds them
//     in a fixed order and forms the output row in double (ReLU before the fractional powers).  No atomics: bit-reproducible,
//     and a batched call's row b is the B = 1 call's row.
#include <math.h>

#include "gp_common.h"

#define MT 32              // output tile edge
#define MH 5               // window half width
#define ME (MT + 2 * MH)   // staged tile edge (42)
#define MP (ME + 1)        // padded LDS row
#define MHP (MT + 1)       // padded row of the horizontally filtered maps
#define M_LEVELS 5
#define M_SUMS0 5          // level 0 slot: sum |d|, sum d^2, sum ssim (all pixels), sum cs, sum ssim (interior)
#define M_SUMSN 2          // levels 1-4 slot: sum cs, sum ssim (interior)

struct MWin11 { float w[11]; };

struct MetricLevel {
    const float* a; const float* b;     // [planes][h][w]
    int h, w;
    float* na; float* nb;               // the pooled next level [planes][nh][nw] (NULL: none)
    int nh, nw, py, px;                 // its size and leading pad (h % 2, w % 2)
    double* sums;                       // [planes][tiles][M_SUMS0 | M_SUMSN]
    uint32_t flags;                     // GP_METRICS_QUANTIZE8 | GP_METRICS_CLAMP01 (level 0 only)
    uint8_t* quant_out;                 // [B][3][h][w]
    uint8_t* deltas_out;                // [B][h][w][3]
};

// K per-thread partial sums -> the workgroup's totals as doubles in out[0..K) (thread 0 stores).  float32 tree: six xor steps in
// the wave, then the four wave sums.
template <int K>
__device__ __forceinline__ void metric_block_sums(float (&v)[K], float (*s_red)[4], double* __restrict__ out) {
#pragma unroll
    for (int q = 0; q < K; ++q) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_xor(v[q], d);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q) s_red[q][wave] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q) out[q] = (double)((s_red[q][0] + s_red[q][1]) + (s_red[q][2] + s_red[q][3]));
    }
}

template <bool L0>
__global__ __launch_bounds__(256) void gp_metric_level_kernel(MetricLevel L, MWin11 win) {
    __shared__ float s_a[ME][MP], s_b[ME][MP];
    __shared__ float s_h[4][ME][MHP];
    __shared__ float s_red[M_SUMS0][4];
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * MT, ty0 = blockIdx.y * MT, plane = blockIdx.z;
    const int H = L.h, W = L.w;
    const size_t HW = (size_t)H * W;
    const float* a_img = L.a + plane * HW;
    const float* b_img = L.b + plane * HW;
    {   // halo staging: every load in flight before the first LDS store (clamped addresses, selected afterwards)
        constexpr int NST = (ME * ME + 255) / 256;
        float va[NST], vb[NST];
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int i = tid + 256 * u, y = i / ME, x = i - y * ME;
            const int gy = ty0 - MH + y, gx = tx0 - MH + x;
            const bool in = i < ME * ME && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const size_t o = in ? (size_t)gy * W + gx : 0;
            va[u] = a_img[o]; vb[u] = b_img[o];
        }
#pragma unroll
        for (int u = 0; u < NST; ++u) {
            const int i = tid + 256 * u, y = i / ME, x = i - y * ME;
            const int gy = ty0 - MH + y, gx = tx0 - MH + x;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
            float a = va[u], b = vb[u];
            if (L0) {
                if (L.flags & GP_METRICS_CLAMP01) { a = fminf(fmaxf(a, 0.f), 1.f); b = fminf(fmaxf(b, 0.f), 1.f); }
                if (L.flags & GP_METRICS_QUANTIZE8) {
                    // one multiply, one add (no FMA), floor, clamp: the byte an 8-bit image file holds; back to [0, 1] by a division
                    const float q = fminf(fmaxf(floorf(__fadd_rn(__fmul_rn(a, 255.f), 0.5f)), 0.f), 255.f);
                    a = __fdiv_rn(q, 255.f);
                    // (the pixel's own tile writes the byte)
                    if (L.quant_out && in && i < ME * ME && y >= MH && y < MH + MT && x >= MH && x < MH + MT)
                        L.quant_out[plane * HW + (size_t)gy * W + gx] = (uint8_t)q;
                }
            }
            if (i < ME * ME) { s_a[y][x] = in ? a : 0.f; s_b[y][x] = in ? b : 0.f; }
        }
    }
    __syncthreads();
    if (L.na) {
        // the next level: output i covers inputs 2i - p and 2i - p + 1 (p = size % 2, the leading pad; inputs outside the image are
        // the staged zeros, the divisor is always 4).  The tile holding input 2i writes output i: 16 x 16 per workgroup.
        const int ox = tid & 15, oy = tid >> 4;
        const int i = (tx0 >> 1) + ox, j = (ty0 >> 1) + oy;
        if (i < L.nw && j < L.nh) {
            const int x = 2 * ox - L.px + MH, y = 2 * oy - L.py + MH;
            const size_t o = (size_t)plane * L.nh * L.nw + (size_t)j * L.nw + i;
            L.na[o] = ((s_a[y][x] + s_a[y][x + 1]) + (s_a[y + 1][x] + s_a[y + 1][x + 1])) * 0.25f;
            L.nb[o] = ((s_b[y][x] + s_b[y][x + 1]) + (s_b[y + 1][x] + s_b[y + 1][x + 1])) * 0.25f;
        }
    }
    // horizontal pass: a thread owns 8 consecutive outputs of one staged row (a sliding window in registers)
    if (tid < ME * 4) {
        const int y = tid >> 2, x0 = (tid & 3) * 8;
        float a[18], b[18], s2[18], ab[18];
#pragma unroll
        for (int j = 0; j < 18; ++j) {
            a[j] = s_a[y][x0 + j]; b[j] = s_b[y][x0 + j];
            s2[j] = a[j] * a[j] + b[j] * b[j]; ab[j] = a[j] * b[j];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float m1 = 0.f, m2 = 0.f, ss2 = 0.f, sab = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float w = win.w[k];
                m1 = fmaf(w, a[e + k], m1); m2 = fmaf(w, b[e + k], m2);
                ss2 = fmaf(w, s2[e + k], ss2); sab = fmaf(w, ab[e + k], sab);
            }
            s_h[0][y][x0 + e] = m1; s_h[1][y][x0 + e] = m2; s_h[2][y][x0 + e] = ss2; s_h[3][y][x0 + e] = sab;
        }
    }
    __syncthreads();
    // vertical pass: a thread owns 4 consecutive outputs of one column
    float acc[M_SUMS0] = {0.f, 0.f, 0.f, 0.f, 0.f};      // |d|, d^2, ssim (all), cs, ssim (interior)
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    {
        const int x = tid & 31, y0 = (tid >> 5) * 4;
        float o[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v[14];
#pragma unroll
            for (int j = 0; j < 14; ++j) v[j] = s_h[q][y0 + j][x];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) t = fmaf(win.w[k], v[e + k], t);
                o[q][e] = t;
            }
        }
        const int gx = tx0 + x;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int y = y0 + e, gy = ty0 + y;
            if (gy >= H || gx >= W) continue;
            const float mu1 = o[0][e], mu2 = o[1][e], s2f = o[2][e], ab = o[3][e];
            const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
            const float s12 = ab - mu12;
            const float N1 = 2.f * mu12 + C1, N2 = 2.f * s12 + C2, D1 = mu1s + mu2s + C1, D2 = ((s2f - mu1s) - mu2s) + C2;
            const float cs = N2 / D2;
            const float ssim = (N1 / D1) * cs;
            if (gy >= MH && gy < H - MH && gx >= MH && gx < W - MH) { acc[3] += cs; acc[4] += ssim; }
            if (L0) {
                const float d = s_a[y + MH][x + MH] - s_b[y + MH][x + MH];
                const float ad = fabsf(d);
                acc[0] += ad; acc[1] += d * d; acc[2] += ssim;
                if (L.deltas_out) {
                    const int ch = plane % 3, img = plane / 3;
                    L.deltas_out[((size_t)img * HW + (size_t)gy * W + gx) * 3 + ch] = (uint8_t)fminf(ad * 255.f, 255.f);
                }
            }
        }
    }
    const size_t slot = (size_t)plane * (gridDim.x * gridDim.y) + blockIdx.y * gridDim.x + blockIdx.x;
    if (L0) {
        metric_block_sums<M_SUMS0>(acc, s_red, L.sums + slot * M_SUMS0);
    } else {
        float two[M_SUMSN] = {acc[3], acc[4]};
        metric_block_sums<M_SUMSN>(two, s_red, L.sums + slot * M_SUMSN);
    }
}

// ---- finalize: one workgroup per image ----------------------------------------------------------
struct MetricFinalize {
    const double* sums[M_LEVELS];       // per level [planes][tiles][K]
    int tiles[M_LEVELS];
    double n_all;                       // H * W
    double n_in[M_LEVELS];              // (h - 10) * (w - 10) per level
    int levels;                         // 1 (no MS-SSIM) or 5
    const uint32_t* invalid;
    double* out;                        // [B][GP_METRIC_COUNT]
    double* levels_out;                 // [B][5][3] or NULL
};

// One workgroup per image, ONE exchange through LDS: all 256 threads walk the level-0 slots of the three channels together (thread
// t: slots t, t + 256, ..., two per trip to memory and channel), then wave w walks the slots of level w + 1 on its own (lane l:
// slots l, l + 64, ...) -- xor butterflies in the waves, the level-0 wave sums through LDS.  Fixed order throughout; every slot
// total is needed by one thread only, so block-wide reductions one per quantity (a dependent trip to memory and two barriers each)
// are avoided.
__global__ __launch_bounds__(256) void gp_metric_finalize_kernel(MetricFinalize f) {
    __shared__ double s_l0[3][M_SUMS0][4];
    __shared__ double s_lv[M_LEVELS - 1][3][M_SUMSN];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double a0[3][M_SUMS0], al[3][M_SUMSN];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int q = 0; q < M_SUMS0; ++q) a0[c][q] = 0.0;
        al[c][0] = al[c][1] = 0.0;
    }
    {
        const int n = f.tiles[0];
        const double* __restrict__ base = f.sums[0] + (size_t)img * 3 * n * M_SUMS0;
        for (int k0 = tid; k0 < n; k0 += 256 * 2) {
            double v[2][3][M_SUMS0];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int k = k0 + 256 * u, kc = k < n ? k : n - 1;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double* p = base + ((size_t)c * n + kc) * M_SUMS0;
#pragma unroll
                    for (int q = 0; q < M_SUMS0; ++q) v[u][c][q] = p[q];
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (k0 + 256 * u < n) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
#pragma unroll
                        for (int q = 0; q < M_SUMS0; ++q) a0[c][q] += v[u][c][q];
                    }
                }
        }
    }
    if (f.levels == M_LEVELS) {
        const int l = wave + 1, n = f.tiles[l];
        const double2* __restrict__ base = reinterpret_cast<const double2*>(f.sums[l]) + (size_t)img * 3 * n;
        for (int k0 = lane; k0 < n; k0 += 64 * 4) {
            double2 v[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + 64 * u, kc = k < n ? k : n - 1;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[u][c] = base[(size_t)c * n + kc];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (k0 + 64 * u < n) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) { al[c][0] += v[u][c].x; al[c][1] += v[u][c].y; }
                }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int q = 0; q < M_SUMS0; ++q) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) a0[c][q] += __shfl_xor(a0[c][q], d);
        }
#pragma unroll
        for (int q = 0; q < M_SUMSN; ++q) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) al[c][q] += __shfl_xor(al[c][q], d);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int q = 0; q < M_SUMS0; ++q) s_l0[c][q][wave] = a0[c][q];
            s_lv[wave][c][0] = al[c][0]; s_lv[wave][c][1] = al[c][1];
        }
    }
    __syncthreads();
    if (tid != 0) return;
    double l1 = 0.0, d2 = 0.0, ss = 0.0, psnr_ch = 0.0, ms = 0.0;
    double term[M_LEVELS][3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double t0[M_SUMS0];
#pragma unroll
        for (int q = 0; q < M_SUMS0; ++q) t0[q] = (s_l0[ch][q][0] + s_l0[ch][q][1]) + (s_l0[ch][q][2] + s_l0[ch][q][3]);
        l1 += t0[0]; d2 += t0[1]; ss += t0[2];
        psnr_ch += 20.0 * log10(1.0 / sqrt(t0[1] / f.n_all));
        term[0][ch] = t0[3] / f.n_in[0];
#pragma unroll
        for (int l = 1; l < M_LEVELS; ++l) term[l][ch] = s_lv[l - 1][ch][l == M_LEVELS - 1 ? 1 : 0] / f.n_in[l];
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const bool bad = f.invalid && f.invalid[img] != 0u;
    double* o = f.out + (size_t)img * GP_METRIC_COUNT;
    const double mse = d2 / (3.0 * f.n_all);
    double ms_ssim = nan;
    if (f.levels == M_LEVELS) {
        const double wgt[M_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
        for (int ch = 0; ch < 3; ++ch) {
            double p = 1.0;
#pragma unroll
            for (int l = 0; l < M_LEVELS; ++l) p *= pow(fmax(term[l][ch], 0.0), wgt[l]);     // ReLU first: a negative base would give NaN
            ms += p;
        }
        ms_ssim = ms / 3.0;
    }
    o[GP_METRIC_L1] = bad ? nan : l1 / (3.0 * f.n_all);
    o[GP_METRIC_MSE] = bad ? nan : mse;
    o[GP_METRIC_PSNR] = bad ? nan : 20.0 * log10(1.0 / sqrt(mse));
    o[GP_METRIC_PSNR_CH] = bad ? nan : psnr_ch / 3.0;
    o[GP_METRIC_SSIM] = bad ? nan : ss / (3.0 * f.n_all);
    o[GP_METRIC_MS_SSIM] = bad ? nan : ms_ssim;
    o[GP_METRIC_D_SSIM] = bad ? nan : (1.0 - ms_ssim) / 2.0;
    o[7] = bad ? nan : 0.0;
    if (f.levels_out) {
        double* lo = f.levels_out + (size_t)img * M_LEVELS * 3;
#pragma unroll
        for (int l = 0; l < M_LEVELS; ++l)
            for (int ch = 0; ch < 3; ++ch) lo[l * 3 + ch] = bad ? nan : term[l][ch];
    }
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static MWin11 metric_window() {
    // [REF utils/loss_utils.py:60-62]: exp(-(x - 5)^2 / (2 * 1.5^2)), normalised
    MWin11 w;
    double s = 0.0, t[11];
    for (int x = 0; x < 11; ++x) { t[x] = exp(-(double)((x - 5) * (x - 5)) / (2.0 * 1.5 * 1.5)); s += (float)t[x]; }
    for (int x = 0; x < 11; ++x) w.w[x] = (float)((float)t[x] / (float)s);
    return w;
}

struct MetricPlan {
    int levels;
    int h[M_LEVELS], w[M_LEVELS];
    size_t tiles[M_LEVELS];
    float* a[M_LEVELS]; float* b[M_LEVELS];     // levels 1-4 (scratch)
    double* sums[M_LEVELS];
    size_t bytes;
};

static void metric_plan(MetricPlan& p, void* scratch, int B, int H, int W, uint32_t flags) {
    p.levels = (flags & GP_METRICS_MS_SSIM) ? M_LEVELS : 1;
    GpCarver c(scratch);
    const size_t planes = (size_t)B * 3;
    int h = H, w = W;
    for (int l = 0; l < p.levels; ++l) {
        p.h[l] = h; p.w[l] = w;
        p.tiles[l] = (size_t)((w + MT - 1) / MT) * ((h + MT - 1) / MT);
        p.sums[l] = c.take<double>(planes * p.tiles[l] * (l == 0 ? M_SUMS0 : M_SUMSN));
        p.a[l] = p.b[l] = nullptr;
        if (l > 0) { p.a[l] = c.take<float>(planes * h * w); p.b[l] = c.take<float>(planes * h * w); }
        h = (h + 1) / 2; w = (w + 1) / 2;       // avg_pool2d(kernel 2, padding size % 2): floor((size + 2 p - 2) / 2) + 1
    }
    p.bytes = c.bytes();
}

static int metric_check_shape(int32_t B, int32_t H, int32_t W, uint32_t flags) {
    if (B <= 0 || H <= 0 || W <= 0) GP_FAIL("gp_image_metrics: B, H, W must be positive (got B=%d H=%d W=%d)", B, H, W);
    if ((int64_t)B * 3 > 65535) GP_FAIL("gp_image_metrics: at most 21845 images per call (got %d)", B);
    // (a tile row per grid.y; the same bound on W keeps the tiles of a plane, <= 65535^2, and every slot index far inside 64 bits)
    if (H > MT * 65535 || W > MT * 65535) GP_FAIL("gp_image_metrics: H and W may not exceed %d (got H=%d W=%d)", MT * 65535, H, W);
    if ((int64_t)((W + MT - 1) / MT) * ((H + MT - 1) / MT) > INT32_MAX)
        GP_FAIL("gp_image_metrics: more than 2^31 - 1 tiles per plane (H=%d W=%d)", H, W);
    if (flags & ~(GP_METRICS_QUANTIZE8 | GP_METRICS_CLAMP01 | GP_METRICS_MS_SSIM)) GP_FAIL("gp_image_metrics: unknown flag bits 0x%x", flags);
    if ((flags & GP_METRICS_MS_SSIM) && (H < W ? H : W) <= 160)
        GP_FAIL("gp_image_metrics: MS-SSIM needs min(H, W) > 160 for its five scales (got H=%d W=%d)", H, W);
    return 0;
}

extern "C" int64_t gp_image_metrics_scratch_bytes(int32_t B, int32_t H, int32_t W, uint32_t flags) {
    if (metric_check_shape(B, H, W, flags)) return -1;
    MetricPlan p;
    metric_plan(p, nullptr, B, H, W, flags);
    return (int64_t)p.bytes;
}

extern "C" int gp_image_metrics(const float* render, const float* gt, int32_t B, int32_t channels, int32_t H, int32_t W, uint32_t flags,
                                void* scratch, const uint32_t* invalid_flag, double* out, double* levels_out, uint8_t* quant_out,
                                uint8_t* deltas_out, gp_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (!render || !gt || !scratch || !out) GP_FAIL("gp_image_metrics: null argument");
    if (channels != 3) GP_FAIL("gp_image_metrics: expects [B,3,H,W] images (got C=%d)", channels);
    if (metric_check_shape(B, H, W, flags)) return 1;
    if (((uintptr_t)scratch & 255) != 0) GP_FAIL("gp_image_metrics: scratch must be 256-byte aligned");
    if (levels_out && !(flags & GP_METRICS_MS_SSIM)) GP_FAIL("gp_image_metrics: levels_out needs GP_METRICS_MS_SSIM");
    if (quant_out && !(flags & GP_METRICS_QUANTIZE8)) GP_FAIL("gp_image_metrics: quant_out needs GP_METRICS_QUANTIZE8");
    MetricPlan p;
    metric_plan(p, scratch, B, H, W, flags);
    const MWin11 win = metric_window();
    MetricFinalize f;
    memset(&f, 0, sizeof(f));
    for (int l = 0; l < p.levels; ++l) {
        MetricLevel L;
        memset(&L, 0, sizeof(L));
        L.a = l == 0 ? render : p.a[l];
        L.b = l == 0 ? gt : p.b[l];
        L.h = p.h[l]; L.w = p.w[l];
        if (l + 1 < p.levels) {
            L.na = p.a[l + 1]; L.nb = p.b[l + 1];
            L.nh = p.h[l + 1]; L.nw = p.w[l + 1];
            L.py = p.h[l] & 1; L.px = p.w[l] & 1;
        }
        L.sums = p.sums[l];
        const dim3 grid((p.w[l] + MT - 1) / MT, (p.h[l] + MT - 1) / MT, B * 3);
        static const char* const scope[M_LEVELS] = {"metrics_level0", "metrics_level1", "metrics_level2", "metrics_level3", "metrics_level4"};
        GpProfScope _p(scope[l], s);
        if (l == 0) {
            L.flags = flags; L.quant_out = quant_out; L.deltas_out = deltas_out;
            hipLaunchKernelGGL(gp_metric_level_kernel<true>, grid, dim3(256), 0, s, L, win);
        } else {
            hipLaunchKernelGGL(gp_metric_level_kernel<false>, grid, dim3(256), 0, s, L, win);
        }
        GP_LAUNCH_CHECK();
        f.sums[l] = p.sums[l];
        f.tiles[l] = (int)p.tiles[l];
        f.n_in[l] = (double)(p.h[l] - 2 * MH) * (double)(p.w[l] - 2 * MH);
    }
    f.n_all = (double)H * W;
    f.levels = p.levels;
    f.invalid = invalid_flag;
    f.out = out;
    f.levels_out = levels_out;
    GpProfScope _pf("metrics_finalize", s);
    hipLaunchKernelGGL(gp_metric_finalize_kernel, dim3(B), dim3(256), 0, s, f);
    GP_LAUNCH_CHECK();
    return 0;
}
