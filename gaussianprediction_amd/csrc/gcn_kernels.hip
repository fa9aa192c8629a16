// gcn_kernels.hip -- the GCN keypoint motion predictor [REF motion_model/gcn.py:108-275, train_GCN.py:19-43,126-143]: one graph-convolution
// layer (forward in three BatchNorm modes, train-mode backward) and the autoregressive eval-mode rollout of both networks.  The contract
// (association, summation orders, what is saved, launch counts) is stated in include/gp_gcn.h.
//
// Every product runs on ONE tiled fp32 GEMM (v_mfma_f32_32x32x2_f32, exact fp32 operands and accumulation; the tiling of
// deform_generic.hip with a k-step of 32 and the next step's operands fetched into registers while the current one is multiplied).  It takes
// strided operands, a batch index (blockIdx.z) over outputs, an ordered loop over "reduction batches", up to two independent problems per
// launch, and the layer's epilogue (bias, eval BatchNorm, activation, residual).  No atomics, no split of any reduction over workgroups.
#include "gp_common.h"
#include "../../include/gp_gcn.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define GC_BM 64
#define GC_BN 64
#define GC_BK 32
#define GC_EPS 1e-5f
#define GC_MOMENTUM 0.1f

struct GcnGemm {
    const float* A; long sa_i, sa_k, sa_z, sa_r;     // A(z, r, i, k) = A[z sa_z + r sa_r + i sa_i + k sa_k]
    const float* B; long sb_k, sb_j, sb_z, sb_r;     // B(z, r, k, j)
    float* C; long sc_i, sc_z;                       // C[z sc_z + i sc_i + j] = sum over r (ascending), k (ascending)
    int I, J, K, Z, R;
    int a_kfast, b_jfast;                            // which index of the operand is contiguous in memory (staging order)
    // epilogue, in this order; residual and pre (the value after the bias) are indexed like C
    const float* bias;                               // [J]
    float* pre;
    const float *bn_mean, *bn_var, *bn_gamma, *bn_beta;   // eval BatchNorm, feature (i % bn_rows) * J + j
    int bn_rows;
    int act;
    const float* residual;
};
struct GcnGemmSet { GcnGemm g[2]; int n; };

__device__ __forceinline__ float gcn_act(float v, int act) {
    if (act == GP_GCN_ACT_TANH) return tanhf(v);
    if (act == GP_GCN_ACT_RELU) return fmaxf(v, 0.f);
    return v;
}
// d act / d (its argument), from the activation's VALUE a
__device__ __forceinline__ float gcn_dact(float a, int act) {
    if (act == GP_GCN_ACT_TANH) return 1.f - a * a;
    if (act == GP_GCN_ACT_RELU) return a > 0.f ? 1.f : 0.f;
    return 1.f;
}

__device__ __forceinline__ void gcn_fetch(const GcnGemm& g, const float* __restrict__ A, const float* __restrict__ B, long i0, long j0, int k0,
                                          int tid, float (&ra)[8], float (&rb)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = tid + 256 * u;
        int m, kk;
        if (g.a_kfast) { m = e >> 5; kk = e & 31; } else { kk = e >> 6; m = e & 63; }
        const long gi = i0 + m;
        const int gk = k0 + kk;
        ra[u] = (gi < g.I && gk < g.K) ? A[gi * g.sa_i + gk * g.sa_k] : 0.f;
        int n;
        if (g.b_jfast) { kk = e >> 6; n = e & 63; } else { n = e >> 5; kk = e & 31; }
        const long gj = j0 + n;
        const int gk2 = k0 + kk;
        rb[u] = (gj < g.J && gk2 < g.K) ? B[gk2 * g.sb_k + gj * g.sb_j] : 0.f;
    }
}

__global__ __launch_bounds__(256) void gp_gcn_gemm_kernel(GcnGemmSet set) {
    __shared__ float As[GC_BK][GC_BM + 1];
    __shared__ float Bs[GC_BK][GC_BN + 1];
    int z = blockIdx.z;
    const int prob = (set.n > 1 && z >= set.g[0].Z) ? 1 : 0;
    if (prob) z -= set.g[0].Z;
    const GcnGemm& g = set.g[prob];
    const long i0 = (long)blockIdx.x * GC_BM, j0 = (long)blockIdx.y * GC_BN;
    if (i0 >= g.I || j0 >= g.J || z >= g.Z) return;          // (uniform over the workgroup: the grid covers the larger problem)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int kt = (g.K + GC_BK - 1) / GC_BK;
    const int steps = g.R * kt;
    const float* Az = g.A + (long)z * g.sa_z;
    const float* Bz = g.B + (long)z * g.sb_z;
    float ra[8], rb[8];
    gcn_fetch(g, Az, Bz, i0, j0, 0, tid, ra, rb);
    for (int s = 0; s < steps; ++s) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 256 * u;
            if (g.a_kfast) As[e & 31][e >> 5] = ra[u]; else As[e >> 6][e & 63] = ra[u];
            if (g.b_jfast) Bs[e >> 6][e & 63] = rb[u]; else Bs[e & 31][e >> 5] = rb[u];
        }
        __syncthreads();
        if (s + 1 < steps) {
            const int r = (s + 1) / kt, k0 = ((s + 1) - r * kt) * GC_BK;
            gcn_fetch(g, Az + (long)r * g.sa_r, Bz + (long)r * g.sb_r, i0, j0, k0, tid, ra, rb);
        }
        // v_mfma_f32_32x32x2_f32: lane l supplies A(m = l % 32, k = l / 32) and B(k = l / 32, n = l % 32)
#pragma unroll
        for (int kk = 0; kk < GC_BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + (lane >> 5)][wm + (lane & 31)], Bs[kk + (lane >> 5)][wn + (lane & 31)], acc, 0, 0, 0);
        __syncthreads();
    }
    // accumulator register r of lane l: row 8 (r / 4) + 4 (l / 32) + r % 4, column l % 32
    const long j = j0 + wn + (lane & 31);
    if (j >= g.J) return;
    const float bj = g.bias ? g.bias[j] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long i = i0 + wm + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        if (i >= g.I) continue;
        const long off = (long)z * g.sc_z + i * g.sc_i + j;
        float v = acc[r] + bj;
        if (g.pre) g.pre[off] = v;
        if (g.bn_mean) {
            const long f = (i % g.bn_rows) * g.J + j;
            v = (v - g.bn_mean[f]) * (1.f / sqrtf(g.bn_var[f] + GC_EPS)) * g.bn_gamma[f] + g.bn_beta[f];
        }
        v = gcn_act(v, g.act);
        if (g.residual) v += g.residual[off];
        g.C[off] = v;
    }
}

// train-mode BatchNorm over the batch + activation + residual: one thread per feature j of n = M * Fout, b ascending
__global__ __launch_bounds__(256) void gp_gcn_bn_train_fwd_kernel(int B, long n, const float* __restrict__ Z, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar,
                                                                 float* __restrict__ smean, float* __restrict__ sinv, int act,
                                                                 const float* __restrict__ residual, float* __restrict__ Y) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)Z[b * n + j];
    const float mean = (float)(s / B);
    double q = 0.0;
    for (int b = 0; b < B; ++b) { const double d = (double)Z[b * n + j] - (double)mean; q += d * d; }
    const float var = (float)(q / B);
    const float inv = 1.f / sqrtf(var + GC_EPS);
    smean[j] = mean; sinv[j] = inv;
    if (rmean) rmean[j] = (1.f - GC_MOMENTUM) * rmean[j] + GC_MOMENTUM * mean;
    if (rvar) rvar[j] = (1.f - GC_MOMENTUM) * rvar[j] + GC_MOMENTUM * (float)(q / (B - 1));
    const float ga = gamma[j], be = beta[j];
    for (int b = 0; b < B; ++b) {
        float v = gcn_act(ga * ((Z[b * n + j] - mean) * inv) + be, act);
        if (residual) v += residual[b * n + j];
        Y[b * n + j] = v;
    }
}

// dZ from dY through the activation and (bn) the batch-statistics BatchNorm; dgamma, dbeta; dresidual = dY
__global__ __launch_bounds__(256) void gp_gcn_bn_bwd_kernel(int B, long n, int bn, const float* __restrict__ Z, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ smean,
                                                           const float* __restrict__ sinv, int act, const float* __restrict__ dY,
                                                           float* __restrict__ dZ, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           float* __restrict__ dres) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    if (!bn) {
        for (int b = 0; b < B; ++b) {
            const float dy = dY[b * n + j];
            dZ[b * n + j] = dy * gcn_dact(gcn_act(Z[b * n + j], act), act);
            if (dres) dres[b * n + j] = dy;
        }
        return;
    }
    const float mean = smean[j], inv = sinv[j], ga = gamma[j], be = beta[j];
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < B; ++b) {
        const float xh = (Z[b * n + j] - mean) * inv;
        const float dy = dY[b * n + j];
        const float gr = dy * gcn_dact(gcn_act(ga * xh + be, act), act);
        s1 += (double)gr; s2 += (double)gr * (double)xh;
        if (dres) dres[b * n + j] = dy;
    }
    if (dbeta) dbeta[j] = (float)s1;
    if (dgamma) dgamma[j] = (float)s2;
    const float m1 = (float)(s1 / B), m2 = (float)(s2 / B);
    for (int b = 0; b < B; ++b) {
        const float xh = (Z[b * n + j] - mean) * inv;
        const float gr = dY[b * n + j] * gcn_dact(gcn_act(ga * xh + be, act), act);
        dZ[b * n + j] = ga * inv * (gr - m1 - xh * m2);
    }
}

// dbias[f] = sum over the rows of dZ[row][f]: one workgroup per f, thread t adds rows t, t + 256, .. in a double, then a fixed tree
__global__ __launch_bounds__(256) void gp_gcn_colsum_kernel(long rows, int cols, const float* __restrict__ dZ, float* __restrict__ out) {
    __shared__ double part[256];
    const int f = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (long r = t; r < rows; r += 256) s += (double)dZ[r * cols + f];
    part[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0) out[f] = (float)part[0];
}

// ---- rollout helpers ---------------------------------------------------------------------------------------------------------------
// operate()'s permutes [REF train_GCN.py:36]: X_net[(c K + k)][t] = window_net[row0 + t][k][c], both networks in one launch
__global__ __launch_bounds__(256) void gp_gcn_gather_kernel(int K, int T, const float* __restrict__ winx, const float* __restrict__ winr,
                                                           float* __restrict__ Xx, float* __restrict__ Xr) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long nx = (long)3 * K * T, nr = (long)4 * K * T;
    if (e >= nx + nr) return;
    const bool isr = e >= nx;
    const long q = isr ? e - nx : e;
    const int C = isr ? 4 : 3;
    const int t = (int)(q % T);
    const long ck = q / T;
    const int c = (int)(ck / K), k = (int)(ck - (long)c * K);
    (isr ? Xr : Xx)[q] = (isr ? winr : winx)[((long)t * K + k) * C + c];
}

// the head's outputs O_net [(c K + k)][out] -> the predicted rows: xyz as it is, rot normalised over its four channels (F.normalize:
// x / max(||x||_2, 1e-12), the squares added in channel order), a second time when norm_rotation; written to the outputs and appended
// to the window
__global__ __launch_bounds__(256) void gp_gcn_finish_kernel(int K, int out, int norm_rotation, const float* __restrict__ Ox, const float* __restrict__ Or,
                                                           const float* __restrict__ base, float* __restrict__ winx_new, float* __restrict__ winr_new,
                                                           float* __restrict__ xyz_out, float* __restrict__ rot_out, float* __restrict__ delta_out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)out * K) return;
    const int o = (int)(e / K), k = (int)(e - (long)o * K);
    float p[3], q[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = Ox[((long)c * K + k) * out + o];
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = Or[((long)c * K + k) * out + o];
    for (int pass = 0; pass < (norm_rotation ? 2 : 1); ++pass) {
        const float nrm = fmaxf(sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]), 1e-12f);
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = q[c] / nrm;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { winx_new[e * 3 + c] = p[c]; xyz_out[e * 3 + c] = p[c]; }
#pragma unroll
    for (int c = 0; c < 4; ++c) { winr_new[e * 4 + c] = q[c]; rot_out[e * 4 + c] = q[c]; }
    if (delta_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) delta_out[e * 7 + c] = p[c] - base[k * 3 + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) delta_out[e * 7 + 3 + c] = q[c];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static int gcn_launch(const GcnGemmSet& set, hipStream_t s) {
    long gx = 0, gy = 0, gz = 0;
    for (int p = 0; p < set.n; ++p) {
        const GcnGemm& g = set.g[p];
        const long x = ((long)g.I + GC_BM - 1) / GC_BM, y = ((long)g.J + GC_BN - 1) / GC_BN;
        gx = x > gx ? x : gx; gy = y > gy ? y : gy; gz += g.Z;
    }
    if (gx < 1 || gy < 1 || gz < 1) return 0;
    if (gx > 0x7FFFFFFFL || gy > 65535 || gz > 65535) GP_FAIL("gcn: %ld x %ld x %ld output blocks exceed the launch limits", gx, gy, gz);
    hipLaunchKernelGGL(gp_gcn_gemm_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(256), 0, s, set);
    GP_LAUNCH_CHECK();
    return 0;
}

struct GcnLayer {
    int B, M, Fin, Fout;
    const float *X, *W; int wt;
    const float *att, *bias;
    int bn_mode; const float *gamma, *beta, *rmean, *rvar;
    int act; const float* residual;
    float *S, *Z, *Y;
};

static GcnGemm gcn_zero() { GcnGemm g; memset(&g, 0, sizeof(g)); g.Z = 1; g.R = 1; g.bn_rows = 1; return g; }

// the layer's epilogue on the product that ends it (train-mode BatchNorm: the product stops at Z; the rest is gp_gcn_bn_train_fwd_kernel)
static void gcn_epilogue(const GcnLayer& a, GcnGemm& g) {
    g.bias = a.bias;
    if (a.bn_mode == GP_GCN_BN_TRAIN) { g.C = a.Z; return; }
    g.C = a.Y; g.pre = a.Z;
    if (a.bn_mode == GP_GCN_BN_EVAL) { g.bn_mean = a.rmean; g.bn_var = a.rvar; g.bn_gamma = a.gamma; g.bn_beta = a.beta; g.bn_rows = a.M; }
    g.act = a.act; g.residual = a.residual;
}

// X @ W over the B * M rows (into S, or with att == NULL the whole layer), then att @ S_b
static bool gcn_forward_problems(const GcnLayer& a, GcnGemm& g1, GcnGemm& g2) {
    g1 = gcn_zero();
    g1.A = a.X; g1.sa_i = a.Fin; g1.sa_k = 1; g1.a_kfast = 1;
    g1.B = a.W;
    if (a.wt) { g1.sb_k = 1; g1.sb_j = a.Fin; g1.b_jfast = 0; } else { g1.sb_k = a.Fout; g1.sb_j = 1; g1.b_jfast = 1; }
    g1.I = a.B * a.M; g1.J = a.Fout; g1.K = a.Fin; g1.sc_i = a.Fout;
    if (!a.att) { gcn_epilogue(a, g1); return false; }
    g1.C = a.S;
    g2 = gcn_zero();
    const long plane = (long)a.M * a.Fout;
    g2.A = a.att; g2.sa_i = a.M; g2.sa_k = 1; g2.a_kfast = 1;
    g2.B = a.S; g2.sb_k = a.Fout; g2.sb_j = 1; g2.sb_z = plane; g2.b_jfast = 1;
    g2.I = a.M; g2.J = a.Fout; g2.K = a.M; g2.Z = a.B; g2.sc_i = a.Fout; g2.sc_z = plane;
    gcn_epilogue(a, g2);
    return true;
}

static int gcn_check_shape(const char* who, long B, long M, long Fin, long Fout) {
    if (B < 1 || B > GP_GCN_MAX_B) GP_FAIL("%s: B = %ld outside [1, %d]", who, B, GP_GCN_MAX_B);
    if (M < 1 || M > GP_GCN_MAX_M) GP_FAIL("%s: M = %ld outside [1, %d]", who, M, GP_GCN_MAX_M);
    if (Fin < 1 || Fin > GP_GCN_MAX_F) GP_FAIL("%s: Fin = %ld outside [1, %d]", who, Fin, GP_GCN_MAX_F);
    if (Fout < 1 || Fout > GP_GCN_MAX_F) GP_FAIL("%s: Fout = %ld outside [1, %d]", who, Fout, GP_GCN_MAX_F);
    return 0;
}

extern "C" int gp_gcn_abi_version(void) { return GP_GCN_ABI_VERSION; }

extern "C" int gp_gcn_layer_forward(int32_t B, int32_t M, int32_t Fin, int32_t Fout, const float* X, const float* W, int32_t w_transposed,
                                    const float* att, const float* bias, int32_t bn_mode, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, int32_t act, const float* residual, float* S, float* Z,
                                    float* save_mean, float* save_invstd, float* Y, gp_stream_t stream) {
    const char* who = "gp_gcn_layer_forward";
    if (gcn_check_shape(who, B, M, Fin, Fout)) return 1;
    if (bn_mode < GP_GCN_BN_OFF || bn_mode > GP_GCN_BN_TRAIN) GP_FAIL("%s: bn_mode = %d is none of off / eval / train", who, bn_mode);
    if (act < GP_GCN_ACT_NONE || act > GP_GCN_ACT_RELU) GP_FAIL("%s: act = %d is none of none / tanh / relu", who, act);
    if (bn_mode == GP_GCN_BN_TRAIN && B < 2) GP_FAIL("%s: Expected more than 1 value per channel when training (B = %d)", who, B);
    if (!X || !W || !Y) GP_FAIL("%s: null X, W or Y", who);
    if (Y == X) GP_FAIL("%s: Y may not alias X", who);
    if (att && !S) GP_FAIL("%s: null S (needed with att)", who);
    if (bn_mode != GP_GCN_BN_OFF && (!gamma || !beta)) GP_FAIL("%s: null gamma or beta", who);
    if (bn_mode == GP_GCN_BN_EVAL && (!running_mean || !running_var)) GP_FAIL("%s: null running_mean or running_var (eval mode)", who);
    if (bn_mode == GP_GCN_BN_TRAIN && (!Z || !save_mean || !save_invstd)) GP_FAIL("%s: null Z, save_mean or save_invstd (train mode)", who);
    hipStream_t s = (hipStream_t)stream;
    GcnLayer a = {B, M, Fin, Fout, X, W, w_transposed != 0, att, bias, bn_mode, gamma, beta, running_mean, running_var, act, residual, S, Z, Y};
    GcnGemmSet s1, s2;
    s1.n = s2.n = 1;
    const bool two = gcn_forward_problems(a, s1.g[0], s2.g[0]);
    if (gcn_launch(s1, s)) return 1;
    if (two && gcn_launch(s2, s)) return 1;
    if (bn_mode == GP_GCN_BN_TRAIN) {
        const long n = (long)M * Fout;
        hipLaunchKernelGGL(gp_gcn_bn_train_fwd_kernel, dim3(gp_blocks(n, 256)), dim3(256), 0, s, B, n, Z, gamma, beta, running_mean, running_var,
                           save_mean, save_invstd, act, residual, Y);
        GP_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gp_gcn_layer_backward(int32_t B, int32_t M, int32_t Fin, int32_t Fout, const float* X, const float* W, int32_t w_transposed,
                                     const float* att, int32_t bn_mode, const float* gamma, const float* beta, int32_t act, const float* S,
                                     const float* Z, const float* save_mean, const float* save_invstd, const float* dY, float* dZ, float* dS,
                                     float* dX, float* dW, float* datt, float* dbias, float* dgamma, float* dbeta, float* dresidual,
                                     gp_stream_t stream) {
    const char* who = "gp_gcn_layer_backward";
    if (gcn_check_shape(who, B, M, Fin, Fout)) return 1;
    if (bn_mode != GP_GCN_BN_OFF && bn_mode != GP_GCN_BN_TRAIN) GP_FAIL("%s: bn_mode = %d (there is no backward of the eval mode)", who, bn_mode);
    if (act < GP_GCN_ACT_NONE || act > GP_GCN_ACT_RELU) GP_FAIL("%s: act = %d is none of none / tanh / relu", who, act);
    if (bn_mode == GP_GCN_BN_TRAIN && B < 2) GP_FAIL("%s: Expected more than 1 value per channel when training (B = %d)", who, B);
    if (!X || !W || !Z || !dY || !dZ) GP_FAIL("%s: null X, W, Z, dY or dZ", who);
    if (att && (!S || !dS)) GP_FAIL("%s: null S or dS (needed with att)", who);
    if (!att && datt) GP_FAIL("%s: datt without att", who);
    if (bn_mode == GP_GCN_BN_TRAIN && (!gamma || !beta || !save_mean || !save_invstd)) GP_FAIL("%s: null gamma, beta, save_mean or save_invstd", who);
    hipStream_t s = (hipStream_t)stream;
    const long n = (long)M * Fout, rows = (long)B * M;
    hipLaunchKernelGGL(gp_gcn_bn_bwd_kernel, dim3(gp_blocks(n, 256)), dim3(256), 0, s, B, n, bn_mode == GP_GCN_BN_TRAIN ? 1 : 0, Z, gamma, beta,
                       save_mean, save_invstd, act, dY, dZ, dgamma, dbeta, dresidual);
    GP_LAUNCH_CHECK();
    if (dbias) {
        hipLaunchKernelGGL(gp_gcn_colsum_kernel, dim3(Fout), dim3(256), 0, s, rows, Fout, dZ, dbias);
        GP_LAUNCH_CHECK();
    }
    GcnGemmSet q;
    q.n = 1;
    const float* dSp = dZ;
    if (att) {
        if (dX || dW) {             // dS_b = att^T @ dZ_b
            GcnGemm g = gcn_zero();
            g.A = att; g.sa_i = 1; g.sa_k = M; g.a_kfast = 0;
            g.B = dZ; g.sb_k = Fout; g.sb_j = 1; g.sb_z = n; g.b_jfast = 1;
            g.C = dS; g.sc_i = Fout; g.sc_z = n; g.I = M; g.J = Fout; g.K = M; g.Z = B;
            q.g[0] = g;
            if (gcn_launch(q, s)) return 1;
            dSp = dS;
        }
        if (datt) {                 // datt = sum over b, then f, of dZ_b[i][f] S_b[j][f]
            GcnGemm g = gcn_zero();
            g.A = dZ; g.sa_i = Fout; g.sa_k = 1; g.sa_r = n; g.a_kfast = 1;
            g.B = S; g.sb_k = 1; g.sb_j = Fout; g.sb_r = n; g.b_jfast = 0;
            g.C = datt; g.sc_i = M; g.I = M; g.J = M; g.K = Fout; g.R = B;
            q.g[0] = g;
            if (gcn_launch(q, s)) return 1;
        }
    }
    if (dW) {                       // over the B * M rows, ascending
        GcnGemm g = gcn_zero();
        const float *P = w_transposed ? dSp : X, *Q = w_transposed ? X : dSp;
        const int pi = w_transposed ? Fout : Fin, qj = w_transposed ? Fin : Fout;
        g.A = P; g.sa_i = 1; g.sa_k = pi; g.a_kfast = 0;
        g.B = Q; g.sb_k = qj; g.sb_j = 1; g.b_jfast = 1;
        g.C = dW; g.sc_i = qj; g.I = pi; g.J = qj; g.K = (int)rows;
        q.g[0] = g;
        if (gcn_launch(q, s)) return 1;
    }
    if (dX) {                       // dS @ W^T
        GcnGemm g = gcn_zero();
        g.A = dSp; g.sa_i = Fout; g.sa_k = 1; g.a_kfast = 1;
        g.B = W;
        if (w_transposed) { g.sb_k = Fin; g.sb_j = 1; g.b_jfast = 1; } else { g.sb_k = 1; g.sb_j = Fout; g.b_jfast = 0; }
        g.C = dX; g.sc_i = Fin; g.I = (int)rows; g.J = Fin; g.K = Fout;
        q.g[0] = g;
        if (gcn_launch(q, s)) return 1;
    }
    return 0;
}

// ---- rollout -------------------------------------------------------------------------------------------------------------------------
struct GcnNetBufs { float *win, *X, *S, *P[3], *Hh, *O; };

static int gcn_rollout_check(const char* who, long K, long T, long H, long stages, long out, long frames) {
    if (K < 1 || 4 * K > GP_GCN_MAX_M) GP_FAIL("%s: K = %ld outside [1, %d]", who, K, GP_GCN_MAX_M / 4);
    if (T < 1 || T > GP_GCN_MAX_F) GP_FAIL("%s: T = %ld outside [1, %d]", who, T, GP_GCN_MAX_F);
    if (H < 1 || H > GP_GCN_MAX_F) GP_FAIL("%s: H = %ld outside [1, %d]", who, H, GP_GCN_MAX_F);
    if (stages < 0 || stages > GP_GCN_MAX_STAGES) GP_FAIL("%s: num_stage = %ld outside [0, %d]", who, stages, GP_GCN_MAX_STAGES);
    if (out < 1 || out > GP_GCN_MAX_F) GP_FAIL("%s: output_size = %ld outside [1, %d]", who, out, GP_GCN_MAX_F);
    if (frames < 1 || frames > GP_GCN_MAX_FRAMES) GP_FAIL("%s: frames = %ld outside [1, %d]", who, frames, GP_GCN_MAX_FRAMES);
    return 0;
}

static size_t gcn_carve(void* scratch, int K, int T, int H, int out, int frames, GcnNetBufs nb[2]) {
    GpCarver c(scratch);
    for (int p = 0; p < 2; ++p) {
        const size_t C = p ? 4 : 3, M = C * K, Hm = (size_t)(H > out ? H : out);
        nb[p].win = c.take<float>(((size_t)T + (size_t)frames * out) * K * C);
        nb[p].X = c.take<float>(M * T);
        nb[p].S = c.take<float>(M * Hm);
        for (int i = 0; i < 3; ++i) nb[p].P[i] = c.take<float>(M * H);
        nb[p].Hh = c.take<float>(M * H);
        nb[p].O = c.take<float>(M * out);
    }
    return c.bytes();
}

extern "C" int64_t gp_gcn_scratch_bytes(int32_t K, int32_t T, int32_t H, int32_t num_stage, int32_t output_size, int32_t frames) {
    if (gcn_rollout_check("gp_gcn_scratch_bytes", K, T, H, num_stage, output_size, frames)) return -1;
    GcnNetBufs nb[2];
    return (int64_t)gcn_carve(nullptr, K, T, H, output_size, frames, nb);
}

extern "C" int gp_gcn_rollout(int32_t K, int32_t T, int32_t H, int32_t num_stage, int32_t output_size, int32_t no_mapping,
                              const void* const* table, int32_t table_len, const float* xyz, const float* rot, int32_t frames,
                              int32_t norm_rotation, const float* base_xyz, float* xyz_out, float* rot_out, float* delta_out, void* scratch,
                              gp_stream_t stream) {
    const char* who = "gp_gcn_rollout";
    if (gcn_rollout_check(who, K, T, H, num_stage, output_size, frames)) return 1;
    if (output_size > T) GP_FAIL("%s: output_size = %d exceeds the window (T = %d)", who, output_size, T);
    const int G = 1 + 2 * num_stage, L = G + (no_mapping ? 1 : 2);
    if (!table || table_len != 2 * L * GP_GCN_TABLE_SLOTS) GP_FAIL("%s: table must hold 2 * %d * %d pointers (got %d)", who, L, GP_GCN_TABLE_SLOTS, table_len);
    if (!xyz || !rot || !xyz_out || !rot_out || !scratch) GP_FAIL("%s: null xyz, rot, xyz_out, rot_out or scratch", who);
    if ((uintptr_t)scratch & 255) GP_FAIL("%s: scratch must be 256-byte aligned", who);
    if ((delta_out != nullptr) != (base_xyz != nullptr)) GP_FAIL("%s: delta_out and base_xyz go together", who);
    for (int p = 0; p < 2; ++p)
        for (int l = 0; l < L; ++l) {
            const void* const* e = table + ((size_t)p * L + l) * GP_GCN_TABLE_SLOTS;
            const bool gc = l < G || no_mapping, bn = l < G;
            if (!e[0] || !e[2] || (gc && !e[1]) || (bn && (!e[3] || !e[4] || !e[5] || !e[6])))
                GP_FAIL("%s: null pointer in the table (network %d, layer %d)", who, p, l);
        }
    hipStream_t s = (hipStream_t)stream;
    GcnNetBufs nb[2];
    gcn_carve(scratch, K, T, H, output_size, frames, nb);
    GP_HIP_CHECK(hipMemcpyAsync(nb[0].win, xyz, (size_t)T * K * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    GP_HIP_CHECK(hipMemcpyAsync(nb[1].win, rot, (size_t)T * K * 4 * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int f = 0; f < frames; ++f) {
        const size_t row0 = (size_t)f * output_size, rowN = row0 + T;
        hipLaunchKernelGGL(gp_gcn_gather_kernel, dim3(gp_blocks((size_t)7 * K * T, 256)), dim3(256), 0, s, K, T, nb[0].win + row0 * K * 3,
                           nb[1].win + row0 * K * 4, nb[0].X, nb[1].X);
        GP_LAUNCH_CHECK();
        int cur[2] = {0, 0};
        for (int l = 0; l < L; ++l) {
            GcnGemmSet s1, s2;
            s1.n = s2.n = 2;
            bool two = false;
            for (int p = 0; p < 2; ++p) {
                const float* const* e = (const float* const*)(table + ((size_t)p * L + l) * GP_GCN_TABLE_SLOTS);
                const int M = (p ? 4 : 3) * K;
                GcnLayer a;
                memset(&a, 0, sizeof(a));
                a.B = 1; a.M = M; a.W = e[0]; a.att = e[1]; a.bias = e[2]; a.S = nb[p].S;
                if (l < G) {                     // gc1 / a block's gc1, gc2: BatchNorm (eval) + tanh; the block's second adds its input
                    a.bn_mode = GP_GCN_BN_EVAL; a.gamma = e[3]; a.beta = e[4]; a.rmean = e[5]; a.rvar = e[6]; a.act = GP_GCN_ACT_TANH;
                    a.Fout = H;
                    if (l == 0) { a.X = nb[p].X; a.Fin = T; a.Y = nb[p].P[0]; }
                    else if (l & 1) { a.X = nb[p].P[cur[p]]; a.Fin = H; a.Y = nb[p].P[(cur[p] + 1) % 3]; }
                    else {
                        a.X = nb[p].P[(cur[p] + 1) % 3]; a.Fin = H; a.residual = nb[p].P[cur[p]]; a.Y = nb[p].P[(cur[p] + 2) % 3];
                        cur[p] = (cur[p] + 2) % 3;
                    }
                } else if (no_mapping) {         // gc_out
                    a.X = nb[p].P[cur[p]]; a.Fin = H; a.Fout = output_size; a.Y = nb[p].O;
                } else if (l == G) {             // Linear, ReLU
                    a.X = nb[p].P[cur[p]]; a.Fin = H; a.Fout = H; a.wt = 1; a.att = nullptr; a.act = GP_GCN_ACT_RELU; a.Y = nb[p].Hh;
                } else {                         // Linear
                    a.X = nb[p].Hh; a.Fin = H; a.Fout = output_size; a.wt = 1; a.att = nullptr; a.Y = nb[p].O;
                }
                two = gcn_forward_problems(a, s1.g[p], s2.g[p]);
            }
            if (gcn_launch(s1, s)) return 1;
            if (two && gcn_launch(s2, s)) return 1;
        }
        const size_t orow = (size_t)f * output_size;
        hipLaunchKernelGGL(gp_gcn_finish_kernel, dim3(gp_blocks((size_t)output_size * K, 256)), dim3(256), 0, s, K, output_size, norm_rotation ? 1 : 0,
                           nb[0].O, nb[1].O, base_xyz, nb[0].win + rowN * K * 3, nb[1].win + rowN * K * 4, xyz_out + orow * K * 3,
                           rot_out + orow * K * 4, delta_out ? delta_out + orow * K * 7 : nullptr);
        GP_LAUNCH_CHECK();
    }
    return 0;
}
