// pca_kernels.hip -- PCA colouring of per-point features and a jet colour map on the device (csrc/gp_pca.h, which states the definition
// in full).  The arithmetic that a CPU can run is csrc/pca_core.h (tests/pca_emulate.cpp runs it).
//   pca_mean_kernel           workgroup b of `parts` takes chunks b, b + parts, ... of 1024 rows; lane t = s*D + j adds column j of the
//                             rows s, s + S, ... (S = 256 / D) in float64 -- the lanes of one load are one contiguous span of X -- and
//                             lane j adds the S sub-sums in ascending s: part[b][j]
//   pca_mean_finish_kernel    mean64[j] = (part[0][j] + part[1][j] + ...) / N, and its one rounding to float32
//   pca_gram_kernel<T>        the same chunks; 64 rows at a time go through LDS as d = (float)(x - mean64), columns padded with zeros
//                             to 16*T; lane (tj, tk) of a 16 x 16 grid owns the T x T entries (tj + 16a, tk + 16b) and adds d_j * d_k
//                             (exact in float64) in float64, row after row: part[b][D][D].  The vector unit, not the matrix cores: the
//                             kernel moves N*D floats once and DESIGN section 22 says what that costs
//   pca_finish_kernel         one workgroup of 1024: C = sum of the parts / (N - 1) into LDS (D rows of D | 1 doubles, up to 129 KB:
//                             the odd stride keeps the lanes that walk down a column on different banks), Jacobi with the
//                             eigenvectors as the ROWS of Vt -- in LDS too while both fit the 160 KB (D <= 96), else in global
//                             scratch, where one workgroup's 128 KB stay in L2 and the lanes that rotate two eigenvectors walk
//                             along rows -- then order, sign and the roundings
//   pca_project_kernel        a tile of rows through LDS by one flat, coalesced copy (any D), row stride D | 1 so that the lanes'
//                             rows fall on different banks; one lane per y_ik, stored coalesced
//   pca_select_kernel         one launch per 8-bit pass: every workgroup first derives the targets' prefixes from the histogram of the
//                             pass before (pca_select_step), then counts its values' next 8 bits per target in LDS (integer atomics)
//                             and adds its counts to the pass's global histogram (integer atomics: the sums do not depend on order)
//   pca_select_finish_kernel  the last 8 bits, the values, the interpolation in float64
//   pca_colorize_kernel, colormap_lut_kernel   one lane per output element / per value
// Every store is an ordinary vector store; there is no floating-point atomic.
#include "gp_common.h"

#include "pca_core.h"

#define PCA_BLOCK 256
#define PCA_FINISH_BLOCK 1024
#define PCA_VT_LDS_MAX_D 96           // 2 * 96 * 97 doubles + the work space: 149 KB
#define PCA_GRAM_ROWS 64
#define PCA_TILE_FLOATS (64 * 129)
#define PCA_PROJECT_MAX_ROWS 1024
#define PCA_SELECT_PER_LANE 8
#define PCA_SELECT_MAX_BLOCKS 1024
#define PCA_TARGETS (2 * GP_PCA_MAX_Q)

__global__ void __launch_bounds__(PCA_BLOCK) pca_mean_kernel(const float* __restrict__ X, int64_t N, int D, int parts, double* __restrict__ part) {
    __shared__ double red[PCA_BLOCK];
    const int t = threadIdx.x, S = PCA_BLOCK / D, s = t / D, j = t - s * D;
    const int64_t chunks = (N + PCA_CHUNK - 1) / PCA_CHUNK;
    double acc = 0.0;
    if (s < S)
        for (int64_t c = blockIdx.x; c < chunks; c += parts) {
            const int64_t r0 = c * PCA_CHUNK, r1 = r0 + PCA_CHUNK < N ? r0 + PCA_CHUNK : N;
#pragma unroll 8
            for (int64_t r = r0 + s; r < r1; r += S) acc += (double)X[r * D + j];       // (unrolled: the loads go ahead of the ordered adds)
        }
    red[t] = acc;
    __syncthreads();
    if (t < D) {
        double sum = 0.0;
        for (int u = 0; u < S; ++u) sum += red[u * D + t];
        part[(int64_t)blockIdx.x * D + t] = sum;
    }
}

__global__ void __launch_bounds__(GP_PCA_MAX_D) pca_mean_finish_kernel(const double* __restrict__ part, int parts, int D, int64_t N,
                                                                       double* __restrict__ mean64, float* __restrict__ mean) {
    const int j = threadIdx.x;
    if (j >= D) return;
    double sum = 0.0;
#pragma unroll 8
    for (int b = 0; b < parts; ++b) sum += part[(int64_t)b * D + j];
    const double m = sum / (double)N;
    mean64[j] = m;
    mean[j] = (float)m;
}

template <int T>
__global__ void __launch_bounds__(PCA_BLOCK) pca_gram_kernel(const float* __restrict__ X, int64_t N, int D, int parts,
                                                             const double* __restrict__ mean64, double* __restrict__ part) {
    constexpr int LD = 16 * T;
    __shared__ float tile[PCA_GRAM_ROWS * LD];
    __shared__ double mu[GP_PCA_MAX_D];
    const int t = threadIdx.x, tj = t & 15, tk = t >> 4;
    for (int e = t; e < PCA_GRAM_ROWS * LD; e += PCA_BLOCK) tile[e] = 0.0f;       // (the padding columns stay zero)
    if (t < D) mu[t] = mean64[t];
    double acc[T][T];
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) acc[a][b] = 0.0;
    const int64_t chunks = (N + PCA_CHUNK - 1) / PCA_CHUNK;
    for (int64_t c = blockIdx.x; c < chunks; c += parts) {
        const int64_t c1 = c * PCA_CHUNK + PCA_CHUNK < N ? c * PCA_CHUNK + PCA_CHUNK : N;
        for (int64_t r0 = c * PCA_CHUNK; r0 < c1; r0 += PCA_GRAM_ROWS) {
            const int rows = (int)(c1 - r0 < PCA_GRAM_ROWS ? c1 - r0 : PCA_GRAM_ROWS);
            __syncthreads();                                   // (the tile's readers are done; the first time: mu and the zeros are stored)
            const float* src = X + r0 * D;
            for (int e = t; e < rows * D; e += PCA_BLOCK) {
                const int r = e / D, j = e - r * D;
                tile[r * LD + j] = (float)((double)src[e] - mu[j]);
            }
            __syncthreads();
#pragma unroll 4
            for (int r = 0; r < rows; ++r) {                   // (unrolled: four rows' LDS reads are in flight under the ordered adds)
                double dj[T], dk[T];
#pragma unroll
                for (int a = 0; a < T; ++a) {
                    dj[a] = (double)tile[r * LD + tj + 16 * a];
                    dk[a] = (double)tile[r * LD + tk + 16 * a];
                }
#pragma unroll
                for (int a = 0; a < T; ++a)
#pragma unroll
                    for (int b = 0; b < T; ++b) acc[a][b] += dj[a] * dk[b];
            }
        }
    }
    // entry (j, k) equals entry (k, j) bit for bit (the same products in the same order): stored transposed, coalesced over tj
    double* out = part + (int64_t)blockIdx.x * D * D;
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) {
            const int j = tj + 16 * a, k = tk + 16 * b;
            if (j < D && k < D) out[k * D + j] = acc[a][b];
        }
}

struct PcaBlockTeam {
    int rank, size;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

__global__ void __launch_bounds__(PCA_FINISH_BLOCK) pca_finish_kernel(const double* __restrict__ part, int parts, int D, int dim, int64_t N,
                                                                      double* Vt_global, float* __restrict__ components,
                                                                      float* __restrict__ explained_variance) {
    extern __shared__ double lds[];
    const int lda = D | 1;
    double* A = lds;                       // [D] rows of lda
    double* work = lds + D * lda;          // the team's PCA_JACOBI_WORK doubles
    double* Vt = D <= PCA_VT_LDS_MAX_D ? work + PCA_JACOBI_WORK : Vt_global;
    __shared__ int col[GP_PCA_MAX_DIM];
    __shared__ double sign[GP_PCA_MAX_DIM];
    const int t = threadIdx.x;
    const double denom = (double)(N - 1);
    for (int e = t; e < D * D; e += PCA_FINISH_BLOCK) {
        double sum = 0.0;
#pragma unroll 8
        for (int b = 0; b < parts; ++b) sum += part[(int64_t)b * D * D + e];
        A[(e / D) * lda + e % D] = sum / denom;
    }
    __syncthreads();
    PcaBlockTeam team = {t, PCA_FINISH_BLOCK};
    pca_jacobi(A, lda, Vt, D, work, team);
    __syncthreads();
    if (t < dim) {
        double sg;
        const int c = pca_pick_component(A, lda, Vt, D, t, &sg);
        col[t] = c;
        sign[t] = sg;
        explained_variance[t] = (float)A[c * lda + c];
    }
    __syncthreads();
    for (int e = t; e < dim * D; e += PCA_FINISH_BLOCK) {
        const int k = e / D, j = e - k * D;
        components[e] = (float)(sign[k] * Vt[col[k] * D + j]);
    }
}

__global__ void __launch_bounds__(PCA_BLOCK) pca_project_kernel(const float* __restrict__ X, int64_t N, int D, int dim, int tile_rows,
                                                                const float* __restrict__ mean, const float* __restrict__ components,
                                                                float* __restrict__ Y) {
    __shared__ float tile[PCA_TILE_FLOATS];
    __shared__ float comp[GP_PCA_MAX_DIM * (GP_PCA_MAX_D + 1)];
    __shared__ float mu[GP_PCA_MAX_D];
    const int t = threadIdx.x, LD = D | 1;
    const int64_t r0 = (int64_t)blockIdx.x * tile_rows;
    const int rows = (int)(N - r0 < tile_rows ? N - r0 : tile_rows);
    const float* src = X + r0 * D;
    for (int e = t; e < rows * D; e += PCA_BLOCK) {
        const int r = e / D, j = e - r * D;
        tile[r * LD + j] = src[e];
    }
    for (int e = t; e < dim * D; e += PCA_BLOCK) {
        const int k = e / D, j = e - k * D;
        comp[k * LD + j] = components[e];
    }
    if (t < D) mu[t] = mean[t];
    __syncthreads();
    float* dst = Y + r0 * dim;
    for (int it = t; it < rows * dim; it += PCA_BLOCK) {
        const int r = it / dim, k = it - r * dim;
        dst[it] = pca_project_row(tile + r * LD, mu, comp + k * LD, D);
    }
}

struct PcaSelectArgs {
    uint32_t rank[PCA_TARGETS];      // the ranks sought
    double frac[GP_PCA_MAX_Q];       // pos - lo of each percentile
    int targets, nq;
};

// hist [4 passes][PCA_TARGETS][256], zero before pass 0; state [4 passes][PCA_TARGETS]: the targets as pass p found them
__global__ void __launch_bounds__(PCA_BLOCK) pca_select_kernel(const float* __restrict__ values, uint32_t M, int pass, PcaSelectArgs args,
                                                               uint32_t* __restrict__ hist, PcaTarget* __restrict__ state) {
    __shared__ uint32_t counts[PCA_TARGETS][256];
    __shared__ PcaTarget target[PCA_TARGETS];
    const int t = threadIdx.x;
    if (pass > 0)
        for (int u = 0; u < args.targets; ++u) counts[u][t] = hist[((pass - 1) * PCA_TARGETS + u) * 256 + t];
    __syncthreads();
    if (t < args.targets) {
        PcaTarget g;
        g.prefix = 0;
        g.rank = args.rank[t];
        if (pass > 0) g = pca_select_step(state[(pass - 1) * PCA_TARGETS + t], counts[t], pass - 1);
        target[t] = g;
        if (blockIdx.x == 0) state[pass * PCA_TARGETS + t] = g;
    }
    __syncthreads();
    for (int u = 0; u < args.targets; ++u) counts[u][t] = 0u;
    __syncthreads();
    PcaTarget g[PCA_TARGETS];
#pragma unroll
    for (int u = 0; u < PCA_TARGETS; ++u) g[u] = target[u < args.targets ? u : 0];
    const int shift = 24 - 8 * pass;
    for (uint32_t i = blockIdx.x * PCA_BLOCK + t; i < M; i += gridDim.x * PCA_BLOCK) {
        const uint32_t key = pca_key(values[i]);
#pragma unroll
        for (int u = 0; u < PCA_TARGETS; ++u)
            if (u < args.targets && pca_key_matches(key, g[u], pass)) atomicAdd(&counts[u][(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    for (int u = 0; u < args.targets; ++u) {
        const uint32_t n = counts[u][t];
        if (n) atomicAdd(&hist[(pass * PCA_TARGETS + u) * 256 + t], n);
    }
}

__global__ void __launch_bounds__(PCA_BLOCK) pca_select_finish_kernel(PcaSelectArgs args, const uint32_t* __restrict__ hist,
                                                                      const PcaTarget* __restrict__ state, float* __restrict__ out,
                                                                      float* __restrict__ selected) {
    __shared__ uint32_t counts[PCA_TARGETS][256];
    __shared__ float value[PCA_TARGETS];
    const int t = threadIdx.x;
    for (int u = 0; u < args.targets; ++u) counts[u][t] = hist[(3 * PCA_TARGETS + u) * 256 + t];
    __syncthreads();
    if (t < args.targets) {
        value[t] = pca_unkey(pca_select_step(state[3 * PCA_TARGETS + t], counts[t], 3).prefix);
        if (selected) selected[t] = value[t];
    }
    __syncthreads();
    if (t < args.nq) out[t] = pca_interpolate(value[2 * t], value[2 * t + 1], args.frac[t]);
}

__global__ void __launch_bounds__(PCA_BLOCK) pca_colorize_kernel(const float* __restrict__ Y, uint32_t elems, int dim, const float* __restrict__ q,
                                                                 float* __restrict__ positions, float* __restrict__ colors) {
    const uint32_t e = blockIdx.x * PCA_BLOCK + threadIdx.x;
    if (e >= elems) return;
    const uint32_t r = e / 3u, ch = e - r * 3u;
    const float q1 = q[0], q99 = q[1];
    colors[e] = pca_clip01(pca_vis(Y[(size_t)r * dim + (dim - 3) + ch], q1, q99));
    if (positions) positions[e] = ch < 2u ? pca_vis(Y[(size_t)r * dim + ch], q1, q99) : 1.0f;
}

__global__ void __launch_bounds__(PCA_BLOCK) colormap_lut_kernel(const float* __restrict__ values, int64_t n, const float* __restrict__ lut,
                                                                 float* __restrict__ out) {
    __shared__ float table[256 * 3];
    for (int e = threadIdx.x; e < 256 * 3; e += PCA_BLOCK) table[e] = lut[e];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * PCA_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int row = pca_lut_index(values[i]);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[i * 3 + ch] = row < 0 ? 0.0f : table[row * 3 + ch];
}

// ---- the entry points ------------------------------------------------------------------------------------------------------------
struct PcaFitScratch {
    double *mean_part, *mean64, *gram_part, *V;
    size_t bytes;
    PcaFitScratch(void* p, int64_t N, int64_t D) {
        GpCarver c(p);
        const size_t parts = (size_t)pca_parts(N);
        mean_part = c.take<double>(parts * D);
        mean64 = c.take<double>(D);
        gram_part = c.take<double>(parts * D * D);
        V = c.take<double>(D * D);
        bytes = c.bytes();
    }
};

struct PcaSelectScratch {
    uint32_t* hist;
    PcaTarget* state;
    size_t bytes, hist_bytes;
    explicit PcaSelectScratch(void* p) {
        GpCarver c(p);
        hist = c.take<uint32_t>(4 * PCA_TARGETS * 256);
        hist_bytes = 4 * PCA_TARGETS * 256 * sizeof(uint32_t);
        state = c.take<PcaTarget>(4 * PCA_TARGETS);
        bytes = c.bytes();
    }
};

extern "C" int gp_pca_abi_version(void) { return GP_PCA_ABI_VERSION; }

extern "C" int64_t gp_pca_scratch_size(int64_t N, int64_t D) {
    const char* why = pca_refusal(N, D, 1);
    if (why) {
        snprintf(gp_err_buf, sizeof(gp_err_buf), "gp_pca_scratch_size: %s (N = %lld, D = %lld)", why, (long long)N, (long long)D);
        return -1;
    }
    const size_t fit = PcaFitScratch(nullptr, N, D).bytes, select = PcaSelectScratch(nullptr).bytes;
    return (int64_t)(fit > select ? fit : select);
}

extern "C" int gp_pca_fit(const float* X, int64_t N, int64_t D, int32_t dim, float* mean, float* components, float* explained_variance,
                          void* scratch, int64_t scratch_bytes, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = pca_refusal(N, D, dim);
    if (why) GP_FAIL("gp_pca_fit: %s (N = %lld, D = %lld, dim = %d)", why, (long long)N, (long long)D, dim);
    if (!X || !mean || !components || !explained_variance || !scratch) GP_FAIL("gp_pca_fit: null argument");
    PcaFitScratch s(scratch, N, D);
    if (scratch_bytes < (int64_t)s.bytes) GP_FAIL("gp_pca_fit: scratch holds %lld bytes, %lld are needed", (long long)scratch_bytes, (long long)s.bytes);
    if ((uintptr_t)scratch % 256) GP_FAIL("gp_pca_fit: scratch must be 256-byte aligned");
    const int parts = (int)pca_parts(N), d = (int)D;
    GpProfScope _p("pca_fit", st);
    hipLaunchKernelGGL(pca_mean_kernel, dim3(parts), dim3(PCA_BLOCK), 0, st, X, N, d, parts, s.mean_part);
    hipLaunchKernelGGL(pca_mean_finish_kernel, dim3(1), dim3(GP_PCA_MAX_D), 0, st, s.mean_part, parts, d, N, s.mean64, mean);
    if (d <= 16) hipLaunchKernelGGL(pca_gram_kernel<1>, dim3(parts), dim3(PCA_BLOCK), 0, st, X, N, d, parts, s.mean64, s.gram_part);
    else if (d <= 32) hipLaunchKernelGGL(pca_gram_kernel<2>, dim3(parts), dim3(PCA_BLOCK), 0, st, X, N, d, parts, s.mean64, s.gram_part);
    else if (d <= 64) hipLaunchKernelGGL(pca_gram_kernel<4>, dim3(parts), dim3(PCA_BLOCK), 0, st, X, N, d, parts, s.mean64, s.gram_part);
    else hipLaunchKernelGGL(pca_gram_kernel<8>, dim3(parts), dim3(PCA_BLOCK), 0, st, X, N, d, parts, s.mean64, s.gram_part);
    const size_t lds = ((size_t)d * (d | 1) + PCA_JACOBI_WORK + (d <= PCA_VT_LDS_MAX_D ? (size_t)d * d : 0)) * sizeof(double);
    if (lds > 48 * 1024) {
        static thread_local bool set = false;
        if (!set) {
            GP_HIP_CHECK(hipFuncSetAttribute((const void*)pca_finish_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)((PCA_VT_LDS_MAX_D * (2 * PCA_VT_LDS_MAX_D + 1) + PCA_JACOBI_WORK) * sizeof(double))));
            set = true;
        }
    }
    hipLaunchKernelGGL(pca_finish_kernel, dim3(1), dim3(PCA_FINISH_BLOCK), lds, st, s.gram_part, parts, d, (int)dim, N, s.V, components, explained_variance);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_pca_project(const float* X, int64_t N, int64_t D, const float* mean, const float* components, int32_t dim, float* Y,
                              gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = N < 1 ? "N must be >= 1" : pca_refusal(N < 8 ? 8 : N, D, dim);      // (a frozen basis projects any number of rows)
    if (why) GP_FAIL("gp_pca_project: %s (N = %lld, D = %lld, dim = %d)", why, (long long)N, (long long)D, dim);
    if (!X || !mean || !components || !Y) GP_FAIL("gp_pca_project: null argument");
    const int d = (int)D;
    int tile_rows = PCA_TILE_FLOATS / (d | 1);
    if (tile_rows > PCA_PROJECT_MAX_ROWS) tile_rows = PCA_PROJECT_MAX_ROWS;
    GpProfScope _p("pca_project", st);
    hipLaunchKernelGGL(pca_project_kernel, dim3(gp_blocks((size_t)N, tile_rows)), dim3(PCA_BLOCK), 0, st, X, N, d, (int)dim, tile_rows, mean,
                       components, Y);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_pca_percentiles(const float* values, int64_t M, const double* qs, int32_t nq, float* out, float* selected, void* scratch,
                                  int64_t scratch_bytes, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (!qs) GP_FAIL("gp_pca_percentiles: null argument");
    const char* why = pca_percentile_refusal(M, nq, qs);
    if (why) GP_FAIL("gp_pca_percentiles: %s (M = %lld, nq = %d)", why, (long long)M, nq);
    if (!values || !out || !scratch) GP_FAIL("gp_pca_percentiles: null argument");
    PcaSelectScratch s(scratch);
    if (scratch_bytes < (int64_t)s.bytes)
        GP_FAIL("gp_pca_percentiles: scratch holds %lld bytes, %lld are needed", (long long)scratch_bytes, (long long)s.bytes);
    if ((uintptr_t)scratch % 256) GP_FAIL("gp_pca_percentiles: scratch must be 256-byte aligned");
    PcaSelectArgs a;
    memset(&a, 0, sizeof(a));
    a.nq = nq;
    a.targets = 2 * nq;
    for (int k = 0; k < nq; ++k) pca_rank(qs[k], M, &a.rank[2 * k], &a.rank[2 * k + 1], &a.frac[k]);
    unsigned blocks = gp_blocks((size_t)M, PCA_BLOCK * PCA_SELECT_PER_LANE);
    if (blocks > PCA_SELECT_MAX_BLOCKS) blocks = PCA_SELECT_MAX_BLOCKS;
    GpProfScope _p("pca_percentiles", st);
    GP_HIP_CHECK(hipMemsetAsync(s.hist, 0, s.hist_bytes, st));
    for (int pass = 0; pass < 4; ++pass)
        hipLaunchKernelGGL(pca_select_kernel, dim3(blocks), dim3(PCA_BLOCK), 0, st, values, (uint32_t)M, pass, a, s.hist, s.state);
    hipLaunchKernelGGL(pca_select_finish_kernel, dim3(1), dim3(PCA_BLOCK), 0, st, a, s.hist, s.state, out, selected);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_pca_colorize(const float* Y, int64_t N, int32_t dim, const float* q, float* positions, float* colors, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const char* why = pca_colorize_refusal(N, dim);
    if (why) GP_FAIL("gp_pca_colorize: %s (N = %lld, dim = %d)", why, (long long)N, dim);
    if (!Y || !q || !colors || (dim == 5 && !positions)) GP_FAIL("gp_pca_colorize: null argument");
    const uint32_t elems = (uint32_t)(N * 3);
    GpProfScope _p("pca_colorize", st);
    hipLaunchKernelGGL(pca_colorize_kernel, dim3(gp_blocks(elems, PCA_BLOCK)), dim3(PCA_BLOCK), 0, st, Y, elems, (int)dim, q,
                       dim == 5 ? positions : nullptr, colors);
    GP_LAUNCH_CHECK();
    return 0;
}

extern "C" int gp_colormap_lut(const float* values, int64_t n, const float* lut, float* out, gp_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (n < 0 || n >= 0x80000000LL) GP_FAIL("gp_colormap_lut: n must be in 0 .. 2^31 - 1 (n = %lld)", (long long)n);
    if (n == 0) return 0;
    if (!values || !lut || !out) GP_FAIL("gp_colormap_lut: null argument");
    GpProfScope _p("colormap_lut", st);
    hipLaunchKernelGGL(colormap_lut_kernel, dim3(gp_blocks((size_t)n, PCA_BLOCK)), dim3(PCA_BLOCK), 0, st, values, n, lut, out);
    GP_LAUNCH_CHECK();
    return 0;
}
