// voxel_core.h -- the arithmetic of the voxel-grid downsample (include/gp_voxel.h), shared by the kernels of voxel_kernels.hip and
// by the host pass gp_voxel_downsample_host, which the tests without a device run (and tests/voxel_emulate.cpp, under the sanitizers).
//
//   vx_finite / vx_index               the non-finite test on the bits, and index = (int32)floor((p - min_bound) / voxel_size)
//   vx_plan                            min_bound, the refusals, the bits of each axis' largest index, the chunks of the sort key
//   vx_chunk_key                       bits [lo, lo + w) of the key  ix : iy : iz  (x most significant, each field as wide as its axis needs)
//   vx_same_voxel / vx_segment_mean    the head test between neighbours of the sorted order, and the mean of one (voxel, channel)
//   vx_downsample_host                 the whole pass on host memory, through the functions above and the same chunked stable sorts
// The file must be compiled with -ffp-contract=off (nothing here may fuse, though nothing here multiplies and adds).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/gp_voxel.h"

#if defined(__HIPCC__)
#define VX_FN __host__ __device__ inline
#else
#define VX_FN inline
#endif

#define VX_MAX_N 0x7FFFFFFFLL        // n < 2^31: rows are addressed by uint32 and counted in int32

struct VxGrid {
    double min_bound[3];
    double voxel_size;
    int bits[3];                     // of the largest index of x, y, z (0 where the axis has one cell)
    int total_bits;                  // max(1, bits x + y + z): the key  ix : iy : iz
    int chunks, chunk_bits;          // the key is sorted in `chunks` stable sorts of at most `chunk_bits` <= 32 bits, least significant first
};

VX_FN bool vx_finite(double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return (u & 0x7FF0000000000000ULL) != 0x7FF0000000000000ULL;
}

VX_FN int32_t vx_index(double p, double min_bound, double voxel_size) { return (int32_t)floor((p - min_bound) / voxel_size); }

VX_FN int vx_bit_length(uint32_t v) {
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

// lo / hi: the exact min and max of the (finite) points.  0, or 1 = "voxel_size is too small" (Open3D's test, on its own operands).
inline int vx_plan(VxGrid& g, const double* lo, const double* hi, double voxel_size) {
    double extent = 0.0;
    for (int a = 0; a < 3; ++a) {
        g.min_bound[a] = lo[a] - voxel_size / 2;
        const double e = (hi[a] + voxel_size / 2) - g.min_bound[a];
        if (a == 0 || e > extent) extent = e;
    }
    g.voxel_size = voxel_size;
    if (voxel_size * (double)INT32_MAX < extent) return 1;
    g.total_bits = 0;
    for (int a = 0; a < 3; ++a) {            // (the index is monotone in p: subtraction, division by a positive and floor all are)
        g.bits[a] = vx_bit_length((uint32_t)vx_index(hi[a], g.min_bound[a], voxel_size));
        g.total_bits += g.bits[a];
    }
    if (g.total_bits < 1) g.total_bits = 1;  // (one voxel: a one-bit sort still writes the identity permutation)
    g.chunks = (g.total_bits + 31) / 32;
    g.chunk_bits = (g.total_bits + g.chunks - 1) / g.chunks;
    return 0;
}

// the part of field `v`, which sits `off` bits up in the key, that falls into the 32 bits from `lo` up
VX_FN uint32_t vx_field_part(uint32_t v, int off, int lo) {
    const int d = off - lo;
    if (d >= 0) return d < 32 ? v << d : 0u;
    return -d < 32 ? v >> -d : 0u;
}

VX_FN uint32_t vx_chunk_key(const VxGrid& g, const int32_t* idx, int chunk) {
    const int lo = chunk * g.chunk_bits;
    const int w = g.total_bits - lo < g.chunk_bits ? g.total_bits - lo : g.chunk_bits;
    const uint32_t k = vx_field_part((uint32_t)idx[2], 0, lo) | vx_field_part((uint32_t)idx[1], g.bits[2], lo) |
                       vx_field_part((uint32_t)idx[0], g.bits[2] + g.bits[1], lo);
    return w < 32 ? k & ((1u << w) - 1u) : k;
}
VX_FN int vx_chunk_width(const VxGrid& g, int chunk) {
    const int lo = chunk * g.chunk_bits;
    return g.total_bits - lo < g.chunk_bits ? g.total_bits - lo : g.chunk_bits;
}

VX_FN bool vx_same_voxel(const int32_t* a, const int32_t* b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

// rows perm[start .. end) of `src` [n][3], channel ch, added one by one from zero, over double(count)
VX_FN double vx_segment_mean(const double* src, const uint32_t* perm, uint32_t start, uint32_t end, int ch) {
    double s = 0.0;
    for (uint32_t i = start; i < end; ++i) s += src[(size_t)perm[i] * 3 + ch];
    return s / (double)(end - start);
}

// 0, or the refusal: 1 voxel_size <= 0, 2 n out of range, 3 a coordinate that is not finite, 4 voxel_size is too small
inline const char* vx_refusal(int code) {
    switch (code) {
        case 1: return "voxel_size <= 0";
        case 2: return "n must be in [0, 2^31)";
        case 3: return "a coordinate is not finite (NaN or Inf)";
        case 4: return "voxel_size is too small";
    }
    return "";
}

inline int vx_downsample_host(int64_t n, const double* points, const double* colors, const double* normals, double voxel_size,
                              double* out_points, double* out_colors, double* out_normals, int32_t* out_index, int64_t* m_out) {
    if (!(voxel_size > 0.0)) return 1;
    if (n < 0 || n >= VX_MAX_N) return 2;
    *m_out = 0;
    if (n == 0) return 0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (int64_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const double v = points[i * 3 + a];
            if (!vx_finite(v)) { bad = true; continue; }
            if (v < lo[a]) lo[a] = v;
            if (v > hi[a]) hi[a] = v;
        }
    if (bad) return 3;
    VxGrid g;
    if (vx_plan(g, lo, hi, voxel_size)) return 4;
    std::vector<int32_t> idx((size_t)n * 3);
    for (int64_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) idx[i * 3 + a] = vx_index(points[i * 3 + a], g.min_bound[a], voxel_size);
    std::vector<uint32_t> perm((size_t)n), key((size_t)n);
    for (int64_t i = 0; i < n; ++i) perm[i] = (uint32_t)i;
    for (int c = 0; c < g.chunks; ++c) {      // as the device: one stable sort per chunk of the key, through the running permutation
        for (int64_t i = 0; i < n; ++i) key[i] = vx_chunk_key(g, &idx[(size_t)i * 3], c);
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    }
    std::vector<uint32_t> starts;
    for (int64_t i = 0; i < n; ++i)
        if (i == 0 || !vx_same_voxel(&idx[(size_t)perm[i] * 3], &idx[(size_t)perm[i - 1] * 3])) starts.push_back((uint32_t)i);
    const int64_t m = (int64_t)starts.size();
    starts.push_back((uint32_t)n);
    const double* src[3] = {points, colors, normals};
    double* dst[3] = {out_points, out_colors, out_normals};
    for (int64_t v = 0; v < m; ++v)
        for (int ch = 0; ch < 9; ++ch) {
            if (!src[ch / 3] || !dst[ch / 3]) continue;
            dst[ch / 3][v * 3 + ch % 3] = vx_segment_mean(src[ch / 3], perm.data(), starts[v], starts[v + 1], ch % 3);
            if (ch < 3 && out_index) out_index[v * 3 + ch] = idx[(size_t)perm[starts[v]] * 3 + ch];
        }
    *m_out = m;
    return 0;
}
