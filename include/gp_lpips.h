/* gp_lpips.h -- LPIPS (Learned Perceptual Image Patch Similarity, v0.1) with the AlexNet and VGG16 backbones on the device:
 * the C entry points of csrc/lpips_kernels.hip, a part of libgp_hip.so with an ABI number of its own.
 *
 * Conventions are those of gp_hip.h: plain device pointers and sizes, a return code != 0 (or -1 from the int64_t queries) plus
 * gp_last_error(), no synchronisation, a gp_stream_t last.  The caller supplies the network weights; nothing is shipped or fetched.
 *
 * Definition [REF lpipsPyTorch/modules/networks.py, lpips.py, utils.py]: both images ([0,1], NO rescaling to [-1,1]) are z-scored
 * with the float32 values of mean = (-.030, -.088, -.188), std = (.458, .448, .450), go through the backbone's `features`, and at
 * each of five tapped ReLU outputs      term_l = mean over pixels of  sum_c w_lc * (x_c / (|x| + 1e-10) - y_c / (|y| + 1e-10))^2
 * with |x| = sqrt(sum_c x_c^2) and w_l the `lin` weights.  LPIPS = term_1 + ... + term_5.
 *
 * Arithmetic: convolutions are implicit GEMMs on the exact-float32 matrix instruction (v_mfma_f32_32x32x2_f32), activations NHWC
 * float32; the per-pixel distance in float32; sums over pixels and everything after them in double, in a fixed order, no atomics:
 * two calls give the same bits, and row b of a batched call is the row of a call on pair b alone (pairs are processed in turn). */
#ifndef GP_LPIPS_H
#define GP_LPIPS_H

#include "gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_LPIPS_ABI_VERSION 1

#define GP_LPIPS_ALEX 0
#define GP_LPIPS_VGG 1
#define GP_LPIPS_SQUEEZE 2 /* refused: nothing in the reference's evaluation asks for it */

#define GP_LPIPS_QUANTIZE8 1u /* the FIRST image goes through 8 bits first: floor(x * 255 + 0.5) clamped, / 255 (GP_METRICS_QUANTIZE8) */
#define GP_LPIPS_TAPS 5
#define GP_LPIPS_COLUMNS 8 /* out row: 0 = LPIPS, 1..5 = the layer terms, 6..7 reserved (0) */

/* layer kinds of the network tables */
#define GP_LPIPS_CONV 0
#define GP_LPIPS_RELU 1
#define GP_LPIPS_POOL 2

int gp_lpips_abi_version(void);

/* The network tables: entry `index` (0-based) is entry `index` of torchvision's `features` Sequential.  gp_lpips_num_layers
 * returns the number of entries (-1: unknown net).  desc[8] = kind, Cin, Cout, kernel size, stride, padding, tapped (1: this
 * ReLU's output feeds a distance term), index of the convolution among the convolutions (-1 for the others).  For ReLU and
 * pool entries Cin = Cout = the channels passing through.  Entries after the fifth tap are listed and never run. */
int gp_lpips_num_layers(int32_t net);
int gp_lpips_layer(int32_t net, int32_t index, int32_t* desc);

/* Weights, packed once: every convolution's [Cout][Cin][k][k] weight reordered to [Cout][k][k][Cin] (the order the B operand is
 * staged in), its bias, then the five lin vectors.  conv_w / conv_b: host arrays of device pointers, one per convolution in
 * network order, torch layout; lin_w: host array of five device pointers, [C_l] each. */
int64_t gp_lpips_weight_floats(int32_t net);
int gp_lpips_pack_weights(int32_t net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, float* packed,
                          gp_stream_t stream);

/* Scratch of ONE pair (two activation buffers and the partial-sum slots); -1 and a message naming H and W for sizes at which a
 * feature map would be empty: min(H, W) < 31 (alex), < 16 (vgg). */
int64_t gp_lpips_scratch_bytes(int32_t net, int32_t B, int32_t H, int32_t W);

/* a, b: [B][3][H][W] float32.  scratch: gp_lpips_scratch_bytes bytes, 256-byte aligned.  invalid_flag (optional): one word per
 * pair, non-zero makes that row NaN.  out: [B][GP_LPIPS_COLUMNS] doubles. */
int gp_lpips(int32_t net, const float* packed, const float* a, const float* b, int32_t B, int32_t H, int32_t W, uint32_t flags,
             void* scratch, const uint32_t* invalid_flag, double* out, gp_stream_t stream);

/* The building blocks on arbitrary shapes, activations NHWC.
 * conv: x [N][H][W][Cin], w [Cout][Cin][k][k] (torch layout), bias [Cout], w_packed: Cout * k * k * Cin floats of scratch,
 * y [N][Ho][Wo][Cout] = relu(conv(x) + bias), Ho = (H + 2 pad - k) / stride + 1.
 * pool: max over k x k windows, floor mode, no padding: y [N][(H - k) / stride + 1][(W - k) / stride + 1][C]. */
int gp_lpips_conv2d_relu(const float* x, const float* w, const float* bias, float* w_packed, float* y, int32_t N, int32_t H, int32_t W,
                         int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride, int32_t pad, gp_stream_t stream);
int gp_lpips_maxpool(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ksize, int32_t stride,
                     gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
