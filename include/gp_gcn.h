/* gp_gcn.h -- the GCN keypoint motion predictor (GCN_xyzr) on the device: the C entry points of csrc/gcn_kernels.hip, a part of
 * libgp_hip.so with an ABI number of its own.
 *
 * Conventions are those of gp_hip.h: plain device pointers and sizes, fp32, contiguous, a return code != 0 (or -1 from the int64_t
 * query) plus gp_last_error(), every argument validated before any launch, no synchronisation and no host read inside any entry,
 * a gp_stream_t last.  No kernel of this header uses a float atomic, none waits on another workgroup: plain launches in stream
 * order, and two calls on equal inputs give equal bits.
 *
 * What they replace [REF motion_model/gcn.py:108-275, train_GCN.py:19-43, 126-143, 165-176].
 *
 * One layer:   Y = act(BN(att @ (X @ W) + bias)) [+ residual]
 *   X [B][M][Fin], W [Fin][Fout] (or [Fout][Fin] with w_transposed, nn.Linear's layout), att [M][M] or NULL, bias [Fout] or NULL,
 *   Y / residual / S / Z [B][M][Fout], the BatchNorm vectors [M * Fout] (feature index m * Fout + f, BatchNorm1d(M * Fout) of the
 *   reference's y.view(b, -1)).
 *
 * CONTRACT
 *   Association: the reference's, att @ (X @ W).  S = X @ W is written to memory (B * M rows), then att @ S_b per batch item.
 *   Products: v_mfma_f32_32x32x2_f32, exact fp32 operands and accumulation.  Every output element is accumulated by ONE lane in
 *   ascending k, two k per instruction, from zero; the bias is added after the sum, then (eval) the BatchNorm affine
 *   (z - running_mean) * (1 / sqrt(running_var + 1e-5)) * gamma + beta, then the activation, then the residual.  The tiling does not
 *   depend on B or on which other problem shares the launch, so a row of a B = 1 call has the bits of the same row inside a rollout.
 *   Sums over B (train-mode statistics and every backward reduction over the batch): one thread per feature adds b = 0 .. B-1 in
 *   ascending order into a double; mean = sum / B, biased variance = sum of (z - mean)^2 / B (second pass, same order), each
 *   rounded once to fp32.  running_mean = 0.9 running_mean + 0.1 mean; running_var = 0.9 running_var + 0.1 var * B / (B - 1).
 *   Backward products with a reduction over the batch (datt: over b then f; dW: over the B * M rows) run in ONE workgroup per
 *   output tile in ascending order -- no split, no atomic.  dbias: one workgroup per f, 256 double partial sums over the rows
 *   r = t, t + 256, .. ascending, folded by a fixed tree.
 *   Saved for the backward (by the caller, train mode): X, S (when att != NULL), Z (the pre-BatchNorm value att @ S + bias),
 *   save_mean, save_invstd.  The activation's derivative is recomputed from Z.
 *   Launches: forward eval / BN off: 2 (1 when att == NULL).  Forward train: 3 (2 when att == NULL).  Backward: at most 6
 *   (BN + activation, dbias, dS, datt, dW, dX).
 *   gp_gcn_rollout, per frame: 1 (the two permutes of both networks) + 2 per graph convolution + 2 for the head + 1 (normalise,
 *   outputs, window) = 6 + 4 num_stage launches; every layer launch serves both networks (blockIdx.z selects the problem). */
#ifndef GP_GCN_H
#define GP_GCN_H

#include "gp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GP_GCN_ABI_VERSION 1

#define GP_GCN_MAX_M 4096
#define GP_GCN_MAX_F 512
#define GP_GCN_MAX_B 1024
#define GP_GCN_MAX_FRAMES 4096
#define GP_GCN_MAX_STAGES 16

#define GP_GCN_ACT_NONE 0
#define GP_GCN_ACT_TANH 1
#define GP_GCN_ACT_RELU 2

#define GP_GCN_BN_OFF 0
#define GP_GCN_BN_EVAL 1
#define GP_GCN_BN_TRAIN 2

#define GP_GCN_TABLE_SLOTS 7 /* per layer: W, att, bias, bn_gamma, bn_beta, bn_running_mean, bn_running_var (NULL where absent) */

int gp_gcn_abi_version(void);

/* Limits: 1 <= M <= GP_GCN_MAX_M, 1 <= Fin, Fout <= GP_GCN_MAX_F, 1 <= B <= GP_GCN_MAX_B; anything outside is refused with a message
 * naming the argument.  BN_TRAIN with B < 2 is refused ("Expected more than 1 value per channel when training").
 * S: needed when att != NULL.  Z: needed in BN_TRAIN; optional otherwise (written when given: what the backward reads).
 * save_mean / save_invstd: BN_TRAIN.  running_mean / running_var: read in BN_EVAL, updated in BN_TRAIN.  Y may not alias X. */
int gp_gcn_layer_forward(int32_t B, int32_t M, int32_t Fin, int32_t Fout, const float* X, const float* W, int32_t w_transposed,
                         const float* att, const float* bias, int32_t bn_mode, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, int32_t act, const float* residual, float* S, float* Z, float* save_mean, float* save_invstd,
                         float* Y, gp_stream_t stream);

/* The backward of a BN_TRAIN or BN_OFF forward that wrote Z.  A NULL output pointer means that gradient is not computed.
 * dZ and dS: [B][M][Fout] work buffers (dS only when att != NULL).  dW has W's layout.  dresidual = dY. */
int gp_gcn_layer_backward(int32_t B, int32_t M, int32_t Fin, int32_t Fout, const float* X, const float* W, int32_t w_transposed,
                          const float* att, int32_t bn_mode, const float* gamma, const float* beta, int32_t act, const float* S,
                          const float* Z, const float* save_mean, const float* save_invstd, const float* dY, float* dZ, float* dS, float* dX,
                          float* dW, float* datt, float* dbias, float* dgamma, float* dbeta, float* dresidual, gp_stream_t stream);

/* Bytes of gp_gcn_rollout's scratch (256-byte aligned); -1 for an argument outside the limits (K = keypoints, 1 <= 4 K <= GP_GCN_MAX_M;
 * T = input_size, H = linear_size, 1 <= T, H, output_size <= GP_GCN_MAX_F; 0 <= num_stage <= GP_GCN_MAX_STAGES;
 * 1 <= frames <= GP_GCN_MAX_FRAMES). */
int64_t gp_gcn_scratch_bytes(int32_t K, int32_t T, int32_t H, int32_t num_stage, int32_t output_size, int32_t frames);

/* The autoregressive eval-mode rollout of GCN_xyzr.  table: a HOST array of 2 * L * GP_GCN_TABLE_SLOTS device pointers, the xyz network
 * (M = 3 K) then the rotation network (M = 4 K), L = 1 + 2 num_stage graph convolutions (each with its BatchNorm) followed by the head:
 * no_mapping = 0: two nn.Linear layers (W [Fout][Fin], att NULL); no_mapping = 1: one graph convolution.  xyz [T][K][3] and
 * rot [T][K][4]: the last window.  Every frame predicts output_size rows (1 <= output_size <= T), writes them to
 * xyz_out / rot_out [frames * output_size][K][3 | 4] (rot normalised over its four channels, x / max(||x||, 1e-12), a second time
 * when norm_rotation) and, with base_xyz [K][3], to delta_out [frames * output_size][K][7] = (xyz - base_xyz, rot), the rows
 * gp_blend_forward reads; the window then drops its first output_size rows and takes the prediction.  Frame f of a rollout of F frames
 * equals frame f of one of f + 1 frames bit for bit. */
int gp_gcn_rollout(int32_t K, int32_t T, int32_t H, int32_t num_stage, int32_t output_size, int32_t no_mapping, const void* const* table,
                   int32_t table_len, const float* xyz, const float* rot, int32_t frames, int32_t norm_rotation, const float* base_xyz,
                   float* xyz_out, float* rot_out, float* delta_out, void* scratch, gp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
