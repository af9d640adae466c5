/*
 * lidargs_decode_options.h -- C ABI of the two model options in front of the fused anchor decode
 * (liblidargs_decode_options.so, built from csrc/decode_options.hip alone).
 *
 * generate_neural_gaussians (gaussian_renderer/__init__.py:17-119) of a model built with use_feat_bank=True and / or
 * appearance_dim > 0 (scene/gaussian_model.py:57-58) does two things the decode of include/lidargs_neural_gaussians.h does not:
 *
 *   feature bank (:37-47)   per visible anchor, with o = anchor - cam_center, dist = |o|, view = o / dist:
 *       w = Softmax(Linear(32,3)(ReLU(Linear(4,32)([view, dist]))))                       (gaussian_model.py:105-111)
 *       feat'[j] = feat[4 (j mod 8)] w0 + feat[2 (j mod 16)] w1 + feat[j] w2,  j = 0..31   (torch.repeat tiles)
 *     feat' replaces the anchor feature for all four MLPs of the decode: the caller hands feat_out to lidargs_ng_forward_select /
 *     _decode / _backward_mfma as their anchor_feat, and their dL_danchor_feat to lidargs_ng_bank_backward as dL_dfeat_out.
 *
 *   appearance (:52-56, :73-79)   every row of one frame gets the same embedding vector e = weight[camera uid], so the appearance
 *     columns of the colour and ray-drop heads' first layer, W1 [32][din + A] with din = 35 + add_color_dist, add a per-frame
 *     constant to the bias:  b1_eff = b1 + W1[:, din:] e.  The decode runs on the packed [32][din] part and b1_eff; the backward
 *     gives  dW1[:, :din] = what the decode returned,  dW1[:, din:] = db1 (x) e,  de = W1[:, din:]^T db1,  db1 = db1_eff.
 *
 * All pointers are device pointers unless stated otherwise; plain float32 row-major arrays; no torch types.  Arguments are
 * validated before any device work.  Functions return 0 (or a count) on success and a negative code on failure,
 * LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT or LIDARGS_NG_OPTIONS_ERR_HIP (the values of LIDARGS_ERR_INVALID_ARGUMENT and LIDARGS_ERR_HIP
 * of include/lidargs_rasterizer.h), with a message in lidargs_ng_options_last_error() (thread-local, this library's own).  N == 0 returns 0 without a
 * launch.  No function waits for the stream, allocates, or uses float atomics: every sum is taken in a fixed order.
 */
#ifndef LIDARGS_DECODE_OPTIONS_H
#define LIDARGS_DECODE_OPTIONS_H

#include <stddef.h>
#include <stdint.h>

#define LIDARGS_NG_OPTIONS_ABI_VERSION 1
#define LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT (-1)   /* bad sizes / NULL required pointer         */
#define LIDARGS_NG_OPTIONS_ERR_HIP (-4)                /* a kernel launch failed                    */
#define LIDARGS_NG_BANK_PARAMS 259          /* W1 [32][4] | b1 [32] | W2 [3][32] | b2 [3] */

#ifdef __cplusplus
extern "C" {
#endif

int lidargs_ng_options_abi_version(void);
const char* lidargs_ng_options_last_error(void);

/* feat_out f32[N][32] = feat' of every visible anchor; the rows of invisible anchors are written as ZEROS.  (The decode's 16x16x4
 * tile kernels request the feature rows of a whole 32-anchor tile before they know the visible flags and drop the invisible ones
 * when the tile is staged: they never compute with such a row, but they do load it, so no row is left unwritten.)
 *   visible_mask u8[N] (torch.bool) or NULL = all visible;  cam_center HOST pointer, 3 floats
 *   W1 [32][4], b1 [32], W2 [3][32], b2 [3]: the bank MLP in nn.Linear layout
 * Reads 140 B and writes 128 B per visible anchor. */
int lidargs_ng_bank_forward(int N, const uint8_t* visible_mask, const float* anchor_feat, const float* anchor,
                            const float* cam_center, const float* W1, const float* b1, const float* W2, const float* b2,
                            float* feat_out, void* stream);

/* Floats of `partials` lidargs_ng_bank_backward needs for N anchors (one row of LIDARGS_NG_BANK_PARAMS per workgroup). */
size_t lidargs_ng_bank_backward_partial_floats(int N);

/* The VJP of lidargs_ng_bank_forward; w is recomputed, nothing of the forward is kept.
 *   dL_dfeat_out    f32[N][32]  (the decode's dL_danchor_feat; rows of invisible anchors are not read)
 *   dL_danchor_feat f32[N][32], dL_danchor f32[N][3]: every row written, zeros for invisible anchors.  dL_danchor is the bank's
 *                   share alone: the caller adds the decode's.
 *   dL_dparams      f32[259] = dW1 [32][4] | db1 [32] | dW2 [3][32] | db2 [3]: each workgroup writes one row of `partials`, a
 *                   second small launch adds the rows in a fixed order (bit-reproducible from run to run).
 * Reads 268 B and writes 140 B per visible anchor. */
int lidargs_ng_bank_backward(int N, const uint8_t* visible_mask, const float* anchor_feat, const float* anchor,
                             const float* cam_center, const float* W1, const float* b1, const float* W2, const float* b2,
                             const float* dL_dfeat_out, float* dL_danchor_feat, float* dL_danchor, float* dL_dparams,
                             float* partials, size_t partial_floats, void* stream);

/* One launch: W1_out f32[2][32][din] = the leading din columns of the colour head's W1 [32][din + A], then of the ray-drop head's;
 * b1_out f32[2][32] = b1 + W1[:, din:] e of each (ascending a).  din = 35 or 36, any A >= 1; e_* f32[A] = the embedding rows. */
int lidargs_ng_appearance_fold(int din, int A, const float* W1_color, const float* b1_color, const float* e_color,
                               const float* W1_raydrop, const float* b1_raydrop, const float* e_raydrop,
                               float* W1_out, float* b1_out, void* stream);

/* One launch: dW1_full f32[2][32][din + A] = [dW1_main | db1 (x) e] of the colour head, then of the ray-drop head, and
 * de_color f32[A], de_raydrop f32[A] = W1[:, din:]^T db1 (ascending hidden unit).  dW1_main_* f32[32][din] and db1_* f32[32] are
 * what the decode's backward returned for the packed weights and the folded biases. */
int lidargs_ng_appearance_backward(int din, int A, const float* W1_color, const float* e_color, const float* W1_raydrop,
                                   const float* e_raydrop, const float* dW1_main_color, const float* db1_color,
                                   const float* dW1_main_raydrop, const float* db1_raydrop, float* dW1_full, float* de_color,
                                   float* de_raydrop, void* stream);

#ifdef __cplusplus
}
#endif
#endif
