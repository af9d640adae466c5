/*
 * lidargs_tcnn.h -- C ABI of the tinycudann stand-in (liblidargs_tcnn.so, built from csrc/raydrop_mlp.hip alone): the frequency encoding
 * and the bias-free fused MLP of the reference's ray-drop refinement network (scene/extre_train_raydrop.py: two tcnn.Encoding
 * "Frequency" modules and one tcnn.Network "FullyFusedMLP", 128 neurons, ReLU, Sigmoid output).  Everything is float32.
 *
 * Frequency encoding of x [n, dims] with F = n_freq frequencies, out [n, dims * 2F] (tinycudann's published column layout):
 *   out[r, d*2F + 2f + s] = sin(pi * 2^f * x[r, d] + s * pi/2)          s = 0: sine, s = 1: cosine
 * evaluated as sinpi / cospi of t = scalbnf(x, f), which is exact in float32: no rounded product with pi is ever formed.
 * `out` and `dout` of the encoding must be 8-byte aligned (they are written and read as sine/cosine pairs).
 * The input gradient is dx[r, d] = sum_f pi 2^f (cos(pi t) dout[.., 2f] - sin(pi t) dout[.., 2f + 1]), f ascending.
 *
 * MLP with h = n_hidden_layers (1..8) hidden layers of 128 neurons, n_in (1..128) inputs, n_out (1..16) outputs, no biases:
 *   h_0 = x;  h_i = relu(W_i h_{i-1}), i = 1..h;  y = W_out h_h;  out = y (out_act 0) or 1 / (1 + exp(-y)) (out_act 1)
 * `params` holds the matrices ROW-MAJOR [out, in], concatenated in this order:
 *   W_1 [128, n_in], W_2 .. W_h [128, 128] each, W_out [n_out, 128]           lidargs_tcnn_param_count() floats in all
 * `dparams` of the backward has the same layout and is OVERWRITTEN (the caller accumulates).  `dx` may be NULL: the input gradient is
 * then neither computed nor written.  The backward saves nothing from the forward: it recomputes the hidden activations of a row tile
 * in LDS (EXPERIMENTS.md).  Every workgroup of the backward owns one block of `param_count` floats in `partials` for its share of the
 * weight gradient; a second launch folds the lidargs_tcnn_backward_blocks(n) blocks in ascending order.  No float atomics: two calls
 * on the same inputs and device give bit-identical results.  `partials` needs no initialisation.
 *
 * All pointers are device memory owned by the caller; rows are dense (x [n, n_in], out / dout [n, n_out], dx [n, n_in]).  A ragged
 * last row tile is masked inside the kernels, and a K that is no multiple of 4 is zero-padded in the operand load.  `stream` is a
 * hipStream_t.  Returns 0, or a negative code with a message in lidargs_tcnn_last_error() (thread-local): -1 for an invalid argument
 * (sizes outside the ranges above, a NULL pointer with n > 0, `partial_floats` below lidargs_tcnn_backward_partial_floats()), -4 for a
 * HIP error.  Arguments are validated before any device work; n == 0 is a no-op (dparams is then zero-filled by the fold).
 */
#ifndef LIDARGS_TCNN_H
#define LIDARGS_TCNN_H

#include <stddef.h>

#define LIDARGS_TCNN_ABI_VERSION 1
#define LIDARGS_TCNN_WIDTH 128
#define LIDARGS_TCNN_MAX_HIDDEN_LAYERS 8
#define LIDARGS_TCNN_MAX_OUT 16
#define LIDARGS_TCNN_MAX_FREQUENCIES 32

#ifdef __cplusplus
extern "C" {
#endif

int lidargs_tcnn_frequency_forward(int n, int dims, int n_freq, const float* x, float* out, void* stream);
int lidargs_tcnn_frequency_backward(int n, int dims, int n_freq, const float* x, const float* dout, float* dx, void* stream);

size_t lidargs_tcnn_param_count(int n_in, int n_hidden_layers, int n_out);
int lidargs_tcnn_mlp_forward(int n, int n_in, int n_hidden_layers, int n_out, int out_act, const float* params, const float* x,
                             float* out, void* stream);

int lidargs_tcnn_forward_row_tile(void);        /* rows per workgroup of the forward */
int lidargs_tcnn_backward_row_tile(void);       /* rows per tile of the backward */
int lidargs_tcnn_backward_blocks(int n);        /* workgroups (= partial blocks) of the backward on the current device */
size_t lidargs_tcnn_backward_partial_floats(int n, int n_in, int n_hidden_layers, int n_out);
int lidargs_tcnn_mlp_backward(int n, int n_in, int n_hidden_layers, int n_out, int out_act, const float* params, const float* x,
                              const float* dout, float* dparams, float* dx, float* partials, size_t partial_floats, void* stream);

const char* lidargs_tcnn_last_error(void);
int lidargs_tcnn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
