/*
 * lidargs_scatter.h -- C ABI of the torch_scatter stand-in (liblidargs_scatter.so, built from lidar-gs_amd/torch_scatter/csrc/scatter.hip
 * alone): scatter_max / scatter_min with the winning position, and their gradient, on the device.
 *
 * Every array pointer is a DEVICE pointer.  `src` is viewed as f32[A, E, B], contiguous; the reduction runs over E.  `index` is never
 * read at src's size: the group of element (a, e, b) is index[a * sa + e * se + b * sb], with the three strides in ELEMENTS and 0 for a
 * dimension the index is broadcast over.  `out` is f32[A, G, B] and `arg` is i64[A, G, B], both contiguous; G is the number of groups.
 *
 * The semantics, stated once (tests/scatter_ref.py restates them in numpy, and that restatement is the definition):
 *   out[a, g, b] = the maximum (op 0) or minimum (op 1) of src[a, e, b] over the e with index(a, e, b) == g.  Exact, so it does not
 *                  depend on execution order.  +0.0 is greater than -0.0.  A NaN in a group makes its result NaN (the canonical quiet
 *                  NaN, bits 0x7fc00000), whatever else the group holds.
 *   arg[a, g, b] = the position e of the winning element; among equal values (and among NaNs) the lowest e.
 *   A group with no member: out = 0 and arg = E.
 *   use_initial = 1: `out` holds initial values on entry.  An element replaces the value held only if it is strictly greater (op 0) or
 *                  smaller (op 1), or if it is a NaN and the value held is not; an initial value that is kept comes back with every
 *                  bit as it was, and its arg is E.  use_initial = 0: nothing is read from `out`.
 *   An index value outside [0, G) is skipped by the kernels: its element takes part in nothing (and its gradient is 0); nothing is
 *   ever written outside out, arg, scratch and grad_src.  Callers that want an error for it check the index themselves.
 *   Every element of out and arg is written exactly once (but a kept initial value, which stays).
 *
 * lidargs_scatter_extreme -- three launches, no float atomics.  `scratch` holds lidargs_scatter_scratch_bytes(A * G * B) bytes, 8-byte
 *   aligned: one 64-bit key (order-preserving image of the value << 32 | position code) per output element.  Nothing is assumed about
 *   its content and nothing is kept in it.
 * lidargs_scatter_extreme_backward -- one launch: grad_src[a, e, b] = arg[a, g, b] == e ? grad_out[a, g, b] : 0 with g = index(a, e, b).
 *   Every element of grad_src f32[A, E, B] is written once; grad_out is f32[A, G, B], contiguous.
 *
 * Each function returns 0, or a negative code with a message in lidargs_scatter_last_error() (thread-local): -1 an invalid argument
 * (op, use_initial, E >= 2^31 -- the position shares the key with the value --, a product of sizes that does not fit, a NULL pointer,
 * scratch too small or misaligned), -4 a HIP error.  Arguments are validated before any device work.  A * G * B == 0 (forward) and
 * A * E * B == 0 (backward) are valid and return 0 at once: there is nothing to write.
 */
#ifndef LIDARGS_SCATTER_H
#define LIDARGS_SCATTER_H

#include <stddef.h>

#define LIDARGS_SCATTER_ABI_VERSION 1
#define LIDARGS_SCATTER_MAX 0
#define LIDARGS_SCATTER_MIN 1

#ifdef __cplusplus
extern "C" {
#endif

size_t lidargs_scatter_scratch_bytes(size_t n_out);
int lidargs_scatter_extreme(int op, size_t A, size_t E, size_t B, size_t G, const float* src, const long long* index,
                            size_t sa, size_t se, size_t sb, int use_initial, float* out, long long* arg,
                            char* scratch, size_t scratch_bytes, void* stream);
int lidargs_scatter_extreme_backward(size_t A, size_t E, size_t B, size_t G, const long long* index, size_t sa, size_t se, size_t sb,
                                     const long long* arg, const float* grad_out, float* grad_src, void* stream);
const char* lidargs_scatter_last_error(void);
int lidargs_scatter_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
