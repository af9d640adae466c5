/*
 * lidargs_optim.h -- C ABI of the optimizer step (liblidargs_optim.so, built from csrc/adam.hip alone).
 *
 * lidargs_adam_step replaces gaussians.optimizer.step() of the reference's training iteration (train.py:256), where the optimizer is
 * torch.optim.Adam(l, lr=0.0, eps=1e-15) over ten parameter groups (scene/gaussian_model.py:372-390): ONE launch updates every tensor
 * of the table.  The table travels inside the kernel argument: no host-to-device copy, no device allocation, no host synchronisation.
 *
 * What is computed is torch.optim.Adam's default (non-capturable, single-tensor) path with weight_decay = 0 and amsgrad = False, each
 * operation rounded to float32 where torch's device kernels round (DESIGN.md section "Optimizer step"):
 *   w1 = (float)(1 - beta1), b2 = (float)beta2, w2 = (float)(1 - beta2), e = (float)eps            (1 - beta in double, as Python does)
 *   m  = w1 < 0.5 ? fma(w1, g - m, m) : fma(-(g - m), 1 - w1, g)                                  exp_avg.lerp_(grad, 1 - beta1)
 *   v  = fma(w2, g * g, v * b2)                                                                     exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
 *   d  = sqrt(v) * inv_bias_correction2_sqrt + e                                                    (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
 *   p  = fma(neg_step_size, m / d, p)                                                               param.addcdiv_(exp_avg, denom, value=-step_size)
 * sqrt and the division are correctly rounded.  The two per-tensor scalars are the caller's, computed in double as torch's Python
 * does and rounded to float once:
 *   neg_step_size = (float)(-(lr / (1 - beta1 ** step)));   inv_bias_correction2_sqrt = (float)(1 / (1 - beta2 ** step) ** 0.5)
 *
 * An entry with n == 0 costs nothing and its pointers are not looked at.  An entry whose four pointers are not all 16-byte aligned is
 * updated with 4-byte accesses.  The tensors of one call must not overlap.  Returns 0, or a negative code with a message in
 * lidargs_optim_last_error() (thread-local): -1 for an invalid argument (n_tensors outside [0, lidargs_adam_max_tensors()], a NULL
 * table, a negative n, a NULL pointer with n > 0, more than 2^31 - 1 chunks in all), -4 for a HIP error.  Arguments are validated
 * before any device work.  lr and step are launch arguments: a captured HIP graph would replay the values of the capture.
 */
#ifndef LIDARGS_OPTIM_H
#define LIDARGS_OPTIM_H

#define LIDARGS_OPTIM_ABI_VERSION 1
#define LIDARGS_ADAM_MAX_TENSORS 64

typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long n;                          /* elements */
    float neg_step_size;
    float inv_bias_correction2_sqrt;
} lidargs_adam_tensor;

#ifdef __cplusplus
extern "C" {
#endif

int lidargs_adam_step(int n_tensors, const lidargs_adam_tensor* table, double beta1, double beta2, double eps, void* stream);
int lidargs_adam_max_tensors(void);
const char* lidargs_optim_last_error(void);
int lidargs_optim_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
