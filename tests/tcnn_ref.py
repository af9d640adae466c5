"""A plain torch restatement of the part of tinycudann the stand-in covers (lidar-gs_amd/tinycudann): the Frequency encoding and the
bias-free ReLU MLP over the documented `params` layout.  TEST INFRASTRUCTURE ONLY.

The definition is RESTATED FROM TINYCUDANN'S DOCUMENTATION and is NOT pinned against tinycudann itself: tinycudann is CUDA-only and
cannot be executed where these tests run, so there is no fixture from it.  What is pinned (tests/test_tcnn_cpu.py): the column layout
against a loop-written float64 evaluation, and the hand-written gradients against float64 autograd.

    encoding   out[:, d*2F + 2f + s] = sin(pi * 2^f * x_d + s * pi/2)                 s = 0 sine, s = 1 cosine
    network    h_0 = x, h_i = relu(h_{i-1} W_i^T), out = act(h_h W_out^T); `params` = W_1 [128, n_in], W_2 .. W_h [128, 128],
               W_out [n_out, 128], each row-major [out, in], concatenated in that order; no biases

Every function takes a `dtype`: float64 is the expectation, float32 on the device is "the same model as framework ops" the native
kernels are measured against.
"""
import math

import torch
import torch.nn.functional as F_

WIDTH = 128


def encode(x, n_frequencies, dtype=torch.float64):
    """[N, D] -> [N, D * 2F]; differentiable."""
    x = x.to(dtype)
    scale = math.pi * (2.0 ** torch.arange(n_frequencies, dtype=dtype, device=x.device))
    arg = x[:, :, None] * scale                                               # [N, D, F]
    return torch.stack((torch.sin(arg), torch.cos(arg)), dim=-1).reshape(x.shape[0], -1)


def encode_grad(x, dout, n_frequencies, dtype=torch.float64):
    """dL/dx of encode(), written out: sum_f pi 2^f (cos(.) dout[.., 2f] - sin(.) dout[.., 2f + 1])."""
    x, dout = x.to(dtype), dout.to(dtype)
    scale = math.pi * (2.0 ** torch.arange(n_frequencies, dtype=dtype, device=x.device))
    arg = x[:, :, None] * scale
    d = dout.reshape(x.shape[0], x.shape[1], n_frequencies, 2)
    return (scale * (torch.cos(arg) * d[..., 0] - torch.sin(arg) * d[..., 1])).sum(-1)


def layer_shapes(n_in, n_hidden_layers, n_out):
    return [(WIDTH, n_in)] + [(WIDTH, WIDTH)] * (n_hidden_layers - 1) + [(n_out, WIDTH)]


def split_params(params, n_in, n_hidden_layers, n_out):
    """The matrices of the flat `params`, as views."""
    mats, o = [], 0
    for r, c in layer_shapes(n_in, n_hidden_layers, n_out):
        mats.append(params[o:o + r * c].view(r, c))
        o += r * c
    assert o == params.numel(), (o, params.numel())
    return mats


def mlp(x, params, n_hidden_layers, n_out, sigmoid, dtype=torch.float64):
    """[N, n_in] -> [N, n_out]; differentiable in x and params."""
    h = x.to(dtype)
    mats = split_params(params.to(dtype), x.shape[1], n_hidden_layers, n_out)
    for W in mats[:-1]:
        h = torch.relu(F_.linear(h, W))
    y = F_.linear(h, mats[-1])
    return torch.sigmoid(y) if sigmoid else y


def mlp_grads(x, params, dout, n_hidden_layers, n_out, sigmoid, dtype=torch.float64):
    """(out, dL/dparams, dL/dx) with the backward written out layer by layer."""
    mats = split_params(params.to(dtype), x.shape[1], n_hidden_layers, n_out)
    hs = [x.to(dtype)]
    for W in mats[:-1]:
        hs.append(torch.relu(hs[-1] @ W.t()))
    y = hs[-1] @ mats[-1].t()
    out = torch.sigmoid(y) if sigmoid else y
    delta = dout.to(dtype) * (out * (1 - out) if sigmoid else 1.0)
    grads = [None] * len(mats)
    grads[-1] = delta.t() @ hs[-1]
    delta = (delta @ mats[-1]) * (hs[-1] > 0)
    for i in range(len(mats) - 2, -1, -1):
        grads[i] = delta.t() @ hs[i]
        delta = delta @ mats[i]
        if i > 0:
            delta = delta * (hs[i] > 0)
    return out, torch.cat([g.reshape(-1) for g in grads]), delta
