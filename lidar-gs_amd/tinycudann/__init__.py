"""`import tinycudann as tcnn` on a ROCm machine: a native stand-in for the part of tinycudann the reference's ray-drop refinement
network uses (scene/extre_train_raydrop.py) -- `Encoding` with otype "Frequency" and `Network` with otype "FullyFusedMLP" /
"CutlassMLP" (include_tcnn/lidargs_tcnn.h, csrc/raydrop_mlp.hip, liblidargs_tcnn.so).

    self.enc_dir = tcnn.Encoding(n_input_dims=3, encoding_config={"otype": "Frequency", "degree": 4}).cuda()
    self.unet = tcnn.Network(n_input_dims=..., n_output_dims=1, network_config={"otype": "FullyFusedMLP", "activation": "ReLU",
                             "output_activation": "Sigmoid", "n_neurons": 128, "n_hidden_layers": 4})

Both are torch.nn.Modules with one flat float32 parameter `params` (empty for the encoding).  What differs from tinycudann, on purpose:
  * everything is float32 (tinycudann computes and returns half);
  * `Network.params` is the matrices W_1 [128, n_in], W_2 .. W_h [128, 128], W_out [n_out, 128], each ROW-MAJOR [out, in], concatenated
    in that order, Xavier-uniform from a torch.Generator seeded with `seed`; a tinycudann checkpoint does not load (its layout and
    padding are not known here);
  * config keys the stand-in does not know (the reference's "degree") are ignored with a warning; every other encoding, activation,
    width, composite encodings, NetworkWithInputEncoding and dtype=torch.half raise NotImplementedError.
There is NO CPU path and no fallback to framework ops: an input that is not a float32 tensor on a HIP device is a RuntimeError.
"""
import math

import torch

import lidargs_abi
from lidargs_abi import poison_scratch as _poison, ptr as _ptr, stream as _stream
from . import _config
from ._config import layer_shapes, parse_encoding, parse_network  # noqa: F401

_lib = lidargs_abi.library("tcnn")
ABI_VERSION = _config.CONSTANTS["LIDARGS_TCNN_ABI_VERSION"]
FORWARD_ROW_TILE = _lib.lidargs_tcnn_forward_row_tile()
BACKWARD_ROW_TILE = _lib.lidargs_tcnn_backward_row_tile()

__all__ = ["Encoding", "Network", "NetworkWithInputEncoding"]


def _check(rc, what):
    lidargs_abi.check(_lib, rc, "tinycudann stand-in: " + what)


def _checked_input(x, width, who):
    if not isinstance(x, torch.Tensor):
        raise RuntimeError(f"{who}: the input must be a torch.Tensor, got {type(x).__name__}")
    if not x.is_cuda:
        raise RuntimeError(f"{who}: the input is on {x.device}, not on a HIP device (device='cuda'); there is no CPU path and no fallback to one")
    if x.dtype != torch.float32:
        raise RuntimeError(f"{who}: the input must be float32, got {x.dtype}")
    if x.dim() != 2 or x.shape[1] != width:
        raise RuntimeError(f"{who}: the input must be [N, {width}], got {list(x.shape)}")
    if x.shape[0] > 2 ** 31 - 1:
        raise RuntimeError(f"{who}: {x.shape[0]} rows are more than one call takes (2^31 - 1)")
    return x.contiguous()


def frequency_forward(x, n_frequencies):
    """out [N, D * 2F] of a contiguous float32 device tensor x [N, D]."""
    n, d = x.shape
    out = torch.empty((n, d * 2 * n_frequencies), dtype=torch.float32, device=x.device)
    if n:
        with torch.cuda.device(x.device):
            _check(_lib.lidargs_tcnn_frequency_forward(n, d, n_frequencies, _ptr(x), _ptr(out), _stream(x)), "frequency_forward")
    return out


def frequency_backward(x, dout, n_frequencies):
    n, d = x.shape
    dx = torch.empty_like(x)
    if n:
        with torch.cuda.device(x.device):
            _check(_lib.lidargs_tcnn_frequency_backward(n, d, n_frequencies, _ptr(x), _ptr(dout), _ptr(dx), _stream(x)), "frequency_backward")
    return dx


def mlp_forward(x, params, n_hidden_layers, n_out, out_act):
    n, n_in = x.shape
    out = torch.empty((n, n_out), dtype=torch.float32, device=x.device)
    if n:
        with torch.cuda.device(x.device):
            _check(_lib.lidargs_tcnn_mlp_forward(n, n_in, n_hidden_layers, n_out, out_act, _ptr(params), _ptr(x), _ptr(out), _stream(x)), "mlp_forward")
    return out


def mlp_backward(x, params, dout, n_hidden_layers, n_out, out_act, want_dx, scratch=None):
    """(dparams, dx or None).  `scratch` (tests) replaces the partial-gradient buffer the call would allocate."""
    n, n_in = x.shape
    dparams = torch.empty_like(params)
    dx = torch.empty_like(x) if want_dx else None
    with torch.cuda.device(x.device):
        need = _lib.lidargs_tcnn_backward_partial_floats(n, n_in, n_hidden_layers, n_out)
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.float32, device=x.device)
            if _poison():
                scratch.view(torch.uint8).fill_(0xFF)
        _check(_lib.lidargs_tcnn_mlp_backward(n, n_in, n_hidden_layers, n_out, out_act, _ptr(params), _ptr(x), _ptr(dout), _ptr(dparams),
                                              _ptr(dx), _ptr(scratch), scratch.numel(), _stream(x)), "mlp_backward")
    return dparams, dx


class _FrequencyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n_frequencies):
        ctx.save_for_backward(x)
        ctx.n_frequencies = n_frequencies
        return frequency_forward(x, n_frequencies)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or x.shape[0] == 0:
            return (torch.zeros_like(x) if ctx.needs_input_grad[0] else None), None
        return frequency_backward(x, dout.contiguous().float(), ctx.n_frequencies), None


class _MlpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, n_hidden_layers, n_out, out_act):
        ctx.save_for_backward(x, params)            # the inputs only: the backward recomputes the hidden activations
        ctx.cfg = (n_hidden_layers, n_out, out_act)
        return mlp_forward(x, params, n_hidden_layers, n_out, out_act)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x, params = ctx.saved_tensors
        want_dx = ctx.needs_input_grad[0]
        if x.shape[0] == 0:
            return (torch.zeros_like(x) if want_dx else None), (torch.zeros_like(params) if ctx.needs_input_grad[1] else None), None, None, None
        dparams, dx = mlp_backward(x, params, dout.contiguous().float(), *ctx.cfg, want_dx)
        return dx, (dparams if ctx.needs_input_grad[1] else None), None, None, None


class Encoding(torch.nn.Module):
    """tcnn.Encoding for otype "Frequency": out[:, d*2F + 2f + s] = sin(pi 2^f x_d + s pi/2), float32 [N, n_input_dims * 2F]."""

    def __init__(self, n_input_dims, encoding_config, seed=1337, dtype=None):
        super().__init__()
        if dtype not in (None, torch.float32):
            raise NotImplementedError(f"tinycudann stand-in: Encoding dtype={dtype!r} is not implemented (everything is float32, "
                                      "dtype=torch.half included); there is no fallback to framework ops")
        cfg = parse_encoding(n_input_dims, encoding_config)
        self.n_input_dims = n_input_dims
        self.n_frequencies = cfg["n_frequencies"]
        self.n_output_dims = cfg["n_output_dims"]
        self.encoding_config = dict(encoding_config)
        self.seed = seed
        self.dtype = torch.float32
        self.params = torch.nn.Parameter(torch.zeros(0, dtype=torch.float32))

    def forward(self, x):
        x = _checked_input(x, self.n_input_dims, "tinycudann.Encoding")
        if torch.is_grad_enabled() and x.requires_grad:
            return _FrequencyFn.apply(x, self.n_frequencies)
        return frequency_forward(x, self.n_frequencies)

    def extra_repr(self):
        return f"n_input_dims={self.n_input_dims}, n_output_dims={self.n_output_dims}, n_frequencies={self.n_frequencies}, float32"


class Network(torch.nn.Module):
    """tcnn.Network for otype "FullyFusedMLP" / "CutlassMLP": 128 neurons, ReLU, no biases, output activation None or Sigmoid."""

    def __init__(self, n_input_dims, n_output_dims, network_config, seed=1337):
        super().__init__()
        cfg = parse_network(n_input_dims, n_output_dims, network_config)
        self.n_input_dims = n_input_dims
        self.n_output_dims = n_output_dims
        self.n_hidden_layers = cfg["n_hidden_layers"]
        self.out_act = cfg["out_act"]
        self.network_config = dict(network_config)
        self.seed = seed
        self.dtype = torch.float32
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        parts = []
        for fan_out, fan_in in layer_shapes(n_input_dims, self.n_hidden_layers, n_output_dims):
            bound = math.sqrt(6.0 / (fan_in + fan_out))             # Xavier-uniform
            parts.append(((torch.rand(fan_out * fan_in, generator=gen, dtype=torch.float32) * 2 - 1) * bound))
        self.params = torch.nn.Parameter(torch.cat(parts))
        assert self.params.numel() == cfg["n_params"] == _lib.lidargs_tcnn_param_count(n_input_dims, self.n_hidden_layers, n_output_dims)

    def forward(self, x):
        x = _checked_input(x, self.n_input_dims, "tinycudann.Network")
        p = self.params
        if not p.is_cuda or p.device != x.device:
            raise RuntimeError(f"tinycudann.Network: `params` is on {p.device}, the input on {x.device}; move the module with .cuda()")
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError(f"tinycudann.Network: `params` must be a contiguous float32 tensor, got {p.dtype}")
        if torch.is_grad_enabled() and (x.requires_grad or p.requires_grad):
            return _MlpFn.apply(x, p, self.n_hidden_layers, self.n_output_dims, self.out_act)
        return mlp_forward(x, p.detach(), self.n_hidden_layers, self.n_output_dims, self.out_act)

    def extra_repr(self):
        return (f"n_input_dims={self.n_input_dims}, n_output_dims={self.n_output_dims}, n_hidden_layers={self.n_hidden_layers}, "
                f"output_activation={'Sigmoid' if self.out_act else 'None'}, float32")


class NetworkWithInputEncoding(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()
        raise NotImplementedError("tinycudann stand-in: NetworkWithInputEncoding is not implemented (build an Encoding and a Network and "
                                  f"concatenate, as the reference does); got args={args!r} kwargs={kwargs!r}")
