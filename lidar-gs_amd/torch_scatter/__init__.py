"""`torch_scatter` -- a native stand-in for the part of torch_scatter the reference uses (scene/gaussian_model.py:15 imports
`scatter_max`, :742 calls it): with lidar-gs_amd/ on PYTHONPATH `import torch_scatter` resolves here and runs on the HIP kernels of
include_scatter/lidargs_scatter.h (csrc/scatter.hip, liblidargs_scatter.so; the entry `scatter` of build_hip.TARGETS).

    scatter_max(src, index, dim=-1, out=None, dim_size=None) -> (out, arg)
    scatter_min(src, index, dim=-1, out=None, dim_size=None) -> (out, arg)
    scatter(src, index, dim=-1, out=None, dim_size=None, reduce="max" | "min") -> out

The semantics are those of the header, which states them once (tests/scatter_ref.py restates them in numpy).  In short: `src` is a float32
tensor on a HIP device, `index` an int64 tensor that is 1-D (placed at `dim`) or broadcastable to src's shape by torch_scatter's rule; it is
never expanded in memory (unless its expanded view has no three strides; then it is copied).  Values are exact, +0.0 > -0.0, a NaN in a
group makes the result NaN; `arg` is the lowest winning position along `dim`; an empty group is (0, src.size(dim)); `out=` holds initial
values, which stay (with arg = src.size(dim)) unless an element is strictly greater / smaller.  The number of groups is `dim_size`, or
out.size(dim), or index.max() + 1; every call reads the index's range once (torch.aminmax) and a value outside [0, groups) is an IndexError.
The gradient goes to `src` only: grad_out at the `arg` positions, 0 elsewhere (torch_scatter's convention; torch.amax splits it among ties).

Everything else of torch_scatter (scatter_sum / add / mean / mul, the segment and composite ops) is NOT here: the name raises
NotImplementedError, which names torch's own device op.  There is NO CPU path and no fallback to framework ops.
"""
import torch

import lidargs_abi
from lidargs_abi import poison_scratch as _poison, ptr as _ptr, stream as _stream

__version__ = "2.1.2"   # the torch_scatter release whose signatures these are

_lib = lidargs_abi.library("scatter")
ABI_VERSION, MAX, MIN = (lidargs_abi.library_constants("scatter")["LIDARGS_SCATTER_" + k] for k in ("ABI_VERSION", "MAX", "MIN"))

__all__ = ["scatter_max", "scatter_min", "scatter"]

# torch_scatter's other public names -> torch's own device op for the same job
_NOT_HERE = {
    "scatter_sum": "Tensor.scatter_add_", "scatter_add": "Tensor.scatter_add_",
    "scatter_mean": "Tensor.scatter_reduce_(reduce='mean')", "scatter_mul": "Tensor.scatter_reduce_(reduce='prod')",
    "scatter_std": "Tensor.scatter_reduce_ (sum and sum of squares)", "scatter_logsumexp": "Tensor.scatter_reduce_ ('amax', then 'sum')",
    "scatter_softmax": "Tensor.scatter_reduce_ ('amax', then 'sum')", "scatter_log_softmax": "Tensor.scatter_reduce_ ('amax', then 'sum')",
    "segment_coo": "Tensor.scatter_reduce_", "segment_sum_coo": "Tensor.scatter_add_", "segment_add_coo": "Tensor.scatter_add_",
    "segment_mean_coo": "Tensor.scatter_reduce_(reduce='mean')", "segment_min_coo": "Tensor.scatter_reduce_(reduce='amin')",
    "segment_max_coo": "Tensor.scatter_reduce_(reduce='amax')", "gather_coo": "Tensor.gather",
    "segment_csr": "torch.segment_reduce", "segment_sum_csr": "torch.segment_reduce", "segment_add_csr": "torch.segment_reduce",
    "segment_mean_csr": "torch.segment_reduce", "segment_min_csr": "torch.segment_reduce", "segment_max_csr": "torch.segment_reduce",
    "gather_csr": "Tensor.gather",
}
_REDUCE_NOT_HERE = {"sum": "scatter_sum", "add": "scatter_add", "mean": "scatter_mean", "mul": "scatter_mul"}


def _not_here(name):
    return NotImplementedError(f"torch_scatter stand-in: `{name}` is not implemented (only scatter_max, scatter_min and "
                               f"scatter(reduce='max' | 'min') are); use torch's own device op, {_NOT_HERE[name]}. There is no fallback to it")


def __getattr__(name):
    if name in _NOT_HERE:
        raise _not_here(name)
    raise AttributeError(f"module 'torch_scatter' has no attribute '{name}'")


def _check(rc, what):
    lidargs_abi.check(_lib, rc, "torch_scatter stand-in: " + what)


def _typed(t, name, dtype, who):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{who}: `{name}` must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise RuntimeError(f"{who}: `{name}` must be {dtype}, got {t.dtype}")


def _on_device(t, name, who):
    if not t.is_cuda:
        raise RuntimeError(f"{who}: `{name}` is on {t.device}, not on a HIP device (device='cuda'); there is no CPU path and no fallback to one")


def _index_view(index, src, dim, who):
    """The index as an [A, E, B] view of src's element count: torch_scatter's `broadcast` (a 1-D index goes to `dim`, missing trailing
    dimensions are added, then expand), and the dimensions before and after `dim` folded.  Strides 0 where it is broadcast."""
    idx = index
    if idx.dim() == 1:
        for _ in range(dim):
            idx = idx.unsqueeze(0)
    for _ in range(idx.dim(), src.dim()):
        idx = idx.unsqueeze(-1)
    try:
        idx = idx.expand(src.shape)
    except RuntimeError:
        raise RuntimeError(f"{who}: an index of shape {list(index.shape)} does not broadcast to src's shape {list(src.shape)} at dim {dim}") from None
    A = 1
    for n in src.shape[:dim]:
        A *= n
    B = 1
    for n in src.shape[dim + 1:]:
        B *= n
    return idx.reshape(A, src.shape[dim], B)        # a view whenever three strides can express it (the usual cases all can), else a copy


class _Extreme(torch.autograd.Function):
    """src [A, E, B] contiguous, idx [A, E, B] (any strides), initial None or [A, G, B] contiguous -> (out [A, G, B], arg [A, G, B])."""

    @staticmethod
    def forward(ctx, src, idx, op, G, initial):
        A, E, B = src.shape
        out = torch.empty((A, G, B), dtype=torch.float32, device=src.device) if initial is None else initial
        arg = torch.empty((A, G, B), dtype=torch.int64, device=src.device)
        nb = _lib.lidargs_scatter_scratch_bytes(A * G * B)
        scratch = torch.empty(nb, dtype=torch.uint8, device=src.device)
        if _poison():
            scratch.fill_(0xFF)
        sa, se, sb = (s if n > 1 else 0 for s, n in zip(idx.stride(), idx.shape))
        with torch.cuda.device(src.device):
            _check(_lib.lidargs_scatter_extreme(op, A, E, B, G, _ptr(src), _ptr(idx), sa, se, sb, 0 if initial is None else 1,
                                                _ptr(out), _ptr(arg), _ptr(scratch), nb, _stream(src)), "scatter_extreme")
        if initial is not None:
            ctx.mark_dirty(initial)
        ctx.mark_non_differentiable(arg)
        ctx.save_for_backward(idx, arg)             # (idx is a view: what is kept is the caller's index)
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, _grad_arg):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        idx, arg = ctx.saved_tensors
        A, E, B = idx.shape
        G = arg.shape[1]
        _typed(grad_out, "grad_out", torch.float32, "torch_scatter stand-in (backward)")
        _on_device(grad_out, "grad_out", "torch_scatter stand-in (backward)")
        grad_out = grad_out.contiguous()
        grad_src = torch.empty((A, E, B), dtype=torch.float32, device=arg.device)
        sa, se, sb = (s if n > 1 else 0 for s, n in zip(idx.stride(), idx.shape))
        with torch.cuda.device(arg.device):
            _check(_lib.lidargs_scatter_extreme_backward(A, E, B, G, _ptr(idx), sa, se, sb, _ptr(arg), _ptr(grad_out), _ptr(grad_src),
                                                         _stream(arg)), "scatter_extreme_backward")
        return grad_src, None, None, None, None


def _extreme(op, who, src, index, dim, out, dim_size):
    who = "torch_scatter stand-in: " + who
    _typed(src, "src", torch.float32, who)
    _typed(index, "index", torch.int64, who)
    if out is not None:
        _typed(out, "out", torch.float32, who)
        if out.requires_grad:
            raise RuntimeError(f"{who}: `out` requires grad; the gradient goes to `src` only, so initial values cannot take one")
    for t, name in ((src, "src"), (index, "index"), (out, "out")):
        if t is not None:
            _on_device(t, name, who)
    if index.device != src.device:
        raise RuntimeError(f"{who}: `src` is on {src.device} and `index` on {index.device}")
    if src.dim() < 1:
        raise RuntimeError(f"{who}: `src` must have at least one dimension")
    if not -src.dim() <= dim < src.dim():
        raise RuntimeError(f"{who}: dim {dim} is out of range for a src of {src.dim()} dimensions")
    dim = dim % src.dim()
    E = src.shape[dim]
    if E >= 1 << 31:
        raise RuntimeError(f"{who}: src.size(dim) = {E}; the position shares a 64-bit key with the value and must be below 2^31")
    idx = _index_view(index, src, dim, who)
    if out is not None:
        if out.device != src.device or out.dim() != src.dim() or any(o != s for k, (o, s) in enumerate(zip(out.shape, src.shape)) if k != dim):
            raise RuntimeError(f"{who}: `out` of shape {list(out.shape)} on {out.device} does not match src's shape {list(src.shape)} outside dim {dim}")
        G = out.shape[dim]
    elif dim_size is not None:
        G = int(dim_size)
        if G < 0:
            raise RuntimeError(f"{who}: dim_size = {G}")
    else:
        G = None
    if index.numel() > 0:
        lo, hi = torch.stack(torch.aminmax(index)).tolist()         # the one host read of a call
        if G is None:
            G = hi + 1
        if lo < 0 or hi >= G:
            raise IndexError(f"{who}: the index holds values in [{lo}, {hi}], outside the {G} groups [0, {G})")
    elif G is None:
        G = 0
    shape = list(src.shape)
    shape[dim] = G
    A, B = idx.shape[0], idx.shape[2]
    if A * E * B == 0 or A * G * B == 0:            # nothing to reduce or nothing to write: every group (if any) is empty or keeps its initial value
        res = out if out is not None else torch.zeros(shape, dtype=torch.float32, device=src.device)
        return res, torch.full(shape, E, dtype=torch.int64, device=src.device)
    initial = None if out is None else out.detach().reshape(A, G, B).clone(memory_format=torch.contiguous_format)
    res, arg = _Extreme.apply(src.contiguous().view(A, E, B), idx, op, G, initial)
    res, arg = res.view(shape), arg.view(shape)
    if out is not None:
        res = out.copy_(res)                        # the caller's tensor comes back, as torch_scatter returns it
    return res, arg


def scatter_max(src, index, dim=-1, out=None, dim_size=None):
    """(out, arg): per group of `index` along `dim` the maximum of `src` and the lowest position that holds it."""
    return _extreme(MAX, "scatter_max", src, index, dim, out, dim_size)


def scatter_min(src, index, dim=-1, out=None, dim_size=None):
    """(out, arg): per group of `index` along `dim` the minimum of `src` and the lowest position that holds it."""
    return _extreme(MIN, "scatter_min", src, index, dim, out, dim_size)


def scatter(src, index, dim=-1, out=None, dim_size=None, reduce="sum"):
    """torch_scatter.scatter for reduce "max" / "min": the values only.  Every other reduction is refused."""
    if reduce == "max":
        return scatter_max(src, index, dim, out, dim_size)[0]
    if reduce == "min":
        return scatter_min(src, index, dim, out, dim_size)[0]
    if reduce in _REDUCE_NOT_HERE:
        raise _not_here(_REDUCE_NOT_HERE[reduce])
    raise ValueError(f"torch_scatter stand-in: unknown reduce {reduce!r} (torch_scatter knows sum, add, mul, mean, min, max)")
