"""`lidargs_optim.Adam` -- torch.optim.Adam's step for the whole model as ONE native launch (include_optim/lidargs_optim.h, csrc/adam.hip).

    from lidargs_optim import Adam
    self.optimizer = Adam(l, lr=0.0, eps=1e-15)          # scene/gaussian_model.py:390, the one edited line

`Adam` is a torch.optim.Optimizer: param_groups, per-parameter state (`step` a float32 CPU scalar tensor, `exp_avg`, `exp_avg_sq`:
torch's keys and types), state_dict() / load_state_dict() (interchangeable with torch.optim.Adam in both directions), zero_grad() and
add_param_group() are the base class's, so code that edits `optimizer.param_groups` and `optimizer.state` by hand -- the learning-rate
schedule, concatenating and pruning anchor rows, replacing a tensor -- works unchanged.  step() computes what torch.optim.Adam computes
on its default path (weight_decay = 0, amsgrad = False), rounded where torch's device kernels round; any other option is refused with
NotImplementedError, never emulated.

There is NO CPU path: a parameter that is not on a HIP device is a RuntimeError.  The step is not capturable in a HIP graph: the
learning rates and step counts are launch arguments, a replayed capture would repeat the captured ones.
"""
import ctypes as C

import torch

import lidargs_abi

_lib = lidargs_abi.library("optim")
ABI_VERSION = lidargs_abi.library_constants("optim")["LIDARGS_OPTIM_ABI_VERSION"]
MAX_TENSORS = _lib.lidargs_adam_max_tensors()


class _Tensor(C.Structure):
    """lidargs_adam_tensor of the header (the header parser types functions; a struct passed by pointer is mirrored here and its size
    is pinned by tests/test_optim_cpu.py against the C compiler's)."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("n", C.c_longlong),
                ("neg_step_size", C.c_float), ("inv_bias_correction2_sqrt", C.c_float)]


_Table = _Tensor * MAX_TENSORS


def _group_name(group, k):
    return f"group `{group['name']}`" if "name" in group else f"group {k}"


class Adam(torch.optim.Optimizer):
    """Drop-in for torch.optim.Adam(params, lr, betas, eps) on a HIP device; see the module docstring."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("lidargs_optim.Adam: a tensor `lr` is not supported (the learning rate is a launch argument)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        # the keys of torch.optim.Adam's defaults, so that a state_dict moves between the two classes as it is
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        for k, group in enumerate(self.param_groups):
            self._check_options(group, k)

    @staticmethod
    def _check_options(group, k):
        for key, allowed in (("weight_decay", (0, 0.0)), ("amsgrad", (False,)), ("maximize", (False,)), ("capturable", (False,)),
                             ("differentiable", (False,)), ("decoupled_weight_decay", (False,))):
            if group.get(key, allowed[0]) not in allowed or isinstance(group.get(key), torch.Tensor):
                raise NotImplementedError(f"lidargs_optim.Adam: {key}={group[key]!r} in {_group_name(group, k)} is not implemented "
                                          "(only torch.optim.Adam's default step is); there is no fallback to torch's")

    def _collect(self):
        """Per device, the (param, grad, exp_avg, exp_avg_sq, step tensor, lr, betas, eps) of every parameter with a gradient, checked."""
        per_device = {}
        for k, group in enumerate(self.param_groups):
            self._check_options(group, k)
            lr, betas, eps = group["lr"], group["betas"], group["eps"]
            if isinstance(lr, torch.Tensor) or isinstance(betas[0], torch.Tensor) or isinstance(betas[1], torch.Tensor):
                raise NotImplementedError(f"lidargs_optim.Adam: tensor hyper-parameters in {_group_name(group, k)} are not supported")
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError(f"lidargs_optim.Adam: a parameter of {_group_name(group, k)} is not on a HIP device "
                                       "(device='cuda'); there is no CPU step and no fallback to one")
                if g.is_sparse or g.layout != torch.strided:
                    raise RuntimeError(f"lidargs_optim.Adam: {_group_name(group, k)} has a sparse gradient; only dense ones are supported")
                if p.dtype != torch.float32 or g.dtype != torch.float32:
                    raise RuntimeError(f"lidargs_optim.Adam: {_group_name(group, k)} must be float32 with a float32 gradient, got {p.dtype} / {g.dtype}")
                if g.shape != p.shape or g.device != p.device:
                    raise RuntimeError(f"lidargs_optim.Adam: the gradient of {_group_name(group, k)} has shape {list(g.shape)} on {g.device}, "
                                       f"the parameter {list(p.shape)} on {p.device}")
                if not p.is_contiguous() or not g.is_contiguous():
                    raise RuntimeError(f"lidargs_optim.Adam: the parameter and gradient of {_group_name(group, k)} must be contiguous")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                for t, what in ((m, "exp_avg"), (v, "exp_avg_sq")):
                    if t.shape != p.shape or t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous():
                        raise RuntimeError(f"lidargs_optim.Adam: state `{what}` of {_group_name(group, k)} must be a contiguous float32 "
                                           f"tensor of the parameter's shape {list(p.shape)} on its device, got {list(t.shape)} {t.dtype} on {t.device}")
                per_device.setdefault(p.device, []).append((p, g, m, v, state["step"], lr, betas, eps))
        return per_device

    @torch.no_grad()
    def step(self, closure=None):
        """One Adam step of every parameter that has a gradient: one native launch per device and per (betas, eps) in use (the model's
        ten groups share one), more only beyond lidargs_adam_max_tensors() tensors.  Not capturable in a HIP graph."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for device, items in self._collect().items():
            calls = {}
            for it in items:
                calls.setdefault((it[6][0], it[6][1], it[7]), []).append(it)
            with torch.cuda.device(device):
                stream = lidargs_abi.stream(device)
                for (beta1, beta2, eps), its in calls.items():
                    for lo in range(0, len(its), MAX_TENSORS):
                        self._launch(its[lo:lo + MAX_TENSORS], beta1, beta2, eps, stream)
        return loss

    def _launch(self, items, beta1, beta2, eps, stream):
        table = _Table()
        for i, (p, g, m, v, step_t, lr, _betas, _eps) in enumerate(items):
            step_t += 1
            step = step_t.item()
            # in Python doubles, expression by expression as torch/optim/adam.py (_single_tensor_adam, the non-capturable branch)
            bias_correction1 = 1 - beta1 ** step
            bias_correction2 = 1 - beta2 ** step
            step_size = lr / bias_correction1
            bias_correction2_sqrt = bias_correction2 ** 0.5
            e = table[i]
            e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
            e.neg_step_size = -step_size
            e.inv_bias_correction2_sqrt = 1.0 / bias_correction2_sqrt      # torch's device kernel for tensor / python_float multiplies by this
        lidargs_abi.check(_lib, _lib.lidargs_adam_step(len(items), table, beta1, beta2, eps, stream), "lidargs_optim.Adam: step")
