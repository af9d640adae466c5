"""sweep_motion -- sweep-motion compensation: a rolling-shutter warp of the means in front of either rasterizer.

    x_warped = sweep_motion.compensate(means3D, viewmatrix, twist, sweep=(-0.5, 0.5), iterations=3)

A spinning sensor on a moving vehicle measures column c at its own time; a static world point x is captured at the time t* at which the
beam's azimuth meets it.  Rendering the static scene from the reference pose `viewmatrix` with x moved to where the sensor saw it at t*
gives the rolling-shutter image, so the motion model is a per-Gaussian warp of `means3D` and the rasterizers stay as they are.  The
definition (the chart of `twist`, the column fraction, the iterates and the seam rule, the limits) is stated once, in
include_sweep/lidargs_sweep.h; the kernels are csrc/sweep_motion.hip (lgsweep_forward / lgsweep_backward of liblidargs_hip.so).  There is
no CPU path and no fallback.

`se3_exp(xi)` is the same chart as framework ops, for building the pose of a time: `viewmatrix @ se3_exp(t * twist)`.
"""
import math

import torch

import lidargs_abi
from diff_lidargs_rasterization import _C as _base

_lib = _base._lib     # the process' one CDLL: lgsweep_* (include_sweep/lidargs_sweep.h) is typed on it with everything else
_ptr, _stream = lidargs_abi.ptr, lidargs_abi.stream
_POISON = lidargs_abi.poison_scratch()


def se3_exp(xi):
    """T(xi) [4, 4] of a twist xi = (w, v) [6]: matrix_exp of the generator K of INTEGRATION.md 3 (row-vector convention: a pose moves as
    `viewmatrix @ T`), in closed form -- Rodrigues and the V matrix, their coefficients as series below |w|^2 = 1e-2 -- and differentiable."""
    if xi.shape != (6,):
        raise RuntimeError("se3_exp: the twist must have shape (6,)")
    w, v = xi[:3], xi[3:]
    m = (w * w).sum()
    small = m < 1e-2
    ms, ml = torch.where(small, m, torch.zeros_like(m)), torch.where(small, torch.ones_like(m), m)
    th = ml.sqrt()
    a = torch.where(small, 1 + ms * (-1 / 6 + ms * (1 / 120 + ms * (-1 / 5040 + ms * (1 / 362880 + ms * (-1 / 39916800))))), th.sin() / th)
    b = torch.where(small, 1 / 2 + ms * (-1 / 24 + ms * (1 / 720 + ms * (-1 / 40320 + ms * (1 / 3628800 + ms * (-1 / 479001600))))), (1 - th.cos()) / ml)
    c = torch.where(small, 1 / 6 + ms * (-1 / 120 + ms * (1 / 5040 + ms * (-1 / 362880 + ms * (1 / 39916800 + ms * (-1 / 6227020800))))), (th - th.sin()) / (ml * th))
    z = torch.zeros_like(m)
    W = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device)
    WW = W @ W
    top = torch.cat([eye + a * W + b * WW, xi.new_zeros(3, 1)], 1)
    bottom = torch.cat([v @ (eye + b * W + c * WW), xi.new_ones(1)])
    return torch.cat([top, bottom[None]], 0)


def _checked(means3D, viewmatrix, twist, sweep, iterations):
    for t, name in ((means3D, "means3D"), (viewmatrix, "viewmatrix"), (twist, "twist")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"sweep_motion: `{name}` must be a tensor on a HIP device (device='cuda'); this build has no CPU path and does not fall back to one")
        if t.dtype != torch.float32:
            raise RuntimeError(f"sweep_motion: expected scalar type Float but found {t.dtype} for `{name}`")
    if means3D.ndim != 2 or means3D.size(1) != 3:
        raise RuntimeError("sweep_motion: means3D must have dimensions (num_points, 3)")
    if tuple(viewmatrix.shape) != (4, 4):
        raise RuntimeError("sweep_motion: viewmatrix must have dimensions (4, 4)")
    if tuple(twist.shape) != (6,):
        raise RuntimeError("sweep_motion: twist must have dimensions (6,)")
    if viewmatrix.device != means3D.device or twist.device != means3D.device:
        raise RuntimeError("sweep_motion: means3D, viewmatrix and twist must be on the same device")
    if not isinstance(iterations, int) or isinstance(iterations, bool) or not 1 <= iterations <= 4:
        raise ValueError("sweep_motion: iterations must be an integer in 1..4")
    t0, t1 = (float(t) for t in sweep)
    if not (math.isfinite(t0) and math.isfinite(t1)):
        raise ValueError("sweep_motion: the sweep times must be finite")
    return t0, t1


class _Compensate(torch.autograd.Function):
    """lgsweep_forward / lgsweep_backward.  Nothing is saved but the three inputs: the backward recomputes the forward."""

    @staticmethod
    def forward(ctx, means3D, viewmatrix, twist, t0, t1, iterations):
        m3, vm, xi = means3D.contiguous(), viewmatrix.contiguous(), twist.contiguous()
        out = torch.empty_like(m3)
        with torch.cuda.device(m3.device):
            rc = _lib.lgsweep_forward(int(m3.size(0)), _ptr(m3), _ptr(vm), _ptr(xi), t0, t1, iterations, _ptr(out), _stream(m3))
        lidargs_abi.check(_lib, rc, "sweep_motion.compensate")
        ctx.sweep = (t0, t1, iterations)
        ctx.save_for_backward(m3, vm, xi)     # (under torch.no_grad() autograd drops the context: nothing is kept)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        m3, vm, xi = ctx.saved_tensors
        t0, t1, iterations = ctx.sweep
        want_x, want_vm, want_xi = ctx.needs_input_grad[:3]
        P, dev = int(m3.size(0)), m3.device
        g = g_out.contiguous()
        g_x = torch.empty_like(m3)             # every row is written by the library
        # the 16 + 6 floats (all written by the library where asked for) in front of the partial rows: 128 bytes, so the rows stay whole lines
        n_part = int(_lib.lgsweep_partial_floats(P)) if (want_vm or want_xi) else 0
        slab = torch.empty(32 + n_part, dtype=torch.float32, device=dev)
        if _POISON:
            slab.fill_(float("nan"))
        g_vm, g_xi, partials = slab[:16].view(4, 4), slab[16:22], slab[32:]
        with torch.cuda.device(dev):
            rc = _lib.lgsweep_backward(P, _ptr(m3), _ptr(vm), _ptr(xi), t0, t1, iterations, _ptr(g), _ptr(g_x), _ptr(g_xi if want_xi else None),
                                       _ptr(g_vm if want_vm else None), _ptr(partials), n_part, _stream(dev))
        lidargs_abi.check(_lib, rc, "sweep_motion.compensate (backward)")
        return (g_x if want_x else None), (g_vm if want_vm else None), (g_xi if want_xi else None), None, None, None


def compensate(means3D, viewmatrix, twist, sweep=(-0.5, 0.5), iterations=3):
    """The world-space means x' [P, 3] to hand a rasterizer whose raster_settings.viewmatrix is `viewmatrix` (float32 [4, 4], as the
    kernels read it), for a sensor that moves by `twist` (float32 [6]: rotation vector, then translation, per unit of time) while the
    columns run from time sweep[0] to sweep[1].  The default sweep makes `viewmatrix` the mid-sweep pose and `twist` the motion per sweep;
    `iterations` (1..4) are the fixed-point steps for the capture time (three leave about a millimetre at 1.5 m per sweep).  Differentiable
    with respect to all three tensors; viewmatrix's share adds to what the rasterizer's own pose gradient returns.  Covariances are not
    rotated, and `prefilter_voxel` still sees the unwarped anchors (include_sweep/lidargs_sweep.h, "Limits")."""
    t0, t1 = _checked(means3D, viewmatrix, twist, sweep, iterations)
    if means3D.size(0) == 0:
        return means3D.new_empty((0, 3))
    return _Compensate.apply(means3D, viewmatrix, twist, t0, t1, iterations)
