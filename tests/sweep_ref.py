"""The sweep-motion compensation of include_sweep/lidargs_sweep.h restated in torch (float64 unless the inputs say otherwise): the
closed-form exponential, the iterates with the seam rule, x'.  Gradients come from autograd; `round` carries none.  Run on float32
inputs the same lines are the float32 framework-op chain the GPU tests and tools/time_sweep_motion.py compare the kernels with."""
import math

import torch

TWIST = (0.01, -0.02, 0.05, 1.5, 0.2, 0.05)     # the twist of the measurements quoted in DESIGN.md: 1.5 m and 3 degrees a sweep
SERIES_BELOW = 1e-2                             # theta^2 under which the three coefficients are their series (six terms: < 1e-17 off)


def generator_matrix(xi):
    """K of the definition: T(xi) = matrix_exp(K), row-vector convention."""
    K = xi.new_zeros(4, 4)
    K[2, 1], K[0, 2], K[1, 0] = xi[0], xi[1], xi[2]
    K[1, 2], K[2, 0], K[0, 1] = -xi[0], -xi[1], -xi[2]
    K[3, :3] = xi[3:]
    return K


def coefficients(m):
    """sin(th)/th, (1 - cos th)/th^2, (th - sin th)/th^3 of m = th^2 (any shape): series below SERIES_BELOW, closed form above."""
    small = m < SERIES_BELOW
    ms = torch.where(small, m, torch.zeros_like(m))                 # the series sees 0 where it is not taken (and has no gradient there)
    a = 1 + ms * (-1 / 6 + ms * (1 / 120 + ms * (-1 / 5040 + ms * (1 / 362880 + ms * (-1 / 39916800)))))
    b = 1 / 2 + ms * (-1 / 24 + ms * (1 / 720 + ms * (-1 / 40320 + ms * (1 / 3628800 + ms * (-1 / 479001600)))))
    c = 1 / 6 + ms * (-1 / 120 + ms * (1 / 5040 + ms * (-1 / 362880 + ms * (1 / 39916800 + ms * (-1 / 6227020800)))))
    ml = torch.where(small, torch.ones_like(m), m)                  # ... and the closed form a harmless 1
    th = ml.sqrt()
    return (torch.where(small, a, th.sin() / th), torch.where(small, b, (1 - th.cos()) / ml), torch.where(small, c, (th - th.sin()) / (ml * th)))


def se3_exp(xi):
    """T(xi) in closed form (Rodrigues + the V matrix), [4, 4]."""
    w, v = xi[:3], xi[3:]
    a, b, c = coefficients((w * w).sum())
    W = generator_matrix(xi)[:3, :3]
    T = xi.new_zeros(4, 4)
    T[:3, :3] = torch.eye(3, dtype=xi.dtype) + a * W + b * (W @ W)
    T[3, :3] = v @ (torch.eye(3, dtype=xi.dtype) + b * W + c * (W @ W))
    T[3, 3] = 1
    return T


def move(p, xi, t):
    """E(t) p = ([p, 1] @ T(t xi))[:3] for a time per point: p [P, 3], t [P].  (x @ K[:3, :3] is the cross product x × w.)"""
    w, u = xi[:3], t[:, None] * xi[3:]
    phi = t[:, None] * w
    a, b, c = (k[:, None] for k in coefficients((phi * phi).sum(1)))
    q, r = torch.linalg.cross(p, phi), torch.linalg.cross(u, phi)
    return p + u + a * q + b * (torch.linalg.cross(q, phi) + r) + c * torch.linalg.cross(r, phi)


def column_fraction(p):
    """s(p): the fraction of the image width, the column convention of both preprocess kernels."""
    return (math.pi - torch.atan2(p[:, 1], p[:, 0])) / (2 * math.pi)


def iterate(p0, xi, sweep, iterations):
    """s_n of the definition ([P]); later iterates stay on the branch of the previous one (the seam rule)."""
    t0, t1 = sweep
    s = column_fraction(p0)
    for _ in range(iterations - 1):
        raw = column_fraction(move(p0, xi, t0 + s * (t1 - t0)))
        s = raw + torch.round((s - raw).detach())
    return s


def compensate(x, vm, xi, sweep=(-0.5, 0.5), iterations=3, margin=None):
    """x' [P, 3].  margin: asserts that every p0 is at least that far (radians) from the image seam and rho >= 2 m, the domain on which
    float32 and float64 agree about the branch of s_1."""
    A, b = vm[:3, :3], vm[3, :3]
    p0 = x @ A + b
    if margin is not None:
        assert bool(((p0[:, 0] ** 2 + p0[:, 1] ** 2).sqrt() >= 2.0 - 1e-6).all())
        assert bool((torch.atan2(p0[:, 1], p0[:, 0]).abs() <= math.pi - margin).all())
    s = iterate(p0, xi, sweep, iterations)
    ps = move(p0, xi, sweep[0] + s * (sweep[1] - sweep[0]))
    return (ps - b) @ torch.linalg.inv(A)


def vjp(x, vm, xi, g, sweep=(-0.5, 0.5), iterations=3):
    """(x', dL/dx, dL/dvm, dL/dxi) for the upstream gradient g at x', in the dtype of the inputs (column 3 of dL/dvm is +0: nothing reads it)."""
    x, vm, xi = (t.detach().clone().requires_grad_(True) for t in (x, vm, xi))
    out = compensate(x, vm, xi, sweep, iterations)
    gx, gvm, gxi = torch.autograd.grad(out, (x, vm, xi), g)
    return out.detach(), gx, gvm, gxi


def points(P, seed, rho=(2.0, 60.0), margin=1e-3, seam=False, dtype=torch.float64):
    """P sensor-frame points: rho in U(rho), azimuth in U(-(pi - margin), pi - margin), height in U(-3, 3) -- or, seam=True, the seam
    scene: azimuth +-(pi - U(1e-3, 0.02)), rho in U(2, 10)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(P, 4, generator=g, dtype=torch.float64)
    if seam:
        az = (math.pi - (1e-3 + u[:, 0] * (0.02 - 1e-3))) * torch.where(u[:, 3] < 0.5, -1.0, 1.0)
        r = 2.0 + u[:, 1] * 8.0
    else:
        az = (2 * u[:, 0] - 1) * (math.pi - margin)
        r = rho[0] + u[:, 1] * (rho[1] - rho[0])
    return torch.stack([r * az.cos(), r * az.sin(), 6 * u[:, 2] - 3], 1).to(dtype)


def world_points(p_sensor, vm):
    """The world points whose sensor-frame images are p_sensor (float64 in, float64 out)."""
    return (p_sensor - vm[3, :3]) @ torch.linalg.inv(vm[:3, :3])
