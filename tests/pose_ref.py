"""The gradient of the 3-D rasterizer with respect to the sensor pose, restated: K1 (tests/preprocess_ref.py `k1`, `record`) once more
with a per-Gaussian copy of the view matrix as the leaf, differentiated by torch.autograd.  tests/test_pose_ref_cpu.py holds this file
against float64 autograd of the whole restated forward; tests/test_pose_gpu.py holds the HIP kernels against it.

`vm` is the 16 floats of the transposed world->lidar matrix, vm[4 r + k] = element [r][k] of the [4,4] tensor.  It enters K1 in two places:
the view-space mean pv[k] = sum_r vm[4r+k] p[r] + vm[12+k] and the world-space tangents t_i[r] = sum_k vm[4r+k] u_i[k].  Column 3 is
read by nobody.  The cotangents are the ones `preprocess_ref.chain` feeds: (gA, 2 gB, gC) on the conic, gdep on the range, gs on the
direction, du_i on the bases, through the damped `record` -- the reference's backward as written, not the analytic gradient.
"""
import numpy as np
import torch

import preprocess_ref as ref

F64 = ref.F64


def k1_per_gaussian(means, cov6, V):
    """preprocess_ref.k1 with one matrix per Gaussian, V [P,4,4] -> dict(pv, dist, dir, u1, u2, abc)."""
    A = V[:, :3, :3]
    pv = torch.einsum("pr,prk->pk", means, A) + V[:, 3, :3]
    dist = torch.sqrt((pv * pv).sum(-1))
    d = pv / dist[:, None]
    zero = torch.zeros_like(dist)
    u1 = torch.stack([d[:, 1], -d[:, 0], zero], -1)
    u1 = u1 / torch.sqrt((u1 * u1).sum(-1))[:, None]
    u2 = torch.linalg.cross(d, u1)
    t1, t2 = torch.einsum("prk,pk->pr", A, u1), torch.einsum("prk,pk->pr", A, u2)
    S = ref._sym(cov6)
    St1, St2 = torch.einsum("pij,pj->pi", S, t1), torch.einsum("pij,pj->pi", S, t2)
    d2 = dist * dist
    a = ((t1 * St1).sum(-1) + 0.01) / d2; b = (t1 * St2).sum(-1) / d2; c = ((t2 * St2).sum(-1) + 0.01) / d2
    return dict(pv=pv, dist=dist, dir=d, u1=u1, u2=u2, abc=torch.stack([a, b, c], -1))


def contributions(line, means, scales, rots, vm, mod=1.0, cov3D=None, dtype=F64):
    """c [P,16] (numpy float64 holding values computed in `dtype`): what each Gaussian's packed gradient line `line` [P,16]
    (preprocess_ref.LINE_SLOTS) adds to dL/dvm.  A Gaussian at range 0 adds nothing (the chain's early return), and neither does one
    whose line is all zeros (the chain is linear in the line; such a Gaussian is not touched and never reaches it)."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dtype)
    line_all = np.asarray(line, np.float64)
    P = line_all.shape[0]
    V0 = np.asarray(vm, np.float64).reshape(4, 4)
    with np.errstate(all="ignore"):
        pv0 = np.asarray(means, np.float64) @ V0[:3, :3] + V0[3, :3]
    act = np.nonzero((np.abs(line_all).sum(1) > 0) & ((pv0 * pv0).sum(1) > 0))[0]
    c = np.zeros((P, 16))
    if act.size == 0:
        return c
    line = t(line_all[act])
    means_t = t(np.asarray(means)[act])
    if cov3D is None:
        c6 = ref.cov6_of(t(np.float32(mod)) * t(np.asarray(scales)[act]), t(np.asarray(rots)[act]))
    else:
        c6 = t(np.asarray(cov3D)[act])
    V = t(V0).expand(act.size, 4, 4).clone().requires_grad_(True)
    k = k1_per_gaussian(means_t, c6, V)
    r = ref.record(k, damped=True)
    gx, gy = line[:, 0], line[:, 1]
    G1, G2 = line[:, 10:13], line[:, 13:16]
    with torch.no_grad():
        u1p, u2p = r["u1p"], r["u2p"]
        du1 = (u1p * u1p).sum(-1)[:, None] * G1 - 2 * u1p * (u1p * G1).sum(-1)[:, None]
        du2 = (u2p * u2p).sum(-1)[:, None] * G2 - 2 * u2p * (u2p * G2).sum(-1)[:, None]
        gs = gx[:, None] * u1p + gy[:, None] * u2p
        gcon = torch.stack([line[:, 3], 2 * line[:, 4], line[:, 5]], -1)
    L = (r["conic"] * gcon).sum() + (k["dist"] * line[:, 9]).sum() + (k["u1"] * du1).sum() + (k["u2"] * du2).sum() + (k["dir"] * gs).sum()
    (g,) = torch.autograd.grad(L, [V])
    c[act] = g.detach().to(F64).numpy().reshape(act.size, 16)
    return c
