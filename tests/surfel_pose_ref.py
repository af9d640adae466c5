"""The gradient of the surfel rasterizer with respect to the sensor pose, restated: the formula of include_surfel_pose/lidargs_surfel_pose.h
vectorised over surfels from the packed 32-slot line (surfel_ref.SLOT).  tests/test_surfel_pose_ref_cpu.py holds this file against
float64 autograd of the forward with the matrix as the only leaf; tests/test_surfel_pose_gpu.py holds the HIP kernels against it.

`vm` is the 16 floats of the transposed world->lidar matrix, vm[4 r + k] = element [r][k] of the [4,4] tensor.  The surfel preprocess reads
it in four rows (surfel_ref.rows_of):
    Tu[k] = sum_r vm[4r+k] m s0 c0[r]     Tv[k] = sum_r vm[4r+k] m s1 c1[r]     Tw[k] = sum_r vm[4r+k] p[r] + vm[12+k]     n[k] = sg sum_r vm[4r+k] c2[r]
(c0, c1, c2: the columns of the rotation of the normalised quaternion, m = scale_modifier, sg = +1 where -(Tw . n) > 0, else -1), so a
surfel adds   dL/dvm[4r+k] += p[r] gTw[k] + m s0 c0[r] gTu[k] + m s1 c1[r] gTv[k] + sg c2[r] gn[k]   and   dL/dvm[12+k] += gTw[k],
gTw being the FINAL dL/dTw, built from the line exactly as surfel_ref.chain builds it (which is why the beam table and the image size
are arguments: the 2-D branch's terms hang on them).  Column 3 is read by nobody.
"""
import numpy as np
import torch

import surfel_ref as ref

F64 = ref.F64


def contributions(line, means, scales, rots, vm, beams, W, H, mod=1.0, dtype=F64):
    """c [P,16] (numpy float64 holding values computed in `dtype`): what each surfel's packed gradient line `line` [P,32] adds to dL/dvm.
    A surfel whose live slots are all zero adds nothing (the formula is linear in the line; such a surfel is not touched and never
    reaches the chain); the dead slots are not read."""
    line_all = np.asarray(line, np.float64)
    P = line_all.shape[0]
    c = np.zeros((P, 16))
    act = np.nonzero(np.abs(line_all[:, list(ref.LIVE)]).sum(1) > 0)[0]
    if act.size == 0:
        return c
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dtype)
    ln = t(line_all[act])
    sl = lambda k: ln[:, list(ref.SLOT[k])]
    p, s = t(np.asarray(means)[act]), t(np.float32(mod)) * t(np.asarray(scales)[act])
    q = t(np.asarray(rots)[act])
    qn = q / torch.sqrt((q * q).sum(-1, keepdim=True))
    vmt = t(np.asarray(vm).reshape(16))
    c0, c1, c2 = ref.quat_cols(qn)
    _, _, Tw, nv = ref.rows_of(p, s, qn, vmt)
    # the final dL/dTw, as surfel_ref.chain (transMat = None: Tw = p_view)
    ddelx, ddely = ref.ddel_dTw(Tw, beams, W, H)
    rho_r = torch.sqrt((Tw * Tw).sum(-1, keepdim=True))
    m2x, m2y = sl("M2X")[:, 0], sl("M2Y")[:, 0]
    gTw = sl("TW") + sl("Z2D") * Tw / rho_r + m2x[:, None] * ddelx + m2y[:, None] * ddely
    gTu, gTv, gn = sl("TU"), sl("TV"), sl("N")
    sg = torch.where(-(Tw * nv).sum(-1) > 0, 1.0, -1.0).to(dtype)[:, None]
    # block[i, r, k] = dL/dvm[4r+k] of surfel i
    outer = lambda a, b: a[:, :, None] * b[:, None, :]
    block = outer(p, gTw) + outer(c0 * s[:, 0:1], gTu) + outer(c1 * s[:, 1:2], gTv) + outer(sg * c2, gn)
    out = torch.zeros((act.size, 4, 4), dtype=dtype)
    out[:, :3, :3] = block
    out[:, 3, :3] = gTw
    c[act] = out.to(F64).numpy().reshape(act.size, 16)
    return c
