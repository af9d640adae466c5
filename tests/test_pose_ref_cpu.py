"""tests/pose_ref.py -- the yardstick of the pose gradient (dL/dviewmatrix) -- held against float64 autograd, without a GPU.

  chain sum    pose_ref on the packed lines of an oracle backward, summed over the Gaussians, against torch.autograd of the whole
               restated forward (K1 as the source writes it + the per-pixel loop) with the 16 floats of the view matrix as the leaf:
               the construction, scene and bars of tests/test_oracle_autograd_cpu.py's whole-chain test.  Nobody's reading of backward.cu
               and no hand-derived formula is involved on the autograd side.  Worst relative error measured over the 12 entries: 1.4e-4.
  translation  the translation row of the sum equals sum_i dL_dmeans3D_i @ V[:3,:3] on the oracle's own mean gradients (the matrix of a
               rigid view is orthonormal, so A^T undoes the A the chain's last step applies).
"""
import numpy as np
import pytest
import torch

import pose_ref
import preprocess_ref as ref
from test_oracle_autograd_cpu import F64, H_, P_, W_, _blend, _close, _k1, _lists_of, _loss, _pixel_dirs, _scene
from oracle import lgo
import lidargs_scenes as sc


@pytest.fixture(scope="module")
def run():
    scene = _scene(P_, H_, 41)
    grads = sc.upstream_grads(H_, W_, 41)
    f = lgo.forward(scene["means3D"], scene["colors"], scene["opacities"], scene["scales"], scene["rotations"], scene["viewmatrix"],
                    scene["beams"], W_, H_, bg=scene["bg"])
    g = lgo.backward(f, *grads)
    f64 = ref.forward64(scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"])
    line = ref.line_from_oracle(g, np.nan_to_num(f64["u1"]), np.nan_to_num(f64["u2"]))
    c = pose_ref.contributions(line, scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"])
    return scene, grads, f, g, c


def test_chain_sum_is_autograd_of_the_whole_forward_with_the_matrix_as_leaf(run):
    scene, grads, f, g, c = run
    P = scene["means3D"].shape[0]
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=F64)
    means, scales, rots = t(scene["means3D"]), t(scene["scales"]), t(scene["rotations"])
    opac, colors = t(scene["opacities"][:, 0]), t(scene["colors"])
    vm = t(np.asarray(scene["viewmatrix"]).reshape(16)).requires_grad_(True)
    vis = f.radii > 0
    conic, depth, u1, u2, sph = [], [], [], [], []
    z3 = torch.zeros(3, dtype=F64)
    for i in range(P):
        if not vis[i]:
            conic.append(z3); depth.append(torch.zeros((), dtype=F64)); u1.append(z3); u2.append(z3); sph.append(z3)
            continue
        abc, dist, a1, a2, s, _ = _k1(means[i], scales[i], rots[i], vm)
        det = abc[0] * abc[2] - abc[1] * abc[1]
        k = (det * det / (det * det + 1e-7)).detach()                   # the damped conic (R3/cr/backward.cu:237), as a scale on the gradient
        ar, br, cr = abc * k + (abc * (1 - k)).detach()
        detr = ar * cr - br * br
        conic.append(torch.stack([cr / detr, -br / detr, ar / detr]))
        depth.append(dist); u1.append(a1); u2.append(a2); sph.append(s)
    conic, depth, u1, u2, sph = torch.stack(conic), torch.stack(depth), torch.stack(u1), torch.stack(u2), torch.stack(sph)
    margins = []
    img = _blend(_lists_of(f, W_, H_), _pixel_dirs(W_, H_, scene["beams"]), W_, H_, conic, opac, colors, depth, u1, u2, sph,
                 torch.zeros(P, 2, dtype=F64), torch.as_tensor(scene["bg"], dtype=F64), margins)
    assert min(margins) > 1e-5
    (gvm,) = torch.autograd.grad(_loss(img, grads), [vm])
    gvm = gvm.numpy()
    got = c.sum(0)
    used = [4 * r + k for r in range(4) for k in range(3)]
    print("[pose] autograd:", gvm[used])
    print("[pose] chain sum:", got[used])
    print("[pose] relative error per entry:", np.abs(got[used] - gvm[used]) / np.abs(gvm[used]))
    assert np.abs(gvm[used]).min() > 0
    _close("dL_dviewmatrix", got[used], gvm[used])
    for k in (3, 7, 11, 15):                                            # column 3 is read by no formula
        assert got[k] == 0.0 and gvm[k] == 0.0
        assert not c[:, k].any()


def test_translation_row_is_the_mean_gradients_rotated_back(run):
    scene, grads, f, g, c = run
    V = np.asarray(scene["viewmatrix"], np.float64).reshape(4, 4)
    assert np.allclose(V[:3, :3] @ V[:3, :3].T, np.eye(3), atol=1e-6)   # a rigid view
    want = g["dL_dmeans3D"].astype(np.float64).sum(0) @ V[:3, :3]
    got = c.sum(0)[12:15]
    print("[pose] translation row:", got, "rotated mean gradients:", want, "relative:", np.abs(got - want) / np.abs(want))
    _close("translation row", got, want)
