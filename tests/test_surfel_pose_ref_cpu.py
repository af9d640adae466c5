"""tests/surfel_pose_ref.py -- the yardstick of the surfel pose gradient (dL/dviewmatrix) -- held against float64 autograd, without a GPU.

  (i) chain sum     the restatement on the packed lines of a surfel-oracle backward (surfel_ref.line_from_oracle), summed over the
                    surfels, against torch.autograd of the forward with the 16 floats of the view matrix as the ONLY leaf:
                    surfel_ref.rows_of(vm) -> the differentiable blend `_blend` of tests/test_surfel_oracle_autograd_cpu.py -> a fixed
                    random cotangent on all nine planes.  The detachments are that file's: the normal's flip is a constant sign, and the
                    projected centre (x, y) follows Tw through the reference's stated linearisation on the average beam spacing
                    (R2/cr/backward.cu:590-598) -- written here as xy = xy0 + J (Tw - Tw.detach()), J = surfel_ref.ddel_dTw.  No
                    hand-derived pose formula is involved on the autograd side.  At scale_modifier 1 and 3.
                    The same autograd pass also yields dL/d(Tu, Tv, Tw, n) per surfel; the restatement fed THOSE rows equals dL/dvm to
                    1e-9 of its size -- the formula itself, free of the oracle's float32 rounding.
                    Scene: the shell scene of tests/test_surfel_oracle_autograd_cpu.py at seed 41, the seed of the 3-D form's
                    tests/test_pose_ref_cpu.py.  (That file's own seed, 43, holds one surfel whose float32 oracle dL/dTw entry lies
                    4e-4 of the row's size from float64 -- inside that file's bars -- and whose 50 m lever arm p[r] turns it into 2.5e-3 of
                    the sum, more than `_close` allows: the oracle's rounding, not the formula, as the exact check shows on either seed.
                    Measured over shell and street scenes, seeds 41-46 without 43: p99 4e-6 .. 1.3e-4.)
  (ii) translation  the translation row of the sum equals sum_i dL_dmeans3D_i @ V[:3,:3] on the oracle's own mean gradients.
  (iii) modifier    mod = 3 scales the Tu / Tv terms and nothing else.
"""
import numpy as np
import pytest
import torch

import surfel_pose_ref
import surfel_ref as ref
from oracle import lgo_surfel
from test_surfel_oracle_autograd_cpu import F64, H_, P_, W_, _blend, _close
from util import surfel_scene, surfel_upstream_grads

USED = [4 * r + k for r in range(4) for k in range(3)]
COLUMN3 = [3, 7, 11, 15]
SEED = 41


@pytest.fixture(scope="module", params=[1.0, 3.0], ids=["mod1", "mod3"])
def run(request):
    mod = request.param
    scene = surfel_scene("shell", P_, H_, SEED, random_view=True)
    scene["opacities"] = np.clip(scene["opacities"], 0.15, 0.9).astype(np.float32)
    scene["bg"] = np.array([0.2, 0.5], np.float32)
    if mod != 1.0:
        scene["scales"] = (scene["scales"] / np.float32(mod)).astype(np.float32)       # the same footprints through the modifier
    grads = surfel_upstream_grads(H_, W_, SEED)
    f = lgo_surfel.forward(scene["means3D"], scene["colors"], scene["opacities"], scene["scales"], scene["rotations"], scene["viewmatrix"],
                           scene["beams"], W_, H_, bg=scene["bg"], scale_modifier=mod)
    g = lgo_surfel.backward(f, *grads)
    Tw = f.array("transMat").reshape(P_, 9)[:, 6:9].astype(np.float64)
    line = ref.line_from_oracle(g, Tw, scene["beams"], W_, H_)
    c = surfel_pose_ref.contributions(line, scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], scene["beams"], W_, H_, mod)
    return scene, grads, f, g, line, c, mod


def test_chain_sum_is_autograd_of_the_forward_with_the_matrix_as_the_only_leaf(run):
    scene, grads, f, g, line, c, mod = run
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=F64)
    vm = t(np.asarray(scene["viewmatrix"]).reshape(16)).requires_grad_(True)
    q = t(scene["rotations"])
    qn = q / torch.sqrt((q * q).sum(-1, keepdim=True))
    Tu, Tv, Tw, nv = ref.rows_of(t(scene["means3D"]), float(np.float32(mod)) * t(scene["scales"]), qn, vm)
    with torch.no_grad():
        sg = torch.where(-(Tw * nv).sum(-1) > 0, 1.0, -1.0).to(F64)[:, None]              # DUAL_VISIABLE: a constant sign
        Tw0 = Tw.detach().clone()
        Tw0[torch.as_tensor(f.radii <= 0)] = 1.0                                            # (culled surfels are in no list; any finite factor)
        ddelx, ddely = ref.ddel_dTw(Tw0, scene["beams"], W_, H_)
    nrm = sg * nv
    no = f.array("normal_opacity").reshape(P_, 4).astype(np.float64)
    tm = f.array("transMat").reshape(P_, 9).astype(np.float64)
    vis = f.radii > 0
    np.testing.assert_allclose(torch.cat([Tu, Tv, Tw], -1).detach().numpy()[vis], tm[vis], rtol=2e-5, atol=2e-5)   # rows_of is the oracle's K1
    np.testing.assert_allclose(nrm.detach().numpy()[vis], no[vis, :3], rtol=2e-5, atol=2e-6)
    d = Tw - Tw.detach()
    xy = t(f.array("means2D").reshape(P_, 2)) + torch.stack([(ddelx * d).sum(-1), (ddely * d).sum(-1)], -1)
    margins = []
    for a in (Tu, Tv, Tw, nrm):
        a.retain_grad()
    color, others = _blend(f, scene, Tu, Tv, Tw, nrm, t(no[:, 3]), t(scene["colors"]), xy, margins)
    assert min(margins) > 1e-5, f"a pair sits within {min(margins):.1e} of a threshold: pick another seed"
    gc, go = (torch.as_tensor(np.asarray(x), dtype=F64) for x in grads)
    loss = (color * gc.reshape(2, H_, W_)).sum() + (others * go.reshape(7, H_, W_)).sum()
    loss.backward()
    gvm = vm.grad.numpy()
    # the formula on autograd's own row gradients (Tw.grad holds the linearised (x, y) terms already: the final dL/dTw)
    exact = np.zeros((P_, 32))
    for k, a in (("TU", Tu), ("TV", Tv), ("TW", Tw), ("N", nrm)):
        exact[:, list(ref.SLOT[k])] = a.grad.numpy()
    ce = surfel_pose_ref.contributions(exact, scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], scene["beams"], W_, H_, mod).sum(0)
    print(f"[surfel pose mod={mod}] formula on autograd's rows: max |diff| {np.abs(ce - gvm).max():.2e} of {np.abs(gvm).max():.2e}")
    assert np.abs(ce - gvm).max() <= 1e-9 * np.abs(gvm).max()
    got = c.sum(0)
    print(f"[surfel pose mod={mod}] autograd:", gvm[USED])
    print(f"[surfel pose mod={mod}] chain sum:", got[USED])
    print(f"[surfel pose mod={mod}] relative error per entry:", np.abs(got[USED] - gvm[USED]) / np.abs(gvm[USED]))
    assert np.abs(gvm[USED]).min() > 0
    _close("dL_dviewmatrix", got[USED], gvm[USED])
    for k in COLUMN3:                                                       # column 3 is read by no formula
        assert got[k] == 0.0 and gvm[k] == 0.0
        assert not c[:, k].any()


def test_translation_row_is_the_mean_gradients_rotated_back(run):
    scene, grads, f, g, line, c, mod = run
    V = np.asarray(scene["viewmatrix"], np.float64).reshape(4, 4)
    assert np.allclose(V[:3, :3] @ V[:3, :3].T, np.eye(3), atol=1e-6)       # a rigid view
    want = g["dL_dmeans3D"].astype(np.float64).sum(0) @ V[:3, :3]
    got = c.sum(0)[12:15]
    print("[surfel pose] translation row:", got, "rotated mean gradients:", want, "relative:", np.abs(got - want) / np.abs(want))
    _close("translation row", got, want)


def test_the_modifier_scales_the_axis_terms_and_nothing_else(run):
    scene, grads, f, g, line, c, mod = run
    args = (scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], scene["beams"], W_, H_)
    axes = np.zeros_like(line)
    for k in ("TU", "TV"):
        axes[:, list(ref.SLOT[k])] = line[:, list(ref.SLOT[k])]
    rest = line - axes
    c_axes, c_rest = surfel_pose_ref.contributions(axes, *args, 1.0), surfel_pose_ref.contributions(rest, *args, 1.0)
    assert np.abs(c_axes[:, USED[:9]]).max() > 0 and not c_axes[:, 12:15].any()            # the axes do not reach the translation row
    assert np.array_equal(surfel_pose_ref.contributions(rest, *args, 3.0), c_rest)          # nothing else sees the modifier
    size = np.abs(c_axes).max() + np.abs(c_rest).max()                     # (products of float64 values in another order: a few ulp of the terms)
    np.testing.assert_allclose(surfel_pose_ref.contributions(axes, *args, 3.0), 3.0 * c_axes, rtol=0, atol=1e-13 * size)
    np.testing.assert_allclose(surfel_pose_ref.contributions(line, *args, 3.0), c_rest + 3.0 * c_axes, rtol=0, atol=1e-13 * size)
