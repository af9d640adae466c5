"""tests/preprocess_ref.py -- the float64 restatement the per-Gaussian HIP kernels are held against (tests/test_preprocess_gpu.py) --
is itself held here, against the oracle, without a GPU:

  forward   its fields against the oracle's state arrays (conic_opacity, depths, basis_u1 / u2, sphere, means2D, radii_xy,
            tiles_touched), at the bars tests/test_oracle_autograd_cpu.py uses for K1 (conic 3e-4 relative, unit vectors 2e-6 absolute);
            the integers exactly, outside the Gaussians the restatement itself marks as sitting on a rounding boundary;
  backward  its autograd chain, fed the oracle's own intermediates of one backward (dL_dconic, dL_dmeans2D, dL_ddepths, the moments
            recovered from dL_dbasis_u_i), against the oracle's dL_dmeans3D / dL_dscales / dL_drotations / dL_dcov3D / dL_dsphere
            within `_close`'s bars (p99 <= 2e-4, worst <= 3e-3); scale_modifier 1 and 0.5, and cov3D_precomp;
  takers    the last blended Gaussian of every pixel (n_contrib / point_list of the oracle) is a taker or undecided.
"""
import numpy as np
import pytest
import torch

import lidargs_scenes as sc
import preprocess_ref as ref
from oracle import lgo
from test_oracle_autograd_cpu import _close, _lists_of

H_, W_, P_ = 8, 96, 600


def _scene(seed=45):
    s = sc.make_scene("shell", P_, H_, seed, random_view=True)
    s["bg"] = np.array([0.25, 0.6], np.float32)
    return s


def _cov6(scene, mod):
    with torch.no_grad():
        return ref.cov6_of(float(np.float32(mod)) * torch.as_tensor(scene["scales"], dtype=ref.F64), torch.as_tensor(scene["rotations"], dtype=ref.F64)).numpy().astype(np.float32)


@pytest.fixture(scope="module", params=[(1.0, False), (0.5, False), (1.0, True)], ids=["mod1", "mod0.5", "cov3D_precomp"])
def run(request):
    mod, precomp = request.param
    scene = _scene()
    cov = _cov6(scene, mod) if precomp else None
    grads = sc.upstream_grads(H_, W_, 45)
    f = lgo.forward(scene["means3D"], scene["colors"], scene["opacities"], scene["scales"], scene["rotations"], scene["viewmatrix"],
                    scene["beams"], W_, H_, bg=scene["bg"], scale_modifier=mod, cov3D_precomp=cov)
    g = lgo.backward(f, *grads)
    mine = ref.forward64(scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], mod, cov)
    geo = ref.geometry(mine, scene["beams"], W_, H_)
    return scene, mod, cov, f, g, mine, geo


def test_vectorised_k1_is_k1_as_written():
    scene = _scene()
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=ref.F64)
    vm = t(scene["viewmatrix"].reshape(16))
    mine = ref.forward64(scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], 0.7)
    for i in range(0, P_, 37):
        abc, dist, u1, u2, s, _ = ref.k1_one(t(scene["means3D"][i]), t(scene["scales"][i]), t(scene["rotations"][i]), vm, float(np.float32(0.7)))
        for name, a in (("abc", abc), ("dist", dist), ("u1", u1), ("u2", u2), ("dir", s)):
            np.testing.assert_allclose(mine[name][i], a.numpy(), rtol=1e-12, atol=1e-15, err_msg=name)


def test_forward_fields_agree_with_the_oracle_state(run):
    scene, mod, cov, f, g, mine, geo = run
    P = P_
    vis = f.radii > 0
    ok = ~geo["near_boundary"]
    assert geo["near_boundary"].sum() <= 0.01 * P
    assert vis.sum() > 0.4 * P                                           # (the random view tilts part of the shell out of the fan)
    assert np.array_equal(vis[ok], geo["live"][ok])
    v = vis & ok
    co = f.array("conic_opacity").reshape(P, 4)
    # (a purely relative bar on B = -b / det, whose numerator is a sum that cancels: a |B| five orders below A and C sits at 3e-4 by fp32
    #  rounding alone -- seen on 4 of 20 seeds; this seed's worst entry is at 1.4e-5)
    np.testing.assert_allclose(co[v, :3], mine["conic"][v], rtol=3e-4)
    assert np.array_equal(co[v, 3], scene["opacities"][v, 0])
    np.testing.assert_allclose(f.array("depths")[v], mine["dist"][v], rtol=1e-6)
    np.testing.assert_allclose(f.array("basis_u1").reshape(P, 3)[v], mine["u1"][v], atol=2e-6)
    np.testing.assert_allclose(f.array("basis_u2").reshape(P, 3)[v], mine["u2"][v], atol=2e-6)
    np.testing.assert_allclose(f.array("sphere").reshape(P, 3)[v], mine["dir"][v], atol=2e-6)
    m2 = f.array("means2D").reshape(P, 2)
    # atan2f within 2 ulps of an angle <= pi (5e-7 rad), over the column step / the beam gap, plus the fp32 rounding of the position
    np.testing.assert_allclose(m2[v, 0], geo["p_c"][v], rtol=0, atol=5e-7 / ref.steps(W_)[0] + 1e-5)
    np.testing.assert_allclose(m2[v, 1], geo["p_r"][v], rtol=0, atol=5e-7 / float(np.diff(scene["beams"]).min()) + 1e-5)
    rxy = f.array("radii_xy").reshape(P, 2)
    assert np.array_equal(rxy[v, 0], geo["rx"][v]) and np.array_equal(rxy[v, 1], geo["ry"][v])
    assert np.array_equal(f.radii[v], np.maximum(geo["rx"], geo["ry"])[v])
    r = geo["rect"]
    assert np.array_equal(f.array("tiles_touched")[v], ((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1]))[v])


def _line_of(g, mine):
    return ref.line_from_oracle(g, mine["u1"], mine["u2"])


def test_chain_reproduces_the_oracle_backward_from_its_own_intermediates(run):
    scene, mod, cov, f, g, mine, geo = run
    line = _line_of(g, mine)
    vis = f.radii > 0
    line[~vis] = 0.0
    assert np.abs(line[vis]).max() > 0
    c = ref.chain(line, scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], mod, cov)
    for k in c:
        c[k][~vis] = 0.0                                                  # (a culled Gaussian at a pole would be 0 * inf)
    _close("dL_dmeans3D", g["dL_dmeans3D"], c["dL_dmean3D"])
    _close("dL_dcov3D", g["dL_dcov3D"], c["dL_dcov3D"])
    _close("dL_dsphere", g["dL_dsphere"], c["dL_dsphere"])
    _close("dL_dbasis_u1", g["dL_dbasis_u1"], c["dL_dbasis_u1"])
    _close("dL_dbasis_u2", g["dL_dbasis_u2"], c["dL_dbasis_u2"])
    if cov is None:
        _close("dL_dscales", g["dL_dscales"], c["dL_dscale"])
        _close("dL_drotations", g["dL_drotations"], c["dL_drot"])
    else:
        assert not c["dL_dscale"].any() and not c["dL_drot"].any()


def test_fp32_yardstick_is_the_same_function(run):
    """The float32 run of the chain is what the HIP kernel's error is measured in: it must itself be close to the float64 one."""
    scene, mod, cov, f, g, mine, geo = run
    line = _line_of(g, mine)
    vis = f.radii > 0
    a = ref.chain(line[vis], scene["means3D"][vis], scene["scales"][vis], scene["rotations"][vis], scene["viewmatrix"], mod, None if cov is None else cov[vis])
    b = ref.chain(line[vis], scene["means3D"][vis], scene["scales"][vis], scene["rotations"][vis], scene["viewmatrix"], mod, None if cov is None else cov[vis],
                  dtype=torch.float32)
    for k in ("dL_dmean3D", "dL_dcov3D", "dL_dsphere", "dL_dbasis_u1", "dL_dbasis_u2") + (("dL_dscale", "dL_drot") if cov is None else ()):
        e = ref.row_error(b[k], a[k])
        print(f"[yardstick] {k:14s} p99 {np.quantile(e, 0.99):.2e} worst {e.max():.2e}")
        assert np.quantile(e, 0.99) < 1e-4 and e.max() < 1e-2, k


def test_the_last_blended_gaussian_of_every_pixel_is_a_taker(run):
    scene, mod, cov, f, g, mine, geo = run
    lists = _lists_of(f, W_, H_)
    ncon = f.array("n_contrib").reshape(H_, W_)
    dirs = ref.pixel_dirs(W_, H_, scene["beams"])
    op = scene["opacities"][:, 0].astype(np.float64)
    tk = ref.takers(mine, geo, scene["opacities"], scene["beams"], W_, H_)
    pairs = und = 0
    for y in range(H_):
        for x in range(W_):
            if ncon[y, x] == 0:
                continue
            gi = int(lists(x, y)[ncon[y, x] - 1])                          # the entry the walk blended last (R3/cr/forward.cu:613-622)
            power, alpha = ref.pair_alpha(mine, op, dirs, gi, np.array([x]), np.array([y]))
            undecided = abs(alpha[0] * 255.0 - 1.0) <= ref.UNDECIDED
            assert undecided or (power[0] <= 0.0 and alpha[0] >= ref.ALPHA_MIN), (x, y, gi, power[0], alpha[0])
            pairs += 1; und += int(undecided)
            # it lies inside the Gaussian's reference rect, and -- unless undecided -- inside the bounding box `takers` reports for it
            r = geo["rect"][gi]
            assert 16 * r[0] <= x < 16 * r[2] and r[1] <= y < r[3]
            if not undecided:
                bx = tk["box"][gi]
                assert tk["n"][gi] > 0 and bx[0] <= x <= bx[2] and bx[1] <= y <= bx[3], (x, y, gi, bx)
    print(f"[takers] {pairs} last-blended pairs, {und} undecided")
    assert pairs >= 50                                                    # (the check is not vacuous)
