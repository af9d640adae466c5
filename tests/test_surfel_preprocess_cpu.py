"""tests/surfel_ref.py -- the float64 restatement the per-surfel HIP kernels are held against (tests/test_surfel_preprocess_gpu.py) --
is itself held here, against the oracle (oracle/lgo_surfel.py), without a GPU:

  forward   its fields against the oracle's fp32 state arrays (transMat, normal_opacity, means2D, depths) at fp32 accuracy; the integers
            (radii_xy, radii, tiles_touched = the rect's area, the cull outcome) exactly, outside the surfels the restatement itself
            marks as sitting on a rounding boundary;
  takers    every pixel a single-surfel frame of the oracle blends the surfel into is a taker or undecided, and every taker is blended;
            the last blended surfel of every pixel of a whole frame is a taker or undecided; `pair` against a scalar transcription;
  backward  `chain`, fed the lines identifiable from one oracle backward, returns the oracle's dL_dscales / dL_drotations / dL_dmeans3D /
            dL_dmeans2D within `_close`'s bars; its reconstructed terms are the derivatives of |Tw|, p_c and the elevation by autograd;
  scenes    every scene of the GPU tests meets its conditions on the reference alone.
"""
import math

import numpy as np
import pytest
import torch

import surfel_ref as ref
import test_surfel_preprocess_gpu as gpu_tests
from oracle import lgo_surfel
from test_oracle_autograd_cpu import _close, _lists_of
from util import surfel_scene, surfel_upstream_grads

H_, W_, P_ = 8, 96, 600


def _scene(seed=45):
    s = surfel_scene("shell", P_, H_, seed, random_view=True)
    s["means3D"] = (s["means3D"] * np.float32(0.3)).astype(np.float32)
    s["bg"] = np.array([0.25, 0.6], np.float32)
    return s


@pytest.fixture(scope="module", params=[(1.0, False), (0.5, False), (1.0, True)], ids=["mod1", "mod0.5", "transMat_precomp"])
def run(request):
    mod, precomp = request.param
    scene = _scene()
    tm = None
    if precomp:
        f0 = ref.forward64(scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"])
        rng = np.random.default_rng(3)
        rows = np.concatenate([f0["Tu"], f0["Tv"], f0["pv"]], 1)
        tm = (rows * (1.0 + 0.05 * rng.normal(size=rows.shape)) + 0.01 * rng.normal(size=rows.shape)).astype(np.float32)
    f = lgo_surfel.forward(scene["means3D"], scene["colors"], scene["opacities"], scene["scales"], scene["rotations"], scene["viewmatrix"], scene["beams"],
                           W_, H_, bg=scene["bg"], scale_modifier=mod, transMat_precomp=tm)
    g = lgo_surfel.backward(f, *surfel_upstream_grads(H_, W_, 45))
    mine = ref.forward64(scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], mod, tm)
    geo = ref.geometry(mine, scene["beams"], W_, H_)
    return scene, mod, tm, f, g, mine, geo


def test_forward_fields_agree_with_the_oracle_state(run):
    scene, mod, tm, f, g, mine, geo = run
    P = P_
    vis = f.radii > 0
    ok = ~geo["near_boundary"]
    assert geo["near_boundary"].sum() <= 0.01 * P
    assert vis.sum() > 0.4 * P
    assert np.array_equal(vis[ok], geo["live"][ok])
    v = vis & ok
    if tm is None:                                                          # (with transMat_precomp the blend reads the given rows, not this state)
        rows = f.array("transMat").reshape(P, 9)
        for sl, k in ((slice(0, 3), "Tu"), (slice(3, 6), "Tv"), (slice(6, 9), "pv")):      # (a component is a sum of three products: fp32 of the row's size)
            scale = np.abs(mine[k][v]).max(1, keepdims=True)
            np.testing.assert_allclose(rows[v, sl] / scale, mine[k][v] / scale, rtol=0, atol=2e-6, err_msg=k)
    no = f.array("normal_opacity").reshape(P, 4)
    np.testing.assert_allclose(no[v, :3], mine["n"][v], atol=2e-6)
    assert np.array_equal(no[v, 3], scene["opacities"][v, 0])
    np.testing.assert_allclose(f.array("depths")[v], mine["dist"][v], rtol=1e-6)
    m2 = f.array("means2D").reshape(P, 2)
    # atan2f within 2 ulps of an angle <= pi (5e-7 rad), over the column step / the beam gap, plus the fp32 rounding of the position
    np.testing.assert_allclose(m2[v, 0], geo["p_c"][v], rtol=0, atol=5e-7 / ref.steps(W_)[0] + 1e-5)
    np.testing.assert_allclose(m2[v, 1], geo["p_r"][v], rtol=0, atol=5e-7 / float(np.diff(scene["beams"]).min()) + 1e-5)
    rxy = f.array("radii_xy").reshape(P, 2)
    assert np.array_equal(rxy[v, 0], geo["rx"][v]) and np.array_equal(rxy[v, 1], geo["ry"][v])
    assert np.array_equal(f.radii[v], np.maximum(geo["rx"], geo["ry"])[v])
    r = geo["rect"]
    assert np.array_equal(f.array("tiles_touched")[v], ((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1]))[v])
    # K2 has no edge-on rule and nothing else differs
    k2 = lgo_surfel.visible_filter(scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], scene["beams"], W_, H_, scale_modifier=mod)
    geo2 = ref.geometry(mine, scene["beams"], W_, H_, filter_only=True)
    assert np.array_equal((k2 > 0)[ok], geo2["live"][ok]) and np.array_equal(k2[v], f.radii[v])


def test_the_last_blended_surfel_of_every_pixel_is_a_taker(run):
    scene, mod, tm, f, g, mine, geo = run
    lists = _lists_of(f, W_, H_)
    ncon = f.array("n_contrib")[:H_ * W_].reshape(H_, W_)
    dirs = ref.pixel_dirs(W_, H_, scene["beams"])
    op = scene["opacities"][:, 0].astype(np.float64)
    tk = ref.takers(mine, geo, scene["opacities"], scene["beams"], W_, H_)
    pairs = und = 0
    for y in range(H_):
        for x in range(W_):
            if ncon[y, x] == 0:
                continue
            gi = int(lists(x, y)[ncon[y, x] - 1])                          # the entry the walk blended last (R2/cr/forward.cu:487-547)
            pr = ref.pair(mine, geo, op, dirs, gi, np.array([x]), np.array([y]))
            undecided = bool(ref.pair_undecided(pr, mine["blen"][gi])[0])
            assert undecided or (not pr["skip"][0] and pr["alpha"][0] >= ref.ALPHA_MIN), (x, y, gi, pr)
            pairs += 1; und += int(undecided)
            r = geo["rect"][gi]
            assert 16 * r[0] <= x < 16 * r[2] and r[1] <= y < r[3]
            if not undecided:
                assert ((tk["xs"][gi] == x) & (tk["ys"][gi] == y)).any(), (x, y, gi)
    print(f"[takers] {pairs} last-blended pairs, {und} undecided")
    assert pairs >= 50                                                    # (the check is not vacuous)


@pytest.mark.parametrize("name", ["1_mix_opacities", "3_edge_on_back_behind", "4_needles_large_discs", "6_seam_W250", "11_transMat_precomp"])
def test_single_surfel_frames_blend_exactly_the_takers(name):
    """A frame that holds one surfel: the pixels with a rendered alpha are the pixels that took it (R2/cr/forward.cu:484-494; the first
    entry of a list never meets the T < 0.0001 stop).  Every such pixel must be a taker or undecided; every taker must be rendered."""
    d, f, geo, tk = gpu_tests.reference(name)
    s, W, H = d["scene"], d["W"], d["H"]
    dirs = ref.pixel_dirs(W, H, s["beams"])
    op = s["opacities"][:, 0].astype(np.float64)
    cand = np.nonzero((tk["n"] > 0) & ~geo["near_boundary"])[0]
    rendered = taken = 0
    for g in cand[:: max(1, cand.size // 40)]:
        one = {k: s[k][g:g + 1] for k in gpu_tests.ARRAYS}
        tm = None if s.get("transMat") is None else s["transMat"][g:g + 1]
        fo = lgo_surfel.forward(one["means3D"], one["colors"], one["opacities"], one["scales"], one["rotations"], s["viewmatrix"], s["beams"], W, H,
                                scale_modifier=d["mod"], transMat_precomp=tm)
        ys, xs = np.nonzero(fo.others[1] > 0)
        assert xs.size > 0, g
        with np.errstate(all="ignore"):
            pr = ref.pair(f, geo, op, dirs, g, xs, ys)
            und = ref.pair_undecided(pr, f["blen"][g])
        mine = set(zip(tk["xs"][g].tolist(), tk["ys"][g].tolist()))
        theirs = set(zip(xs.tolist(), ys.tolist()))
        for i, (x, y) in enumerate(zip(xs.tolist(), ys.tolist())):
            assert und[i] or (x, y) in mine, f"{name}: surfel {g} is blended into pixel ({x}, {y}), which is not among its takers: alpha {pr['alpha'][i]!r}"
        assert mine <= theirs, f"{name}: surfel {g}: takers the oracle does not blend: {sorted(mine - theirs)[:5]}"
        rendered += len(theirs); taken += len(mine)
    print(f"[single-surfel frames {name}] {rendered} rendered pixels, {taken} takers")
    assert taken >= 200


def _pair_scalar(Tu, Tv, Tw, n, xy, op, beams, W, H, x, y):
    """R2/cr/forward.cu:435-484 for one pair, line by line, in Python floats -> alpha, or None when the pair is passed over."""
    beta_pix = -(x - W / 2.0) / W * 2.0 * ref.PI_F
    alpha_pix = float(beams[H - 1 - y])
    rho_r = math.sqrt(Tw[0] * Tw[0] + Tw[1] * Tw[1] + Tw[2] * Tw[2])
    p = (math.cos(alpha_pix) * math.cos(beta_pix), math.cos(alpha_pix) * math.sin(beta_pix), math.sin(alpha_pix))
    cos_phi1 = (Tw[0] * n[0] + Tw[1] * n[1] + Tw[2] * n[2]) / rho_r
    lam = rho_r * cos_phi1
    cos_phi2 = p[0] * n[0] + p[1] * n[1] + p[2] * n[2]
    if cos_phi2 == 0:
        return None
    real_depth = lam / cos_phi2
    dp = [real_depth * p[k] - Tw[k] for k in range(3)]
    s = (sum(dp[k] * Tu[k] for k in range(3)) / sum(t * t for t in Tu), sum(dp[k] * Tv[k] for k in range(3)) / sum(t * t for t in Tv))
    rho3d = s[0] * s[0] + s[1] * s[1]
    dx, dy = xy[0] - x, xy[1] - y
    rho2d = 2.0 * (40 * dx * dx + 100 * dy * dy)
    rho = min(rho3d, rho2d) if real_depth > 0 else rho2d
    depth = real_depth if (rho3d <= rho2d and real_depth > 0) else rho_r
    if depth < ref.NEAR_N:
        return None
    power = -0.5 * rho
    if power > 0:
        return None
    return min(0.99, op * math.exp(power))


def test_pair_against_a_scalar_transcription():
    checked = 0
    for name in ("3_edge_on_back_behind", "11_transMat_precomp"):
        d, f, geo, tk = gpu_tests.reference(name)
        s, W, H = d["scene"], d["W"], d["H"]
        dirs = ref.pixel_dirs(W, H, s["beams"])
        op = np.nan_to_num(s["opacities"][:, 0].astype(np.float64), nan=0.5)
        rng = np.random.default_rng(1)
        for g in rng.choice(np.nonzero(geo["live"])[0], 150, replace=False):
            x0, y0, x1, y1 = geo["rect"][g]
            x, y = int(rng.integers(16 * x0, min(16 * x1, W))), int(rng.integers(y0, y1))
            pr = ref.pair(f, geo, op, dirs, g, np.array([x]), np.array([y]))
            a = _pair_scalar(f["Bu"][g], f["Bv"][g], f["Bw"][g], f["n"][g], (geo["p_c"][g], geo["p_r"][g]), op[g], s["beams"].astype(np.float64), W, H, x, y)
            assert (a is None) == bool(pr["skip"][0]), (name, g, x, y)
            if a is not None:
                assert abs(a - pr["alpha"][0]) <= 1e-9 * max(a, 1e-30) + 1e-300, (name, g, x, y, a, pr["alpha"][0])
            checked += 1
    assert checked == 300


def _chain_args(scene, f, tm):
    return (scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], scene["beams"], W_, H_, f.radii, tm)


def test_chain_reproduces_the_oracle_backward_from_its_own_intermediates(run):
    scene, mod, tm, f, g, mine, geo = run
    vis = f.radii > 0
    line = ref.line_from_oracle(g, mine["Bw"], scene["beams"], W_, H_)
    line[~vis] = 0.0
    assert np.abs(line[vis]).max() > 0 and (np.abs(line[vis][:, list(ref.SLOT["M2X"])]) > 0).sum() > 20 and (np.abs(line[vis][:, list(ref.SLOT["AW"])]) > 0).sum() > 20
    assert not line[:, list(ref.DEAD)].any()
    # dL_dmeans2D and the TW row below come back by construction (line_from_oracle subtracts what chain adds).  What the derived lines
    # can say about the abs-linear coefficients mx3 / my3: the reference adds a signed term to dL_dmean2D.x and its absolute value to .z
    # (R2/cr/backward.cu:582-585), so M2AX >= |M2X| and M2AY >= |M2Y| up to the fp32 rounding of the oracle's sums; coefficients that are too
    # large break it on every surfel whose 2-D term is negative.  Coefficients that are too small rest on whole-frame parity alone.
    m2 = np.abs(g["dL_dmeans2D"].astype(np.float64))
    for a, b, cols, half in (("M2AX", "M2X", (0, 2), 0.5 * W_), ("M2AY", "M2Y", (1, 3), 0.5 * H_)):
        A, B = line[vis][:, ref.SLOT[a][0]], line[vis][:, ref.SLOT[b][0]]
        tol = 4e-6 * m2[vis][:, list(cols)].max(1) / half
        assert (A >= np.abs(B) - tol).all(), (a, float((A - np.abs(B) + tol).min()))
        assert (B < -tol).sum() >= 10, (b, int((B < -tol).sum()))            # (negative 2-D terms occur: the check is not vacuous)
    c = ref.chain(line, *_chain_args(scene, f, tm))
    for k in c:
        c[k][~vis] = 0.0
    _close("dL_dmeans3D", g["dL_dmeans3D"], c["dL_dmean3D"])
    _close("dL_dscales", g["dL_dscales"], c["dL_dscale"])
    _close("dL_drotations", g["dL_drotations"], c["dL_drot"])
    _close("dL_dmeans2D", g["dL_dmeans2D"], c["dL_dmean2D"])
    _close("dL_dtransMat", g["dL_dtransMat"], c["dL_dtransMat"])
    _close("depth", g["depth"], c["depth"])
    assert not c["depth"][~vis].any()


def test_reconstructed_terms_are_derivatives_by_autograd(run):
    """The Z2D slot multiplies d|Tw|/dTw; the M2X slot d(p_c)/dTw; the M2Y slot grad_alpha times d(elevation)/dTw
    (R2/cr/backward.cu:590-598), each taken here by autograd of the forward's own expression (R2/cr/forward.cu:151-153)."""
    scene, mod, tm, f, g, mine, geo = run
    vis = np.nonzero(f.radii > 0)[0]
    Tw = torch.as_tensor(mine["Bw"][vis], dtype=ref.F64).requires_grad_(True)
    col_step = 2.0 * math.pi / W_
    ga = abs(float(scene["beams"][H_ - 1]) - float(scene["beams"][0])) / (H_ - 1.0)
    exprs = dict(Z2D=torch.sqrt((Tw * Tw).sum(-1)), M2X=(math.pi - torch.atan2(Tw[:, 1], Tw[:, 0])) / col_step,
                 M2Y=ga * torch.atan2(Tw[:, 2], torch.sqrt(Tw[:, 0] ** 2 + Tw[:, 1] ** 2)))
    sub = {k: scene[k][vis] for k in ("means3D", "scales", "rotations")}
    for slot, e in exprs.items():
        want = torch.autograd.grad(e.sum(), Tw)[0].numpy()
        line = np.zeros((vis.size, 32)); line[:, ref.SLOT[slot][0]] = 1.0
        c = ref.chain(line, sub["means3D"], sub["scales"], sub["rotations"], scene["viewmatrix"], scene["beams"], W_, H_, f.radii[vis], None if tm is None else tm[vis])
        np.testing.assert_allclose(c["dL_dtransMat"][:, 6:9], want, rtol=1e-9, atol=1e-12, err_msg=slot)


def test_fp32_yardstick_is_the_same_function(run):
    """The float32 run of the chain is what the HIP kernel's error is measured in: it must itself be close to the float64 one."""
    scene, mod, tm, f, g, mine, geo = run
    vis = f.radii > 0
    line = ref.line_from_oracle(g, mine["Bw"], scene["beams"], W_, H_)[vis]
    args = (scene["means3D"][vis], scene["scales"][vis], scene["rotations"][vis], scene["viewmatrix"], scene["beams"], W_, H_, f.radii[vis], None if tm is None else tm[vis])
    a = ref.chain(line, *args)
    b = ref.chain(line, *args, dtype=torch.float32)
    for k in ("dL_dmean2D", "dL_dtransMat", "dL_dmean3D", "dL_dscale", "dL_drot", "depth"):
        e = ref.row_error(b[k], a[k])
        print(f"[yardstick] {k:14s} p99 {np.quantile(e, 0.99):.2e} worst {e.max():.2e}")
        assert np.quantile(e, 0.99) < 1e-4 and e.max() < 1e-2, k


@pytest.mark.parametrize("name", list(gpu_tests.SCENES))
def test_every_scene_meets_its_conditions_on_the_reference_alone(name):
    gpu_tests.scene_conditions(name)
    d, f, geo, tk = gpu_tests.reference(name)
    if name.startswith("6_"):
        wrap, hull, first, last = gpu_tests.seam_classes(name)
        print(f"[scene {name}] takers at both ends: rect over every tile column {wrap.size}, rect short of one end {hull.size}; one run at the first columns "
              f"{first.size}, at the last {last.size}")
        assert wrap.size > 50 and hull.size > 10 and first.size > 50 and last.size > 50
    if name.startswith("4_"):
        e = d["escapes"] & geo["live"]
        assert (e & d["needle"]).sum() > 1000 and (e & ~d["needle"]).sum() > 300
    if name.startswith("3_"):
        # each third does what it was built for: 2-D takers of edge-on surfels, flipped normals, planes behind part of their rays
        dirs = ref.pixel_dirs(d["W"], d["H"], d["scene"]["beams"])
        behind = 0
        for g in np.nonzero((d["kind"] == 2) & geo["live"])[0][:200]:
            x0, y0, x1, y1 = geo["rect"][g]
            xs, ys = (v.ravel() for v in np.meshgrid(np.arange(16 * x0, min(16 * x1, d["W"])), np.arange(y0, y1)))
            behind += int(((dirs[ys, xs] @ f["n"][g]) * f["lam"][g] <= 0).any())
        assert behind > 100, behind
        assert (f["c"][d["kind"] == 1] < 0).sum() > 900                     # normals that pointed away
        assert (tk["n"][(d["kind"] == 0) & geo["live"]] > 0).sum() > 500
