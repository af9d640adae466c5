"""GPU parity over the whole opacity domain (3-D and surfel variants): opacities above 1, at the 1/255 cut and the 0.99 clamp, zero and
negative, NaN and +-inf.  Every other rasterizer test draws its opacities from U(0.1, 1) times a scale; the kernels' decisions that hang
on the opacity -- the cull `op * 255 < 1`, both footprint prunings (their reach follows tau = ln(255 op)), the blend's
fminf(0.99, op G) and its 1/255 test -- are pinned here against the oracle, entry by entry where a budget could hide a dropped pixel."""
import numpy as np
import pytest

import lidargs_scenes as sc
from util import (FLOOR, GRAD_KEYS_SR, GRAD_KEYS_SURFEL, SOFT_MAX, hip_forward_backward, hip_surfel_forward_backward, oracle_forward_backward,
                  oracle_surfel_forward_backward, parity, placed_scene, run_child, surfel_scene, surfel_upstream_grads)

pytestmark = pytest.mark.gpu

OTHERS = ("depth", "alpha", "normal_x", "normal_y", "normal_z")          # the surfel planes compared pixel by pixel (not the median / distortion)


def _entrywise(name, hip, ref, tol=SOFT_MAX, scale=None):
    """Every entry within `tol` under parity()'s metric (`scale`: max|ref| of the whole array the entries are taken from): no flip budget
    (MIN_COUNT lets two dropped pixels through parity())."""
    h = np.asarray(hip, np.float64).ravel(); r = np.asarray(ref, np.float64).ravel()
    assert h.shape == r.shape, (name, h.shape, r.shape)
    scale = np.abs(r).max() if scale is None else float(scale)
    err = np.abs(h - r) / (np.abs(r) + FLOOR * scale + 1e-30)
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, f"{name}: {bad.size} of {r.size} entries off by more than {tol}: first at {bad[:8]}, hip {h[bad[:4]]} vs ref {r[bad[:4]]}"


def _run(variant, scene, W, H, grads, ref_scene=None):
    """HIP on `scene`, the oracle on `ref_scene` (default: the same scene)."""
    ref_scene = scene if ref_scene is None else ref_scene
    if variant == "surfel":
        return hip_surfel_forward_backward(scene, W, H, grads), oracle_surfel_forward_backward(ref_scene, W, H, grads)
    return hip_forward_backward(scene, W, H, grads), oracle_forward_backward(ref_scene, W, H, grads)


def _grads(variant, W, H, seed):
    if variant == "surfel":
        g = surfel_upstream_grads(H, W, seed)
        g[1][5:] = 0.0             # median depth (a selection) and distortion: their own rules in tests/test_surfel_gpu.py
        return g
    return sc.upstream_grads(H, W, seed)


def _images(variant, out):
    if variant == "surfel":
        return {"color": out["color"], **{"others." + n: out["others"][k] for k, n in enumerate(OTHERS)}}
    return {k: out[k] for k in ("color", "depth", "occ")}


def _keys(variant):
    return GRAD_KEYS_SURFEL if variant == "surfel" else GRAD_KEYS_SR


# ---- A1: opacity above 1 --------------------------------------------------------------------------------------------------------------
def _above_one_scene(variant, op):
    """Splats that reach one pixel each, and only because op > 1: at op = 1 the oracle leaves every pixel of the frame empty.
    surfel: surfels facing the sensor, axes 2.5e-4 x their distance (the 3-D disc spans < 0.15 columns, < 0.05 rows), centred on a pixel
            column and `dy` rows from a pixel row, dy halfway between the 0.24 rows the 2-D filter (rho2d = 2 (40 dx^2 + 100 dy^2),
            R2/cr/forward.cu:469) reaches at op <= 1 and the sqrt(2 tau / 200) rows it reaches at op.  The column analogue cannot be built:
            the reference rect reaches a neighbouring tile column only through an axis end point more than a column away (R2/cr/
            auxiliary.h:99-112), and then the 3-D disc itself covers that column.
    3d:     isotropic Gaussians whose first-column-of-the-next-tile pixel (0.45 columns away) or neighbouring row pixel (0.45 rows away)
            takes alpha = 3/255: ~0.93 of the tau-derived reach of preprocess.hip's pruning, beyond the reach at op = 1."""
    H = 16
    W, dist = (800, 20.0) if variant == "surfel" else (400, 70.0)
    tau = np.log(255.0 * op)
    off = 0.5 * (0.24 + np.sqrt(2 * tau / 200)) if variant == "surfel" else 0.45
    pc, py, tx, ty, col = [], [], [], [], []
    for t in range(1, W // 16):
        if variant == "3d":
            for y in range(0, H, 2):
                pc.append(16 * t - off); py.append(y); tx.append(16 * t); ty.append(y); col.append(True)
        for y in range(1, H - 1, 2):
            s = 1 if (t + y) % 4 < 2 else -1
            pc.append(16 * t + 8); py.append(y + s * off); tx.append(16 * t + 8); ty.append(y); col.append(False)
    pc, py, col = np.array(pc), np.array(py), np.array(col)
    if variant == "surfel":
        sigma = 2.5e-4 * dist
    else:
        cs, gap = 2 * np.pi / W, np.deg2rad(20.0) / (H - 1)
        el = np.deg2rad(np.interp(H - 1 - py, np.arange(H), np.linspace(-17.6, 2.4, H)))
        ang = np.where(col, off * cs * np.cos(el), off * gap) / np.sqrt(2 * np.log(op * 255.0 / 3.0))
        sigma = np.sqrt((ang * dist) ** 2 - 0.01)                  # the 2-D covariance gets + 0.01 (R3/cr/forward.cu:166-167)
    scene = placed_scene(pc, py, dist, sigma, op, W, H, surfel=variant == "surfel", seed=int(op))
    return scene, W, H, np.array(ty), np.array(tx)


@pytest.mark.parametrize("op", [5.0, 10.0, 50.0])
@pytest.mark.parametrize("variant", ["surfel", "3d"])
def test_opacity_above_one_reaches_its_true_footprint(variant, op):
    scene, W, H, ty, tx = _above_one_scene(variant, op)
    g = _grads(variant, W, H, 3)
    hip, ref = _run(variant, scene, W, H, g)
    ref_img, hip_img = _images(variant, ref), _images(variant, hip)
    # guard: the construction really reaches its pixels (and only because op > 1)
    cover = ref["others"][1] if variant == "surfel" else ref["occ"][0]
    assert (cover[ty, tx] > 0).all(), f"the oracle leaves {int((cover[ty, tx] == 0).sum())} constructed pixels empty"
    one = dict(scene, opacities=np.ones_like(scene["opacities"]))
    ref1 = oracle_surfel_forward_backward(one, W, H) if variant == "surfel" else oracle_forward_backward(one, W, H)
    assert not ((ref1["others"][1] if variant == "surfel" else ref1["occ"][0]) > 0).any()
    hip_cover = hip["others"][1] if variant == "surfel" else hip["occ"][0]
    print(f"[op>1] {variant} op={op:g}: {ty.size} constructed pixels, HIP leaves {int((hip_cover[ty, tx] == 0).sum())} of them empty")
    assert np.array_equal(hip["radii"], ref["radii"])
    for k in ref_img:
        _entrywise(f"{variant}.op{op:g}.{k}[constructed]", hip_img[k][..., ty, tx], ref_img[k][..., ty, tx])
        parity(f"{variant}.op{op:g}.{k}", hip_img[k], ref_img[k])
    for k in _keys(variant):
        _entrywise(f"{variant}.op{op:g}.{k}", hip[k], ref[k])
        parity(f"{variant}.op{op:g}.{k}", hip[k], ref[k])


@pytest.mark.parametrize("variant", ["surfel", "3d"])
def test_street_scene_with_opacities_up_to_20(variant):
    H, W, seed = 32, 1024, 21
    scene = surfel_scene("street", 30_000, H, seed) if variant == "surfel" else sc.make_scene("street", 30_000, H, seed, random_view=True)
    scene["opacities"] = np.random.default_rng(seed).uniform(0.1, 20.0, scene["opacities"].shape).astype(np.float32)
    g = _grads(variant, W, H, seed)
    hip, ref = _run(variant, scene, W, H, g)
    assert int((hip["radii"] != ref["radii"]).sum()) <= 1
    for k, v in _images(variant, ref).items():
        parity(f"{variant}.op20.{k}", _images(variant, hip)[k], v)
    for k in _keys(variant):
        parity(f"{variant}.op20.{k}", hip[k], ref[k])


# ---- A2: opacity at the thresholds ----------------------------------------------------------------------------------------------------
CUT = np.float32(1 / 255)
CLAMP = np.float32(0.99)
THRESHOLD_OPS = [("cut", CUT), ("cut_down", np.nextafter(CUT, np.float32(0))), ("cut_up", np.nextafter(CUT, np.float32(1))),
                 ("clamp", CLAMP), ("clamp_down", np.nextafter(CLAMP, np.float32(0))), ("clamp_up", np.nextafter(CLAMP, np.float32(1))),
                 ("one", np.float32(1.0)), ("zero", np.float32(0.0)), ("minus_zero", np.float32(-0.0)), ("negative", np.float32(-0.5))]


def _threshold_scene(variant, op):
    """A street scene with every 7th opacity set to `op`, plus one splat at (2, 0, 0): straight down the centre column (W / 2 looks along
    +x exactly) of a row whose beam is exactly 0, so its power is exactly 0 (3-D: pixel ray == centre direction; surfel: the ray hits the
    centre exactly, every product with the power-of-two distance is exact) and alpha = fminf(0.99, op) there."""
    H, W, seed = 16, 512, 31
    beams = sc.beam_inclinations(H).copy()
    beams[13] = 0.0                                                    # row H - 1 - 13 = 2
    scene = sc.make_scene("street", 4000, H, seed, beams=beams)
    if variant == "surfel":
        scene["scales"] = np.ascontiguousarray(scene["scales"][:, :2])
    P = scene["means3D"].shape[0]
    one = placed_scene([W / 2], [2.0], 2.0, 0.03, op, W, H, beams=beams, surfel=variant == "surfel")
    one["means3D"][:] = np.array([[2.0, 0.0, 0.0]], np.float32)
    for k in ("means3D", "scales", "rotations", "opacities", "colors"):
        scene[k] = np.ascontiguousarray(np.concatenate([scene[k], one[k]]))
    sel = np.zeros(P + 1, bool)
    sel[::7] = True
    sel[P] = True
    scene["opacities"][sel] = op
    return scene, W, H, sel


@pytest.mark.parametrize("op", [o for _, o in THRESHOLD_OPS], ids=[n for n, _ in THRESHOLD_OPS])
@pytest.mark.parametrize("variant", ["surfel", "3d"])
def test_opacity_at_the_thresholds(variant, op):
    scene, W, H, sel = _threshold_scene(variant, op)
    g = _grads(variant, W, H, 31)
    hip, ref = _run(variant, scene, W, H, g)
    assert int((hip["radii"] != ref["radii"]).sum()) <= 1               # the radii do not depend on the opacity
    hip_img, ref_img = _images(variant, hip), _images(variant, ref)
    name = f"{variant}.op{float(op)!r}"
    # the power-0 pixel: alpha = fminf(0.99, op), taken iff op >= 1/255 (the oracle on the splat alone: 1 - T = alpha)
    alone = dict(scene, **{k: np.ascontiguousarray(scene[k][-1:]) for k in ("means3D", "scales", "rotations", "opacities", "colors")})
    cover = oracle_surfel_forward_backward(alone, W, H)["others"][1] if variant == "surfel" else oracle_forward_backward(alone, W, H)["occ"][0]
    expect = float(min(CLAMP, op)) if op >= CUT else 0.0
    assert cover[2, W // 2] == pytest.approx(expect, rel=1e-4, abs=0.0), (cover[2, W // 2], expect)
    for k in ref_img:
        _entrywise(f"{name}.{k}[power 0]", hip_img[k][..., 2, W // 2], ref_img[k][..., 2, W // 2], scale=np.abs(ref_img[k]).max())
        parity(f"{name}.{k}", hip_img[k], ref_img[k])
    for k in _keys(variant):
        _entrywise(f"{name}.{k}[power 0]", hip[k][-1], ref[k][-1], scale=np.abs(ref[k]).max())
        parity(f"{name}.{k}", hip[k], ref[k])
    if not op > 0:
        # no image contribution and no gradient: the frame is the frame without them
        for k in _keys(variant):
            assert (hip[k][sel] == 0).all() and (ref[k][sel] == 0).all(), k
        keep = ~sel
        sub = dict(scene, **{k: np.ascontiguousarray(scene[k][keep]) for k in ("means3D", "scales", "rotations", "opacities", "colors")})
        ref_sub = (oracle_surfel_forward_backward if variant == "surfel" else oracle_forward_backward)(sub, W, H, g)
        for k, v in _images(variant, ref_sub).items():
            parity(f"{name}.{k} vs without them", hip_img[k], v)
        for k in _keys(variant):
            parity(f"{name}.{k} vs without them", hip[k][keep], ref_sub[k])


# ---- A3: NaN and +-inf ----------------------------------------------------------------------------------------------------------------
def parity_nonfinite(name, hip, ref, rows):
    """parity() on the finite entries; the non-finite ones must sit at the same places on both sides, NaN where the oracle has NaN, and
    only in the gradient rows `rows` (the Gaussians whose opacity is not finite): a cross-lane reduction that masks by multiplying
    (x * 0) instead of selecting leaks NaN into its neighbours' rows."""
    h = np.asarray(hip, np.float64); r = np.asarray(ref, np.float64)
    assert h.shape == r.shape
    bad_h, bad_r = ~np.isfinite(h), ~np.isfinite(r)
    assert np.array_equal(bad_h, bad_r), f"{name}: non-finite at {int(bad_h.sum())} entries in HIP, {int(bad_r.sum())} in the oracle, " \
                                         f"{int((bad_h != bad_r).sum())} places differ (rows {np.unique(np.nonzero(bad_h != bad_r)[0])[:10]})"
    assert np.array_equal(np.isnan(h), np.isnan(r)), f"{name}: NaN at {int(np.isnan(h).sum())} entries in HIP, {int(np.isnan(r).sum())} in the oracle"
    out = np.setdiff1d(np.unique(np.nonzero(bad_r.reshape(r.shape[0], -1))[0]), rows)
    assert out.size == 0, f"{name}: non-finite gradient rows {out[:10]} of Gaussians with a finite opacity"
    return parity(name, h[~bad_r], r[~bad_r])


def _nonfinite_case(variant):
    """A street scene with NaN and +inf on a few visible Gaussians (-inf: test below).  The reference's alpha = fminf(0.99, op G) is 0.99 on
    every pixel of their rects (for +inf too: inf x 0 is NaN where G underflows), so nothing may be pruned."""
    H, W, seed = 16, 512, 41
    scene = surfel_scene("street", 6000, H, seed, random_view=False) if variant == "surfel" else sc.make_scene("street", 6000, H, seed)
    g = _grads(variant, W, H, seed)
    vis = np.flatnonzero(oracle_surfel_forward_backward(scene, W, H)["radii"] > 0 if variant == "surfel" else oracle_forward_backward(scene, W, H)["radii"] > 0)
    pick = vis[np.random.default_rng(seed).choice(vis.size, 8, replace=False)]
    scene["opacities"][pick[:4]] = np.nan
    scene["opacities"][pick[4:]] = np.inf
    hip, ref = _run(variant, scene, W, H, g)
    assert int((hip["radii"] != ref["radii"]).sum()) <= 1
    cover = ref["others"][1] if variant == "surfel" else ref["occ"][0]
    assert (cover >= 0.99 * 0.999).sum() > 64                          # the rects really are covered at 0.99
    for k, v in _images(variant, ref).items():
        assert np.isfinite(v).all()
        parity(f"{variant}.nonfinite.{k}", _images(variant, hip)[k], v)
    n_bad = 0
    for k in _keys(variant):
        parity_nonfinite(f"{variant}.nonfinite.{k}", hip[k], ref[k], pick)
        n_bad += int((~np.isfinite(ref[k])).sum())
    assert n_bad > 0                                                   # their geometry gradients are not finite (dL/dG = op dL/dalpha)
    for k in ("dL_dcolors", "dL_dopacity"):
        assert np.isfinite(ref[k]).all(), k                            # dL/dcolour = alpha T dL/dC, dL/do = G dL/dalpha
    print(f"[nonfinite] {variant}: OK, {n_bad} non-finite gradient entries on both sides")


@pytest.mark.parametrize("variant", ["3d", "surfel"])
def test_nonfinite_opacity(variant):
    _nonfinite_case(variant)


def test_nonfinite_opacity_on_the_five_launch_forward_and_work_list_backward():
    """The 3-D variant's other forward (five launches) and the backward over the work list the combine fills (its default there)."""
    run_child("import test_opacity_domain_gpu as t\nt._nonfinite_case('3d')\nprint('OK')", {"LIDARGS_FUSED": "0"})


@pytest.mark.parametrize("variant", ["3d", "surfel"])
def test_minus_inf_opacity_is_culled(variant):
    """-inf: the reference's -inf x G is -inf (skipped) where G > 0 but NaN where G underflows, so it paints the FAR pixels of the Gaussian's
    rect with alpha 0.99.  The kernels' cull `op * 255 < 1` drops the Gaussian entirely instead ("Opacity domain"): pinned here,
    the frame equals the oracle's frame without those Gaussians, and the oracle's own frame differs from it."""
    H, W, seed = 16, 512, 43
    scene = surfel_scene("street", 6000, H, seed, random_view=False) if variant == "surfel" else sc.make_scene("street", 6000, H, seed)
    g = _grads(variant, W, H, seed)
    fwd = oracle_surfel_forward_backward if variant == "surfel" else oracle_forward_backward
    vis = np.flatnonzero(fwd(scene, W, H)["radii"] > 0)
    pick = vis[np.random.default_rng(seed).choice(vis.size, 4, replace=False)]
    scene["opacities"][pick] = -np.inf
    keep = np.ones(scene["opacities"].shape[0], bool)
    keep[pick] = False
    sub = dict(scene, **{k: np.ascontiguousarray(scene[k][keep]) for k in ("means3D", "scales", "rotations", "opacities", "colors")})
    hip, ref_sub = _run(variant, scene, W, H, g, ref_scene=sub)
    ref_full = fwd(scene, W, H)
    assert not np.array_equal(ref_full["color"], ref_sub["color"])    # the divergence is real: the reference paints far pixels
    for k in _keys(variant):
        assert (hip[k][pick] == 0).all(), k
        parity(f"{variant}.minus_inf.{k}", hip[k][keep], ref_sub[k])
    for k, v in _images(variant, ref_sub).items():
        parity(f"{variant}.minus_inf.{k}", _images(variant, hip)[k], v)
