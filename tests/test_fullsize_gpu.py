"""Full-size GPU checks (BASELINE.json configs 2-4).  The oracle is too slow at these sizes, so the checks are
size-independent properties of the path plus a spot comparison against the oracle on a cropped sub-problem:

  * determinism of the forward (bit-identical images run to run);
  * occ == 1 - T, T in [1e-4 (stop threshold, up to the last factor), 1];
  * linearity of the colour channels in the colours, independence of depth/occ from them;
  * background enters only as T_final * bg;
  * the colour gradient is the exact adjoint of the (linear) colour forward: <g, J d> == <dL/dcolors, d>;
  * every gradient finite; Gaussians with radii == 0 get exactly zero gradient rows;
  * invariance to the internal tiling/segmentation knobs is covered at small size in test_parity_gpu;
  * VALUE checks of the production code path (test_fullsize_wedge_matches_oracle): the FULL frame is rendered on the GPU -- so the
    segment plan, slot count, gated pass-1 rounds, `alive` limits and the adaptive tile height are the ones the bench's
    number comes from -- and the oracle renders every Gaussian that can reach an azimuth wedge of it; the wedge's pixels and
    the gradients of the Gaussians whose whole footprint rect lies inside the wedge are compared value by value.
"""
import numpy as np
import pytest
import torch

import lidargs_scenes as sc
from util import make_settings, to_torch

pytestmark = pytest.mark.gpu


def _render(st, W, H, colors=None, bg=None, grads=None):
    from diff_lidargs_rasterization import GaussianRasterizer
    s2 = dict(st)
    if bg is not None:
        s2["bg"] = bg
    rast = GaussianRasterizer(make_settings(s2, W, H))
    P = st["means3D"].shape[0]
    leaves = {k: st[k].clone().requires_grad_(grads is not None) for k in ("means3D", "opacities", "scales", "rotations")}
    col = (st["colors"] if colors is None else colors).clone().requires_grad_(grads is not None)
    m2 = torch.zeros(P, 4, device="cuda", requires_grad=grads is not None)
    c, d, o, r = rast(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], colors_precomp=col,
                      scales=leaves["scales"], rotations=leaves["rotations"])
    out = dict(color=c, depth=d, occ=o, radii=r)
    if grads is not None:
        torch.autograd.backward([c, d, o], list(grads))
        out.update(g_means3D=leaves["means3D"].grad, g_means2D=m2.grad, g_colors=col.grad, g_opacity=leaves["opacities"].grad,
                   g_scales=leaves["scales"].grad, g_rot=leaves["rotations"].grad)
    return out


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3"])
def test_fullsize_properties(cfg, hip_lib_built):
    kind, P, H, W, seed = sc.BASELINE_CONFIGS[cfg]
    st = to_torch(sc.make_scene(kind, P, H, seed))
    gc, gd, go = (torch.from_numpy(g).cuda() for g in sc.upstream_grads(H, W, seed))
    a = _render(st, W, H, grads=(gc, gd, go))
    b = _render(st, W, H)
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["depth"], b["depth"]) and torch.equal(a["radii"], b["radii"])
    T = 1.0 - a["occ"]
    assert float(T.max()) <= 1.0 and float(T.min()) >= 1e-4 * 0.009          # last blended factor is >= 1 - 0.99
    assert int((a["radii"] > 0).sum()) > 0.5 * P
    # background: colour += T_final * bg, nothing else moves
    bg = torch.tensor([0.25, 0.75], device="cuda")
    c = _render(st, W, H, bg=bg)
    torch.testing.assert_close(c["color"][0], a["color"][0] + T[0] * 0.25, rtol=0, atol=2e-6)
    torch.testing.assert_close(c["color"][1], a["color"][1] + T[0] * 0.75, rtol=0, atol=2e-6)
    assert torch.equal(c["depth"], a["depth"]) and torch.equal(c["occ"], a["occ"])
    # linearity in the colours / adjoint identity for dL/dcolors
    gen = torch.Generator(device="cuda").manual_seed(seed)
    dcol = torch.randn(st["colors"].shape, device="cuda", generator=gen)
    d = _render(st, W, H, colors=dcol)
    e = _render(st, W, H, colors=st["colors"] + dcol)
    torch.testing.assert_close(e["color"], a["color"] + d["color"], rtol=1e-4, atol=2e-5)
    assert torch.equal(d["depth"], a["depth"]) and torch.equal(d["occ"], a["occ"])
    lhs = float((gc.double() * d["color"].double()).sum())
    rhs = float((a["g_colors"].double() * dcol.double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)
    # gradients: finite everywhere, exactly zero for culled Gaussians, sphere-norm statistic >= 0, .w untouched
    culled = a["radii"] == 0
    for k in ("g_means3D", "g_means2D", "g_colors", "g_opacity", "g_scales", "g_rot"):
        g = a[k]
        assert bool(torch.isfinite(g).all()), k
        assert float(g[culled].abs().max()) == 0.0 if bool(culled.any()) else True
    assert float(a["g_means2D"][:, 2].min()) >= 0.0 and float(a["g_means2D"][:, 3].abs().max()) == 0.0


def test_cfg4_size_runs_on_one_gpu(hip_lib_built):
    """8 M Gaussians at 128 x 4096 (config 4's scene) through one GPU: sizing / overflow check of every buffer."""
    kind, P, H, W, seed = sc.BASELINE_CONFIGS["cfg4"]
    st = to_torch(sc.make_scene(kind, P, H, seed))
    gc, gd, go = (torch.from_numpy(g).cuda() for g in sc.upstream_grads(H, W, seed))
    a = _render(st, W, H, grads=(gc, gd, go))
    assert a["color"].shape == (2, H, W) and bool(torch.isfinite(a["color"]).all()) and bool(torch.isfinite(a["depth"]).all())
    assert int((a["radii"] > 0).sum()) == P            # the shell scene lies entirely inside the beam fan and range gate
    for k in ("g_means3D", "g_colors", "g_opacity", "g_scales", "g_rot"):
        assert bool(torch.isfinite(a[k]).all()), k
    assert float((1.0 - a["occ"]).min()) >= 1e-4 * 0.009


def test_crop_of_fullsize_scene_matches_oracle(hip_lib_built):
    """cfg2-density scene restricted to a narrow azimuth wedge so the oracle finishes in seconds: same per-tile list
    lengths and saturation behaviour as the full problem, checked value by value."""
    from util import GRAD_KEYS_SR, hip_forward_backward, oracle_forward_backward, parity
    kind, P, H, W, seed = sc.BASELINE_CONFIGS["cfg2"]
    scene = sc.make_scene(kind, P, H, seed)
    az = np.arctan2(scene["means3D"][:, 1], scene["means3D"][:, 0])
    keep = np.abs(az) < 0.12                               # ~ 100 of 2650 columns
    for k in ("means3D", "scales", "rotations", "opacities", "colors"):
        scene[k] = np.ascontiguousarray(scene[k][keep])
    grads = sc.upstream_grads(H, W, seed)
    ref = oracle_forward_backward(scene, W, H, grads)
    hip = hip_forward_backward(scene, W, H, grads)
    assert int((hip["radii"] != ref["radii"]).sum()) <= max(1, int(1e-4 * keep.sum()))
    for k in ("color", "depth", "occ") + GRAD_KEYS_SR:
        parity(k, hip[k], ref[k])


def _wedge_subset(scene, W, radii, c0, c1):
    """Gaussians that can touch pixel columns [c0, c1): projected column within the Gaussian's own pixel radius (+ margin) of the
    wedge.  `radii` = max(rx, ry) >= rx from the HIP forward; culled Gaussians (radii 0) are kept when within 64 columns, so that
    a cull decision that flips between the two sides shows up as a radii mismatch instead of being hidden by the selection."""
    vm = scene["viewmatrix"].astype(np.float64)
    p = scene["means3D"].astype(np.float64) @ vm[:3, :3] + vm[3, :3]
    pc = (np.pi - np.arctan2(p[:, 1], p[:, 0])) / (2 * np.pi / W)
    reach = np.where(radii > 0, radii.astype(np.float64) + 32.0, 64.0)
    return (pc >= c0 - reach) & (pc <= c1 + reach)


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3", "cfg4", "cfg3_waymo", "cfg2_neartie", "cfg3_thin", "cfg3_bimodal"])
def test_fullsize_wedge_matches_oracle(cfg, hip_lib_built):
    """The headline frame's own code path, value by value (see the module docstring).  cfg4 (8 M Gaussians @ 128 x 4096) runs at
    the adaptive 16- or 32-row tile height; cfg2 / cfg3 on the fine segment plan (64-entry segments, 45 slots, gated first round).
    `cfg3_waymo` / `cfg2_neartie` (round 3): the same frames on NON-UNIFORM beam tables (lidargs_scenes.beam_table) -- what the Waymo
    configs really read from the dataset json (scene/dataset_readers.py:358-359); radii must then agree with 0 mismatches.
    `cfg3_thin` (round 6): the 2 M-Gaussian frame with every opacity x 0.1 -- the semi-transparent state training starts in
    (gaussian_renderer/__init__.py:60-70): no pixel saturates early, every segment of every list is walked and handed over, the
    `alive` gates stay open and the slot plan fills; the regime the saturating street scene never visits at this size.
    `cfg3_bimodal`: the same frame with a trained model's opacities (lidargs_scenes.make_scene opacity="bimodal": 70 % U(0.01, 0.1),
    30 % U(0.7, 1)) -- saturating and nearly transparent lists in one patch, what the gated rounds and the slot plans see in training."""
    from diff_lidargs_rasterization import _C
    from util import GRAD_KEYS_SR, hip_forward_backward, oracle_forward_backward, parity
    cfg, _, table = cfg.partition("_")
    thin, bimodal = table == "thin", table == "bimodal"
    if thin or bimodal:
        table = ""
    kind, P, H, W, seed = sc.BASELINE_CONFIGS[cfg]
    scene = sc.make_scene(kind, P, H, seed, beams=table or None, opacity_scale=0.1 if thin else 1.0, opacity="bimodal" if bimodal else None)
    grads = sc.upstream_grads(H, W, seed)
    hip = hip_forward_backward(scene, W, H, grads)                    # the FULL frame
    cnt = _C.last_counters()
    print(f"[wedge] {cfg}: instances {cnt['instances']}, tile_rows {cnt['tile_rows']}, segment slots {cnt['segments']}, "
          f"visible {int((hip['radii'] > 0).sum())}")
    if cfg == "cfg4":
        assert cnt["tile_rows"] in (16, 32), cnt                      # the adaptive choice the bench line of this config runs with (32 since r02)
    elif not table:
        assert cnt["tile_rows"] == 4 and cnt["segments"] == 45, cnt   # the fine plan of api.hip plan_segments
    half = 96 if cfg != "cfg4" else 64
    # two wedges: looking down the street (long lists, early saturation) and at a wall / across the shell
    for centre in (W // 2, W // 4 + 8):
        c0 = (centre - half) // 16 * 16
        c1 = c0 + 2 * half
        keep = _wedge_subset(scene, W, hip["radii"], c0, c1)
        sub = dict(scene)
        for k in ("means3D", "scales", "rotations", "opacities", "colors"):
            sub[k] = np.ascontiguousarray(scene[k][keep])
        ref = oracle_forward_backward(sub, W, H, grads)
        rows = np.nonzero(keep)[0]
        mism = int((hip["radii"][rows] != ref["radii"]).sum())
        print(f"[wedge] {cfg} columns [{c0},{c1}): {keep.sum()} Gaussians in reach, radii mismatches {mism}")
        assert mism <= (0 if table else max(1, int(1e-4 * keep.sum())))
        for k in ("color", "depth", "occ"):
            parity(f"{cfg}.{k}[{c0}:{c1}]", hip[k][..., c0:c1], ref[k][..., c0:c1])
        # Gaussians whose whole reference rect (R3/cr/auxiliary.h:80-92, 16-pixel tile columns) lies inside the wedge: every pixel
        # that feeds their gradient was rendered by both sides from the same, complete, list
        m2 = ref["fwd"].array("means2D").reshape(-1, 2)
        rx = ref["fwd"].array("radii_xy").reshape(-1, 2)[:, 0].astype(np.float64)
        x_lo = np.floor((m2[:, 0] - rx) / 16.0) * 16
        x_hi = np.floor((m2[:, 0] + rx + 15.0) / 16.0) * 16
        inside = (ref["radii"] > 0) & (hip["radii"][rows] > 0) & (x_lo >= c0) & (x_hi <= c1)
        assert inside.sum() > 2000, inside.sum()
        print(f"[wedge] {cfg} columns [{c0},{c1}): {int(inside.sum())} Gaussians with their whole rect inside")
        if thin or bimodal:    # opacities 0.01-0.1: a large share of the (pixel, Gaussian) pairs sits near the alpha >= 1/255 threshold (R3/cr/forward.cu:607),
                    # and every gradient row is a long float32 sum: where the plain budget is exceeded the excess must be the oracle's
                    # summation error or lie in the reference's own band (util.parity_or_closer)
            from util import oracle_backward_exact_sums, oracle_envelope, parity_or_closer
            ref64 = oracle_backward_exact_sums(ref, grads)
            env = {}

            def band(k):
                if not env:
                    _b, lo, hi = oracle_envelope(sub, W, H, grads, {}, GRAD_KEYS_SR)
                    env.update(lo=lo, hi=hi)
                return env["lo"][k][inside], env["hi"][k][inside]
            for k in GRAD_KEYS_SR:
                parity_or_closer(f"{cfg}_{'thin' if thin else 'bimodal'}.{k}[wedge]", hip[k][rows[inside]], ref[k][inside], ref64[k][inside], band=lambda k=k: band(k))
            continue
        for k in GRAD_KEYS_SR:
            parity(f"{cfg}.{k}[wedge]", hip[k][rows[inside]], ref[k][inside])


def test_frame_far_above_the_baseline_sizes(hip_lib_built):
    """Maximum-size behaviour (round 6): 24 M Gaussians @ 128 x 4096 -- three times BASELINE config 4, ~10^8 instances, the LSD range sort, 32-row
    tiles -- through the drop-in package: deterministic forward, occ = 1 - T inside [0, 1], finite gradients, exact zero rows for the
    Gaussians no pixel took.  (tools/big_frame.py ran 200 M Gaussians / 8.7e8 instances / 90 GB the same way: profiles/r06_big_frames.txt.)"""
    P, H, W = 24_000_000, 128, 4096
    st = to_torch(sc.make_scene("shell", P, H, 9))
    g = tuple(torch.from_numpy(x).cuda() for x in sc.upstream_grads(H, W, 9))
    a = _render(st, W, H, grads=g)
    b = _render(st, W, H)
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["depth"], b["depth"]) and torch.equal(a["radii"], b["radii"])
    T = 1.0 - a["occ"]
    assert float(T.max()) <= 1.0 and float(T.min()) >= 1e-4 * 0.009
    for k in ("g_means3D", "g_means2D", "g_colors", "g_opacity", "g_scales", "g_rot"):
        assert bool(torch.isfinite(a[k]).all()), k
    touched = a["g_opacity"].view(-1) != 0
    assert 1000 < int(touched.sum()) < P // 100                      # a saturating shell scene: a few thousand Gaussians carry every gradient
    assert bool((a["g_means3D"][~touched] == 0).all()) and bool((a["g_scales"][~touched] == 0).all())
