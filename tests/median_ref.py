"""LIDARGS_DEPTH=median restated (DESIGN.md "Median-range depth"): the rule on top of the CPU oracle's forward state, and a float64 torch
forward whose depth output is depth[median_id], so that torch.autograd gives the mode's reference gradients.

The rule (2DGS's, as the surfel oracle already has it).  Per pixel, walk its list in blend order from T = 1; an entry is TAKEN as the
blend takes it (power <= 0, alpha = min(0.99, o exp(power)) >= 1/255, in front of the T < 1e-4 stop).  For every taken entry j:
    if T > 0.5 (strict):  median = depth_j, median_id = j;         then  T *= 1 - alpha_j
A pixel whose T never reaches 0.5 keeps its last taker; a pixel without a taker has depth 0 and no id (-1 here).

Undecided pixels.  A decision of the rule that sits within rounding of its threshold can fall either way in float32, and then another
Gaussian -- metres away -- is the median.  Such a pixel gives no vote in a comparison and gets a zero upstream depth gradient:
  * some entry the decision rests on (up to and including the crossing entry; the whole list if T never crosses) has alpha within
    UNDECIDED = 1e-3 (relative) of 1/255, or its power within that band of 0 (tests/preprocess_ref.py's band);
  * at a taken entry up to the crossing, T before or after it lies within T_BAND = 1e-4 (relative) of 0.5.

Which Gaussians a pixel's list holds, and in which order, is the oracle's forward state (its 16 x 1 tiles); everything behind it is
re-evaluated here, vectorised over [pixels, longest list].
"""
import numpy as np
import torch

import preprocess_ref as pr

F64 = torch.float64
UNDECIDED = pr.UNDECIDED       # 1e-3
T_BAND = 1e-4
GRAD_KEYS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dscales", "dL_drotations")


def pixel_lists(f, W, H):
    """The oracle's lists as a padded table: idx [H W, L] Gaussian ids in blend order, valid [H W, L].  Pads name a listed Gaussian
    (so that every row evaluates to finite numbers) and are masked by `valid`."""
    pl = f.array("point_list").astype(np.int64)
    rg = f.array("ranges").reshape(-1, 2).astype(np.int64)
    tiles_x = (W + 15) // 16
    L = max(1, int((rg[:, 1] - rg[:, 0]).max()) if rg.size else 1)
    pad = int(pl[0]) if pl.size else 0
    idx = np.full((H * W, L), pad, np.int64)
    valid = np.zeros((H * W, L), bool)
    for y in range(H):
        for tx in range(tiles_x):
            a, b = rg[y * tiles_x + tx]
            rows = y * W + np.arange(16 * tx, min(W, 16 * tx + 16))
            idx[rows, :b - a] = pl[a:b]
            valid[rows, :b - a] = True
    return idx, valid


def blend(idx, valid, dirs, conic, opac, colors, depth, u1, u2, sph, bg, e=None):
    """The per-pixel loop of the blend (R3/cr/forward.cu:578-637) and the median rule over the padded lists, in float64 torch.
    conic [P,3], opac [P], colors [P,2], depth [P], u1 / u2 / sph [P,3] (u_i unscaled: d = delta . u_i / u_i . u_i); e: optional
    [N, L, 2] probe added to d (its gradient is the per-pair dL/dd).  -> dict of [N]-leading tensors."""
    I = torch.as_tensor(idx)
    V = torch.as_tensor(valid)
    N, L = I.shape
    delta = sph[I] - dirs[:, None, :]
    U1, U2 = u1[I], u2[I]
    dx = (delta * U1).sum(-1) / (U1 * U1).sum(-1)
    dy = (delta * U2).sum(-1) / (U2 * U2).sum(-1)
    if e is not None:
        dx = dx + e[..., 0]; dy = dy + e[..., 1]
    A, B, C = conic[I, 0], conic[I, 1], conic[I, 2]
    power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy                 # :601
    raw = opac[I] * torch.exp(torch.clamp(power, max=0.0))
    alpha = torch.clamp(raw, max=0.99)                                       # :604
    hit = V & (power <= 0.0) & (alpha >= 1.0 / 255.0)                        # :602, :605
    one = torch.ones_like(alpha)
    fct = torch.where(hit, 1.0 - alpha, one)
    T_incl = torch.cumprod(fct, 1)
    T_excl = torch.cat([torch.ones(N, 1, dtype=F64), T_incl[:, :-1]], 1)
    trip = hit & (T_incl < 0.0001)                                           # :607-611: the first one ends the walk
    live = torch.cumsum(trip.long(), 1) == 0
    taken = hit & live
    wgt = torch.where(taken, alpha * T_excl, torch.zeros_like(alpha))        # :615-617
    col = (wgt[..., None] * colors[I]).sum(1)
    D = (wgt * depth[I]).sum(1)
    T_fin = torch.where(taken, 1.0 - alpha, one).prod(1)
    # the median rule
    cand = taken & (T_excl > 0.5)
    has = cand.any(1)
    ar = torch.arange(L)
    pos = (cand.long() * ar).max(1).values                                   # the last candidate (candidates are a prefix of the takers)
    mid = torch.where(has, I[torch.arange(N), pos], torch.full((N,), -1, dtype=torch.long))
    mdepth = torch.where(has, depth[I[torch.arange(N), pos]], torch.zeros(N, dtype=F64))
    with torch.no_grad():
        crossing = taken & (T_incl <= 0.5)
        upto = (torch.cumsum(crossing.long(), 1) - crossing.long()) == 0    # positions up to and including the first crossing
        rests = V & upto                                                     # (a crossing lies in front of any T < 1e-4 stop)
        near_alpha = rests & (power <= UNDECIDED) & ((raw * 255.0 - 1.0).abs() <= UNDECIDED)
        near_power = rests & (power.abs() <= UNDECIDED) & (opac[I] * 255.0 >= 1.0 - UNDECIDED)
        half = 0.5 * T_BAND
        near_T = taken & upto & (((T_excl - 0.5).abs() <= half) | ((T_incl - 0.5).abs() <= half))
        decided = ~(near_alpha | near_power | near_T).any(1)
    return dict(color=col + T_fin[:, None] * bg, expected=D, occ=1.0 - T_fin, median_id=mid, median_depth=mdepth, decided=decided,
                has_taker=taken.any(1), crossed=(taken & (T_incl <= 0.5)).any(1), n_takers_to_median=(cand.long().sum(1)))


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64), dtype=F64)


def restate(f, scene, W, H):
    """The rule on the oracle's float32 record values.  -> numpy: median_id [H,W] (-1: none), median_depth [H,W], decided [H,W],
    has_taker [H,W], crossed [H,W], expected [H,W], color [2,H,W], occ [H,W]."""
    P = scene["means3D"].shape[0]
    idx, valid = pixel_lists(f, W, H)
    co = f.array("conic_opacity").reshape(P, 4)
    with torch.no_grad():
        r = blend(idx, valid, _t(pr.pixel_dirs(W, H, scene["beams"]).reshape(-1, 3)), _t(co[:, :3]), _t(co[:, 3]), _t(scene["colors"]),
                  _t(f.array("depths")), _t(f.array("basis_u1").reshape(P, 3)), _t(f.array("basis_u2").reshape(P, 3)),
                  _t(f.array("sphere").reshape(P, 3)), _t(scene["bg"]))
    out = {k: v.numpy().reshape(H, W) for k, v in r.items() if k != "color"}
    out["color"] = r["color"].numpy().T.reshape(2, H, W)
    return out


def undecided_fraction(r):
    """Undecided pixels as a fraction of the pixels that have a taker."""
    return float((~r["decided"] & r["has_taker"]).sum()) / max(1, int(r["has_taker"].sum()))


def reference(scene, W, H, grads, f=None):
    """The float64 reference of a median-mode forward + backward: K1's formulas (preprocess_ref.k1 + record, with the reference's damped
    conic gradient) in front of `blend`, leaves = means3D / scales / rotations / opacities / colours, upstream gradients `grads` =
    (dL_dcolor [2,H,W], dL_ddepth [1,H,W], dL_docc [1,H,W]) with dL_ddepth zeroed on undecided pixels.  Scale modifier 1.
    -> dict: the restatement's planes (restate), the forward's color / depth / occ, `dL_ddepth_masked`, and the six gradient arrays
    named as util.GRAD_KEYS_SR."""
    from oracle import lgo
    if f is None:
        f = lgo.forward(scene["means3D"], scene["colors"], scene["opacities"], scene["scales"], scene["rotations"], scene["viewmatrix"],
                        scene["beams"], W, H, bg=scene["bg"])
    P = scene["means3D"].shape[0]
    rs = restate(f, scene, W, H)
    idx, valid = pixel_lists(f, W, H)
    vis = np.asarray(f.radii).reshape(-1) > 0
    assert vis[idx[valid]].all()
    remap = np.cumsum(vis) - 1                                               # Gaussian id -> row among the visible ones
    leaf = lambda a: _t(a).requires_grad_(True)
    means, scales, rots = leaf(scene["means3D"]), leaf(scene["scales"]), leaf(scene["rotations"])
    opac, colors = leaf(scene["opacities"].reshape(-1)), leaf(scene["colors"])
    sel = torch.as_tensor(np.nonzero(vis)[0])
    k = pr.k1(means[sel], pr.cov6_of(scales[sel], rots[sel]), _t(np.asarray(scene["viewmatrix"]).reshape(16)))
    rec = pr.record(k, damped=True)
    e = torch.zeros(idx.shape + (2,), dtype=F64, requires_grad=True)
    r = blend(remap[idx], valid, _t(pr.pixel_dirs(W, H, scene["beams"]).reshape(-1, 3)), rec["conic"], opac[sel], colors[sel], k["dist"],
              k["u1"], k["u2"], k["dir"], _t(scene["bg"]), e)
    mine = np.where(r["median_id"].numpy() >= 0, sel[r["median_id"].clamp(min=0)].numpy(), -1)
    same = mine == rs["median_id"].ravel()
    assert same[rs["decided"].ravel()].all(), "the float64 chain and the oracle's float32 records disagree on a decided pixel"
    gc, gd, go = (_t(g) for g in grads)
    gd_masked = gd.reshape(-1) * torch.as_tensor(rs["decided"].ravel() & same, dtype=F64)
    loss = (r["color"].T.reshape(-1) * gc.reshape(-1)).sum() + (r["median_depth"] * gd_masked).sum() + (r["occ"] * go.reshape(-1)).sum()
    gm, gs, gq, gop, gcol, ge = torch.autograd.grad(loss, [means, scales, rots, opac, colors, e])
    g2 = np.zeros((P, 4))
    pair = ge.numpy()
    np.add.at(g2[:, 0], idx[valid], pair[valid][:, 0])
    np.add.at(g2[:, 1], idx[valid], pair[valid][:, 1])
    np.add.at(g2[:, 2], idx[valid], np.sqrt((pair[valid] ** 2).sum(-1)))      # the densification statistic: a sum of per-pixel norms
    out = dict(rs)
    out.update(fwd=f, depth=r["median_depth"].detach().numpy().reshape(1, H, W), dL_ddepth_masked=gd_masked.numpy().reshape(1, H, W).astype(np.float32),
               dL_dmeans3D=gm.numpy(), dL_dmeans2D=g2, dL_dcolors=gcol.numpy(), dL_dopacity=gop.numpy().reshape(P, 1), dL_dscales=gs.numpy(),
               dL_drotations=gq.numpy())
    return out


# ---- the scenes of tests/test_median_depth_cpu.py (the cap on undecided pixels) and tests/test_median_depth_gpu.py ------------------
H = 16
CAP = 0.02          # undecided pixels / pixels with a taker, at most, on every scene below (asserted on the CPU)
# name: (kind, P, W, seed, factor on the scales): footprints of several pixels, so that many rays cross one half behind a few takers
RANDOM = {"shell256": ("shell", 400, 256, 74, 10.0), "street250": ("street", 400, 250, 79, 8.0), "shell64": ("shell", 300, 64, 77, 8.0),
          "shell250": ("shell", 400, 250, 92, 12.0)}
SIGMA = 0.02        # angular width (radians) of the hand-placed Gaussians: under one row gap (20 degrees / 15 rows = 0.023), rays 4 rows apart do not meet
OFF = 0.1           # ... which sit OFF x SIGMA beside their pixel's centre, in azimuth: power = -0.5 OFF^2 = -5e-3, outside the band of 0
THIN_N, THIN_OP = 300, 0.02
THIN_SHORT = 100    # the thin ray of the `placedshort` scenes: two 64-entry chunks, crossing at the 35th as the long one


def placed(W, thin_n=THIN_N):
    """Hand-placed rays (util.placed_scene), every Gaussian SIGMA wide and OFF x SIGMA beside the centre of its pixel, so that alpha =
    opacity x exp(-0.5 OFF^2) = 0.995 x opacity there (a little less off the equator).  -> scene, {case: (x, y, median range or 0, index of
    the median Gaussian or -1)}.  Rows and columns far enough apart that no ray sees another's Gaussians."""
    from util import placed_scene
    rays = {   # case: (x, y, [(range, opacity)])
        "0.4/0.9": (8, 2, [(10.0, 0.4), (20.0, 0.9)]),              # T = 0.60 behind the first: the second is the median (expected: 14.8)
        "0.6/0.9": (24, 2, [(10.0, 0.6), (20.0, 0.9)]),             # T = 0.40 behind the first
        "opaque": (40, 2, [(15.0, 0.99)]),
        "never": (8, 8, [(10.0, 0.2), (20.0, 0.2)]),                # T ends at 0.64: the last taker
        "thin": (24, 8, [(10.0 + 0.01 * k, THIN_OP) for k in range(thin_n)]),   # 0.98^34 > 0.5 > 0.98^35: the 35th
        "last column": (W - 1, 13, [(10.0, 0.4), (20.0, 0.9)]),
        "first column": (0, 6, [(12.0, 0.4), (18.0, 0.9)]),         # (its footprint reaches over the seam into the last tile column)
    }
    pc, py, dist, op, want = [], [], [], [], {}
    for case, (x, y, gs) in rays.items():
        T, med = 1.0, -1
        for d, o in gs:
            a = o * np.exp(-0.5 * OFF * OFF)
            if T > 0.5:
                med = len(dist)
            T *= 1.0 - a
            pc.append(x + OFF * SIGMA / (2 * np.pi / W)); py.append(float(y)); dist.append(d); op.append(o)
        want[case] = (x, y, dist[med], med)
    want["nothing"] = (40, 8, 0.0, -1)
    dist = np.array(dist)
    sigma = np.sqrt((SIGMA * dist) ** 2 - 0.01)               # the 2-D covariance gets + 0.01 (R3/cr/forward.cu:166-167)
    return placed_scene(pc, py, dist, sigma, op, W, H), want


def scene(name):
    """-> scene, W.  `placed64 / placed250 / placed256`: placed(W); `placedshort64`: placed(64, THIN_SHORT); the others: RANDOM, opacities
    U(0.15, 0.9) (below the 0.99 clamp, where the blend's backward is the analytic gradient)."""
    import lidargs_scenes as sc
    if name.startswith("placedshort"):
        W = int(name[11:])
        return placed(W, THIN_SHORT)[0], W
    if name.startswith("placed"):
        W = int(name[6:])
        return placed(W)[0], W
    kind, P, W, seed, k = RANDOM[name]
    s = sc.make_scene(kind, P, H, seed, random_view=True)
    s["opacities"] = np.random.default_rng([seed, 0x3ED]).uniform(0.15, 0.9, (P, 1)).astype(np.float32)
    s["scales"] = (s["scales"] * k).astype(np.float32)
    return s, W


SCENES = ("shell256", "street250", "shell64", "placed64", "placed250", "placed256", "shell250", "placedshort64")
# The scenes whose gradients are compared with the float64 reference at util.parity's default budget.  That budget (1e-4 relative; two
# entries, or 2.5e-4 of them, up to 1e-3) is at the edge of what ANY float32 evaluation keeps against float64 where a sum's terms cancel,
# and the reference itself does not pin the last bits: its cos / sin / atan2 / exp are good to a few ulp, its atomics add in scheduling
# order.  A scene qualifies only if EVERY conforming float32 evaluation of the reference the project has -- the CPU oracle as it is,
# the four with those functions moved inside their error bounds (util.ULP_MODES) and the one with the pixels in reverse order; default
# mode, no depth gradient, nothing of the median mode in it -- meets the budget against this file's float64 chain on all six arrays.
# tests/test_median_depth_cpu.py asserts that these do and that the other scenes above do not.  Entries in (1e-4, 1e-3] where 2 are
# allowed, worst of the six evaluations, on the ones that do not: placed64 53 and placed256 9 of the 311 dL_dopacity (the 300-Gaussian
# ray's: a weighted mean over up to 300 entries behind is taken from each colour, and where the two nearly cancel the recurrence's
# float32 rounding shows), street250 4 of the 1200 dL_dmeans3D.  Such a scene says nothing about a kernel: another conforming evaluation
# of the same formulas fails on it.  Hence shell250 beside street250, and placedshort64 -- placed64's rays with the thin one cut to
# THIN_SHORT entries -- beside placed64; hand-placed rays at W = 256 do not qualify with a short thin ray either (dL_dcolors, 5 of 222).
BACKWARD_SCENES = ("shell256", "shell64", "shell250", "placed250", "placedshort64")


def upstream(name):
    """The upstream gradients (dL_dcolor [2,H,W], dL_ddepth [1,H,W], dL_docc [1,H,W]) the tests use for scene `name`."""
    import lidargs_scenes as sc
    return sc.upstream_grads(H, scene(name)[1], 300 + SCENES.index(name))
