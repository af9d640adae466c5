"""LIDARGS_DEPTH=strongest restated (DESIGN.md "Median-range depth", the strongest-return rule): the rule on top of the CPU oracle's
forward state, and a float64 torch forward whose depth output is depth[strongest_id], so that torch.autograd gives the mode's reference
gradients.  The lists, the float64 helpers and the random scenes are tests/median_ref.py's; the pick is written here.

The rule.  Per pixel, walk its list in blend order from T = 1, best = 0; an entry is TAKEN as the blend takes it (power <= 0,
alpha = min(0.99, o exp(power)) >= 1/255).  For every taken entry j:
    test = T (1 - alpha_j);  if test < 1e-4 the pixel ends and j does not count (the blend's stop);
    w = alpha_j T;  if w > best (strict: among equal weights the nearer entry stays):  best = w, strongest = depth_j, strongest_id = j;
    T = test
A pixel without a taker has depth 0 and no id (-1 here).  Nothing behind the first T <= best can win (alpha' T' <= 0.99 T), which is
where the kernel's walk leaves; this restatement walks every list to its end and tests/test_strongest_depth_cpu.py checks that bound.

Undecided pixels give no vote in a comparison and get a zero upstream depth gradient.  A pixel is undecided if
  * its runner-up weight is >= (1 - TIE) x its top weight (another Gaussian, metres away, wins in float32), or
  * any valid entry of its list has alpha within UNDECIDED (relative) of 1/255, or its power within that band of 0 (median_ref's two
    tests, here over the whole list: every taker moves T for all behind it), or
  * some taken entry's T behind it lies within STOP_BAND (relative) of 1e-4.
"""
import numpy as np
import torch

import median_ref as mr
import preprocess_ref as pr
from median_ref import F64, H, SIGMA, OFF, THIN_N, THIN_OP, _t, pixel_lists

UNDECIDED = mr.UNDECIDED       # 1e-3
TIE = 1e-3
STOP_BAND = 1e-2
CAP = 0.02                     # undecided pixels / pixels with a taker, at most, on every scene below (asserted on the CPU)
GRAD_KEYS = mr.GRAD_KEYS


def blend(idx, valid, dirs, conic, opac, colors, depth, u1, u2, sph, bg, e=None):
    """The per-pixel loop of the blend (R3/cr/forward.cu:578-637) and the strongest-return rule over the padded lists, in float64 torch.
    Arguments as median_ref.blend.  -> dict of [N]-leading tensors; `table`: the [N, L] tensors the CPU tests look into."""
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
    T_incl = torch.cumprod(torch.where(hit, 1.0 - alpha, one), 1)
    T_excl = torch.cat([torch.ones(N, 1, dtype=F64), T_incl[:, :-1]], 1)
    trip = hit & (T_incl < 0.0001)                                           # :607-611: the first one ends the walk and does not count
    taken = hit & (torch.cumsum(trip.long(), 1) == 0)
    wgt = torch.where(taken, alpha * T_excl, torch.zeros_like(alpha))        # :615-617
    col = (wgt[..., None] * colors[I]).sum(1)
    D = (wgt * depth[I]).sum(1)
    T_fin = torch.where(taken, 1.0 - alpha, one).prod(1)
    # the strongest-return rule: the first entry that holds the largest weight
    rows, ar = torch.arange(N), torch.arange(L)
    with torch.no_grad():
        has = taken.any(1)
        top = wgt.max(1).values
        pos = torch.where(taken & (wgt >= top[:, None]), ar, L).min(1).values.clamp(max=L - 1)
    sid = torch.where(has, I[rows, pos], torch.full((N,), -1, dtype=torch.long))
    sdepth = torch.where(has, depth[I[rows, pos]], torch.zeros(N, dtype=F64))
    with torch.no_grad():
        others = wgt.clone()
        others[rows, pos] = 0.0
        runner = others.max(1).values
        near_tie = has & (runner >= (1.0 - TIE) * top)
        near_alpha = V & (power <= UNDECIDED) & ((raw * 255.0 - 1.0).abs() <= UNDECIDED)
        near_power = V & (power.abs() <= UNDECIDED) & (opac[I] * 255.0 >= 1.0 - UNDECIDED)
        near_stop = taken & ((T_incl - 1e-4).abs() <= STOP_BAND * 1e-4)
        decided = ~(near_tie | (near_alpha | near_power | near_stop).any(1))
    return dict(color=col + T_fin[:, None] * bg, expected=D, occ=1.0 - T_fin, strongest_id=sid, strongest_depth=sdepth, decided=decided,
                has_taker=has, top_weight=top.detach(), runner_up=runner,
                table=dict(idx=I, valid=V, hit=hit, taken=taken, weight=wgt.detach(), T_after=T_incl.detach(), pos=pos))


def restate(f, scene, W, H):
    """The rule on the oracle's float32 record values.  -> numpy: strongest_id [H,W] (-1: none), strongest_depth, decided, has_taker,
    top_weight, runner_up, expected, occ [H,W], color [2,H,W]; `table`: numpy [H W, L] arrays (blend)."""
    P = scene["means3D"].shape[0]
    idx, valid = pixel_lists(f, W, H)
    co = f.array("conic_opacity").reshape(P, 4)
    with torch.no_grad():
        r = blend(idx, valid, _t(pr.pixel_dirs(W, H, scene["beams"]).reshape(-1, 3)), _t(co[:, :3]), _t(co[:, 3]), _t(scene["colors"]),
                  _t(f.array("depths")), _t(f.array("basis_u1").reshape(P, 3)), _t(f.array("basis_u2").reshape(P, 3)),
                  _t(f.array("sphere").reshape(P, 3)), _t(scene["bg"]))
    out = {k: v.numpy().reshape(H, W) for k, v in r.items() if k not in ("color", "table")}
    out["color"] = r["color"].numpy().T.reshape(2, H, W)
    out["table"] = {k: v.numpy() for k, v in r["table"].items()}
    return out


def undecided_fraction(r):
    """Undecided pixels as a fraction of the pixels that have a taker."""
    return float((~r["decided"] & r["has_taker"]).sum()) / max(1, int(r["has_taker"].sum()))


def exit_positions(table):
    """Per pixel with a taker: the 0-based list position of the first taken entry behind which T <= best (the kernel's pixel leaves
    there), or of the list's last valid entry if there is none.  -> (positions [n], largest weight behind that position [n], best there [n])."""
    w, T, taken, valid = table["weight"], table["T_after"], table["taken"], table["valid"]
    best = np.maximum.accumulate(w, axis=1)
    left = taken & (T <= best)
    has = taken.any(1)
    L = w.shape[1]
    last = np.maximum(valid.sum(1) - 1, 0)
    first = np.where(left.any(1), left.argmax(1), last)
    behind = np.where(np.arange(L)[None, :] > first[:, None], w, 0.0).max(1)
    return first[has], behind[has], best[np.arange(w.shape[0]), first][has]


def reference(scene, W, H, grads, f=None):
    """The float64 reference of a strongest-mode forward + backward, built as median_ref.reference is: K1's formulas in front of `blend`,
    upstream gradients `grads` = (dL_dcolor [2,H,W], dL_ddepth [1,H,W], dL_docc [1,H,W]) with dL_ddepth zeroed on undecided pixels.
    -> dict: the restatement's planes (restate), `fwd`, `depth`, `dL_ddepth_masked` and the six gradient arrays (util.GRAD_KEYS_SR)."""
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
    mine = np.where(r["strongest_id"].numpy() >= 0, sel[r["strongest_id"].clamp(min=0)].numpy(), -1)
    same = mine == rs["strongest_id"].ravel()
    assert same[rs["decided"].ravel()].all(), "the float64 chain and the oracle's float32 records disagree on a decided pixel"
    gc, gd, go = (_t(g) for g in grads)
    gd_masked = gd.reshape(-1) * torch.as_tensor(rs["decided"].ravel() & same, dtype=F64)
    loss = (r["color"].T.reshape(-1) * gc.reshape(-1)).sum() + (r["strongest_depth"] * gd_masked).sum() + (r["occ"] * go.reshape(-1)).sum()
    gm, gs, gq, gop, gcol, ge = torch.autograd.grad(loss, [means, scales, rots, opac, colors, e])
    g2 = np.zeros((P, 4))
    pair = ge.numpy()
    np.add.at(g2[:, 0], idx[valid], pair[valid][:, 0])
    np.add.at(g2[:, 1], idx[valid], pair[valid][:, 1])
    np.add.at(g2[:, 2], idx[valid], np.sqrt((pair[valid] ** 2).sum(-1)))      # the densification statistic: a sum of per-pixel norms
    out = dict(rs)
    out.update(fwd=f, depth=r["strongest_depth"].detach().numpy().reshape(1, H, W),
               dL_ddepth_masked=gd_masked.numpy().reshape(1, H, W).astype(np.float32), dL_dmeans3D=gm.numpy(), dL_dmeans2D=g2,
               dL_dcolors=gcol.numpy(), dL_dopacity=gop.numpy().reshape(P, 1), dL_dscales=gs.numpy(), dL_drotations=gq.numpy())
    return out


# ---- the scenes of tests/test_strongest_depth_cpu.py and tests/test_strongest_depth_gpu.py ------------------------------------------
VEIL_N, VEIL_OP = 10, 0.1          # ten thin layers, 1 cm apart, in front of a wall
LATE_N, LATE_OP = 100, 0.005       # 100 layers that leave T = 0.61: the wall behind them sits in the list's second 64-entry chunk
WALL = (20.0, 0.9)


def placed(W):
    """Hand-placed rays, laid out and sized as median_ref.placed's (SIGMA wide, OFF x SIGMA beside their pixel's centre: alpha =
    0.995 x opacity).  -> scene, {case: (x, y, range of the strongest return or 0, index of its Gaussian or -1)}, {case: indices of
    the ray's Gaussians}.  The wanted answer is worked out here by the rule's arithmetic on the nominal alphas."""
    from util import placed_scene
    rays = {   # case: (x, y, [(range, opacity)])
        "0.4/0.9": (8, 2, [(10.0, 0.4), (20.0, 0.9)]),              # weights 0.40, 0.54: the second
        "0.6/0.9": (24, 2, [(10.0, 0.6), (20.0, 0.9)]),             # weights 0.60, 0.36: the first
        "veil": (40, 2, [(10.0 + 0.01 * k, VEIL_OP) for k in range(VEIL_N)] + [WALL]),   # layers <= 0.10, wall 0.31 (the median: the 7th layer)
        "never": (8, 8, [(10.0, 0.2), (20.0, 0.2)]),                # weights 0.20, 0.16: the first (the median mode says the last taker)
        "thin": (24, 8, [(10.0 + 0.01 * k, THIN_OP) for k in range(THIN_N)]),             # falling weights: the first (the median: the 35th)
        "late wall": (56, 10, [(10.0 + 0.01 * k, LATE_OP) for k in range(LATE_N)] + [WALL]),   # layers <= 0.005, wall 0.54 at entry 101
        "last column": (W - 1, 13, [(10.0, 0.4), (20.0, 0.9)]),
        "first column": (0, 6, [(12.0, 0.4), (18.0, 0.9)]),         # (its footprint reaches over the seam into the last tile column)
    }
    pc, py, dist, op, want, members = [], [], [], [], {}, {}
    for case, (x, y, gs) in rays.items():
        T, best, pick = 1.0, 0.0, -1
        first = len(dist)
        for d, o in gs:
            a = o * np.exp(-0.5 * OFF * OFF)
            if a * T > best:
                best, pick = a * T, len(dist)
            T *= 1.0 - a
            pc.append(x + OFF * SIGMA / (2 * np.pi / W)); py.append(float(y)); dist.append(d); op.append(o)
        want[case] = (x, y, dist[pick], pick)
        members[case] = np.arange(first, len(dist))
    want["nothing"] = (40, 8, 0.0, -1)
    members["nothing"] = np.arange(0)
    dist = np.array(dist)
    sigma = np.sqrt((SIGMA * dist) ** 2 - 0.01)               # the 2-D covariance gets + 0.01 (R3/cr/forward.cu:166-167)
    return placed_scene(pc, py, dist, sigma, op, W, H), want, members


PLACED = ("strongest64", "strongest250", "strongest256")
SCENES = mr.SCENES + PLACED
BACKWARD_SCENES = mr.BACKWARD_SCENES       # their float32 budget is asserted by tests/test_median_depth_cpu.py and does not depend on the mode


def scene(name):
    """-> scene, W.  `strongest64 / 250 / 256`: placed(W); every other name: median_ref.scene."""
    if name in PLACED:
        W = int(name[9:])
        return placed(W)[0], W
    return mr.scene(name)


def upstream(name):
    """The upstream gradients (dL_dcolor [2,H,W], dL_ddepth [1,H,W], dL_docc [1,H,W]) the tests use for scene `name`."""
    import lidargs_scenes as sc
    return sc.upstream_grads(H, scene(name)[1], 300 + SCENES.index(name))
