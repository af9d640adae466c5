"""LIDARGS_DEPTH=strongest restated (DESIGN.md "Median-range depth", the strongest-return rule): the rule on top of the float64 blend
table (tests/depth_modes.py), as a RULE for depth_modes.reference -- the float64 torch forward whose depth output is
depth[strongest_id] -- and the hand-placed rays of the strongest tests.  The random scenes are tests/median_ref.py's.

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
import types

import numpy as np
import torch

import depth_modes as dm
import median_ref as mr
from depth_modes import F64, H
from median_ref import SIGMA, OFF, THIN_N, THIN_OP

UNDECIDED = mr.UNDECIDED       # 1e-3
TIE = 1e-3
STOP_BAND = 1e-2
CAP = 0.02                     # undecided pixels / pixels with a taker, at most, on every scene below (asserted on the CPU)


def blend(idx, valid, dirs, conic, opac, colors, depth, u1, u2, sph, bg, e=None):
    """depth_modes.blend_table and the strongest-return rule on it.  -> dict of [N]-leading tensors; `table`: the [N, L] tensors the
    CPU tests and the second-return rule look into."""
    t = dm.blend_table(idx, valid, dirs, conic, opac, colors, depth, u1, u2, sph, bg, e)
    I, V, N, L, taken, wgt, T_incl = t["I"], t["V"], t["N"], t["L"], t["taken"], t["wgt"], t["T_incl"]
    # the first entry that holds the largest weight
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
        near_stop = taken & ((T_incl - 1e-4).abs() <= STOP_BAND * 1e-4)
        decided = ~(near_tie | (dm.near_threshold(t, V, UNDECIDED) | near_stop).any(1))
    return dict(color=t["color"], expected=t["expected"], occ=t["occ"], strongest_id=sid, strongest_depth=sdepth, decided=decided,
                has_taker=has, top_weight=top.detach(), runner_up=runner,
                table=dict(idx=I, valid=V, hit=t["hit"], taken=taken, weight=wgt.detach(), T_after=T_incl.detach(), pos=pos))


def restate(f, scene, W, H):
    """The rule on the oracle's float32 record values.  -> numpy: strongest_id [H,W] (-1: none), strongest_depth, decided, has_taker,
    top_weight, runner_up, expected, occ [H,W], color [2,H,W]; `table`: numpy [H W, L] arrays (blend)."""
    return dm.restate_records(blend, f, scene, W, H, keep=("table",))


RULE = types.SimpleNamespace(blend=blend, restate=restate, id_key="strongest_id", chosen=lambda r, dist: (r["strongest_id"], r["strongest_depth"]))


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


# ---- the scenes of tests/test_strongest_depth_cpu.py and tests/test_strongest_depth_gpu.py ------------------------------------------
VEIL_N, VEIL_OP = 10, 0.1          # ten thin layers, 1 cm apart, in front of a wall
LATE_N, LATE_OP = 100, 0.005       # 100 layers that leave T = 0.61: the wall behind them sits in the list's second 64-entry chunk
WALL = (20.0, 0.9)
RAYS = {   # case: (x, y, [(range, opacity)]); W - 1 is written as -1
    "0.4/0.9": (8, 2, [(10.0, 0.4), (20.0, 0.9)]),              # weights 0.40, 0.54: the second
    "0.6/0.9": (24, 2, [(10.0, 0.6), (20.0, 0.9)]),             # weights 0.60, 0.36: the first
    "veil": (40, 2, [(10.0 + 0.01 * k, VEIL_OP) for k in range(VEIL_N)] + [WALL]),   # layers <= 0.10, wall 0.31 (the median: the 7th layer)
    "never": (8, 8, [(10.0, 0.2), (20.0, 0.2)]),                # weights 0.20, 0.16: the first (the median mode says the last taker)
    "thin": (24, 8, [(10.0 + 0.01 * k, THIN_OP) for k in range(THIN_N)]),             # falling weights: the first (the median: the 35th)
    "late wall": (56, 10, [(10.0 + 0.01 * k, LATE_OP) for k in range(LATE_N)] + [WALL]),   # layers <= 0.005, wall 0.54 at entry 101
    "last column": (-1, 13, [(10.0, 0.4), (20.0, 0.9)]),
    "first column": (0, 6, [(12.0, 0.4), (18.0, 0.9)]),         # (its footprint reaches over the seam into the last tile column)
}


def nominal_weights(gs):
    """The weights alpha T of a hand-placed ray [(range, opacity)] on its nominal alphas 0.995 x opacity -> list, T behind the ray."""
    T, w = 1.0, []
    for _, o in gs:
        a = o * np.exp(-0.5 * OFF * OFF)
        w.append(a * T)
        T *= 1.0 - a
    return w, T


def placed(W):
    """Hand-placed rays, laid out and sized as median_ref.placed's (SIGMA wide, OFF x SIGMA beside their pixel's centre: alpha =
    0.995 x opacity).  -> scene, {case: (x, y, range of the strongest return or 0, index of its Gaussian or -1)}, {case: indices of
    the ray's Gaussians}.  The wanted answer is worked out here by the rule's arithmetic on the nominal alphas."""
    scene, first, members = dm.placed_layout(RAYS, W, SIGMA, OFF)
    want = {}
    for case, (_, _, gs) in RAYS.items():
        w = nominal_weights(gs)[0]
        pick = max(range(len(gs)), key=lambda j: (w[j], -j))                # (strict >: the nearer entry among equal weights)
        x, y, base = first[case]
        want[case] = (x, y, gs[pick][0], base + pick)
    want["nothing"] = (40, 8, 0.0, -1)
    members["nothing"] = np.arange(0)
    return scene, want, members


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
    return mr.upstream(name, SCENES, scene)
