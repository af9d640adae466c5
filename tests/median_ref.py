"""LIDARGS_DEPTH=median restated (DESIGN.md "Median-range depth"): the rule on top of the float64 blend table (tests/depth_modes.py), as
a RULE for depth_modes.reference -- the float64 torch forward whose depth output is depth[median_id], so that torch.autograd gives the
mode's reference gradients -- and the scenes of the median tests.

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
re-evaluated in float64, vectorised over [pixels, longest list].
"""
import types

import numpy as np
import torch

import depth_modes as dm
import preprocess_ref as pr
from depth_modes import F64, H

UNDECIDED = pr.UNDECIDED       # 1e-3
T_BAND = 1e-4


def blend(idx, valid, dirs, conic, opac, colors, depth, u1, u2, sph, bg, e=None):
    """depth_modes.blend_table and the median rule on it.  -> dict of [N]-leading tensors."""
    t = dm.blend_table(idx, valid, dirs, conic, opac, colors, depth, u1, u2, sph, bg, e)
    I, N, taken, T_incl, T_excl = t["I"], t["N"], t["taken"], t["T_incl"], t["T_excl"]
    cand = taken & (T_excl > 0.5)
    has = cand.any(1)
    ar = torch.arange(t["L"])
    pos = (cand.long() * ar).max(1).values                                   # the last candidate (candidates are a prefix of the takers)
    mid = torch.where(has, I[torch.arange(N), pos], torch.full((N,), -1, dtype=torch.long))
    mdepth = torch.where(has, depth[I[torch.arange(N), pos]], torch.zeros(N, dtype=F64))
    with torch.no_grad():
        crossing = taken & (T_incl <= 0.5)
        upto = (torch.cumsum(crossing.long(), 1) - crossing.long()) == 0    # positions up to and including the first crossing
        rests = t["V"] & upto                                                # (a crossing lies in front of any T < 1e-4 stop)
        half = 0.5 * T_BAND
        near_T = taken & upto & (((T_excl - 0.5).abs() <= half) | ((T_incl - 0.5).abs() <= half))
        decided = ~(dm.near_threshold(t, rests, UNDECIDED) | near_T).any(1)
    return dict(color=t["color"], expected=t["expected"], occ=t["occ"], median_id=mid, median_depth=mdepth, decided=decided,
                has_taker=taken.any(1), crossed=(taken & (T_incl <= 0.5)).any(1), n_takers_to_median=(cand.long().sum(1)))


def restate(f, scene, W, H):
    """The rule on the oracle's float32 record values.  -> numpy: median_id [H,W] (-1: none), median_depth [H,W], decided [H,W],
    has_taker [H,W], crossed [H,W], expected [H,W], color [2,H,W], occ [H,W]."""
    return dm.restate_records(blend, f, scene, W, H)


RULE = types.SimpleNamespace(blend=blend, restate=restate, id_key="median_id", chosen=lambda r, dist: (r["median_id"], r["median_depth"]))


# ---- the scenes of tests/test_median_depth_cpu.py (the cap on undecided pixels) and tests/test_median_depth_gpu.py ------------------
CAP = 0.02          # undecided pixels / pixels with a taker, at most, on every scene below (asserted on the CPU)
# name: (kind, P, W, seed, factor on the scales): footprints of several pixels, so that many rays cross one half behind a few takers
RANDOM = {"shell256": ("shell", 400, 256, 74, 10.0), "street250": ("street", 400, 250, 79, 8.0), "shell64": ("shell", 300, 64, 77, 8.0),
          "shell250": ("shell", 400, 250, 92, 12.0)}
SIGMA = 0.02        # angular width (radians) of the hand-placed Gaussians: under one row gap (20 degrees / 15 rows = 0.023), rays 4 rows apart do not meet
OFF = 0.1           # ... which sit OFF x SIGMA beside their pixel's centre, in azimuth: power = -0.5 OFF^2 = -5e-3, outside the band of 0
THIN_N, THIN_OP = 300, 0.02
THIN_SHORT = 100    # the thin ray of the `placedshort` scenes: two 64-entry chunks, crossing at the 35th as the long one


def placed(W, thin_n=THIN_N):
    """Hand-placed rays (depth_modes.placed_layout), every Gaussian SIGMA wide and OFF x SIGMA beside the centre of its pixel, so that
    alpha = opacity x exp(-0.5 OFF^2) = 0.995 x opacity there (a little less off the equator).  -> scene, {case: (x, y, median range or
    0, index of the median Gaussian or -1)}.  Rows and columns far enough apart that no ray sees another's Gaussians."""
    rays = {   # case: (x, y, [(range, opacity)]); W - 1 is written as -1
        "0.4/0.9": (8, 2, [(10.0, 0.4), (20.0, 0.9)]),              # T = 0.60 behind the first: the second is the median (expected: 14.8)
        "0.6/0.9": (24, 2, [(10.0, 0.6), (20.0, 0.9)]),             # T = 0.40 behind the first
        "opaque": (40, 2, [(15.0, 0.99)]),
        "never": (8, 8, [(10.0, 0.2), (20.0, 0.2)]),                # T ends at 0.64: the last taker
        "thin": (24, 8, [(10.0 + 0.01 * k, THIN_OP) for k in range(thin_n)]),   # 0.98^34 > 0.5 > 0.98^35: the 35th
        "last column": (-1, 13, [(10.0, 0.4), (20.0, 0.9)]),
        "first column": (0, 6, [(12.0, 0.4), (18.0, 0.9)]),         # (its footprint reaches over the seam into the last tile column)
    }
    scene, first, _ = dm.placed_layout(rays, W, SIGMA, OFF)
    want = {}
    for case, (_, _, gs) in rays.items():
        T, med = 1.0, -1
        for j, (d, o) in enumerate(gs):
            if T > 0.5:
                med = j
            T *= 1.0 - o * np.exp(-0.5 * OFF * OFF)
        x, y, base = first[case]
        want[case] = (x, y, gs[med][0], base + med)
    want["nothing"] = (40, 8, 0.0, -1)
    return scene, want


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


def upstream(name, scenes=SCENES, scene_of=scene):
    """The upstream gradients (dL_dcolor [2,H,W], dL_ddepth [1,H,W], dL_docc [1,H,W]) the tests use for scene `name`, numbered by its
    place in `scenes` (the strongest and second tests append theirs, so a scene keeps its gradients from mode to mode: the float32
    budget of BACKWARD_SCENES is asserted for exactly these)."""
    import lidargs_scenes as sc
    return sc.upstream_grads(H, scene_of(name)[1], 300 + scenes.index(name))
