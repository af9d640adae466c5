"""LIDARGS_DEPTH=second restated (csrc/switches.h DepthMode::Second): the second-return rule on top of
tests/strongest_ref.py's blend table, as a RULE (`rule(gap)`) for depth_modes.reference -- the float64 torch forward whose depth
output is depth[second_id] -- and the hand-placed rays of the second-return tests with their worked-out answers.

The rule.  Entries are taken and count as under `strongest` (strongest_ref.blend: `taken`, weight w = alpha T).  Per pixel:
    1. s = the strongest return: the largest w, the nearer entry among equal weights (the table's `pos`);
    2. the candidates are the counting entries j != s with |depths[j] - depths[s]| >= G, in float32 on the oracle's float32 `depths`;
    3. the second return is the candidate with the largest w, the nearer one among equal weights;
    4. no candidate (no taker, one taker, every other taker inside the gap): depth 0 and no id (-1 here).
Nothing behind the first T <= best2 (best2 > 0) can win, which is where the kernel's second walk leaves a pixel; this restatement looks
at every list to its end and tests/test_second_depth_cpu.py checks that bound.

Undecided pixels give no vote in a comparison and get a zero upstream depth gradient.  A pixel is undecided if
  * strongest_ref calls it undecided (s must be decided), or
  * the runner-up candidate's weight is >= (1 - TIE) x the second's, or
  * some counting entry other than s has ||depth_j - depth_s| - G| <= EDGE metres (it falls inside or outside the gap by rounding).
"""
import types

import numpy as np
import torch

import depth_modes as dm
import median_ref as mr
import strongest_ref as sr
from depth_modes import F64, H
from median_ref import SIGMA, OFF, THIN_N, THIN_OP

TIE = sr.TIE                   # 1e-3
EDGE = 1e-3                    # metres
CAP = sr.CAP                   # undecided pixels / pixels with a taker, at most, on every scene and gap used (asserted on the CPU)
GAPS = (None, 0.505)           # LIDARGS_RETURN_GAP of the tests: unset (0) and a gap between the 1-cm layers of the hand-placed rays
PLACED_GAPS = GAPS + (2.005,)


def gap_value(gap):
    return 0.0 if gap is None else float(gap)


def pick(weight, taken, pos, d, gap):
    """Steps 2-4 of the rule on a table: weight, taken [N, L], pos [N] (the strongest return's list position), d [N, L] the entries'
    ranges -- float32 for the rule itself -- and the gap.  -> dict: pos2 [N], has [N], top2, runner2 [N], candidate [N, L], near_edge [N]."""
    N, L = weight.shape
    rows, ar = np.arange(N), np.arange(L)
    other = taken & (ar[None, :] != pos[:, None])
    away = np.abs(d - d[rows, pos][:, None])                               # (float32 - float32 where d is float32)
    cand = other & (away >= d.dtype.type(gap))
    wc = np.where(cand, weight, 0.0)
    top2 = wc.max(1)
    has = cand.any(1)
    pos2 = np.where(cand & (wc >= top2[:, None]), ar[None, :], L).min(1).clip(max=L - 1)
    rest = wc.copy()
    rest[rows, pos2] = 0.0
    near_edge = (other & (np.abs(away.astype(np.float64) - float(gap)) <= EDGE)).any(1)
    return dict(pos2=pos2, has=has, top2=top2, runner2=rest.max(1), candidate=cand, near_edge=near_edge)


def restate(f, rs, gap):
    """The rule on the oracle's float32 record values: `f` the oracle's forward, `rs` = strongest_ref.restate of it, `gap` in metres
    (None: unset).  -> numpy [H, W]: second_id (-1: none), second_depth, has_second, decided, has_taker, strongest_id; `pick`: pick()'s
    arrays; `table`: strongest_ref's."""
    t = rs["table"]
    shape = rs["strongest_id"].shape
    depths = np.asarray(f.array("depths"), np.float32)
    G = np.float32(gap_value(gap))
    p = pick(t["weight"], t["taken"], t["pos"], depths[t["idx"]], G)
    rows = np.arange(t["idx"].shape[0])
    gid = t["idx"][rows, p["pos2"]]
    sid = np.where(p["has"], gid, -1)
    sdepth = np.where(p["has"], depths[gid].astype(np.float64), 0.0)
    near_tie = p["has"] & (p["runner2"] >= (1.0 - TIE) * p["top2"])
    decided = rs["decided"].ravel() & ~near_tie & ~p["near_edge"]
    return dict(second_id=sid.reshape(shape), second_depth=sdepth.reshape(shape), has_second=p["has"].reshape(shape),
                decided=decided.reshape(shape), has_taker=rs["has_taker"], strongest_id=rs["strongest_id"], pick=p, table=t)


def chosen(r, dist, gap):
    """The float64 chain's own pick, on the weights of its table `r` (strongest_ref.blend) and its ranges `dist`."""
    t = r["table"]
    I = t["idx"]
    p = pick(t["weight"].numpy(), t["taken"].numpy(), t["pos"].numpy(), dist.detach().numpy()[I.numpy()], gap_value(gap))
    has = torch.as_tensor(p["has"])
    picked = I[torch.arange(I.shape[0]), torch.as_tensor(p["pos2"])]
    return torch.where(has, picked, torch.full_like(picked, -1)), torch.where(has, dist[picked], torch.zeros(I.shape[0], dtype=F64))


def rule(gap):
    """The RULE at `gap` metres (None: unset)."""
    return types.SimpleNamespace(blend=sr.blend, restate=lambda f, scene, W, H: restate(f, sr.restate(f, scene, W, H), gap), id_key="second_id",
                                 chosen=lambda r, dist: chosen(r, dist, gap))


def exit_positions(r):
    """The second walk's exit on the float64 table.  Per pixel with a second return: the 0-based list position of the first taken entry
    behind which T <= best2 with best2 > 0 (best2: the largest candidate weight up to and including it), or the list's last valid entry.
    -> (positions [n], largest candidate weight behind that position [n], best2 there [n], position of the second return [n])."""
    t, p = r["table"], r["pick"]
    wc = np.where(p["candidate"], t["weight"], 0.0)
    best2 = np.maximum.accumulate(wc, axis=1)
    left = t["taken"] & (best2 > 0) & (t["T_after"] <= best2)
    L = wc.shape[1]
    last = np.maximum(t["valid"].sum(1) - 1, 0)
    first = np.where(left.any(1), left.argmax(1), last)
    behind = np.where(np.arange(L)[None, :] > first[:, None], wc, 0.0).max(1)
    has = p["has"]
    return first[has], behind[has], best2[np.arange(wc.shape[0]), first][has], p["pos2"][has]


# ---- the scenes of tests/test_second_depth_cpu.py and tests/test_second_depth_gpu.py ------------------------------------------------
VEIL_N, VEIL_OP, LATE_N, LATE_OP, WALL = sr.VEIL_N, sr.VEIL_OP, sr.LATE_N, sr.LATE_OP, sr.WALL
FAR_N, FAR_OP = 80, 0.005          # 80 layers behind a 0.5 surface: the wall behind them sits in the list's second 64-entry chunk
RAYS = {   # case: (x, y, [(range, opacity)]); W - 1 is written as -1
    "0.4/0.9": (8, 2, [(10.0, 0.4), (20.0, 0.9)]),                      # weights 0.40, 0.54: s the second, the first is 10 m away
    "split surface": (24, 2, [(10.0, 0.5), (10.02, 0.6), (20.0, 0.9)]),  # weights 0.50, 0.30, 0.18: the neighbour, or past the gap the wall
    "single": (40, 2, [(15.0, 0.6)]),
    "pair inside the gap": (56, 2, [(10.0, 0.5), (10.02, 0.6)]),
    "veil": (8, 8, [(10.0 + 0.01 * k, VEIL_OP) for k in range(VEIL_N)] + [WALL]),            # s the wall (0.31); layers fall from 0.10
    "thin": (24, 8, [(10.0 + 0.01 * k, THIN_OP) for k in range(THIN_N)]),                    # falling weights: s the first layer
    "late wall": (40, 8, [(10.0 + 0.01 * k, LATE_OP) for k in range(LATE_N)] + [WALL]),      # s the wall at entry 101, in the second chunk
    "far second": (56, 8, [(10.0, 0.5)] + [(10.01 + 0.01 * k, FAR_OP) for k in range(FAR_N)] + [WALL]),   # s the first; wall 0.30 at entry 82
    "last column": (-1, 13, [(10.0, 0.4), (20.0, 0.9)]),
    "first column": (0, 6, [(12.0, 0.4), (18.0, 0.9)]),                 # (its footprint reaches over the seam into the last tile column)
}
NOTHING = (40, 13)
# The worked-out answers (range in m; 0 = no second return) at G = 0 and G = 0.505, from the nominal alphas 0.995 x opacity:
#   0.4/0.9              weights 0.40, 0.54: s = 20 m, the other is 10 m away
#   split surface        weights 0.50, 0.30, 0.18: s = 10.00 m; its neighbour at 10.02 m, or past the gap the wall
#   veil                 s = the wall (0.31); the layers' weights fall from 0.10: the first layer
#   thin                 s = layer 0; weights fall: layer 1 (10.01 m), or the first layer past the gap (10.51 m)
#   late wall            s = the wall (0.54, list position 100): layer 0
#   far second           weights 0.4975, 80 layers of at most 0.0025, the wall 0.8955 x 0.5025 x 0.995^80 = 0.30: s = 10 m, and the wall is
#                        the heaviest other entry at EITHER gap -- the rule's arithmetic, step 3.  (The layer at 10.01 m is the FIRST
#                        candidate at G = 0: the second walk carries best2 = 0.0025 past list position 64 and must not leave before the wall.)
ANSWERS = {"0.4/0.9": (10.0, 10.0), "split surface": (10.02, 20.0), "single": (0.0, 0.0), "pair inside the gap": (10.02, 0.0), "veil": (10.0, 10.0),
           "thin": (10.01, 10.51), "late wall": (10.0, 10.0), "far second": (20.0, 20.0), "first column": (12.0, 12.0), "last column": (10.0, 10.0),
           "nothing": (0.0, 0.0)}


def placed(W, gap=None):
    """Hand-placed rays, laid out and sized as strongest_ref.placed's (SIGMA wide, OFF x SIGMA beside their pixel's centre: alpha =
    0.995 x opacity).  -> scene, {case: (x, y, range of the second return or 0, index of its Gaussian or -1)} for `gap`, {case: indices
    of the ray's Gaussians}.  The wanted answer is worked out here by the rule's arithmetic on the nominal alphas and ranges."""
    G = gap_value(gap)
    scene, first, members = dm.placed_layout(RAYS, W, SIGMA, OFF)
    want = {}
    for case, (_, _, gs) in RAYS.items():
        w, T = sr.nominal_weights(gs)
        assert T >= 1e-4                                                  # (no ray reaches the blend's stop: every entry counts)
        s = max(range(len(gs)), key=lambda j: (w[j], -j))
        cand = [j for j in range(len(gs)) if j != s and abs(gs[j][0] - gs[s][0]) >= G]
        second = max(cand, key=lambda j: (w[j], -j)) if cand else -1
        x, y, base = first[case]
        want[case] = (x, y, gs[second][0] if cand else 0.0, base + second if cand else -1)
    want["nothing"] = NOTHING + (0.0, -1)
    members["nothing"] = np.arange(0)
    return scene, want, members


PLACED = ("second64", "second250", "second256")
SCENES = sr.SCENES + PLACED
BACKWARD_SCENES = mr.BACKWARD_SCENES       # their float32 budget is asserted by tests/test_median_depth_cpu.py and does not depend on the mode
BACKWARD_UNSET = "shell64"                 # the one of them that runs with the gap unset as well


def gaps(name):
    """The gaps scene `name` is run at: unset and 0.505 m; the hand-placed scenes of this file at 2.005 m as well."""
    return PLACED_GAPS if name in PLACED else GAPS


def gap_tag(gap):
    return "unset" if gap is None else f"{gap:g}"


def scene(name):
    """-> scene, W.  `second64 / 250 / 256`: placed(W); every other name: strongest_ref.scene."""
    if name in PLACED:
        W = int(name[6:])
        return placed(W)[0], W
    return sr.scene(name)


def upstream(name):
    return mr.upstream(name, SCENES, scene)
