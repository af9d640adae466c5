"""The two per-surfel stages of csrc/surfel.hip -- k_sf_preprocess<false|true> with sf_prune, and k_zero_touched<8> +
k_sf_gaussian_backward / sf_gb_row -- on their own, against the float64 restatement of tests/surfel_ref.py (itself held against the
oracle by tests/test_surfel_preprocess_cpu.py).

The library's own launchers are reached through two test hooks of the C ABI (`lidargs_debug_surfel_preprocess`,
`lidargs_debug_surfel_gaussian_backward`).  Every device array lies between two guards that must come back untouched (`Arr` of
tests/test_preprocess_gpu.py); outputs start out as 0xFF bytes (NaN as floats).

  (a) containment   every pixel that takes a surfel (the restatement's `takers`) lies inside the span the preprocess gives it -- tile
                    columns modulo the grid width, a seam span wraps -- and the pruned span inside the unpruned one: exact integers, on
                    scenes built for each branch of sf_prune; the 0.02-column margin of dcol, which guards last bits no float64 taker
                    can see, is asked of the span itself (a centre dcol - 0.01 columns from a tile boundary is binned across it)
  (b) record       copies bit for bit; Tu' / Tv' / Tw / n / lambda / Tw.n / |Tw| / p_c / p_r against float64 with the oracle's fp32 state
                    as the yardstick (4 x); radii and the unpruned span against the restatement's
  (c) block sums    the 64 slots of the totals against the per-surfel outputs of the same call
  (d) cull rules    on rows built for each     (e) filter_only     (f) lists, cleared lines, zeroed rows
  (g) chain         sf_gb_row's rows against surfel_ref.chain in float64 with its float32 run as the yardstick (4 x)
  (h) refusals
"""
import functools
import math

import numpy as np
import pytest

import lidargs_scenes as sc
import surfel_ref as ref
from test_preprocess_gpu import (CULLED, DIAG_WORD, KEYSPAN_WORD, SLOT_WORD, SLOTS, TOTALS_WORDS, Arr, _binding, _ptr, _stream, _sync, check_lists)

pytestmark = pytest.mark.gpu

ARRAYS = ("means3D", "scales", "rotations", "opacities", "colors")


# ---- the preprocess through its hook ------------------------------------------------------------------------------------------------
def run_preprocess(scene, W, H, prune=1, compact=0, th=4, near=0.0, far=80.0, mod=1.0, filter_only=0):
    """One call of lidargs_debug_surfel_preprocess -> dict of host arrays; the spans are unpacked to tx0, tx1 (tx1 > tiles_x: the span
    wraps), ty_lo, ty_hi, binned."""
    lib = _binding()._lib
    P = scene["means3D"].shape[0]
    f32 = lambda a: Arr(np.asarray(a, np.float32))
    ins = dict(means=f32(scene["means3D"]), colors=f32(scene["colors"]), op=f32(scene["opacities"]), scales=f32(scene["scales"]), rots=f32(scene["rotations"]),
               view=f32(scene["viewmatrix"]), beams=f32(scene["beams"]))
    ins["tm"] = f32(scene["transMat"]) if scene.get("transMat") is not None else None
    out = dict(rec=Arr.filled((P, 20), np.float32), rowspan=Arr.filled(P, np.uint32), spans=Arr.filled((P,) if compact else (P, 4), np.uint32),
               key=Arr.filled(P, np.uint32), touched=Arr.filled(P, np.uint8), totals=Arr.filled(TOTALS_WORDS, np.uint32, 0xFF if filter_only else 0xEE),
               radii=Arr.filled(P, np.int32), radii_xy=Arr.filled((P, 2), np.int32))
    rc = lib.lidargs_debug_surfel_preprocess(P, W, H, ins["means"].ptr, ins["colors"].ptr, ins["op"].ptr, ins["scales"].ptr, mod, ins["rots"].ptr, _ptr(ins["tm"]),
                                             ins["view"].ptr, ins["beams"].ptr, near, far, th, compact, prune, filter_only, out["rec"].ptr, out["rowspan"].ptr,
                                             out["spans"].ptr, out["key"].ptr, out["touched"].ptr, out["totals"].ptr, out["radii"].ptr, out["radii_xy"].ptr, _stream())
    assert rc == 0, _binding()._err()
    _sync()
    for a in ins.values():
        if a is not None:
            a.read()                                                        # (the guards of the inputs)
    r = {k: a.read() for k, a in out.items()}
    if filter_only:
        return r
    sp = r["spans"]
    if compact:
        none = sp == CULLED
        x0 = sp & 255; nx = ((sp >> 8) & 255) + 1; lo_ = (sp >> 16) & 255; hi_ = (sp >> 24) + 1
        r.update(binned=~none, tx0=np.where(none, 0, x0), tx1=np.where(none, 0, x0 + nx), ty_lo=np.where(none, 0, lo_), ty_hi=np.where(none, 0, hi_))
    else:
        assert not sp[:, 2:].any()
        r.update(binned=sp[:, 1] != 0, tx0=sp[:, 1] & 0xFFFF, tx1=sp[:, 1] >> 16, ty_lo=sp[:, 0] & 0xFFFF, ty_hi=sp[:, 0] >> 16)
        assert not sp[sp[:, 1] == 0].any()                                  # binned nowhere: the whole record is zero
    for k in ("tx0", "tx1", "ty_lo", "ty_hi"):
        r[k] = r[k].astype(np.int64)
    return r


def instances(r, th=4):
    """Instances of every surfel at tile height th, from its unpacked span."""
    rows = (np.maximum(r["ty_hi"], 1) - 1) // th - r["ty_lo"] // th + 1
    return np.where(r["binned"], (r["tx1"] - r["tx0"]) * rows, 0)


# ---- scenes, each built for a branch of sf_prune or of the preprocess -----------------------------------------------------------------
def _surfel(scene):
    scene["scales"] = np.ascontiguousarray(scene["scales"][:, :2])
    return scene


def _concat(a, b):
    out = {k: np.concatenate([a[k], b[k]], 0) for k in ARRAYS}
    out.update(beams=a["beams"], viewmatrix=a["viewmatrix"], bg=a["bg"])
    return out


def _rows(scene, idx):
    out = dict(scene)
    for k in ARRAYS + (("transMat",) if scene.get("transMat") is not None else ()):
        out[k] = np.ascontiguousarray(scene[k][idx])
    return out


def _quat_of(c0, c1, c2):
    """The unit quaternion (w, x, y, z) whose rotation matrix has the columns c0, c1, c2 (orthonormal, right-handed) [P,3] each."""
    R = np.stack([c0, c1, c2], 2)                                           # R[p, row, col]
    w = np.sqrt(np.maximum(1e-12, 1 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2])) / 2
    q = np.stack([w, (R[:, 2, 1] - R[:, 1, 2]) / (4 * w), (R[:, 0, 2] - R[:, 2, 0]) / (4 * w), (R[:, 1, 0] - R[:, 0, 1]) / (4 * w)], 1)
    small = w < 0.1                                                         # near a half turn: build it from the largest diagonal instead
    for i in np.nonzero(small)[0]:
        vals, vecs = np.linalg.eigh((R[i] + R[i].T) / 2)
        ax = vecs[:, -1]
        q[i] = (0.0, *ax)
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _frames(normal, rng):
    """Orthonormal right-handed frames (c0, c1, c2 = normal) with a random in-plane angle."""
    n = normal / np.linalg.norm(normal, axis=1, keepdims=True)
    a = np.where(np.abs(n[:, 2:3]) < 0.9, np.array([[0.0, 0.0, 1.0]]), np.array([[1.0, 0.0, 0.0]]))
    t0 = np.cross(a, n); t0 /= np.linalg.norm(t0, axis=1, keepdims=True)
    t1 = np.cross(n, t0)
    ph = rng.uniform(0, 2 * np.pi, n.shape[0])[:, None]
    c0 = np.cos(ph) * t0 + np.sin(ph) * t1
    return c0, np.cross(n, c0), n


def _polar(r, el, az):
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1)


def _build(P, beams, rng, pos, scales, quat, op):
    return dict(means3D=pos.astype(np.float32), scales=scales.astype(np.float32), rotations=quat.astype(np.float32),
                opacities=np.asarray(op, np.float32).reshape(P, 1), colors=rng.uniform(0, 1, (P, 2)).astype(np.float32),
                beams=np.asarray(beams, np.float32), bg=np.zeros(2, np.float32), viewmatrix=sc.rigid_viewmatrix(None))


SPECIAL_OPACITIES = 8                                                       # kinds of special rows in scene 1, eight rows of each


def scene1(P=4096, seed=11):
    """W = 256, H = 32, uniform table, street + shell mix pulled towards the sensor, random view; opacities log-uniform over [1e-3, 1] with
    rows at 1/255 exactly, one ulp either side, 0, NaN, 1, and 3 and 10 (the reach of the 2-D filter grows with tau; the C ABI does not
    bound the opacity)."""
    W, H = 256, 32
    s = _surfel(_concat(sc.make_scene("street", P // 2, H, seed, random_view=True), sc.make_scene("shell", P - P // 2, H, seed + 1, random_view=True)))
    s["means3D"] = (s["means3D"] * np.float32(0.15)).astype(np.float32)
    rng = np.random.default_rng([seed, 1])
    op = np.exp(rng.uniform(math.log(1e-3), 0.0, P)).astype(np.float32)
    t = np.float32(1.0) / np.float32(255.0)
    special = [t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)), np.float32(0), np.float32(np.nan), np.float32(1), np.float32(3), np.float32(10)]
    assert len(special) == SPECIAL_OPACITIES
    for j, v in enumerate(special * 8):                                     # eight rows of each
        op[7 + 61 * j] = v
    s["opacities"] = op.reshape(P, 1)
    return dict(scene=s, W=W, H=H, mod=1.0)


def scene2(table):
    """The geometry of tests/test_beam_tables_gpu.py _stress_scene (centres beside beams, high opacity) at P = 3000, as surfels facing the
    sensor that are tall along z: local z -> view x, local y -> view z (the quaternion of the cyclic permutation), scales about (0.03, 0.25)."""
    from test_beam_tables_gpu import _stress_scene
    s, W, H, _ = _stress_scene(table)
    s = _rows(s, np.arange(0, s["means3D"].shape[0], 4))
    s["scales"] = np.ascontiguousarray(s["scales"][:, [0, 2]])
    s["rotations"] = np.tile(np.array([[0.5, 0.5, 0.5, 0.5]], np.float32), (s["means3D"].shape[0], 1))
    return dict(scene=s, W=W, H=H, mod=1.0)


def scene3(P=3000, seed=5):
    """Thirds: normals within 4 degrees of perpendicular to the view ray (the 3-D branch degenerates, the 2-D filter takes the pixels);
    normals pointing away from the sensor (the DUAL_VISIABLE flip); planes tilted 5-15 degrees off the view ray with axes of 0.4-1 m at
    3-6 m, which pass behind part of their footprint's rays (lam2 <= 0)."""
    W, H = 256, 32
    rng = np.random.default_rng(seed)
    beams = sc.beam_inclinations(H)
    kind = np.arange(P) % 3
    r = np.where(kind == 2, rng.uniform(3.0, 6.0, P), rng.uniform(3.0, 12.0, P))
    pos = _polar(r, rng.uniform(float(beams[0]), float(beams[-1]), P), rng.uniform(-np.pi, np.pi, P))
    d = pos / np.linalg.norm(pos, axis=1, keepdims=True)
    perp = np.cross(d, rng.normal(size=(P, 3))); perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    tilt = np.where(kind == 0, rng.uniform(-4.0, 4.0, P), rng.uniform(5.0, 15.0, P) * rng.choice([-1.0, 1.0], P)) * np.pi / 180
    edge = np.cos(tilt)[:, None] * perp + np.sin(tilt)[:, None] * d
    away = d + 0.5 * rng.normal(size=(P, 3)) * 0.5
    normal = np.where((kind == 1)[:, None], away, edge)
    scales = np.where((kind == 2)[:, None], rng.uniform(0.4, 1.0, (P, 2)), 0.1 * np.exp(0.5 * rng.normal(size=(P, 2))))
    return dict(scene=_build(P, beams, rng, pos, scales, _quat_of(*_frames(normal, rng)), rng.uniform(0.3, 1.0, P)), W=W, H=H, mod=1.0, kind=kind)


def prune_k(op):
    """sf_prune's inflated cut-off k = sqrt(2 (tau + 0.02)) 1.01 + 0.02, tau = ln(255 op)."""
    return np.sqrt(2.0 * (np.log(255.0 * np.asarray(op, np.float64)) + 0.02)) * 1.01 + 0.02


def prune_columns(f, op, W):
    """sf_prune's column reach as its comment states it, in float64: (dcol, rmin / rc) with dcol = max(m / rmin / col_step, f_col) + 0.02,
    m = k hypot(a x e, b x e), rmin = rc - k hypot(a . e, b . e), e the centre's horizontal direction, f_col = max(0.373,
    sqrt(2 (tau + 0.01) / 80) 1.001) the 2-D filter's reach."""
    c, Tu, Tv = f["pv"], f["Tu"], f["Tv"]
    k = prune_k(op)
    rc = np.hypot(c[:, 0], c[:, 1])
    ex, ey = c[:, 0] / rc, c[:, 1] / rc
    par = np.hypot(Tu[:, 0] * ex + Tu[:, 1] * ey, Tv[:, 0] * ex + Tv[:, 1] * ey)
    prp = np.hypot(Tu[:, 1] * ex - Tu[:, 0] * ey, Tv[:, 1] * ex - Tv[:, 0] * ey)
    rmin = rc - k * par
    with np.errstate(all="ignore"):
        f_col = np.maximum(0.373, np.sqrt(2.0 * (np.log(255.0 * np.asarray(op, np.float64)) + 0.01) / 80.0) * 1.001)
        dcol = np.maximum(k * prp / rmin / ref.steps(W)[0], f_col) + 0.02
    return dcol, rmin / rc


def scene4(P=3000, seed=6):
    """Even rows: needles, one axis 1e-5 of the range (uu < 1e-8 d^2: no bound on s, the whole rect must be binned).  Odd rows: discs with
    axes of 0.5-1.5 m lying flat 2-4 m from the sensor, which come closer than a quarter of the centre's horizontal distance
    (rmin < 0.25 rc: the azimuth / elevation bounds degenerate, the whole rect must be binned).  `escapes`: the rows for which float64
    puts the surfel clear of the branch's threshold (a hundredth of it for the needles, rmin < 0.2 rc for the discs)."""
    W, H = 256, 32
    rng = np.random.default_rng(seed)
    beams = sc.beam_inclinations(H)
    needle = np.arange(P) % 2 == 0
    r = np.where(needle, rng.uniform(3.0, 15.0, P), rng.uniform(2.0, 4.0, P))
    pos = _polar(r, rng.uniform(float(beams[0]), float(beams[-1]), P), rng.uniform(-np.pi, np.pi, P))
    d = pos / np.linalg.norm(pos, axis=1, keepdims=True)
    normal = np.where(needle[:, None], -d + 0.3 * rng.normal(size=(P, 3)), np.array([[0.0, 0.0, 1.0]]) + 0.05 * rng.normal(size=(P, 3)))
    scales = np.where(needle[:, None], np.stack([1e-5 * r, rng.uniform(0.1, 0.3, P)], 1), rng.uniform(0.5, 1.5, (P, 2)))
    swap = needle & (rng.random(P) < 0.5)                                   # the needle's thin axis: either one
    scales[swap] = scales[swap][:, ::-1]
    op = rng.uniform(0.5, 1.0, P)
    c0, c1, c2 = _frames(normal, rng)
    s = _build(P, beams, rng, pos, scales, _quat_of(c0, c1, c2), op)
    e = pos[:, :2] / np.linalg.norm(pos[:, :2], axis=1, keepdims=True)
    rc = np.linalg.norm(pos[:, :2], axis=1)
    a_par = scales[:, 0] * (c0[:, :2] * e).sum(1); b_par = scales[:, 1] * (c1[:, :2] * e).sum(1)
    escapes = np.where(needle, True, rc - prune_k(op) * np.hypot(a_par, b_par) < 0.2 * rc)
    return dict(scene=s, W=W, H=H, mod=1.0, needle=needle, escapes=escapes)


def scene5(P=3000, seed=7):
    """A beam fan from -0.3 to 1.4 rad: half the surfels over the whole fan (zlo, zhi of either sign: rmin / rmax choose by it), half within
    0.2 rad of its top, where rc is small and the azimuth bound widens."""
    W, H = 256, 32
    rng = np.random.default_rng(seed)
    beams = np.linspace(-0.3, 1.4, H)
    el = np.where(np.arange(P) % 2 == 0, rng.uniform(-0.3, 1.4, P), rng.uniform(1.2, 1.4, P))
    pos = _polar(rng.uniform(2.0, 8.0, P), el, rng.uniform(-np.pi, np.pi, P))
    normal = -pos / np.linalg.norm(pos, axis=1, keepdims=True) + 0.6 * rng.normal(size=(P, 3))
    return dict(scene=_build(P, beams, rng, pos, 0.08 * np.exp(0.5 * rng.normal(size=(P, 2))), _quat_of(*_frames(normal, rng)), rng.uniform(0.3, 1.0, P)),
                W=W, H=H, mod=1.0)


def scene6(W):
    """tests/test_surfel_gpu.py _seam_scene at H = 32 pulled to 1-12 m: surfels on both sides of the panorama's seam.  Every seventh one
    is a disc of 0.2-0.5 m at 1.5-3 m: its +-3 sigma end point crosses the seam by more than a tile, so its reference rect -- which
    does not wrap -- stops short of the last (or starts after the first) tile column, and the two intervals of its takers can only be
    binned as their hull."""
    from test_surfel_gpu import _seam_scene
    H, P = 32, 3000
    s = _seam_scene(P, H, 21)
    rng = np.random.default_rng(22)
    s["means3D"] = (s["means3D"] * np.float32(0.3)).astype(np.float32)
    s["opacities"] = rng.uniform(0.3, 1.0, (P, 1)).astype(np.float32)
    big = np.arange(P) % 7 == 0
    r = np.linalg.norm(s["means3D"], axis=1)
    s["means3D"][big] = (s["means3D"][big] * (rng.uniform(1.5, 3.0, P)[big] / r[big])[:, None]).astype(np.float32)
    s["scales"] = np.where(big[:, None], rng.uniform(0.2, 0.5, (P, 2)), s["scales"]).astype(np.float32)
    return dict(scene=s, W=W, H=H, mod=1.0)


def scene7(W):
    """Narrow images at H = 4: where 2 dcol + 32 >= W the columns are not pruned.  That is every surfel at W = 25 and 32 (dcol >= 0.39);
    at W = 48 it takes dcol >= 8 columns, a reach of more than a radian: discs of 0.5-1.5 m at 1-2.5 m."""
    H, P = 4, 3000
    rng = np.random.default_rng(100 + W)
    beams = sc.beam_inclinations(H)
    pos = _polar(rng.uniform(1.0, 4.0 if W <= 32 else 2.5, P), rng.uniform(float(beams[0]), float(beams[-1]), P), rng.uniform(-np.pi, np.pi, P))
    normal = -pos / np.linalg.norm(pos, axis=1, keepdims=True) + 0.5 * rng.normal(size=(P, 3))
    scales = 0.3 * np.exp(0.5 * rng.normal(size=(P, 2))) if W <= 32 else rng.uniform(0.5, 1.5, (P, 2))
    return dict(scene=_build(P, beams, rng, pos, scales, _quat_of(*_frames(normal, rng)), rng.uniform(0.3, 1.0, P)), W=W, H=H, mod=1.0)


def scene8(P=4096, seed=9):
    """The first 2500 rows: small opaque surfels well inside a gap of an 8-beam table over the same fan (gaps of 0.05 rad, discs of
    ~0.003 rad): the disc's elevation interval holds no beam (b_hi == b_lo) and the 2-D filter's rows alone are binned -- at most one
    pixel each.  The first 600 of them (`edge`) lie 0.2-0.23 rows from a pixel row, on a pixel column: there the row's pixel takes the
    disc only through the last 0.04 rows of the 2-D filter's reach, which is what `f_row` has to cover.  The others lie within 0.2 of a
    row.  All keep away from the rows' half-way lines, where no pixel takes them.  The rows behind are ordinary surfels of several
    pixels, which bring the scene's takers to the number every scene must have."""
    W, H, n_small, n_edge = 256, 8, 2500, 600
    rng = np.random.default_rng(seed)
    beams = sc.beam_inclinations(H).astype(np.float64)
    small, edge = np.arange(P) < n_small, np.arange(P) < n_edge
    g = rng.integers(0, H - 1, P)
    near, far = np.where(edge, 0.2, 0.05), np.where(edge, 0.23, 0.2)        # distance to the row, in rows
    d = rng.uniform(near, far, P)
    frac = np.where(small, np.where(rng.random(P) < 0.5, d, 1.0 - d), rng.uniform(0.0, 1.0, P))
    el = beams[g] + frac * (beams[g + 1] - beams[g])                        # (small: p_r within 0.23 of a row, so that row takes it)
    r = np.where(small, rng.uniform(5.0, 20.0, P), rng.uniform(2.0, 6.0, P))
    az = np.where(edge, ref.PI_F - (rng.integers(1, W - 1, P) + rng.uniform(-0.05, 0.05, P)) * ref.steps(W)[0], rng.uniform(-np.pi, np.pi, P))
    pos = _polar(r, el, az)
    normal = -pos / np.linalg.norm(pos, axis=1, keepdims=True) + 0.3 * rng.normal(size=(P, 3))
    scales = np.where(small, r * 4e-4, 0.15)[:, None] * np.exp(0.3 * rng.normal(size=(P, 2)))
    return dict(scene=_build(P, beams, rng, pos, scales, _quat_of(*_frames(normal, rng)), rng.uniform(0.9, 1.0, P)), W=W, H=H, mod=1.0, small=small,
                edge=edge)


def scene9(H):
    """H = 1025 at W = 64: the beam table lives outside LDS; H = 1024: the same surfels on the first 1024 beams.  Footprints tens of rows
    tall, centred on the 60 highest beams (the image's first rows: a pixel row in the hundreds would put one surfel in a hundred within
    the 1e-5 relative band of a rounding boundary, per bound)."""
    P = 1500
    rng = np.random.default_rng(77)
    table = sc.beam_inclinations(1025).astype(np.float64)
    pos = _polar(rng.uniform(3.0, 15.0, P), rng.uniform(table[1025 - 60], table[1023], P), rng.uniform(-np.pi, np.pi, P))
    normal = -pos / np.linalg.norm(pos, axis=1, keepdims=True) + 0.5 * rng.normal(size=(P, 3))
    s = _build(P, table[:H], rng, pos, 0.12 * np.exp(0.5 * rng.normal(size=(P, 2))), _quat_of(*_frames(normal, rng)), rng.uniform(0.3, 1.0, P))
    return dict(scene=s, W=64, H=H, mod=1.0)


def scene10():
    """scale_modifier 6 on the first thousand rows of scene 1."""
    d = scene1()
    return dict(scene=_rows(d["scene"], np.arange(1000)), W=d["W"], H=d["H"], mod=6.0)


def scene11():
    """Scene 1 with transMat_precomp: the rows the preprocess would build (float64, rounded), axes scaled and tilted and centres moved by
    a few per cent."""
    d = scene1()
    s = dict(d["scene"])
    f = ref.forward64(s["means3D"], s["scales"], s["rotations"], s["viewmatrix"])
    tm = np.nan_to_num(np.concatenate([f["Tu"], f["Tv"], f["pv"]], 1))
    rng = np.random.default_rng(111)
    s["transMat"] = (tm * (1.0 + 0.05 * rng.normal(size=tm.shape)) + 0.01 * rng.normal(size=tm.shape)).astype(np.float32)
    return dict(scene=s, W=d["W"], H=d["H"], mod=1.0)


SCENES = {
    "1_mix_opacities": scene1, "2_stress_waymo": lambda: scene2("waymo"), "2_stress_uniform": lambda: scene2("uniform"), "3_edge_on_back_behind": scene3,
    "4_needles_large_discs": scene4, "5_fan_top_1.4": scene5, "6_seam_W256": lambda: scene6(256), "6_seam_W250": lambda: scene6(250),
    "7_narrow_W25": lambda: scene7(25), "7_narrow_W32": lambda: scene7(32), "7_narrow_W48": lambda: scene7(48), "8_rows_between_beams": scene8,
    "9_H1025": lambda: scene9(1025), "9_H1024": lambda: scene9(1024), "10_scale_modifier_6": scene10, "11_transMat_precomp": scene11,
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The scene and its float64 reference (forward fields, geometry, takers): computed once, shared, never written to."""
    d = SCENES[name]()
    s, W, H = d["scene"], d["W"], d["H"]
    f = ref.forward64(s["means3D"], s["scales"], s["rotations"], s["viewmatrix"], d["mod"], s.get("transMat"))
    geo = ref.geometry(f, s["beams"], W, H)
    tk = ref.takers(f, geo, s["opacities"], s["beams"], W, H)
    for a in list(f.values()) + list(geo.values()) + [tk["n"], tk["undecided"]] + tk["xs"] + tk["ys"] + [v for v in s.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return d, f, geo, tk


def scene_conditions(name, say=print):
    """The conditions a scene must meet on the reference alone: >= 20 000 takers, undecided <= 5 %, rounding-boundary surfels <= 1 %."""
    d, f, geo, tk = reference(name)
    n, und, nb, live = int(tk["n"].sum()), int(tk["undecided"].sum()), int(geo["near_boundary"].sum()), int(geo["live"].sum())
    say(f"[scene {name}] P {geo['live'].size} live {live} takers {n} undecided {und} ({100.0 * und / max(n + und, 1):.3f} %) near a rounding boundary {nb}")
    assert n >= 20000, f"{name}: only {n} takers"
    assert und <= 0.05 * (n + und)
    assert nb <= 0.01 * geo["live"].size
    return n, und, nb


def seam_classes(name):
    """Scene 6 on the reference alone: surfels whose takers lie on both sides of the seam with tile columns without takers between --
    where the reference rect covers every tile column the span may wrap, where it stops short of one end the span can only be the hull
    of the two intervals -- and surfels whose takers are one run of tile columns that touches the first / the last column.
    -> (wrap, hull, first, last) ids."""
    d, f, geo, tk = reference(name)
    gx = (d["W"] + 15) // 16
    wrap, hull, first, last = [], [], [], []
    for g in np.nonzero((tk["n"] > 0) & ~geo["near_boundary"])[0]:
        cols = np.unique(tk["xs"][g] // 16)
        run = cols.size == cols[-1] - cols[0] + 1
        full = geo["rect"][g, 0] == 0 and geo["rect"][g, 2] == gx
        if not run and full and cols[0] == 0 and cols[-1] == gx - 1:
            wrap.append(g)
        elif not run and not full:                                          # two groups of taker columns inside a rect that stops short of one end
            hull.append(g)
        elif run and cols[0] == 0 and cols[-1] < gx - 1:
            first.append(g)
        elif run and cols[-1] == gx - 1 and cols[0] > 0:
            last.append(g)
    return tuple(np.array(v, np.int64) for v in (wrap, hull, first, last))


# ---- (a) containment ----------------------------------------------------------------------------------------------------------------
def _check_contained(name, what, r, geo, tk, gx):
    ok = ~geo["near_boundary"]
    has = (tk["n"] > 0) & ok
    assert r["binned"][has].all(), f"{name} {what}: {(~r['binned'][has]).sum()} surfels that pixels take are binned nowhere; first: {np.nonzero(has & ~r['binned'])[0][:5]}"
    bad = []
    for g in np.nonzero(has)[0]:
        cols, ys = np.unique(tk["xs"][g] // 16), tk["ys"][g]
        inside = ((cols - r["tx0"][g]) % gx < r["tx1"][g] - r["tx0"][g]).all() and ys.min() >= r["ty_lo"][g] and ys.max() < r["ty_hi"][g]
        if not inside:
            bad.append((g, cols, ys))
    if bad:
        g, cols, ys = bad[0]
        raise AssertionError(f"{name} {what}: {len(bad)} surfels have takers outside their span; first: surfel {g}: takers in tile columns {cols.tolist()} "
                             f"rows [{ys.min()}, {ys.max()}], span tile columns [{r['tx0'][g]}, {r['tx1'][g]}) modulo {gx}, rows [{r['ty_lo'][g]}, {r['ty_hi'][g]})")


@pytest.mark.parametrize("name", list(SCENES))
def test_every_taker_lies_inside_the_pruned_span(name, hip_lib_built):
    d, f, geo, tk = reference(name)
    scene_conditions(name)
    s, W, H = d["scene"], d["W"], d["H"]
    P = s["means3D"].shape[0]
    gx = (W + 15) // 16
    can_compact = gx <= 256 and H <= 256
    runs = {(p, c): run_preprocess(s, W, H, prune=p, compact=c, mod=d["mod"]) for p in (1, 0) for c in ((0, 1) if can_compact else (0,))}
    pr, un = runs[(1, 0)], runs[(0, 0)]
    ok = ~geo["near_boundary"]
    for (p, c), r in runs.items():
        _check_contained(name, f"prune={p} compact={c}", r, geo, tk, gx)
    # compact and full spans unpack to the same integers
    for p in (1, 0):
        if can_compact:
            a, b = runs[(p, 0)], runs[(p, 1)]
            assert np.array_equal(a["binned"], b["binned"])
            for k in ("tx0", "tx1", "ty_lo", "ty_hi", "key", "radii", "radii_xy", "rowspan", "touched", "totals"):
                assert np.array_equal(a[k], b[k]), (p, k)
    # the pruned span inside the unpruned one, as sets of tile columns and rows; the other outputs independent of the flag
    assert not (pr["binned"] & ~un["binned"]).any()
    b = pr["binned"]
    wraps = b & (pr["tx1"] > gx)
    plain = b & ~wraps
    assert (un["tx1"][b] <= gx).all()                                       # (the reference rect never wraps)
    assert (pr["tx0"][plain] >= un["tx0"][plain]).all() and (pr["tx1"][plain] <= un["tx1"][plain]).all()
    assert (un["tx0"][wraps] == 0).all() and (un["tx1"][wraps] == gx).all() and (pr["tx1"][wraps] - pr["tx0"][wraps] <= gx).all() and (pr["tx0"][wraps] < gx).all()
    assert (pr["ty_lo"][b] >= un["ty_lo"][b]).all() and (pr["ty_hi"][b] <= un["ty_hi"][b]).all()
    for k in ("radii", "radii_xy"):
        assert np.array_equal(pr[k], un[k]), k
    assert np.array_equal(pr["rowspan"][b], un["rowspan"][b])
    # the unpruned span is the restatement's rect (every live surfel: without pruning the opacity is not looked at)
    live = geo["live"] & ok
    assert un["binned"][live].all() and not un["binned"][~geo["live"] & ok].any()
    assert np.array_equal(np.stack([un["tx0"], un["ty_lo"], un["tx1"], un["ty_hi"]], 1)[live], geo["rect"][live])
    # below 1/255 a pruned surfel is binned nowhere
    op = s["opacities"][:, 0].astype(np.float32)
    faint = op * np.float32(255.0) < np.float32(1.0)
    if s.get("transMat") is None:
        assert not pr["binned"][faint].any() and (pr["key"][faint] == CULLED).all()
    else:                                                                   # the blend's rows are not the rect's: nothing is pruned
        for k in ("spans", "key", "rec", "rowspan", "totals", "radii", "radii_xy", "touched"):
            assert np.array_equal(pr[k].view(np.uint32) if pr[k].dtype == np.float32 else pr[k], un[k].view(np.uint32) if un[k].dtype == np.float32 else un[k]), k
    ip, iu = int(instances(pr).sum()), int(instances(un).sum())
    print(f"[scene {name}] instances at tile height 4: {ip} pruned, {iu} unpruned ({100.0 * ip / max(iu, 1):.1f} %)")
    if name == "1_mix_opacities":
        assert ip < 0.8 * iu
        assert sum(int(np.isclose(op, v).sum()) for v in (3.0, 10.0)) == 16 and int(np.isnan(op).sum()) == 8
    if name.startswith("4_"):
        e = d["escapes"] & geo["live"] & ~faint
        print(f"[scene {name}] needles {int((e & d['needle']).sum())}, large discs clear of rmin >= 0.25 rc: {int((e & ~d['needle']).sum())}")
        assert (e & d["needle"]).sum() > 1000 and (e & ~d["needle"]).sum() > 300
        for k in ("tx0", "tx1", "ty_lo", "ty_hi"):
            assert np.array_equal(pr[k][e], un[k][e]), k
        assert pr["binned"][e].all()
    if name.startswith("6_"):
        w, h, first, last = seam_classes(name)
        print(f"[scene {name}] takers at both ends of the image: {w.size} surfels whose rect covers every tile column, {int((pr['tx1'][w] > gx).sum())} of them "
              f"with a wrapped span; {h.size} whose rect does not (hull); one run at the first columns {first.size}, at the last {last.size}")
        assert w.size > 0 and h.size > 0 and first.size > 0 and last.size > 0
        assert (pr["tx1"][w] > gx).sum() > 0.5 * w.size                     # the wrapped span occurs
        assert (pr["tx1"][h] <= gx).all()                                   # the hull: one plain span over both groups (containment above)
        strict = lambda idx: ((pr["tx1"][idx] - pr["tx0"][idx]) < (un["tx1"][idx] - un["tx0"][idx])).sum()
        assert strict(w) > 0 and strict(first) > 0 and strict(last) > 0     # (the three-interval logic prunes, it does not only pass the rect on)
    if name.startswith("7_"):                                               # 2 dcol + 32 >= W: columns are not pruned
        dcol, rmin_rc = prune_columns(f, np.nan_to_num(op.astype(np.float64), nan=1.0), W)
        wide = b & ((2.0 * dcol + 32.0 >= W + 0.1) | (rmin_rc < 0.2))       # (clear of the threshold in float64, or clear of rmin >= 0.25 rc: no pruning at all)
        print(f"[scene {name}] binned surfels with 2 dcol + 32 >= W: {int(wide.sum())} of {int(b.sum())}")
        assert wide.sum() > 1000 and (W > 32 or wide.sum() == b.sum())
        assert np.array_equal(pr["tx0"][wide], un["tx0"][wide]) and np.array_equal(pr["tx1"][wide], un["tx1"][wide])
    if name.startswith("8_"):
        dy = np.abs(geo["p_r"] - np.round(geo["p_r"]))
        decided_by_f_row = d["edge"] & (tk["n"] > 0) & (dy > 0.2)           # the taker's row is binned only if f_row reaches beyond 0.2
        print(f"[scene {name}] discs whose only taker lies 0.2-0.23 rows from the centre: {int(decided_by_f_row.sum())}")
        assert decided_by_f_row.sum() > 300
        sm = b & d["small"]
        assert sm.sum() > 1500 and (pr["ty_hi"][sm] - pr["ty_lo"][sm] == 1).all()      # the 2-D filter's row alone
    if name.startswith("9_"):
        assert geo["ry"].max() >= 64                                        # footprints taller than any tile


def _boundary_scene(delta_of, W, H):
    """Four kinds of surfel facing the sensor at 10 m, one of each `delta` columns right of every inner tile boundary, on a beam:
    discs of 0.02 columns (sigma) at opacity 1, 3 and 10 (the 2-D filter's reach f_col decides) and discs of 1.5 columns (sigma) at
    opacity 0.02 (the disc's azimuth hull decides).  delta_of(dcol) is the offset, dcol the reach of the kind by prune_columns."""
    gx = (W + 15) // 16
    col_step = ref.steps(W)[0]
    kinds = [(1.0, 0.02), (3.0, 0.02), (10.0, 0.02), (0.02, 1.5)]           # (sigma 0.02 columns = 5 mm: above the 1e-4 d of the needle escape)
    op = np.repeat([k[0] for k in kinds], gx - 1); sig = np.repeat([k[1] for k in kinds], gx - 1) * 10.0 * col_step
    tile = np.tile(np.arange(1, gx), len(kinds))
    P = op.size
    rng = np.random.default_rng(4)

    def build(p_c):
        beams = sc.beam_inclinations(H)                                     # on a beam: the row takes the small discs (between two beams no pixel does)
        pos = _polar(np.full(P, 10.0), np.full(P, float(beams[H // 2])), ref.PI_F - p_c * col_step)
        return _build(P, beams, rng, pos, np.stack([sig, sig], 1), _quat_of(*_frames(-pos, rng)), op)

    s = build(16.0 * tile + 0.5)
    dcol, rmin_rc = prune_columns(ref.forward64(s["means3D"], s["scales"], s["rotations"], s["viewmatrix"]), op, W)
    assert (rmin_rc > 0.5).all() and (dcol[op >= 1] < 0.5).all() and (dcol[op < 1] > 2.0).all() and (2 * dcol + 32 < W).all()
    return build(16.0 * tile + delta_of(dcol)), tile, dcol


def test_the_column_reach_keeps_its_stated_margin(hip_lib_built):
    """sf_prune's comment states the columns in reach as |x - p_c| <= dcol = max(m / rmin / col_step, f_col) + 0.02, the 0.02 columns being
    the margin for what the bound is computed with (float atan2f, the centre's own pixel coordinates).  No float64 taker can tell whether
    that margin is there -- it guards last bits -- so the span itself is asked: a centre dcol - 0.01 columns right of a tile boundary
    (float64; the fp32 position moves it by < 1e-3) must still be binned in the tile on the left, and one dcol + 0.5 right of it is not
    (the pruning is at work on these rows).
    prune_columns restates sf_prune's own constants (0.373, 1.01, 0.02): this test pins the margin the kernel states, not a taker, and
    has to be updated together with those constants when the margin is retuned."""
    W, H = 256, 32
    for delta_of, inside in ((lambda dcol: dcol - 0.01, True), (lambda dcol: dcol + 0.5, False)):
        s, tile, dcol = _boundary_scene(delta_of, W, H)
        f = ref.forward64(s["means3D"], s["scales"], s["rotations"], s["viewmatrix"])
        geo = ref.geometry(f, s["beams"], W, H)
        assert np.abs(geo["p_c"] - (16.0 * tile + delta_of(dcol))).max() < 1e-3
        assert geo["live"].all() and (geo["rect"][:, 0] <= tile - 1).all() and (geo["rect"][:, 2] >= tile + 1).all()      # the rect holds both tiles
        r = run_preprocess(s, W, H, prune=1)
        assert r["binned"].all()
        if inside:
            bad = np.nonzero(r["tx0"] > tile - 1)[0]
            assert bad.size == 0, (f"{bad.size} surfels whose centre lies dcol - 0.01 columns from a tile boundary are not binned in the tile across it; first: "
                                   f"surfel {bad[0]}: p_c {geo['p_c'][bad[0]]!r}, opacity {s['opacities'][bad[0], 0]}, dcol {dcol[bad[0]]!r}, span tile columns "
                                   f"[{r['tx0'][bad[0]]}, {r['tx1'][bad[0]]})")
        else:
            assert np.array_equal(r["tx0"], tile)


# ---- (b) record ---------------------------------------------------------------------------------------------------------------------
def _oracle_state(d):
    from oracle import lgo_surfel
    s = d["scene"]
    P = s["means3D"].shape[0]
    fo = lgo_surfel.forward(s["means3D"], s["colors"], s["opacities"], s["scales"], s["rotations"], s["viewmatrix"], s["beams"], d["W"], d["H"],
                            scale_modifier=d["mod"], transMat_precomp=s.get("transMat"))
    f32 = np.float32
    tm = fo.array("transMat").reshape(P, 9)
    if s.get("transMat") is not None:
        tm = np.asarray(s["transMat"], f32).reshape(P, 9)                   # (what the blend reads, R2/cr/rasterizer_impl.cu:332)
    Tu, Tv, Tw = tm[:, 0:3], tm[:, 3:6], tm[:, 6:9]
    n = fo.array("normal_opacity").reshape(P, 4)[:, :3]
    with np.errstate(all="ignore"):
        blen = np.sqrt((Tw * Tw).sum(1, dtype=f32)).astype(f32)
        wn = (Tw * n).sum(1, dtype=f32).astype(f32)
        out = dict(vis=fo.radii > 0, radii=fo.radii, Tup=Tu / (Tu * Tu).sum(1, keepdims=True, dtype=f32), Tvp=Tv / (Tv * Tv).sum(1, keepdims=True, dtype=f32),
                   Bw=Tw, n=n, lam=(blen * (wn / blen)).reshape(P, 1), wn=wn.reshape(P, 1), blen=blen.reshape(P, 1),
                   pix=fo.array("means2D").reshape(P, 2), radii_xy=fo.array("radii_xy").reshape(P, 2), tiles_touched=fo.array("tiles_touched"))
    return out


def _record_fields(rec):
    return dict(Tup=rec[:, [0, 2, 4]], Tvp=rec[:, [1, 3, 5]], Bw=rec[:, 8:11], n=rec[:, 12:15], lam=rec[:, 15:16], wn=rec[:, 19:20], blen=rec[:, 18:19],
                pix=rec[:, 16:18])


@pytest.mark.parametrize("name", ["1_mix_opacities", "2_stress_waymo", "2_stress_uniform", "3_edge_on_back_behind", "10_scale_modifier_6", "11_transMat_precomp"])
def test_record_against_float64_with_the_oracle_as_yardstick(name, hip_lib_built):
    d, f, geo, tk = reference(name)
    s, W, H = d["scene"], d["W"], d["H"]
    P = s["means3D"].shape[0]
    r = run_preprocess(s, W, H, mod=d["mod"])
    o = _oracle_state(d)
    b = r["binned"]
    rec = r["rec"]
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    # copies, bit for bit
    assert np.array_equal(u(rec[b, 6]), u(s["opacities"][b, 0])) and np.array_equal(u(rec[b, 7]), u(s["colors"][b, 0])) and np.array_equal(u(rec[b, 11]), u(s["colors"][b, 1]))
    # the key: the range |p_view| (with transMat_precomp the record's r4.z is |Tw| of the given rows; the sort depth still comes from means3D)
    if s.get("transMat") is None:
        assert np.array_equal(r["key"], np.where(b, u(rec[:, 18]), CULLED))
    else:
        assert (r["key"][~b] == CULLED).all()
        np.testing.assert_allclose(r["key"][b].view(np.float32), f["dist"][b], rtol=1e-6)
        assert np.array_equal(u(rec[b][:, [8, 9, 10]]), u(s["transMat"].reshape(P, 9)[b, 6:9]))       # Tw: the given row, copied
    ok = ~geo["near_boundary"]
    m = b & ok
    assert np.array_equal(r["rowspan"][m] & 0xFFFF, geo["rect"][m, 1]) and np.array_equal(r["rowspan"][m] >> 16, geo["rect"][m, 3])
    assert (u(rec[~b]) == CULLED).all() and (r["rowspan"][~b] == CULLED).all()          # records of the unbinned: never written
    assert not r["touched"].any()
    assert np.array_equal(r["radii"], r["radii_xy"].max(1))
    # radii: the restatement's, outside its own rounding boundaries
    print(f"[record {name}] surfels near a rounding boundary, left out: {int((~ok).sum())} of {P}")
    assert (~ok).sum() <= 0.01 * P
    assert np.array_equal(r["radii"][ok] > 0, geo["live"][ok])
    assert np.array_equal(r["radii_xy"][ok, 0], geo["rx"][ok]) and np.array_equal(r["radii_xy"][ok, 1], geo["ry"][ok])
    # values: HIP's error against float64 over the oracle's, per field group
    v = b & o["vis"]
    assert v.sum() > 0.9 * b.sum() and v.sum() > 300
    mine = _record_fields(rec)
    want = dict(Tup=f["Tup"], Tvp=f["Tvp"], Bw=f["Bw"], n=f["n"], lam=f["lam"], wn=f["wn"], blen=f["blen"], pix=np.stack([geo["p_c"], geo["p_r"]], 1))
    ids = np.nonzero(v)[0]
    for k in ("Tup", "Tvp", "Bw", "n", "lam", "wn", "blen", "pix"):
        p99h, p99y, mxh, mxy, where = ref.ratios(f"{name[:11]} {k}", mine[k][v], o[k][v], want[k].reshape(P, -1)[v])
        assert p99h <= 4.0 * p99y and mxh <= 4.0 * mxy, f"{k}: {where} (rows are positions among the binned surfels: row i is surfel ids[i], e.g. row 0 = {ids[0]})"


# ---- (c) block sums -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", [4, 16])
def test_block_sums_against_the_outputs_of_the_same_call(th, hip_lib_built):
    P, W, H = 16700, 512, 16                                                # 66 blocks of 256: the 64 slots wrap
    s = _surfel(sc.make_scene("shell", P, H, 300 + th, random_view=True))
    s["means3D"] = (s["means3D"] * np.float32(0.3)).astype(np.float32)
    sums = {}
    for prune in (1, 0):
        r = run_preprocess(s, W, H, prune=prune, th=th)
        t = r["totals"]
        what = f"th={th} prune={prune}"
        inst = t[SLOT_WORD:SLOT_WORD + 8 * SLOTS].view(np.uint64).reshape(SLOTS, 4)
        assert int(inst[:, 0].sum()) == int(instances(r, th).sum()) > 0, what
        assert (inst[:, 0] > 0).all(), what                                 # every slot took part
        diag = t[DIAG_WORD:DIAG_WORD + 4 * SLOTS].view(np.uint64).reshape(SLOTS, 2).sum(0)
        assert int(diag[0]) == int((r["radii"] > 0).sum()) > 0.3 * P, what
        ks = t[KEYSPAN_WORD:KEYSPAN_WORD + 2 * SLOTS].reshape(SLOTS, 2)
        keys = r["key"][r["key"] != CULLED]
        assert int(~ks[:, 0].max() & 0xFFFFFFFF) == int(keys.min()) and int(ks[:, 1].max()) == int(keys.max()), what
        # every other word of the totals is zero
        assert not t[:SLOT_WORD].any() and not inst[:, 1:].any() and not t[SLOT_WORD + 8 * SLOTS:KEYSPAN_WORD].any(), what
        assert not t[KEYSPAN_WORD + 2 * SLOTS:DIAG_WORD].any() and not t[DIAG_WORD + 4 * SLOTS:].any(), what
        sums[prune] = int(diag[1])
        if prune == 0:                                                      # the reference's tiles_touched: the whole rect, which is the unpruned span
            assert np.array_equal(r["binned"], r["radii"] > 0)
            assert sums[0] == int(np.where(r["binned"], (r["tx1"] - r["tx0"]) * (r["ty_hi"] - r["ty_lo"]), 0).sum())
    assert sums[1] == sums[0]                                               # the reference's rect does not know about the pruning


# ---- (d) cull rules, (e) filter_only --------------------------------------------------------------------------------------------------
def _at(r, el, az=0.3):
    return [r * math.cos(el) * math.cos(az), r * math.cos(el) * math.sin(az), r * math.sin(el)]


def test_cull_rules_on_rows_built_for_each(hip_lib_built):
    H, W = 16, 256
    beams = sc.beam_inclinations(H)
    b0, b1, g = float(beams[0]), float(beams[-1]), ref.GUARD
    f32 = np.float32
    rows = []                                                               # (position, quaternion, scales, live in the preprocess, live in the filter, what)
    q_face = [0.5, 0.5, 0.5, 0.5]                                           # local z -> view x: the normal looks along the x axis
    add = lambda pos, live, what, q=q_face, sc2=(0.05, 0.05), flive=None: rows.append((pos, q, sc2, live, live if flive is None else flive, what))
    add([80.0, 0.0, 0.0], False, "range == far")
    add([float(np.nextafter(f32(80), f32(0))), 0.0, 0.0], True, "range one ulp under far")
    add([2.0, 0.0, 0.0], False, "range == near")
    add([float(np.nextafter(f32(2), f32(3))), 0.0, 0.0], True, "range one ulp over near")
    add(_at(20.0, b1 + 0.8 * g), True, "above the last beam, inside the guard")
    add(_at(20.0, b1 + 1.2 * g), False, "above the last beam, beyond the guard")
    add(_at(20.0, b0 - 0.8 * g), True, "below the first beam, inside the guard")
    add(_at(20.0, b0 - 1.2 * g), False, "below the first beam, beyond the guard")
    add([10.0, 0.0, 0.0], False, "Tw . n == 0 exactly (normal along z, centre on the x axis)", q=[1.0, 0.0, 0.0, 0.0], flive=True)
    add([float("nan"), 0.0, 0.0], False, "NaN position")
    add([float("inf"), 0.0, 0.0], False, "infinite position")
    add([10.0, 1.0, 0.0], True, "zero quaternion (every axis NaN: the extent is the one-pixel minimum)", q=[0.0, 0.0, 0.0, 0.0])
    add([10.0, -1.0, 0.0], True, "zero scale (the extent is the one-pixel minimum)", sc2=(0.0, 0.0))
    P = len(rows)
    rng = np.random.default_rng(3)
    s = _build(P, beams, rng, np.array([r[0] for r in rows], np.float64), np.array([r[2] for r in rows]), np.array([r[1] for r in rows]), np.full(P, 0.9))
    want, fwant = np.array([r[3] for r in rows]), np.array([r[4] for r in rows])
    full = run_preprocess(s, W, H, near=2.0, far=80.0)
    filt = run_preprocess(s, W, H, near=2.0, far=80.0, filter_only=1)
    for i in range(P):
        assert (full["radii"][i] > 0) == want[i], rows[i][5]
        assert (filt["radii"][i] > 0) == fwant[i], "filter_only: " + rows[i][5]
    for r, w in ((full, want), (filt, fwant)):
        assert not r["radii_xy"][~w].any() and not r["radii"][~w].any()
        assert (r["radii_xy"][w] >= 1).all() and (r["radii_xy"][w] <= W).all() and np.array_equal(r["radii"], r["radii_xy"].max(1))
    dead = ~want
    assert (full["key"][dead] == CULLED).all() and not full["spans"][dead].any() and not full["touched"].any()
    assert full["binned"][want].all() and (full["key"][want] != CULLED).all()
    assert (full["tx1"][want] > full["tx0"][want]).all() and (full["ty_hi"][want] > full["ty_lo"][want]).all() and (full["ty_hi"] <= H).all()
    both = want & fwant
    assert np.array_equal(full["radii_xy"][both], filt["radii_xy"][both])
    # the oracle agrees on every row (its K1 and K2)
    from oracle import lgo_surfel
    fo = lgo_surfel.forward(s["means3D"], s["colors"], s["opacities"], s["scales"], s["rotations"], s["viewmatrix"], s["beams"], W, H, far=80, near=2)
    assert np.array_equal(fo.radii, full["radii"])
    assert np.array_equal(lgo_surfel.visible_filter(s["means3D"], s["scales"], s["rotations"], s["viewmatrix"], s["beams"], W, H, far=80, near=2), filt["radii"])


def test_filter_only_writes_the_radii_alone(hip_lib_built):
    d, f, geo, tk = reference("1_mix_opacities")
    s, W, H = d["scene"], d["W"], d["H"]
    full = run_preprocess(s, W, H)
    filt = run_preprocess(s, W, H, filter_only=1)
    edge_on = f["c"] == 0.0
    assert np.array_equal(filt["radii"][~edge_on], full["radii"][~edge_on]) and np.array_equal(filt["radii_xy"][~edge_on], full["radii_xy"][~edge_on])
    assert (full["radii"] > 0).sum() > 1000
    for k in ("rec", "rowspan", "spans", "key", "touched", "totals"):       # every other array: still 0xFF (the guards were checked by read())
        assert (filt[k].view(np.uint8) == 0xFF).all(), k


# ---- (f) touched lists and zeroing --------------------------------------------------------------------------------------------------
ROWS = (("dL_dmean2D", 4), ("dL_dnormal", 3), ("dL_dopacity", 1), ("dL_dcolor", 2), ("dL_dmean3D", 3), ("dL_dtransMat", 9), ("dL_dtransMat_2dtemp", 3),
        ("dL_dscale", 2), ("dL_drot", 4))                                   # in the hook's argument order; depth [P,1] follows
OPTIONAL = ("dL_dnormal", "dL_dtransMat", "dL_dtransMat_2dtemp")
SENTINEL = np.float32(7.25)


class Backward:
    """The arrays of one lidargs_debug_surfel_gaussian_backward call sequence on P surfels."""

    def __init__(self, P, W=256, H=32, scene=None, radii=None, skip=()):
        self.P, self.W, self.H = P, W, H
        self.touched = Arr(np.zeros(P, np.uint8))
        self.gacc = Arr(np.full((P, 32), SENTINEL, np.float32))
        self.rows = {k: (None if k in skip else Arr.filled((P, w), np.float32)) for k, w in ROWS}
        self.depth = Arr.filled((P, 1), np.float32)
        self.tlist = Arr.filled(P + 256, np.uint8, 0xEE)
        self.tcount = Arr.filled(P // 256 + 64, np.uint16, 0xEE)
        f32 = lambda a: Arr(np.asarray(a, np.float32))
        self.ins = {}
        if scene is not None:
            self.ins = dict(means=f32(scene["means3D"]), scales=f32(scene["scales"]), rots=f32(scene["rotations"]), view=f32(scene["viewmatrix"]),
                            beams=f32(scene["beams"]), radii=Arr(np.asarray(radii, np.int32)))
            if scene.get("transMat") is not None:
                self.ins["tm"] = f32(scene["transMat"])

    def call(self, stage):
        lib = _binding()._lib
        i = self.ins
        rc = lib.lidargs_debug_surfel_gaussian_backward(self.P, self.W, self.H, stage, self.touched.ptr, self.gacc.ptr, _ptr(i.get("means")), _ptr(i.get("scales")),
                                                        _ptr(i.get("rots")), _ptr(i.get("tm")), _ptr(i.get("view")), _ptr(i.get("beams")), _ptr(i.get("radii")),
                                                        *[_ptr(self.rows[k]) for k, _ in ROWS], self.depth.ptr, self.tlist.ptr, self.tcount.ptr, _stream())
        _sync()
        return rc

    def read_rows(self):
        for a in self.ins.values():
            a.read()
        return {k: a.read() for k, a in self.rows.items() if a is not None}


@pytest.mark.parametrize("P", [1, 255, 256, 257, 5000])
def test_touched_lists_cleared_lines_and_zeroed_rows(P, hip_lib_built):
    rng = np.random.default_rng(P)
    for density, skip in ((0.0, ()), (0.4, ()), (1.0, ()), (0.05, OPTIONAL)):
        what = f"P={P} density={density}"
        marks = np.where(rng.random(P) < density, rng.choice(np.array([1, 255], np.uint8), P), 0).astype(np.uint8)
        b = Backward(P, skip=skip)
        b.touched.write(marks)
        assert b.call(1) == 0, (what, _binding()._err())
        check_lists(b, marks, what)
        assert np.array_equal(b.touched.read(), marks), what
        acc = b.gacc.read().view(np.uint32)
        m = marks != 0
        assert not acc[m].any(), what                                       # marked lines: +0 in all 32 words
        assert (acc[~m] == SENTINEL.view(np.uint32)).all(), what            # the others: untouched
        for k, a in b.read_rows().items():
            assert not a.view(np.uint32).any(), (what, k)                   # every row of every supplied array: +0
        assert (b.depth.read().view(np.uint32) == CULLED).all(), what       # (the first launch does not write the depth)


# ---- (g) chain ----------------------------------------------------------------------------------------------------------------------
COPIED = ("dL_dnormal", "dL_dopacity", "dL_dcolor", "dL_dtransMat_2dtemp")
CHAINED = ("dL_dmean2D", "dL_dtransMat", "dL_dmean3D", "dL_dscale", "dL_drot", "depth")


def chain_lines(P, touched, seed):
    """Packed lines as a blend leaves them: touched surfels carry random cotangents in the 23 live slots (magnitudes over a few decades,
    mixed signs, the two abs-sums >= 0) and NaN in the nine dead ones; untouched surfels' lines are all NaN."""
    rng = np.random.default_rng(seed)
    line = np.full((P, 32), np.nan, np.float32)
    vals = (rng.normal(size=(P, len(ref.LIVE))) * np.exp(rng.uniform(math.log(1e-3), math.log(10.0), (P, len(ref.LIVE))))).astype(np.float32)
    live_line = np.full((P, 32), np.nan, np.float32)
    live_line[:, list(ref.LIVE)] = vals
    for k in ("M2AX", "M2AY", "AW"):                                        # sums of absolute values
        live_line[:, list(ref.SLOT[k])] = np.abs(live_line[:, list(ref.SLOT[k])])
    line[touched] = live_line[touched]
    assert np.isnan(line[:, list(ref.DEAD)]).all()
    return line


def run_chain(d, geo, line, touched, skip=()):
    s = d["scene"]
    radii = np.where(geo["live"], np.maximum(geo["rx"], geo["ry"]), 0)
    b = Backward(line.shape[0], d["W"], d["H"], s, radii, skip)
    b.touched.write(touched.astype(np.uint8))
    assert b.call(1) == 0, _binding()._err()
    b.gacc.write(line)
    assert b.call(2) == 0, _binding()._err()
    b.gacc.read(); b.tlist.read(); b.tcount.read()
    out = b.read_rows()
    out["depth"] = b.depth.read()
    return out, radii


@pytest.mark.parametrize("name", ["1_mix_opacities", "3_edge_on_back_behind", "6_seam_W256", "6_seam_W250", "11_transMat_precomp"])
def test_chain_against_the_float64_restatement(name, hip_lib_built):
    import torch
    d, f, geo, tk = reference(name)
    s, W, H = d["scene"], d["W"], d["H"]
    P = s["means3D"].shape[0]
    rng = np.random.default_rng(P)
    touched = geo["live"] & (rng.random(P) < 0.6)
    assert touched.sum() > 500
    line = chain_lines(P, touched, 8)
    got, radii = run_chain(d, geo, line, touched)
    t = np.nonzero(touched)[0]
    args = (np.nan_to_num(line[t]), s["means3D"][t], s["scales"][t], s["rotations"][t], s["viewmatrix"], s["beams"], W, H, radii[t],
            None if s.get("transMat") is None else s["transMat"][t])
    want = ref.chain(*args)
    yard = ref.chain(*args, dtype=torch.float32)
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for k, a in got.items():                                                # dead slots are not read: no NaN anywhere
        assert np.isfinite(a).all(), f"{k}: NaN or infinity in rows {np.nonzero(~np.isfinite(a).all(1))[0][:5]}"
        if k != "depth":                                                    # untouched rows: exact zeros
            assert not a[~touched].view(np.uint32).any(), k
    for k in COPIED:
        assert np.array_equal(u(got[k][t]), u(want[k])), k
    assert np.array_equal(u(got["dL_dtransMat"][t][:, :6]), u(want["dL_dtransMat"][:, :6]))
    for k in CHAINED:
        p99h, p99y, mxh, mxy, where = ref.ratios(f"{name[:11]} {k[3:] if k != 'depth' else k}", got[k][t], yard[k], want[k])
        assert p99h <= 4.0 * p99y and mxh <= 4.0 * mxy, f"{k}: {where} (row i is surfel t[i], e.g. row 0 = surfel {t[0]})"
    # the depth of every surfel, touched or not: the planar range for radii > 0, else 0
    pv = f["pv"]
    dep = np.where(radii > 0, np.sqrt(pv[:, 0] ** 2 + pv[:, 2] ** 2), 0.0)
    np.testing.assert_allclose(got["depth"][:, 0], np.nan_to_num(dep), rtol=2e-6)
    assert not got["depth"][radii == 0].view(np.uint32).any()
    if s.get("transMat") is not None:                                       # the reconstructed terms use the given Tw, the chain p_view
        plain = dict(d); plain["scene"] = {k: v for k, v in s.items() if k != "transMat"}
        other, _ = run_chain(plain, geo, line, touched)
        assert np.array_equal(u(other["dL_dscale"]), u(got["dL_dscale"])) and np.array_equal(u(other["depth"]), u(got["depth"]))
        assert np.abs(other["dL_dmean2D"][t] - got["dL_dmean2D"][t]).max() > 0 and np.abs(other["dL_dmean3D"][t] - got["dL_dmean3D"][t]).max() > 0
    if name == "1_mix_opacities":                                           # NULL optional outputs are skipped, the others do not move
        part, _ = run_chain(d, geo, line, touched, skip=OPTIONAL)
        assert set(part) == set(got) - set(OPTIONAL)
        for k, a in part.items():
            assert np.array_equal(u(a), u(got[k])), k


def test_both_launches_in_one_call_chain_the_cleared_lines(hip_lib_built):
    """stage 0: the first launch clears the marked lines and the chain then reads those zeros -- a backward whose blend added nothing."""
    d, f, geo, tk = reference("1_mix_opacities")
    s = d["scene"]
    P = s["means3D"].shape[0]
    radii = np.where(geo["live"], np.maximum(geo["rx"], geo["ry"]), 0)
    marks = (geo["live"] & (np.arange(P) % 3 == 0)).astype(np.uint8)
    b = Backward(P, d["W"], d["H"], s, radii)
    b.touched.write(marks)
    assert b.call(0) == 0, _binding()._err()
    check_lists(b, marks, "stage 0")
    acc = b.gacc.read().view(np.uint32)
    m = marks != 0
    assert not acc[m].any() and (acc[~m] == SENTINEL.view(np.uint32)).all()
    for k, a in b.read_rows().items():
        assert (a == 0).all(), k                                            # (a chained row may hold -0: 0 times a negative factor)
        if k in COPIED:
            assert not a.view(np.uint32).any(), k
    dep = b.depth.read()[:, 0]
    assert (dep[radii > 0] > 0).all() and not dep[radii == 0].view(np.uint32).any()


# ---- (h) refusals -------------------------------------------------------------------------------------------------------------------
def test_hooks_refuse_what_they_cannot_launch(hip_lib_built):
    lib = _binding()._lib
    b = Arr.filled(4096, np.uint32)
    p = b.ptr

    def pre(P=8, W=64, H=8, th=4, compact=0, filter_only=0, **null):
        a = dict(means=p, colors=p, op=p, scales=p, rots=p, tm=None, view=p, beams=p, rec=p, rowspan=p, spans=p, key=p, touched=p, totals=p, radii=p, radii_xy=p)
        a.update(null)
        return lib.lidargs_debug_surfel_preprocess(P, W, H, a["means"], a["colors"], a["op"], a["scales"], 1.0, a["rots"], a["tm"], a["view"], a["beams"], 0.0, 80.0,
                                                   th, compact, 1, filter_only, a["rec"], a["rowspan"], a["spans"], a["key"], a["touched"], a["totals"], a["radii"],
                                                   a["radii_xy"], _stream())

    assert pre(P=-1) < 0 and pre(H=1) < 0 and pre(W=0) < 0 and pre(H=65536) < 0
    for th in (0, 1, 2, 3, 5, 12, 64, -4):
        assert pre(th=th) < 0, th
    for k in ("means", "colors", "op", "scales", "rots", "view", "beams", "rec", "rowspan", "spans", "key", "touched", "totals", "radii", "radii_xy"):
        assert pre(**{k: None}) < 0, k
    for k in ("means", "scales", "rots", "view", "beams", "radii", "radii_xy"):
        assert pre(filter_only=1, **{k: None}) < 0, k
    assert pre(tm=p, scales=None) < 0 and pre(tm=p, rots=None) < 0
    assert pre(W=16 * 257, compact=1) < 0 and pre(H=257, compact=1) < 0     # compact where it does not fit
    assert pre(P=0) == 0 and pre(P=0, filter_only=1) == 0

    def bwd(P=8, W=64, H=8, stage=1, **null):
        a = dict(touched=p, gacc=p, means=p, scales=p, rots=p, tm=None, view=p, beams=p, radii=p, depth=p, tlist=p, tcount=p, **{k: p for k, _ in ROWS})
        a.update(null)
        return lib.lidargs_debug_surfel_gaussian_backward(P, W, H, stage, a["touched"], a["gacc"], a["means"], a["scales"], a["rots"], a["tm"], a["view"], a["beams"],
                                                          a["radii"], *[a[k] for k, _ in ROWS], a["depth"], a["tlist"], a["tcount"], _stream())

    assert bwd(P=-1) < 0 and bwd(W=0) < 0 and bwd(H=1) < 0
    assert bwd(stage=3) < 0 and bwd(stage=-1) < 0
    for k in ("touched", "gacc", "tlist", "tcount"):
        for stage in (0, 1, 2):
            assert bwd(stage=stage, **{k: None}) < 0, k
    for k in ("means", "scales", "rots", "view", "beams", "radii", "dL_dmean2D", "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dscale", "dL_drot", "depth"):
        assert bwd(stage=0, **{k: None}) < 0 and bwd(stage=2, **{k: None}) < 0, k
    assert bwd(P=0) == 0 and bwd(P=0, stage=0) == 0
    _sync()
    assert (b.read() == CULLED).all()                                       # nothing was launched
