"""The two per-Gaussian stages of csrc/preprocess.hip -- k_preprocess<false>, and k_zero_touched<4|8> + k_gaussian_backward -- on their
own, against the float64 restatement of tests/preprocess_ref.py (itself held against the oracle by tests/test_preprocess_cpu.py).

The library's own launchers are reached through two test hooks of the C ABI (`lidargs_debug_preprocess`,
`lidargs_debug_gaussian_backward`).  Every device array lies between two guards that must come back untouched (`Arr`, the `Buf` of
tests/test_sort_gpu.py for any element type); outputs start out as 0xFF bytes (NaN as floats).

  (a) containment   every pixel that takes a Gaussian (the restatement's `takers`) lies inside the span the preprocess gives it, and the
                    pruned span inside the unpruned one: exact integers, on scenes built for each branch of the pruning
  (b) record        copies bit for bit; dir / dist / u1' / u2' / conic against float64 with the oracle's fp32 state as the yardstick (4 x);
                    radii and the unpruned span against the restatement's; the cull rules on rows built for each
  (c) block sums    the 64 slots of the totals against the per-Gaussian outputs of the same call
  (d) lists         tlist / tcount, the cleared lines, the zeroed rows: integers and exact zeros
  (e) chain         k_gaussian_backward's rows against the float64 VJP with its float32 run as the yardstick (4 x)
  (f) refusals
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import lidargs_scenes as sc
import preprocess_ref as ref

pytestmark = pytest.mark.gpu

GUARD_BYTES = 256
GUARD_BYTE = 0x5A
TOTALS_WORDS, SLOT_WORD, KEYSPAN_WORD, DIAG_WORD, SLOTS = 920, 8, 536, 664, 64      # LG_TOTALS_* / LG_INST_SLOTS of csrc/lidargs_common.h
CULLED = 0xFFFFFFFF
INF = float("inf")


def _binding():
    from diff_lidargs_rasterization import _C as binding
    return binding


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    import torch
    torch.cuda.synchronize()


class Arr:
    """A device array of any element type between two guards of 256 bytes."""

    def __init__(self, payload):
        import torch
        payload = np.ascontiguousarray(payload)
        self.dtype, self.shape, self.bytes = payload.dtype, payload.shape, payload.nbytes
        guard = np.full(GUARD_BYTES, GUARD_BYTE, np.uint8)
        self.t = torch.from_numpy(np.concatenate([guard, payload.reshape(-1).view(np.uint8), guard])).cuda()

    @classmethod
    def filled(cls, shape, dtype, byte=0xFF):
        return cls(np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, byte, np.uint8).view(dtype).reshape(shape))

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + GUARD_BYTES)

    def write(self, payload):
        import torch
        payload = np.ascontiguousarray(payload, self.dtype)
        assert payload.nbytes == self.bytes
        self.t[GUARD_BYTES:GUARD_BYTES + self.bytes] = torch.from_numpy(payload.reshape(-1).view(np.uint8)).cuda()

    def read(self):
        """The payload, after checking both guards."""
        full = self.t.cpu().numpy()
        assert (full[:GUARD_BYTES] == GUARD_BYTE).all(), "guard in front of the array was written"
        assert (full[GUARD_BYTES + self.bytes:] == GUARD_BYTE).all(), "guard behind the array was written"
        return full[GUARD_BYTES:GUARD_BYTES + self.bytes].view(self.dtype).reshape(self.shape).copy()


def _ptr(a):
    return a.ptr if a is not None else None


# ---- the preprocess through its hook ------------------------------------------------------------------------------------------------
def run_preprocess(scene, W, H, prune=1, compact=0, window=None, near=0.0, far=80.0, shell=(-INF, INF), mod=1.0, n_valid=None, cov=None,
                   tables=False):
    """One call of lidargs_debug_preprocess -> dict of host arrays; the spans are unpacked to tx0, tx1, ty_lo, ty_hi, binned."""
    lib = _binding()._lib
    P = scene["means3D"].shape[0]
    tiles_x = (W + 15) // 16
    f32 = lambda a: Arr(np.asarray(a, np.float32))
    ins = dict(means=f32(scene["means3D"]), colors=f32(scene["colors"]), op=f32(scene["opacities"]), view=f32(scene["viewmatrix"]), beams=f32(scene["beams"]))
    ins["scales"] = None if cov is not None else f32(scene["scales"])
    ins["rots"] = None if cov is not None else f32(scene["rotations"])
    ins["cov"] = f32(cov) if cov is not None else None
    ins["n_valid"] = Arr(np.array([n_valid], np.uint32)) if n_valid is not None else None
    out = dict(rec=Arr.filled((P, 16), np.float32), rowspan=Arr.filled(P, np.uint32), spans=Arr.filled((P,) if compact else (P, 4), np.uint32),
               key=Arr.filled(P, np.uint32), touched=Arr.filled(P, np.uint8), totals=Arr.filled(TOTALS_WORDS, np.uint32, 0xEE),
               radii=Arr.filled(P, np.int32), radii_xy=Arr.filled((P, 2), np.int32))
    if tables:
        out["coltab"], out["rowtab"] = Arr.filled((W, 2), np.float32), Arr.filled((H, 2), np.float32)
    lo, hi = window if window is not None else (0, tiles_x)
    rc = lib.lidargs_debug_preprocess(P, W, H, ins["means"].ptr, ins["colors"].ptr, ins["op"].ptr, _ptr(ins["scales"]), mod, _ptr(ins["rots"]), _ptr(ins["cov"]),
                                      ins["view"].ptr, ins["beams"].ptr, near, far, shell[0], shell[1], lo, hi, compact, prune, _ptr(ins["n_valid"]),
                                      out["rec"].ptr, out["rowspan"].ptr, out["spans"].ptr, out["key"].ptr, out["touched"].ptr, out["totals"].ptr,
                                      out["radii"].ptr, out["radii_xy"].ptr, _ptr(out.get("coltab")), _ptr(out.get("rowtab")), _stream())
    assert rc == 0, _binding()._err()
    _sync()
    for a in ins.values():
        if a is not None:
            a.read()                                                        # (the guards of the inputs)
    r = {k: a.read() for k, a in out.items()}
    sp = r["spans"]
    if compact:
        none = sp == CULLED
        x0 = sp & 255; nx = ((sp >> 8) & 255) + 1; lo_ = (sp >> 16) & 255; hi_ = (sp >> 24) + 1
        r.update(binned=~none, tx0=np.where(none, 0, x0), tx1=np.where(none, 0, x0 + nx), ty_lo=np.where(none, 0, lo_), ty_hi=np.where(none, 0, hi_))
    else:
        assert not sp[:, 2:].any()
        r.update(binned=sp[:, 1] != 0, tx0=sp[:, 1] & 0xFFFF, tx1=sp[:, 1] >> 16, ty_lo=sp[:, 0] & 0xFFFF, ty_hi=sp[:, 0] >> 16, rspan_word=sp[:, 0])
    for k in ("tx0", "tx1", "ty_lo", "ty_hi"):
        r[k] = r[k].astype(np.int64)
    return r


def instances(r, th=4):
    """Instances of every Gaussian at tile height th, from its unpacked span."""
    rows = (np.maximum(r["ty_hi"], 1) - 1) // th - r["ty_lo"] // th + 1
    return np.where(r["binned"], (r["tx1"] - r["tx0"]) * rows, 0)


# ---- scenes, each built for a branch of the pruning ---------------------------------------------------------------------------------
def _near(scene, factor):
    """The scene pulled towards the sensor: footprints of several pixels at the small images used here."""
    scene["means3D"] = (scene["means3D"] * np.float32(factor)).astype(np.float32)
    return scene


def _concat(a, b):
    out = {k: np.concatenate([a[k], b[k]], 0) for k in ("means3D", "scales", "rotations", "opacities", "colors")}
    out.update(beams=a["beams"], viewmatrix=a["viewmatrix"], bg=a["bg"])
    return out


def _rows(scene, idx):
    out = dict(scene)
    for k in ("means3D", "scales", "rotations", "opacities", "colors"):
        out[k] = np.ascontiguousarray(scene[k][idx])
    return out


def scene1(P=4096, seed=11):
    """W = 256, H = 32, uniform table, street + shell mix, random view; opacities log-uniform over [1e-3, 1] with rows at 1/255 exactly, one
    ulp either side, 0, NaN and 1."""
    W, H = 256, 32
    s = _concat(sc.make_scene("street", P // 2, H, seed, random_view=True), sc.make_scene("shell", P - P // 2, H, seed + 1, random_view=True))
    s = _near(s, 0.15)
    rng = np.random.default_rng([seed, 1])
    op = np.exp(rng.uniform(math.log(1e-3), 0.0, P)).astype(np.float32)
    t = np.float32(1.0) / np.float32(255.0)
    special = [t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)), np.float32(0), np.float32(np.nan), np.float32(1)]
    for j, v in enumerate(special * 8):                                     # eight rows of each
        op[7 + 83 * j] = v
    s["opacities"] = op.reshape(P, 1)
    return dict(scene=s, W=W, H=H, mod=1.0)


def scene2(table):
    """The geometry of tests/test_beam_tables_gpu.py _stress_scene (tall footprints beside beams) at P = 3000."""
    from test_beam_tables_gpu import _stress_scene
    s, W, H, _ = _stress_scene(table)
    return dict(scene=_rows(s, np.arange(0, s["means3D"].shape[0], 4)), W=W, H=H, mod=1.0)


def scene3(P=1200, seed=5):
    """Footprints elongated along azimuth (scales about (0.03, 0.4, 0.03), the long axis tangential), centred on the first and the last
    beam, range 3-10 m, opacity 0.99: off the horizon the great circle such a footprint lies on leaves its row, which is what the
    (1 - cos dbeta) term of the row bound covers."""
    W, H = 256, 32
    rng = np.random.default_rng(seed)
    beams = sc.beam_inclinations(H)
    el = np.where(np.arange(P) % 2 == 0, beams[0] + 1e-3, beams[H - 1] - 1e-3).astype(np.float64) + rng.uniform(-5e-4, 5e-4, P)
    az = rng.uniform(-np.pi, np.pi, P); r = rng.uniform(3.0, 10.0, P)
    s = dict(means3D=np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32),
             scales=(np.array([[0.03, 0.4, 0.03]]) * np.exp(0.2 * rng.normal(size=(P, 3)))).astype(np.float32),
             rotations=np.stack([np.cos(az / 2), np.zeros(P), np.zeros(P), np.sin(az / 2)], 1).astype(np.float32),      # local y -> the azimuthal tangent
             opacities=np.full((P, 1), 0.99, np.float32), colors=rng.uniform(0, 1, (P, 2)).astype(np.float32), beams=beams,
             bg=np.zeros(2, np.float32), viewmatrix=sc.rigid_viewmatrix(None))
    return dict(scene=s, W=W, H=H, mod=1.0)


def _blob_scene(P, beams, seed, r_lo, r_hi, scale=0.1, op_lo=0.3):
    rng = np.random.default_rng(seed)
    H = beams.size
    r = rng.uniform(r_lo, r_hi, P); az = rng.uniform(-np.pi, np.pi, P); el = rng.uniform(float(beams[0]), float(beams[-1]), P)
    q = rng.normal(size=(P, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(means3D=np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32),
                scales=(scale * np.exp(0.5 * rng.normal(size=(P, 3)))).astype(np.float32), rotations=q.astype(np.float32),
                opacities=rng.uniform(op_lo, 1.0, (P, 1)).astype(np.float32), colors=rng.uniform(0, 1, (P, 2)).astype(np.float32),
                beams=beams.astype(np.float32), bg=np.zeros(2, np.float32), viewmatrix=sc.rigid_viewmatrix(None))


def scene4(W, H):
    """The antipode rule: images of one or two tile columns, where a Gaussian's own tile holds the pixels looking the other way."""
    return dict(scene=_blob_scene(4096, sc.beam_inclinations(H), 100 * W + H, 1.0, 4.0, scale=0.3), W=W, H=H, mod=1.0)


def scene5(lo, hi):
    """Beam fans of 1.4 and 1.6 rad in all (the second gives up the small-angle forms), and one whose end reaches 1.4 rad (cfan <= 0.05:
    no column bound, the row bound with its worst-case term)."""
    H, W = 32, 128
    return dict(scene=_blob_scene(1500, np.linspace(lo, hi, H), int(1000 * hi), 1.5, 8.0), W=W, H=H, mod=1.0)


def scene6():
    """scale_modifier 6 on the first thousand rows of scene 1: sb, sa >= 0.7."""
    d = scene1()
    return dict(scene=_rows(d["scene"], np.arange(1000)), W=d["W"], H=d["H"], mod=6.0)


def scene7(H):
    """H = 1025 at W = 64: the beams live outside LDS and tanf runs per Gaussian; H = 1024: the same Gaussians on the first 1024 beams."""
    beams = sc.beam_inclinations(1025)[:H]
    s = sc.make_scene("shell", 1500, 1025, 77, random_view=False)
    s["beams"] = beams
    return dict(scene=s, W=64, H=H, mod=1.0)


SCENES = {
    "1_mix_opacities": scene1, "2_stress_waymo": lambda: scene2("waymo"), "2_stress_uniform": lambda: scene2("uniform"), "3_azimuthal": scene3,
    "4_antipode_W25_H2": lambda: scene4(25, 2), "4_antipode_W25_H4": lambda: scene4(25, 4), "4_antipode_W32_H2": lambda: scene4(32, 2),
    "4_antipode_W32_H4": lambda: scene4(32, 4), "4_antipode_W48_H2": lambda: scene4(48, 2), "4_antipode_W48_H4": lambda: scene4(48, 4),
    "5_fan_1.4": lambda: scene5(-0.7, 0.7), "5_fan_1.6": lambda: scene5(-0.8, 0.8), "5_fan_end_1.4": lambda: scene5(0.2, 1.4),
    "6_scale_modifier_6": scene6, "7_H1025": lambda: scene7(1025), "7_H1024": lambda: scene7(1024),
}
PRUNING_PAYS = ("1_mix_opacities", "2_stress_waymo", "2_stress_uniform", "3_azimuthal")     # scenes 1-3: pruning removes >= a quarter


@functools.lru_cache(maxsize=None)
def reference(name):
    """The scene and its float64 reference (forward fields, geometry, takers): computed once, shared, never written to."""
    d = SCENES[name]()
    s, W, H = d["scene"], d["W"], d["H"]
    f = ref.forward64(s["means3D"], s["scales"], s["rotations"], s["viewmatrix"], d["mod"])
    geo = ref.geometry(f, s["beams"], W, H)
    tk = ref.takers(f, geo, s["opacities"], s["beams"], W, H)
    for a in list(f.values()) + list(geo.values()) + list(tk.values()) + [v for v in s.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return d, f, geo, tk


def scene_conditions(name, say=print):
    """The conditions a scene must meet on the reference alone: >= 20 000 takers, undecided <= 5 %, rounding-boundary Gaussians <= 1 %."""
    d, f, geo, tk = reference(name)
    n, und, nb, live = int(tk["n"].sum()), int(tk["undecided"].sum()), int(geo["near_boundary"].sum()), int(geo["live"].sum())
    say(f"[scene {name}] P {geo['live'].size} live {live} takers {n} undecided {und} ({100.0 * und / max(n + und, 1):.3f} %) near a rounding boundary {nb}")
    assert n >= 20000, f"{name}: only {n} takers"
    assert und <= 0.05 * (n + und)
    assert nb <= 0.01 * geo["live"].size
    return n, und, nb


# ---- (a) containment ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_every_taker_lies_inside_the_pruned_span(name, hip_lib_built):
    d, f, geo, tk = reference(name)
    scene_conditions(name)
    s, W, H = d["scene"], d["W"], d["H"]
    pr = run_preprocess(s, W, H, prune=1, mod=d["mod"])
    un = run_preprocess(s, W, H, prune=0, mod=d["mod"])
    ok = ~geo["near_boundary"]
    # every taker inside the span
    has = (tk["n"] > 0) & ok
    assert pr["binned"][has].all(), f"{(~pr['binned'][has]).sum()} Gaussians that pixels take are binned nowhere; first: {np.nonzero(has & ~pr['binned'])[0][:5]}"
    box = tk["box"]
    bad = has & ((box[:, 0] < 16 * pr["tx0"]) | (box[:, 2] >= 16 * pr["tx1"]) | (box[:, 1] < pr["ty_lo"]) | (box[:, 3] >= pr["ty_hi"]))
    if bad.any():
        g = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{bad.sum()} Gaussians have takers outside their pruned span; first: {g}: takers in columns [{box[g, 0]}, {box[g, 2]}] rows "
                             f"[{box[g, 1]}, {box[g, 3]}], span columns [{16 * pr['tx0'][g]}, {16 * pr['tx1'][g]}) rows [{pr['ty_lo'][g]}, {pr['ty_hi'][g]})")
    # the pruned span inside the unpruned one, the other outputs independent of the flag
    assert not (pr["binned"] & ~un["binned"]).any()
    b = pr["binned"]
    assert (pr["tx0"][b] >= un["tx0"][b]).all() and (pr["tx1"][b] <= un["tx1"][b]).all()
    assert (pr["ty_lo"][b] >= un["ty_lo"][b]).all() and (pr["ty_hi"][b] <= un["ty_hi"][b]).all()
    assert np.array_equal(pr["radii"], un["radii"]) and np.array_equal(pr["radii_xy"], un["radii_xy"])
    ip, iu = int(instances(pr).sum()), int(instances(un).sum())
    print(f"[scene {name}] instances at tile height 4: {ip} pruned, {iu} unpruned ({100.0 * ip / max(iu, 1):.1f} %)")
    if name in PRUNING_PAYS:
        assert ip <= 0.75 * iu
    if name.startswith("4_antipode_W25"):
        far = int((tk["far_col"] > W / 4.0).sum())
        print(f"[scene {name}] Gaussians with a taker more than W / 4 columns from their centre: {far}")
        assert far > 0
    if name.startswith("7_"):
        assert geo["ry"].max() >= 64                                        # footprints taller than any tile


def _row_bound_probe(r, mirror, b):
    """One elongated Gaussian at elevation -0.1 (mirror: +0.1, on the mirrored table) between the beams -0.15 and b; whether the row of
    beam b -- dalpha above the centre (mirror: of beam -b, dalpha below it) -- is in the pruned span."""
    az, el = 0.3, -0.1
    beams = np.array([-0.45, -0.3, -0.15, b, 0.1, 0.25], np.float32)
    z = r * math.sin(el)
    if mirror:
        beams, z = (-beams[::-1]).copy(), -z
    s = dict(means3D=np.array([[r * math.cos(el) * math.cos(az), r * math.cos(el) * math.sin(az), z]], np.float32),
             scales=np.array([[0.03, 0.4, 0.03]], np.float32), rotations=np.array([[math.cos(az / 2), 0, 0, math.sin(az / 2)]], np.float32),
             opacities=np.array([[0.99]], np.float32), colors=np.zeros((1, 2), np.float32), beams=beams, viewmatrix=sc.rigid_viewmatrix(None))
    o = run_preprocess(s, 256, 6)
    assert o["binned"][0] and o["ty_hi"][0] - o["ty_lo"][0] in (1, 2), (o["ty_lo"][0], o["ty_hi"][0])
    return o["ty_hi"][0] - o["ty_lo"][0] == 2


@pytest.mark.parametrize("r", [5.0, 5.5])                                     # (alpha + dalpha = -0.0251 and -0.0324: inside the bisected window)
def test_row_bound_takes_a_beam_exactly_on_it_at_either_end(r, hip_lib_built):
    """The rows in reach are the beams in [alpha - dalpha, alpha + dalpha], both ends included.  No test can place a beam on alpha + dalpha
    from outside (the bound is formed with the hardware's log and atan2f), so the kernel itself is asked where its ends are: the movable
    beam b is bisected over the floats to the last one still in reach from below (the upper end), and, on the scene mirrored in elevation
    -- where every quantity of the bound is the same number or its negative -- to the last one in reach from above (the lower end of the
    mirrored scene).  Treated alike, the two ends are the same float; an end that leaves out the beam lying exactly on it is one float short."""
    bits = lambda x: int(np.float32(x).view(np.uint32))
    val = lambda k: float(np.array([k], np.uint32).view(np.float32)[0])
    ends = []
    for mirror in (False, True):
        near, far = bits(-0.04), bits(-0.012)                                # negative floats: fewer bits = closer to zero = higher
        assert _row_bound_probe(r, mirror, val(near)) and not _row_bound_probe(r, mirror, val(far))
        lo, hi = far, near                                                  # not in reach at lo, in reach at hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if _row_bound_probe(r, mirror, val(mid)):
                hi = mid
            else:
                lo = mid
        ends.append(val(hi))
    print(f"[row bound r={r}] alpha + dalpha = {ends[0]!r}, -(alpha' - dalpha') of the mirrored scene = {ends[1]!r}")
    assert ends[0] == ends[1]


def test_window_clips_the_span_exactly(hip_lib_built):
    d, f, geo, tk = reference("1_mix_opacities")
    s, W, H = d["scene"], d["W"], d["H"]
    full = run_preprocess(s, W, H)
    for lo, hi in ((3, 9), (0, 1), (15, 16)):
        w = run_preprocess(s, W, H, window=(lo, hi))
        x0, x1 = np.maximum(full["tx0"], lo), np.minimum(full["tx1"], hi)
        want = full["binned"] & (x1 > x0)
        assert want.sum() > 10 and (full["binned"] & ~want).sum() > 10
        assert np.array_equal(w["binned"], want)
        for k, v in (("tx0", x0), ("tx1", x1), ("ty_lo", full["ty_lo"]), ("ty_hi", full["ty_hi"])):
            assert np.array_equal(w[k][want], v[want]), k
        assert np.array_equal(w["key"], np.where(want, full["key"], CULLED))
        assert np.array_equal(w["radii"], full["radii"])


def test_compact_spans_unpack_to_the_full_ones(hip_lib_built):
    for name in ("1_mix_opacities", "4_antipode_W25_H2"):
        d, f, geo, tk = reference(name)
        a = run_preprocess(d["scene"], d["W"], d["H"], compact=0)
        b = run_preprocess(d["scene"], d["W"], d["H"], compact=1)
        assert np.array_equal(a["binned"], b["binned"]) and a["binned"].sum() > 100
        m = a["binned"]
        for k in ("tx0", "tx1", "ty_lo", "ty_hi"):
            assert np.array_equal(a[k][m], b[k][m]), k
        for k in ("key", "radii", "radii_xy", "totals", "touched"):
            assert np.array_equal(a[k], b[k]), k


# ---- (b) record ---------------------------------------------------------------------------------------------------------------------
def _oracle_state(d):
    from oracle import lgo
    s = d["scene"]
    P = s["means3D"].shape[0]
    fo = lgo.forward(s["means3D"], s["colors"], s["opacities"], s["scales"], s["rotations"], s["viewmatrix"], s["beams"], d["W"], d["H"], scale_modifier=d["mod"])
    u1, u2 = fo.array("basis_u1").reshape(P, 3), fo.array("basis_u2").reshape(P, 3)
    with np.errstate(all="ignore"):
        u1p = u1 / (u1 * u1).sum(1, keepdims=True, dtype=np.float32); u2p = u2 / (u2 * u2).sum(1, keepdims=True, dtype=np.float32)
    return dict(vis=fo.radii > 0, radii=fo.radii, dir=fo.array("sphere").reshape(P, 3), dist=fo.array("depths").reshape(P, 1), u1p=u1p, u2p=u2p,
                conic=fo.array("conic_opacity").reshape(P, 4)[:, :3], radii_xy=fo.array("radii_xy").reshape(P, 2), tiles_touched=fo.array("tiles_touched"))


def _record_fields(rec):
    return dict(dir=rec[:, 0:3], dist=rec[:, 3:4], u1p=rec[:, [4, 6, 8]], u2p=rec[:, [5, 7, 9]], conic=rec[:, [10, 12, 11]])     # conic as (A, B, C)


@pytest.mark.parametrize("name", ["1_mix_opacities", "2_stress_waymo", "6_scale_modifier_6"])
def test_record_against_float64_with_the_oracle_as_yardstick(name, hip_lib_built):
    d, f, geo, tk = reference(name)
    s, W, H = d["scene"], d["W"], d["H"]
    P = s["means3D"].shape[0]
    r = run_preprocess(s, W, H, mod=d["mod"], tables=True)
    o = _oracle_state(d)
    b = r["binned"]
    rec = r["rec"]
    # copies, bit for bit
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert np.array_equal(u(rec[b, 13]), u(s["opacities"][b, 0])) and np.array_equal(u(rec[b, 14:16]), u(s["colors"][b]))
    assert np.array_equal(r["key"], np.where(b, u(rec[:, 3]), CULLED))
    assert np.array_equal(r["rowspan"][b], r["rspan_word"][b])
    assert (u(rec[~b]) == CULLED).all() and (r["rowspan"][~b] == CULLED).all()          # records of the unbinned: never written
    assert not r["touched"].any()
    assert np.array_equal(r["radii"], r["radii_xy"].max(1))
    # radii and the unpruned span: the restatement's, outside its own rounding boundaries
    ok = ~geo["near_boundary"]
    print(f"[record {name}] Gaussians near a rounding boundary, left out: {int((~ok).sum())} of {P}")
    assert (~ok).sum() <= 0.01 * P
    assert np.array_equal(r["radii"][ok] > 0, geo["live"][ok])
    assert np.array_equal(r["radii_xy"][ok, 0], geo["rx"][ok]) and np.array_equal(r["radii_xy"][ok, 1], geo["ry"][ok])
    un = run_preprocess(s, W, H, prune=0, mod=d["mod"])
    opaque = ~(s["opacities"][:, 0].astype(np.float32) * np.float32(255.0) < np.float32(1.0))       # (below 1/255 a Gaussian is binned nowhere, pruning or not)
    m = ok & geo["live"] & opaque
    assert un["binned"][m].all() and not un["binned"][geo["live"] & ~opaque].any()
    assert np.array_equal(np.stack([un["tx0"], un["ty_lo"], un["tx1"], un["ty_hi"]], 1)[m], geo["rect"][m])
    # values: HIP's error against float64 over the oracle's, per field group
    v = b & o["vis"]
    assert v.sum() > 0.9 * b.sum()
    mine = _record_fields(rec)
    ids = np.nonzero(v)[0]
    for k in ("dir", "dist", "u1p", "u2p", "conic"):
        p99h, p99y, mxh, mxy, where = ref.ratios(f"{name[:1]} {k}", mine[k][v], o[k][v], f[k].reshape(P, -1)[v])
        assert p99h <= 4.0 * p99y and mxh <= 4.0 * mxy, f"{k}: {where} (rows are positions among the binned Gaussians: row i is Gaussian ids[i], e.g. row 0 = {ids[0]})"
    # the pixel-ray tables: (cos, sin) of the float angle, correctly rounded
    alp = s["beams"][H - 1 - np.arange(H)].astype(np.float64)
    assert np.array_equal(r["rowtab"], np.stack([np.cos(alp), np.sin(alp)], 1).astype(np.float32))
    beta = (-(np.arange(W, dtype=np.float64) - W / 2.0) / W * 2.0 * ref.PI_F).astype(np.float32).astype(np.float64)
    assert np.array_equal(r["coltab"], np.stack([np.cos(beta), np.sin(beta)], 1).astype(np.float32))


def _at(r, el, az=0.3):
    return [r * math.cos(el) * math.cos(az), r * math.cos(el) * math.sin(az), r * math.sin(el)]


def test_cull_rules_on_rows_built_for_each(hip_lib_built):
    """near / far at equality, the shell, det == 0, the guard beyond the first and the last beam, padding rows behind n_valid.
    (The zero-area rect of R3/cr/forward.cu:367 has no row: a rect's height is at least max(round(p_r + ry), round(p_r) + 1) - round(p_r - ry)
    with ry >= 1, its width at least one tile, and neither clamp can close it while the centre passes the guard test -- the smallest
    3 r is 0.017 rad against a guard of 0.004.)"""
    H, W = 16, 256
    beams = sc.beam_inclinations(H)
    b0, b1, g = float(beams[0]), float(beams[-1]), ref.GUARD
    f32 = np.float32
    rows = []                                                               # (position, expected live, what)
    add = lambda pos, live, what: rows.append((pos, live, what))
    add([80.0, 0.0, 0.0], False, "range == far")
    add([float(np.nextafter(f32(80), f32(0))), 0.0, 0.0], True, "range one ulp under far")
    add([2.0, 0.0, 0.0], False, "range == near")
    add([float(np.nextafter(f32(2), f32(3))), 0.0, 0.0], True, "range one ulp over near")
    add(_at(20.0, b1 + 0.8 * g), True, "above the last beam, inside the guard")
    add(_at(20.0, b1 + 1.2 * g), False, "above the last beam, beyond the guard")
    add(_at(20.0, b0 - 0.8 * g), True, "below the first beam, inside the guard")
    add(_at(20.0, b0 - 1.2 * g), False, "below the first beam, beyond the guard")
    add([float("nan"), 0.0, 0.0], False, "NaN position")
    add([float("inf"), 0.0, 0.0], False, "infinite position")
    shell_rows = [([10.0, 0.0, 0.0], True, "range == shell_lo"), ([float(np.nextafter(f32(10), f32(0))), 0.0, 0.0], False, "range one ulp under shell_lo"),
                  ([40.0, 0.0, 0.0], False, "range == shell_hi"), ([float(np.nextafter(f32(40), f32(0))), 0.0, 0.0], True, "range one ulp under shell_hi")]
    for rows_, kw in ((rows, dict(near=2.0, far=80.0)), (shell_rows, dict(shell=(10.0, 40.0)))):
        n_real = len(rows_)
        P = n_real + 5                                                      # five padding rows behind n_valid, all NaN
        s = _blob_scene(P, beams, 3, 5.0, 30.0)
        s["means3D"][:n_real] = np.array([r[0] for r in rows_], np.float32)
        s["opacities"][:] = 0.9
        for k in ("means3D", "scales", "rotations", "opacities", "colors"):
            s[k][n_real:] = np.nan
        r = run_preprocess(s, W, H, n_valid=n_real, **kw)
        want = np.array([x[1] for x in rows_] + [False] * 5)
        for i in range(P):
            assert (r["radii"][i] > 0) == want[i], rows_[i][2] if i < n_real else "padding row"
        dead = ~want
        assert not r["radii_xy"][dead].any() and (r["key"][dead] == CULLED).all() and not r["spans"][dead].any() and not r["touched"].any()
        assert r["binned"][want].all()
        assert np.array_equal(r["key"][want], r["rec"][want, 3].view(np.uint32))
    # det == 0: at 1e19 m the footprint a c - b b underflows to zero (far raised out of the way)
    s2 = _blob_scene(4, beams, 4, 5.0, 30.0)
    s2["means3D"][1] = np.array(_at(1e19, -0.1), np.float32)
    r2 = run_preprocess(s2, W, H, far=3e38)
    assert list(r2["radii"] > 0) == [True, False, True, True]
    assert r2["key"][1] == CULLED and not r2["spans"][1].any()


# ---- (c) block sums -----------------------------------------------------------------------------------------------------------------
def check_block_sums(r, what):
    t = r["totals"]
    assert not t[:SLOT_WORD].any() and not t[SLOT_WORD + 8 * SLOTS:KEYSPAN_WORD].any(), what       # cleared, and written by nobody here
    inst = t[SLOT_WORD:SLOT_WORD + 8 * SLOTS].view(np.uint64).reshape(SLOTS, 4).sum(0)
    for j, th in enumerate((4, 8, 16, 32)):
        assert int(inst[j]) == int(instances(r, th).sum()), (what, th)
    diag = t[DIAG_WORD:DIAG_WORD + 4 * SLOTS].view(np.uint64).reshape(SLOTS, 2).sum(0)
    assert int(diag[0]) == int((r["radii"] > 0).sum()), what
    ks = t[KEYSPAN_WORD:KEYSPAN_WORD + 2 * SLOTS].reshape(SLOTS, 2)
    keys = r["key"][r["key"] != CULLED]
    if keys.size:
        assert int(~ks[:, 0].max() & 0xFFFFFFFF) == int(keys.min()) and int(ks[:, 1].max()) == int(keys.max()), what
    else:
        assert not ks.any() and not inst.any(), what
    return int(diag[1])


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 16385, 16700])
def test_block_sums_against_the_outputs_of_the_same_call(P, hip_lib_built):
    W, H = 512, 16
    s = _near(sc.make_scene("shell", P, H, 300 + P % 97, random_view=True), 0.3)       # opacities U(0.1, 1): every visible Gaussian is binned
    pr = run_preprocess(s, W, H, prune=1)
    reftiles_pruned = check_block_sums(pr, f"P={P} pruned")
    un = run_preprocess(s, W, H, prune=0)
    reftiles = check_block_sums(un, f"P={P} unpruned")
    assert reftiles_pruned == reftiles                                      # the reference's rect does not know about the pruning
    assert np.array_equal(un["binned"], un["radii"] > 0)
    # the reference's tiles_touched: the whole rect in 16 x 1 tiles, which is the unpruned span
    theirs = np.where(un["binned"], (un["tx1"] - un["tx0"]) * (un["ty_hi"] - un["ty_lo"]), 0)
    assert reftiles == int(theirs.sum())
    if P >= 255:
        assert (un["radii"] > 0).sum() > 0.3 * P
        f = ref.forward64(s["means3D"], s["scales"], s["rotations"], s["viewmatrix"])
        geo = ref.geometry(f, s["beams"], W, H)
        rect = geo["rect"]
        mine = np.where(geo["live"], (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]), 0)
        ok = ~geo["near_boundary"]                                          # (those on a rounding boundary of the restatement: left out of both sums)
        print(f"[block sums P={P}] Gaussians near a rounding boundary, left out: {int((~ok).sum())}")
        assert (~ok).sum() <= 0.01 * P
        assert np.array_equal(theirs[ok], mine[ok])
        assert reftiles - int(theirs[~ok].sum()) == int(mine[ok].sum())


def test_block_sums_of_a_frame_with_nothing_visible(hip_lib_built):
    s = sc.make_scene("shell", 700, 16, 9)
    r = run_preprocess(s, 512, 16, far=1.0)
    assert not r["radii"].any() and (r["key"] == CULLED).all() and not r["binned"].any()
    assert check_block_sums(r, "nothing visible") == 0
    assert not r["totals"].any()


# ---- (d) touched lists and zeroing --------------------------------------------------------------------------------------------------
ROWS = (("dL_dmean2D", 4), ("dL_dconic", 4), ("dL_dopacity", 1), ("dL_dcolor", 2), ("dL_ddepths", 1), ("dL_dmean3D", 3), ("dL_dsphere", 3),
        ("dL_dbasis_u1", 3), ("dL_dbasis_u2", 3), ("dL_dcov3D", 6), ("dL_dscale", 3), ("dL_drot", 4))       # in the hook's argument order
OPTIONAL = ("dL_dconic", "dL_ddepths", "dL_dsphere", "dL_dbasis_u1", "dL_dbasis_u2", "dL_dcov3D")
SENTINEL = np.float32(7.25)


class Backward:
    """The arrays of one lidargs_debug_gaussian_backward call sequence on P Gaussians."""

    def __init__(self, P, line_f4=4, scene=None, mod=1.0, cov=None, skip=()):
        self.P, self.line_f4, self.mod = P, line_f4, mod
        self.touched = Arr(np.zeros(P, np.uint8))
        self.gacc = Arr(np.full((P, 4 * line_f4), SENTINEL, np.float32))
        self.rows = {k: (None if k in skip else Arr.filled((P, w), np.float32)) for k, w in ROWS}
        self.tlist = Arr.filled(P + 256, np.uint8, 0xEE)
        self.tcount = Arr.filled(P // 256 + 64, np.uint16, 0xEE)
        f32 = lambda a: Arr(np.asarray(a, np.float32))
        self.ins = {}
        if scene is not None:
            self.ins = dict(means=f32(scene["means3D"]), view=f32(scene["viewmatrix"]))
            if cov is None:
                self.ins.update(scales=f32(scene["scales"]), rots=f32(scene["rotations"]))
            else:
                self.ins["cov"] = f32(cov)

    def call(self, stage):
        lib = _binding()._lib
        i = self.ins
        rc = lib.lidargs_debug_gaussian_backward(self.P, self.line_f4, stage, self.touched.ptr, self.gacc.ptr, _ptr(i.get("means")), _ptr(i.get("scales")),
                                                 self.mod, _ptr(i.get("rots")), _ptr(i.get("cov")), _ptr(i.get("view")),
                                                 *[_ptr(self.rows[k]) for k, _ in ROWS], self.tlist.ptr, self.tcount.ptr, _stream())
        _sync()
        return rc

    def read_rows(self):
        for a in self.ins.values():
            a.read()
        return {k: a.read() for k, a in self.rows.items() if a is not None}


def _marks(kind, P, rng):
    m = np.zeros(P, np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "first":
        m[0] = 1
    elif kind == "last":
        m[P - 1] = 1
    elif kind == "every_third":
        m[::3] = 1
    elif kind == "one_wave":                                                # the last whole wave, alone (P < 64: everybody)
        w = max(P // 64 - 1, 0)
        m[64 * w:64 * w + 64] = 1
    elif kind == "one_region":                                              # the last whole region: count 256, offsets up to 255 (P < 256: everybody)
        r = max(P // 256 - 1, 0)
        m[256 * r:256 * r + 256] = 1
    elif kind == "value_255":
        m[rng.random(P) < 0.4] = 255
    elif kind != "none":
        raise ValueError(kind)
    return m


MARKS = ("none", "all", "first", "last", "every_third", "one_wave", "one_region", "value_255")


def check_lists(b, marks, what):
    P = b.P
    regions = (P + 255) // 256
    tcount, tlist = b.tcount.read(), b.tlist.read()
    want_c = np.full(tcount.size, 0xEEEE, np.uint16); want_l = np.full(tlist.size, 0xEE, np.uint8)
    for r in range(regions):
        off = np.nonzero(marks[256 * r:256 * r + 256])[0]
        want_c[r] = off.size
        want_l[256 * r:256 * r + off.size] = off
    assert np.array_equal(tcount, want_c), what
    assert np.array_equal(tlist, want_l), what


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 511, 513, 1281])
def test_touched_lists_cleared_lines_and_zeroed_rows(P, hip_lib_built):
    rng = np.random.default_rng(P)
    for line_f4 in (4, 8):
        for kind in MARKS:
            what = f"P={P} line_f4={line_f4} marks={kind}"
            marks = _marks(kind, P, rng)
            if kind == "one_region" and P >= 256:
                assert np.count_nonzero(marks) == 256
            b = Backward(P, line_f4, skip=("dL_dconic", "dL_dbasis_u2") if kind == "every_third" else ())     # (NULL optional arrays are skipped)
            b.touched.write(marks)
            assert b.call(1) == 0, (what, _binding()._err())
            check_lists(b, marks, what)
            assert np.array_equal(b.touched.read(), marks), what
            acc = b.gacc.read().view(np.uint32)
            m = marks != 0
            assert not acc[m].any(), what                                   # marked lines: +0 in every word
            assert (acc[~m] == SENTINEL.view(np.uint32)).all(), what        # the others: untouched
            for k, a in b.read_rows().items():
                assert not a.view(np.uint32).any(), (what, k)               # every row of every supplied array: +0


def _chain_scene(P, seed=21):
    """P Gaussians of scene 1's recipe that the restatement finds visible (positions inside the fan, as the product's touched ones are)."""
    d = scene1(3 * P + 512, seed)
    s = d["scene"]
    s["opacities"] = np.clip(np.nan_to_num(s["opacities"], nan=0.5), 0.05, 0.9).astype(np.float32)
    f = ref.forward64(s["means3D"], s["scales"], s["rotations"], s["viewmatrix"])
    geo = ref.geometry(f, s["beams"], d["W"], d["H"])
    idx = np.nonzero(geo["live"])[0][:P]
    assert idx.size == P
    return _rows(s, idx), d["W"], d["H"]


def run_chain(scene, line, marks, mod=1.0, cov=None, skip=()):
    """The backward's two launches around a blend that leaves `line` in the packed lines: lists and zeros, the fill, the chain."""
    b = Backward(line.shape[0], 4, scene, mod, cov, skip)
    b.touched.write(marks)
    assert b.call(1) == 0, _binding()._err()
    b.gacc.write(line)
    assert b.call(2) == 0, _binding()._err()
    b.gacc.read(); b.tlist.read(); b.tcount.read()
    return b.read_rows()


def test_a_touched_row_does_not_depend_on_the_other_marks(hip_lib_built):
    P = 1281
    scene, W, H = _chain_scene(P)
    scene["viewmatrix"] = sc.rigid_viewmatrix(None)                         # identity: the world origin is the sensor's, exactly
    scene["means3D"][5] = 0.0
    rng = np.random.default_rng(2)
    line = rng.normal(size=(P, 16)).astype(np.float32)
    full = run_chain(scene, line, np.ones(P, np.uint8))
    others = np.arange(P) != 5
    assert (np.abs(full["dL_dmean3D"]).sum(1)[others] > 0).all() and np.isfinite(full["dL_dmean3D"]).all()
    for k, a in full.items():
        assert not a[5].view(np.uint32).any(), k                            # range 0: the chain leaves the rows as zeroed (R3/cr/backward.cu:488)
    for kind in ("first", "every_third", "one_wave", "value_255", "none"):
        marks = _marks(kind, P, rng)
        if kind != "none":
            marks[5] = 1
        got = run_chain(scene, line, marks)
        m = marks != 0
        for k, a in got.items():
            assert np.array_equal(a[m].view(np.uint32), full[k][m].view(np.uint32)), (kind, k)
            assert not a[~m].view(np.uint32).any(), (kind, k)


def test_both_launches_in_one_call_chain_the_cleared_lines(hip_lib_built):
    """stage 0: the first launch clears the marked lines and the chain then reads those zeros -- a backward whose blend added nothing.
    The copied rows are +0 bit for bit, every chained row is zero, the unmarked lines keep what they held."""
    P = 1281
    scene, W, H = _chain_scene(P)
    rng = np.random.default_rng(3)
    for kind in ("all", "every_third"):
        marks = _marks(kind, P, rng)
        b = Backward(P, 4, scene)
        b.touched.write(marks)
        assert b.call(0) == 0, _binding()._err()
        check_lists(b, marks, f"stage 0 {kind}")
        acc = b.gacc.read().view(np.uint32)
        m = marks != 0
        assert not acc[m].any() and (acc[~m] == SENTINEL.view(np.uint32)).all()
        for k, a in b.read_rows().items():
            if k in ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor", "dL_ddepths"):
                assert not a.view(np.uint32).any(), (kind, k)
            assert (a == 0).all(), (kind, k)                                # (a chained row may hold -0: 0 times a negative factor)


# ---- (e) chain values ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain_inputs():
    from oracle import lgo
    P = 4096
    scene, W, H = _chain_scene(P)
    grads = sc.upstream_grads(H, W, 21)
    fo = lgo.forward(scene["means3D"], scene["colors"], scene["opacities"], scene["scales"], scene["rotations"], scene["viewmatrix"], scene["beams"], W, H)
    g = lgo.backward(fo, *grads)
    f = ref.forward64(scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"])
    lo = ref.line_from_oracle(g, f["u1"], f["u2"])
    hit = np.abs(lo).sum(1) > 0
    assert hit.sum() > 0.3 * P
    mag = np.sqrt((lo[hit] ** 2).mean(0))                                   # per-slot magnitudes of one real backward
    assert (mag > 0).all()
    line = (np.random.default_rng(8).normal(size=(P, 16)) * mag).astype(np.float32)
    return scene, line, f


CHAINED = ("dL_dmean3D", "dL_dcov3D", "dL_dscale", "dL_drot", "dL_dsphere", "dL_dbasis_u1", "dL_dbasis_u2")


@pytest.mark.parametrize("variant", ["mod1", "mod0.5", "cov3D_precomp", "optional_outputs_NULL"])
def test_chain_against_the_float64_vjp(variant, hip_lib_built):
    scene, line, f = _chain_inputs()
    P = line.shape[0]
    mod = 0.5 if variant == "mod0.5" else 1.0
    cov = None
    if variant == "cov3D_precomp":
        import torch
        cov = ref.cov6_of(torch.as_tensor(scene["scales"], dtype=ref.F64), torch.as_tensor(scene["rotations"], dtype=ref.F64)).numpy().astype(np.float32)
    skip = tuple(k for k in OPTIONAL if not (k == "dL_dcov3D" and cov is not None)) if variant == "optional_outputs_NULL" else ()
    got = run_chain(scene, line, np.ones(P, np.uint8), mod, cov, skip)
    args = (line, scene["means3D"], scene["scales"], scene["rotations"], scene["viewmatrix"], mod, cov)
    want = ref.chain(*args)
    import torch
    yard = ref.chain(*args, dtype=torch.float32)
    det2 = f["det"] ** 2
    print(f"[chain {variant}] Gaussians with denom^2 < 1e-9: {(det2 < 1e-9).sum()}, > 1e-7: {(det2 > 1e-7).sum()} of {P}")
    assert (det2 < 1e-9).sum() > 100                                        # the conic's damping (1 / (denom^2 + 1e-7)) is what decides there
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for k in ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor", "dL_ddepths"):      # pure copies of the line
        if k in got:
            assert np.array_equal(u(got[k]), u(want[k])), k
    for k in CHAINED:
        if k not in got:
            continue
        if cov is not None and k in ("dL_dscale", "dL_drot"):
            assert not got[k].view(np.uint32).any(), k
            continue
        p99h, p99y, mxh, mxy, where = ref.ratios(f"{variant} {k[3:]}", got[k], yard[k], want[k])
        assert p99h <= 4.0 * p99y and mxh <= 4.0 * mxy, f"{k}: {where}"
    if variant == "optional_outputs_NULL":
        full = run_chain(scene, line, np.ones(P, np.uint8), mod, cov)
        for k, a in got.items():
            assert np.array_equal(u(a), u(full[k])), k


# ---- (f) refusals -------------------------------------------------------------------------------------------------------------------
def test_hooks_refuse_what_they_cannot_launch(hip_lib_built):
    lib = _binding()._lib
    b = Arr.filled(4096, np.uint32)
    p = b.ptr

    def pre(P=8, W=64, H=8, lo=0, hi=4, compact=0, **null):
        a = dict(means=p, colors=p, op=p, scales=p, rots=p, cov=None, view=p, beams=p, rec=p, rowspan=p, spans=p, key=p, touched=p, totals=p, radii=p,
                 radii_xy=p, coltab=None, rowtab=None)
        a.update(null)
        return lib.lidargs_debug_preprocess(P, W, H, a["means"], a["colors"], a["op"], a["scales"], 1.0, a["rots"], a["cov"], a["view"], a["beams"], 0.0, 80.0,
                                            -INF, INF, lo, hi, compact, 1, None, a["rec"], a["rowspan"], a["spans"], a["key"], a["touched"], a["totals"],
                                            a["radii"], a["radii_xy"], a["coltab"], a["rowtab"], _stream())

    assert pre(P=-1) < 0 and pre(H=1) < 0 and pre(W=0) < 0
    for k in ("means", "colors", "op", "view", "beams", "rec", "rowspan", "spans", "key", "touched", "totals", "radii"):
        assert pre(**{k: None}) < 0, k
    assert pre(scales=None) < 0 and pre(rots=None) < 0 and pre(coltab=p) < 0
    assert pre(lo=-1) < 0 and pre(lo=2, hi=2) < 0 and pre(hi=5) < 0                       # a window outside the grid
    assert pre(W=16 * 257, hi=257, compact=1) < 0 and pre(H=257, compact=1) < 0            # compact where it does not fit
    assert pre(P=0) == 0

    def bwd(P=8, line_f4=4, stage=1, **null):
        a = dict(touched=p, gacc=p, means=p, scales=p, rots=p, cov=None, view=p, tlist=p, tcount=p, **{k: p for k, _ in ROWS})
        a.update(null)
        return lib.lidargs_debug_gaussian_backward(P, line_f4, stage, a["touched"], a["gacc"], a["means"], a["scales"], 1.0, a["rots"], a["cov"], a["view"],
                                                   *[a[k] for k, _ in ROWS], a["tlist"], a["tcount"], _stream())

    assert bwd(P=-1) < 0
    for lf in (0, 1, 2, 3, 5, 16):
        assert bwd(line_f4=lf) < 0
    assert bwd(stage=3) < 0 and bwd(stage=-1) < 0 and bwd(line_f4=8, stage=0) < 0 and bwd(line_f4=8, stage=2) < 0
    for k in ("touched", "gacc", "tlist", "tcount"):
        assert bwd(**{k: None}) < 0, k
    for k in ("means", "view", "dL_dmean2D", "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dscale", "dL_drot", "scales", "rots"):
        assert bwd(stage=0, **{k: None}) < 0 and bwd(stage=2, **{k: None}) < 0, k
    assert bwd(stage=2, cov=p, dL_dcov3D=None) < 0
    assert bwd(P=0) == 0
    _sync()
    assert (b.read() == CULLED).all()                                       # nothing was launched
