"""What the tests of the three picked LIDARGS_DEPTH modes (median, strongest, second: csrc/switches.h DepthMode) share, each written once:
the float64 chain (`blend_table`, `reference`), the GPU harness (`with_env`, `Frame`, the refusing forwards, `start_children`, the pieces
of the fifth child), the bodies of the mode-independent tests (`check_*`) and the switch probe.  A plain helper module: the mode's own
rule, undecided bands, placed rays and scene lists are in tests/{median,strongest,second}_ref.py, the test functions in
tests/test_{median,strongest,second}_depth_{cpu,gpu}.py.

A RULE, as `reference` takes it, is an object with
    blend(idx, valid, dirs, conic, opac, colors, depth, u1, u2, sph, bg, e)   the float64 blend and the mode's table over the padded lists
    restate(f, scene, W, H)     the rule on the oracle's float32 records -> numpy planes, `decided` and `id_key` among them
    chosen(r, dist)             on blend's result r and the float64 ranges: (row of the picked Gaussian or -1 [N], its range or 0 [N])
    id_key                      the name of restate's id plane
"""
import os
import shutil
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

import preprocess_ref as pr

F64 = torch.float64
H = 16
SWITCH = "LIDARGS_DEPTH"
GAP = "LIDARGS_RETURN_GAP"
PLANS = {"fused_rows4": {"LIDARGS_FUSED": "1", "LIDARGS_TILE_ROWS": "4"}, "fused_rows32": {"LIDARGS_FUSED": "1", "LIDARGS_TILE_ROWS": "32"},
         "segmented_rows4": {"LIDARGS_FUSED": "0", "LIDARGS_TILE_ROWS": "4"}, "segmented_rows32": {"LIDARGS_FUSED": "0", "LIDARGS_TILE_ROWS": "32"}}
IMAGE_KEYS = ("color", "depth", "occ", "radii")
BUFFER_SCENE = "shell256"
CHILD_SECONDS = 300
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-gs_amd", "csrc")


# ---- the float64 chain --------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64), dtype=F64)


def oracle_forward(scene, W):
    from oracle import lgo
    return lgo.forward(scene["means3D"], scene["colors"], scene["opacities"], scene["scales"], scene["rotations"], scene["viewmatrix"],
                       scene["beams"], W, H, bg=scene["bg"])


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


def blend_table(idx, valid, dirs, conic, opac, colors, depth, u1, u2, sph, bg, e=None):
    """The per-pixel loop of the blend (R3/cr/forward.cu:578-637) over the padded lists, in float64 torch: what every rule starts from.
    conic [P,3], opac [P], colors [P,2], depth [P], u1 / u2 / sph [P,3] (u_i unscaled: d = delta . u_i / u_i . u_i); e: optional
    [N, L, 2] probe added to d (its gradient is the per-pair dL/dd).  -> dict: I, V, N, L; [N, L] power, raw, alpha, hit, T_incl (T behind
    the entry), T_excl (in front of it), taken, wgt; the images color [N, 2], expected, occ [N]."""
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
    return dict(I=I, V=V, N=N, L=L, power=power, raw=raw, alpha=alpha, hit=hit, T_incl=T_incl, T_excl=T_excl, taken=taken, wgt=wgt,
                opac=opac[I], color=col + T_fin[:, None] * bg, expected=D, occ=1.0 - T_fin)


def near_threshold(t, where, band):
    """[N, L]: entries of `where` whose alpha lies within `band` (relative) of 1/255, or whose power lies within it of 0 -- the entry is
    taken or not by rounding (tests/preprocess_ref.py's band)."""
    near_alpha = where & (t["power"] <= band) & ((t["raw"] * 255.0 - 1.0).abs() <= band)
    near_power = where & (t["power"].abs() <= band) & (t["opac"] * 255.0 >= 1.0 - band)
    return near_alpha | near_power


def restate_records(blend, f, scene, W, H, keep=()):
    """`blend` on the oracle's float32 record values.  -> numpy: every [N] tensor as [H, W], color as [2, H, W]; dicts named in `keep`
    (tables) with numpy values."""
    P = scene["means3D"].shape[0]
    idx, valid = pixel_lists(f, W, H)
    co = f.array("conic_opacity").reshape(P, 4)
    with torch.no_grad():
        r = blend(idx, valid, _t(pr.pixel_dirs(W, H, scene["beams"]).reshape(-1, 3)), _t(co[:, :3]), _t(co[:, 3]), _t(scene["colors"]),
                  _t(f.array("depths")), _t(f.array("basis_u1").reshape(P, 3)), _t(f.array("basis_u2").reshape(P, 3)),
                  _t(f.array("sphere").reshape(P, 3)), _t(scene["bg"]))
    out = {k: v.numpy().reshape(H, W) for k, v in r.items() if k != "color" and k not in keep}
    out["color"] = r["color"].numpy().T.reshape(2, H, W)
    for k in keep:
        out[k] = {kk: v.numpy() for kk, v in r[k].items()}
    return out


def undecided_fraction(r):
    """Undecided pixels as a fraction of the pixels that have a taker."""
    return float((~r["decided"] & r["has_taker"]).sum()) / max(1, int(r["has_taker"].sum()))


def reference(scene, W, H, grads, rule, f=None):
    """The float64 reference of a picked mode's forward + backward: K1's formulas (preprocess_ref.k1 + record, with the reference's damped
    conic gradient) in front of rule.blend, the depth output being the range of the Gaussian `rule` picks, leaves = means3D / scales /
    rotations / opacities / colours, upstream gradients `grads` = (dL_dcolor [2,H,W], dL_ddepth [1,H,W], dL_docc [1,H,W]) with
    dL_ddepth zeroed on undecided pixels.  Scale modifier 1.  -> dict: the restatement's planes (rule.restate), `fwd`, the forward's
    `depth`, `dL_ddepth_masked`, and the six gradient arrays named as util.GRAD_KEYS_SR."""
    if f is None:
        f = oracle_forward(scene, W)
    P = scene["means3D"].shape[0]
    rs = rule.restate(f, scene, W, H)
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
    r = rule.blend(remap[idx], valid, _t(pr.pixel_dirs(W, H, scene["beams"]).reshape(-1, 3)), rec["conic"], opac[sel], colors[sel], k["dist"],
                   k["u1"], k["u2"], k["dir"], _t(scene["bg"]), e)
    row, depth = rule.chosen(r, k["dist"])                                   # the float64 chain's own pick, on its own weights and ranges
    mine = np.where(row.numpy() >= 0, sel[row.clamp(min=0)].numpy(), -1)
    same = mine == rs[rule.id_key].ravel()
    assert same[rs["decided"].ravel()].all(), "the float64 chain and the oracle's float32 records disagree on a decided pixel"
    gc, gd, go = (_t(g) for g in grads)
    gd_masked = gd.reshape(-1) * torch.as_tensor(rs["decided"].ravel() & same, dtype=F64)
    loss = (r["color"].T.reshape(-1) * gc.reshape(-1)).sum() + (depth * gd_masked).sum() + (r["occ"] * go.reshape(-1)).sum()
    gm, gs, gq, gop, gcol, ge = torch.autograd.grad(loss, [means, scales, rots, opac, colors, e])
    g2 = np.zeros((P, 4))
    pair = ge.numpy()
    np.add.at(g2[:, 0], idx[valid], pair[valid][:, 0])
    np.add.at(g2[:, 1], idx[valid], pair[valid][:, 1])
    np.add.at(g2[:, 2], idx[valid], np.sqrt((pair[valid] ** 2).sum(-1)))      # the densification statistic: a sum of per-pixel norms
    out = dict(rs)
    out.update(fwd=f, depth=depth.detach().numpy().reshape(1, H, W), dL_ddepth_masked=gd_masked.numpy().reshape(1, H, W).astype(np.float32),
               dL_dmeans3D=gm.numpy(), dL_dmeans2D=g2, dL_dcolors=gcol.numpy(), dL_dopacity=gop.numpy().reshape(P, 1), dL_dscales=gs.numpy(),
               dL_drotations=gq.numpy())
    return out


def placed_layout(rays, W, sigma_rad, off):
    """Hand-placed rays {case: (x, y, [(range, opacity)])} (x = -1: the last column) as util.placed_scene's arguments: every Gaussian
    `sigma_rad` radians wide and off x sigma_rad beside the centre of its pixel, in azimuth.  -> scene, {case: (x, y, index of the ray's
    first Gaussian)}, {case: indices of the ray's Gaussians}."""
    from util import placed_scene
    pc, py, dist, op, first, members = [], [], [], [], {}, {}
    for case, (x, y, gs) in rays.items():
        x = W - 1 if x < 0 else x
        first[case] = (x, y, len(dist))
        for d, o in gs:
            pc.append(x + off * sigma_rad / (2 * np.pi / W)); py.append(float(y)); dist.append(d); op.append(o)
        members[case] = np.arange(first[case][2], len(dist))
    dist = np.array(dist)
    sigma = np.sqrt((sigma_rad * dist) ** 2 - 0.01)           # the 2-D covariance gets + 0.01 (R3/cr/forward.cu:166-167)
    return placed_scene(pc, py, dist, sigma, op, W, H), first, members


# ---- the GPU harness ----------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def with_env(depth, gap, fn):
    """fn() under LIDARGS_DEPTH = depth and LIDARGS_RETURN_GAP = gap (a string or a number; None: unset); both unset behind it."""
    for name, value in ((SWITCH, depth), (GAP, gap)):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value if isinstance(value, str) else f"{value:g}"
    try:
        return fn()
    finally:
        os.environ.pop(SWITCH, None)
        os.environ.pop(GAP, None)


class Frame:
    """A forward through the binding (`_C`), keeping the opaque buffers at hand so that a backward can be run on them, on clones of
    them, or again (as tests/test_deterministic_gpu.py does)."""

    def __init__(self, scene, W, grads):
        from diff_lidargs_rasterization import _C
        from util import to_torch
        self._C = _C
        self.scene, self.W = scene, W
        self.st = to_torch(self.scene)
        self.grads = [torch.from_numpy(np.ascontiguousarray(g)).cuda() for g in grads]
        self.empty = torch.empty(0, device="cuda")

    def forward(self):
        st, e = self.st, self.empty
        return self._C.rasterize_gaussians(st["bg"], st["means3D"], st["colors"], st["opacities"], st["scales"], st["rotations"], 1.0, e,
                                           st["viewmatrix"], st["viewmatrix"], H, self.W, st["beams"], e, 1, e, False, 80, 0, False)

    def backward(self, fwd, clone=False):
        st, e = self.st, self.empty
        R, radii, geom, binning, img = fwd[0], fwd[4], fwd[5], fwd[6], fwd[7]
        if clone:
            radii, geom, binning, img = (t.clone() for t in (radii, geom, binning, img))
        g = self._C.rasterize_gaussians_backward(st["bg"], st["means3D"], radii, st["colors"], st["scales"], st["rotations"], 1.0, e,
                                                 st["viewmatrix"], st["viewmatrix"], st["beams"], 1.0, 1.0, *self.grads, e, 1, e,
                                                 geom, R, binning, img, False)
        return {k: g[i].cpu().numpy() for k, i in (("dL_dmeans2D", 0), ("dL_dcolors", 1), ("dL_dopacity", 2), ("dL_dmeans3D", 3), ("dL_dscales", 6),
                                                   ("dL_drotations", 7))}

    def sizes(self, fwd):
        """Bytes of the geometry, binning and image buffers."""
        return np.array([int(t.numel()) for t in fwd[5:8]], np.int64)

    def images(self, fwd):
        return {k: fwd[i].cpu().numpy() for k, i in (("color", 1), ("depth", 2), ("occ", 3), ("radii", 4))}

    def id_plane(self, fwd, n_img):
        """The id plane of a picked forward's image buffer as uint32 words, `n_img` being the size of a default forward's image buffer
        (lidargs_common.h img_carve: the plane starts at the next 128-byte boundary).  Shorter than H x W words where the forward asked
        for no plane: the tests say so."""
        off = (n_img - 128 + 127) // 128 * 128
        p = fwd[7][off:off + 4 * H * self.W].cpu().numpy()
        return p[:p.size // 4 * 4].view(np.uint32)

    def backward_rounds(self, on, res):
        """With both variables unset (the mode travels in the buffers, the gap nowhere): backward on the picked forward `on`, again, and
        on clones; a default forward in a process that has made such buffers, its backward, and that on clones; `on` once more behind
        them.  Gradients into `res`; -> the default forward."""
        for what, fn in (("first", lambda: self.backward(on)), ("second", lambda: self.backward(on)), ("cloned", lambda: self.backward(on, clone=True))):
            res.update({f"{what}.{k}": v for k, v in fn().items()})
        off_again = self.forward()
        res.update({f"default_after.{k}": v for k, v in self.backward(off_again).items()})
        res.update({f"default_after_cloned.{k}": v for k, v in self.backward(off_again, clone=True).items()})
        res.update({f"third.{k}": v for k, v in self.backward(on).items()})
        return off_again


def _surfel_forward(scene, W):
    from util import hip_surfel_forward_backward, surfel_scene
    return hip_surfel_forward_backward(surfel_scene("street", 2000, 16, 93), 256, 16)["color"]


def _sharded_forward(cls):
    import lidargs_dist
    import lidargs_scenes as sc
    from util import make_settings, to_torch
    st = to_torch(sc.make_scene("shell", 2000, 16, 94, random_view=True))
    mod = cls(make_settings(st, 256, 16), lidargs_dist.SingleComm())
    means2D = torch.zeros((2000, 4), device="cuda")
    return mod(st["means3D"], means2D, st["opacities"], st["colors"], st["scales"], st["rotations"])[0].cpu().numpy()


def _shell_forward(scene, W):
    import lidargs_dist
    return _sharded_forward(lidargs_dist.ShellRasterizer)


def _wedge_forward(scene, W):
    import lidargs_dist
    return _sharded_forward(lidargs_dist.WedgeRasterizer)


def _enqueue_only_forward(scene, W):
    """Two frames: the module's first frame is an ordinary lidargs_forward that teaches it its capacity, the second is enqueue-only.
    The switch is set for the second only."""
    import lidargs_scenes as sc
    from diff_lidargs_rasterization import GaussianRasterizer
    from util import make_settings, to_torch
    st = to_torch(sc.make_scene("street", 2000, 16, 95, random_view=True))
    rast = GaussianRasterizer(make_settings(st, 256, 16))
    rast.enqueue_only = True
    want = os.environ.pop(SWITCH, None)
    out = None
    for i in range(2):
        if i == 1 and want is not None:
            os.environ[SWITCH] = want
        out = rast(means3D=st["means3D"], means2D=torch.zeros((2000, 4), device="cuda"), opacities=st["opacities"], colors_precomp=st["colors"],
                   scales=st["scales"], rotations=st["rotations"])
    assert rast._enqueue.frames == 1
    return out[0].cpu().numpy()


def _deterministic_and_median(scene, W):
    """lidargs_forward on the caller's scene under LIDARGS_DETERMINISTIC=1 (the other refusing forwards have scenes of their own)."""
    from util import hip_forward_backward
    os.environ["LIDARGS_DETERMINISTIC"] = "1"
    try:
        return hip_forward_backward(scene, W, H)["color"]
    finally:
        del os.environ["LIDARGS_DETERMINISTIC"]


# case: forward(scene, W) -- one signature for refusals(); all but the last have scenes of their own and ignore the arguments
REFUSING = {"surfel": _surfel_forward, "shell_world_of_one": _shell_forward, "wedge_world_of_one": _wedge_forward,
            "enqueue_only": _enqueue_only_forward, "deterministic_and_median": _deterministic_and_median}
ENTRY = {"surfel": "lidargs_surfel_forward", "shell_world_of_one": "lidargs_forward_shell", "wedge_world_of_one": "lidargs_forward_wedge",
         "enqueue_only": "lidargs_forward_enqueue", "deterministic_and_median": "lidargs_forward"}


def refusals(depth, gap, res, scene, W):
    """Every refusing forward without the switch, under it (the error's text, or "no error"), and without it again -> res["refusal.<case>"].
    Every entry of REFUSING takes (scene, W); only the deterministic case, which is lidargs_forward itself, renders them."""
    for case, fn in REFUSING.items():
        forward = lambda: fn(scene, W)
        ok_before = bool(np.isfinite(with_env(None, None, forward)).all()) if case != "deterministic_and_median" else True
        try:
            with_env(depth, gap, forward)
            msg = "no error"
        except RuntimeError as e:
            msg = "RuntimeError: " + str(e)
        ok_after = bool(np.isfinite(with_env(None, None, forward)).all())
        res[f"refusal.{case}"] = np.array([msg, str(ok_before), str(ok_after)])


def start_children(module, refs_path, d):
    """The five children of test module `module` side by side, each under its own time limit: child_plan under each of PLANS and
    child_buffers, with (refs_path, output file) as arguments and both variables unset.  -> {plan: arrays, "buffers": arrays}."""
    from util import run_child
    code = f"import os\nos.environ.pop({SWITCH!r}, None)\nos.environ.pop({GAP!r}, None)\nimport {module} as t\nt.%s(sys.argv[1], sys.argv[2])"
    jobs = {plan: (code % "child_plan", env) for plan, env in PLANS.items()}
    jobs["buffers"] = (code % "child_buffers", {})
    outs = {k: str(d / f"{k}.npz") for k in jobs}
    with ThreadPoolExecutor(len(jobs)) as pool:
        fut = [pool.submit(run_child, body, env, (refs_path, outs[k]), CHILD_SECONDS) for k, (body, env) in jobs.items()]
        for f in fut:
            f.result()
    return {k: dict(np.load(o)) for k, o in outs.items()}


def child_plan(mod, mode, refs, out, also=None):
    """One child process of a mode that has one rule per scene (mod = median_ref or strongest_ref): every scene's forward + backward
    under LIDARGS_DEPTH = mode and in the default mode, with the reference's masked depth gradient and with none (key suffix 0: the
    scene's second forward under the mode).  also(name, scene, W) -> further arrays of the scene."""
    from util import GRAD_KEYS_SR, hip_forward_backward
    assert SWITCH not in os.environ
    up = np.load(refs)
    res = {}
    for name in mod.SCENES:
        scene, W = mod.scene(name)
        masked = (up[f"{name}.gc"], up[f"{name}.gd_masked"], up[f"{name}.go"])
        nodepth = (masked[0], np.zeros_like(masked[1]), masked[2])
        for tag, value in ((mode, mode), ("default", None)):
            for suffix, grads in (("", masked), ("0", nodepth)):
                r = with_env(value, None, lambda: hip_forward_backward(scene, W, H, grads))
                res.update({f"{name}.{tag}{suffix}.{k}": r[k] for k in IMAGE_KEYS + GRAD_KEYS_SR})
        if also:
            res.update(also(name, scene, W))
    np.savez(out, **res)
    print("OK")


def child_buffers(mod, mode, rejected, other_modes, refs, out):
    """The fifth child of such a mode: buffer sizes (`rejected`: values of the switch that ask for the default mode; `other_modes`: picked
    modes whose sizes must be the same), the id plane, backward twice / on clones with the variable unset, a default forward's backward
    in a process that has made median buffers, and the refusals."""
    assert SWITCH not in os.environ
    up = np.load(refs)
    name = BUFFER_SCENE
    fr = Frame(*mod.scene(name), (up[f"{name}.gc"], up[f"{name}.gd_masked"], up[f"{name}.go"]))
    res = {}
    plain = fr.forward()
    res["sizes_never_set"] = fr.sizes(plain)
    res["never_set.depth"] = plain[2].cpu().numpy()
    res.update({f"before.{k}": v for k, v in fr.backward(plain).items()})     # (no picked forward yet in this process: the default launches)
    for value in rejected:
        res[f"sizes[{value}]"] = with_env(value, None, lambda: fr.sizes(fr.forward()))
    on = with_env(mode, None, fr.forward)
    res["sizes_switch_on"] = fr.sizes(on)
    res[f"{mode}.depth"] = on[2].cpu().numpy()
    res[f"{mode}_id"] = fr.id_plane(on, int(res["sizes_never_set"][2]))
    res["sizes_set_and_unset"] = fr.sizes(fr.backward_rounds(on, res))         # the variable is unset from here on: the mode travels in the buffers
    for other in other_modes:
        res[f"sizes_{other}"] = with_env(other, None, lambda: fr.sizes(fr.forward()))
    refusals(mode, None, res, *mod.scene("shell64"))
    np.savez(out, **res)
    print("OK")


def scene_refs(mod, d):
    """The `refs` of a mode that has one rule per scene (mod = median_ref or strongest_ref).  Per scene of mod.SCENES: the restatement and
    the float64 reference gradients for upstream gradients whose depth part is masked on undecided pixels (`ref`), the CPU oracle's
    default-mode backward for the same upstream gradients without a depth part with its exact sums (`oracle0`, `oracle0_64`), and on
    mod.BACKWARD_SCENES the float64 reference for those (`ref0`).  Computed once; "path": the upstream gradients for the children, a
    file in directory `d`."""
    from util import oracle_backward_exact_sums, oracle_forward_backward
    out, up = {}, {}
    for name in mod.SCENES:
        scene, W = mod.scene(name)
        gc, gd, go = mod.upstream(name)
        ref = reference(scene, W, H, (gc, gd, go), mod.RULE)
        nodepth = (gc, np.zeros_like(gd), go)
        ora = oracle_forward_backward(scene, W, H, nodepth)
        ora64 = oracle_backward_exact_sums(ora, nodepth)
        ref0 = reference(scene, W, H, nodepth, mod.RULE, f=ref["fwd"]) if name in mod.BACKWARD_SCENES else None
        out[name] = dict(scene=scene, W=W, ref=ref, ref0=ref0, oracle0=ora, oracle0_64=ora64)
        up.update({f"{name}.gc": gc, f"{name}.gd_masked": ref["dL_ddepth_masked"], f"{name}.go": go})
    out["path"] = str(d / "upstream.npz")
    np.savez(out["path"], **up)
    return out


def miss_detail(r, name, entry):
    """For check_backward_against_float64, where the budget is missed: the same count for the default mode's backward of the same child
    without a depth gradient (no code of the picked modes runs there) and for the float32 CPU oracle, each against its own float64
    reference (`entry` = scene_refs()[name])."""
    return lambda k, over: (f" in this mode, default mode without a depth gradient {over(r[f'{name}.default0.{k}'], entry['ref0'][k])}, "
                            f"CPU oracle {over(entry['oracle0'][k], entry['ref0'][k])}")


# ---- the bodies of the tests that do not depend on the mode: `r` a plan's arrays, `b` the fifth child's, `on` / `on0` the key prefixes of
# ---- the picked forward + backward with the masked depth gradient / with none, `default0` that of the default mode with none --------
def check_decided_pixels_return_the_restatements_range(label, got, ref, want, has):
    """Every decided pixel is held to RTOL against the range of the restatement's Gaussian (a wrong neighbour differs by metres, which
    no tolerance hides; none is excused), 0 where `has` says the rule picks nothing; at least 98 % of the pixels with a taker decide."""
    from util import FLOOR, RTOL
    dec = ref["decided"]
    assert dec.sum() >= 0.98 * ref["has_taker"].sum()
    err = np.abs(got[dec] - want[dec]) / (np.abs(want[dec]) + FLOOR * np.abs(want[dec]).max())
    print(f"{label}: decided pixels {int(dec.sum())} of {dec.size}, worst error {err.max():.2e}, wrong Gaussians: {int((err > 1e-3).sum())}")
    assert err.max() <= RTOL, f"{label}: {int((err > RTOL).sum())} decided pixels return another range than the restatement's Gaussian's"
    assert (got[~has & dec] == 0).all()


def check_backward_against_float64(label, r, on, ref, detail=None):
    """All six gradient arrays against `ref` (reference): util.parity, default tolerances.  detail(k, over): more for the message of a miss."""
    from util import FLOOR, GRAD_KEYS_SR, RTOL, parity
    over = lambda got, want: int((np.abs(got - want) / (np.abs(want) + FLOOR * np.abs(want).max() + 1e-30) > RTOL).sum())
    failed = []
    for k in GRAD_KEYS_SR:
        try:
            parity(f"{label}.{k}", r[f"{on}.{k}"], ref[k])
        except AssertionError as e:
            failed.append(f"{e} [entries over {RTOL:g}: {over(r[f'{on}.{k}'], ref[k])}{detail(k, over) if detail else ''}]")
    assert not failed, failed


def check_no_depth_gradient_gives_the_default_backward(label, r, on0, default0, oracle64):
    from util import GRAD_KEYS_SR, parity_or_closer
    for k in GRAD_KEYS_SR:
        parity_or_closer(f"{label}.{k} (no depth gradient)", r[f"{on0}.{k}"], r[f"{default0}.{k}"], oracle64[k])


def check_depth_gradient_lands_on_one_gaussian(label, r, on, on0, ref, id_key, oracle64):
    """on - on0 is the depth part alone: dL/dmeans3D rows differ exactly for the Gaussians that are some decided pixel's pick with a
    non-zero upstream gradient (one Gaussian per pixel), and colours / opacities carry none of it."""
    from util import parity_or_closer
    gd = ref["dL_ddepth_masked"][0]
    ok = (ref[id_key] >= 0) & (gd != 0)
    want = np.zeros(ref["dL_dmeans3D"].shape[0])
    np.add.at(want, ref[id_key][ok], gd[ok].astype(np.float64))
    part = r[f"{on}.dL_dmeans3D"].astype(np.float64) - r[f"{on0}.dL_dmeans3D"]
    moved = np.abs(part).max(1)
    scale = np.abs(r[f"{on0}.dL_dmeans3D"]).max(1) + np.abs(want)
    assert not (moved[want == 0] > 1e-3 * (scale[want == 0] + 1e-6)).any(), label
    big = np.abs(want) > 1e-2 * np.abs(want).max()
    assert (moved[big] > 0).all() and big.sum() >= 20, label
    np.testing.assert_allclose(np.linalg.norm(part, axis=1)[big], np.abs(want[big]), rtol=2e-2)   # |d range / d mean| = 1 (differences of float32 sums)
    for k in ("dL_dcolors", "dL_dopacity"):
        parity_or_closer(f"{label}.{k} (depth part)", r[f"{on}.{k}"], r[f"{on0}.{k}"], oracle64[k])


def check_id_plane(label, plane, ref, id_key):
    """The id plane names the restatement's Gaussian on every decided pixel (0xFFFFFFFF read as -1).  -> the plane as int64 [H, W]."""
    dec = ref["decided"]
    assert plane.size == dec.size, "the image buffer has no id plane"
    ids = plane.astype(np.int64).reshape(dec.shape)
    ids[ids == 0xFFFFFFFF] = -1
    assert dec.sum() >= 0.98 * ref["has_taker"].sum()
    wrong = int((ids[dec] != ref[id_key][dec]).sum())
    print(f"{label}: decided pixels {int(dec.sum())}, other Gaussian than the restatement's: {wrong}")
    assert wrong == 0
    return ids


def check_buffer_sizes(never_set, on, others_on, like_default, n_pixels):
    """Only the image buffer grows, by the id plane (4 B per pixel, plus alignment); `others_on` (the other picked modes' sizes) are the
    same; every forward of `like_default` {what: sizes} asks for the default sizes."""
    extra = on - never_set
    assert extra[0] == 0 and extra[1] == 0 and 4 * n_pixels <= extra[2] <= 4 * n_pixels + 256, extra
    for other in others_on:
        assert (on == other).all()
    for what, sizes in like_default.items():
        assert (sizes == never_set).all(), what


def check_backward_twice_and_on_clones(b, ref):
    """Backward, backward again and backward on clones of every saved tensor, the variables unset -- all the reference's gradients, and
    each other's within the run-to-run band."""
    from util import GRAD_KEYS_SR, parity
    for k in GRAD_KEYS_SR:
        for what in ("first", "second", "cloned", "third"):
            parity(f"buffers.{what}.{k}", b[f"{what}.{k}"], ref[k], verbose=False)
        for what in ("second", "cloned", "third"):
            parity(f"buffers.{what} against first.{k}", b[f"{what}.{k}"], b[f"first.{k}"], verbose=False)
    assert np.abs(b["first.dL_dmeans3D"] - b["before.dL_dmeans3D"]).max() > 1e-2 * np.abs(b["first.dL_dmeans3D"]).max()   # (the modes do differ)


def check_default_buffer_after_a_picked_forward(b, scene, W, grads):
    """The buffer's mode bit decides, not the process: a default forward's backward after the process has made median buffers (its
    backward now asks the mode word and queues the median add, which must retire) is the default backward of before -- the CPU oracle's
    gradients for the same upstream gradients, depth part included; on the buffers and on clones of them."""
    from util import GRAD_KEYS_SR, oracle_backward_exact_sums, oracle_forward_backward, parity_or_closer
    ora = oracle_forward_backward(scene, W, H, grads)
    ora64 = oracle_backward_exact_sums(ora, grads)
    for k in GRAD_KEYS_SR:
        for what in ("before", "default_after", "default_after_cloned"):
            parity_or_closer(f"buffers.{what}.{k}", b[f"{what}.{k}"], ora[k], ora64[k])
        parity_or_closer(f"buffers.default_after against before.{k}", b[f"default_after.{k}"], b[f"before.{k}"], ora64[k])


def check_refusal(case, b):
    """A RuntimeError naming the variable and the entry point.  Without the switch the forward runs, before and after."""
    msg, ok_before, ok_after = b[f"refusal.{case}"]
    assert msg.startswith("RuntimeError") and SWITCH in msg and ENTRY[case] in msg, msg
    assert ok_before == "True" and ok_after == "True"


# ---- the switch probe: csrc/switches.h as a plain C++ program -----------------------------------------------------------------------
PROBE = r"""
#include <stdio.h>
#include <string.h>
#include "switches.h"
int main() {
    const float g = lg::return_gap();
    unsigned bits;
    memcpy(&bits, &g, 4);
    printf("%s %08x\n", lg::DEPTH_MODE_NAMES[(int)lg::depth_mode()], bits);
    return 0;
}
"""
# value of LIDARGS_DEPTH: the mode, as the probe prints lg::depth_mode() and as the Python package's depth_mode() returns it -- the cases of
# all three modes' tests.  Only the literal names select a mode; `picked` is mode != "expected".
DEPTH_CASES = {None: "expected", "": "expected", "median": "median", "strongest": "strongest", "second": "second", "Median": "expected",
               "Strongest": "expected", "Second": "expected", "median ": "expected", "strongest ": "expected", "second ": "expected",
               "1": "expected", "2": "expected", "expected": "expected", "seconds": "expected", "secon": "expected"}
FLT_MAX = "340282346638528859811704183484516925440"
FIRST_INFINITE = "340282356779733661637539395458142568448"       # 2^128 - 2^103: from here on the nearest float32 is infinity
# value of LIDARGS_RETURN_GAP: the gap in metres (as a float32)
GAP_CASES = {None: 0.0, "": 0.0, "0": 0.0, "0.505": 0.505, ".5": 0.5, "2.": 2.0, "1e0": 0.0, "-1": 0.0, "+1": 0.0, "0.5 ": 0.0, " 0.5": 0.0,
             "nan": 0.0, "inf": 0.0, "1,5": 0.0, "7" * 400: 0.0, ".": 0.0, "0x10": 0.0, "1_0": 0.0, "007.250": 7.25, "1.5.2": 0.0,
             "0." + "0" * 400 + "1": 0.0, FLT_MAX: 3.4028234663852886e38, FIRST_INFINITE: 0.0, FLT_MAX + ".5": 3.4028234663852886e38}


def float32_bits(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", np.float32(x)))[0]


def build_probe(tmp_path_factory, name="plain"):
    """The probe under -Wall -Wextra -Werror: "plain", or "sanitized" with the address and undefined-behaviour sanitizers -- host code in
    a program of its own, their runtimes linked statically (as tests/test_switches_cpu.py builds its probe).  Each is built when first
    asked for, once per session.  -> the executable, or None without g++."""
    gxx = shutil.which("g++")
    if not gxx:
        return None
    d = tmp_path_factory.getbasetemp() / "depth_probe"
    exe = str(d / name)
    if not os.path.exists(exe):
        d.mkdir(exist_ok=True)
        (d / "probe.cpp").write_text(PROBE)
        sanitize = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
        flags = ["-O1"] + (sanitize if name == "sanitized" else [])
        subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, str(d / "probe.cpp"), "-o", exe + ".tmp"], check=True)
        os.replace(exe + ".tmp", exe)
    return exe


def probe(exe, depth, gap):
    """-> [mode name, the gap's bits] as the probe prints them under LIDARGS_DEPTH = depth, LIDARGS_RETURN_GAP = gap (None: unset)."""
    env = {k: v for k, v in os.environ.items() if k not in (SWITCH, GAP)}
    if depth is not None:
        env[SWITCH] = depth
    if gap is not None:
        env[GAP] = gap
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (depth, gap, r.stderr[-3000:])
    return r.stdout.split()
