"""The two per-Gaussian stages of csrc/preprocess.hip restated in float64, vectorised over Gaussians (torch on the CPU, numpy for the
integer part).  tests/test_preprocess_cpu.py holds this file against the oracle without a GPU; tests/test_preprocess_gpu.py holds the
HIP kernels against it.

  forward    `k1` (R3/cr/forward.cu:216-253, :95-119, :146-169, :298-322) and `k1_one`, the same for one Gaussian exactly as the source
             writes it (GLM matrices; moved here from tests/test_oracle_autograd_cpu.py, which still differentiates it);
             `record`: what the splat record holds on top (u_i' = u_i / (u_i . u_i), the conic);
             `geometry`: p_c, p_r, the beam bisection, rx, ry, the reference rect and the cull rules in the kernel's order (:304-368).
  takers     `takers`: the pixels of a Gaussian's reference rect that blend it (R3/cr/forward.cu:589-606).
  backward   `chain`: the VJP of `k1` + `record` by torch.autograd, fed the cotangents the packed gradient line carries, with the
             reference's three deliberate deviations from the analytic gradient (R3/cr/backward.cu:237, :428-432, :440-447).
             Run in torch.float32 it is the yardstick of the HIP chain: a second fp32 evaluation in another operation order.
"""
import math

import numpy as np
import torch

F64 = torch.float64
PI_F = float(np.float32(math.pi))                       # the kernels' pi is the float
GUARD = float(np.float32(0.002) * np.float32(2.0))      # Ray_Divergence_Angle * 2 (R3/cr/forward.cu:22, :347, :356)
ALPHA_MIN = 1.0 / 255.0
UNDECIDED = 1e-3                                        # pixels with alpha within this (relative) of 1/255 are nobody's evidence

CULL_NONE, CULL_PADDING, CULL_RANGE, CULL_SHELL, CULL_DET, CULL_GUARD, CULL_RECT = range(7)


def _mat3_cols(*c):
    """glm::mat3(a, b, c, d, e, f, g, h, i): consecutive triples are COLUMNS -> math matrix [row, col]."""
    return torch.stack([torch.stack(c[0:3]), torch.stack(c[3:6]), torch.stack(c[6:9])], 1)


def k1_one(means3D, scales, rotations, vm, mod=1.0):
    """preprocessCUDA's per-Gaussian outputs for one Gaussian, as written (R3/cr/forward.cu:216-253, :95-119, :146-169, :298-322, :369-372).
    Returns (conic [3], dist, u1 [3], u2 [3], sphere [3], (a, b, c))."""
    p = means3D
    pv = torch.stack([vm[0] * p[0] + vm[4] * p[1] + vm[8] * p[2] + vm[12], vm[1] * p[0] + vm[5] * p[1] + vm[9] * p[2] + vm[13],
                      vm[2] * p[0] + vm[6] * p[1] + vm[10] * p[2] + vm[14]])                   # transformPoint4x3, auxiliary.h:94-102
    dist = torch.sqrt((pv * pv).sum())
    one, zero = torch.ones((), dtype=F64), torch.zeros((), dtype=F64)
    S = torch.diag(torch.stack([mod * scales[0], mod * scales[1], mod * scales[2]]))
    r, x, y, z = rotations
    R = _mat3_cols(1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                   2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                   2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y))
    M = S @ R
    Sigma = M.T @ M                                                                        # :244
    dirv = pv / dist                                                                       # normalize_f3
    u1 = torch.stack([dirv[1], -dirv[0], zero]); u1 = u1 / torch.sqrt((u1 * u1).sum())
    u2 = torch.stack([dirv[1] * u1[2] - dirv[2] * u1[1], dirv[2] * u1[0] - dirv[0] * u1[2], dirv[0] * u1[1] - dirv[1] * u1[0]])
    Pm = _mat3_cols(u1[0], u1[1], u1[2], u2[0], u2[1], u2[2], zero, zero, zero)
    Wm = _mat3_cols(vm[0], vm[4], vm[8], vm[1], vm[5], vm[9], vm[2], vm[6], vm[10])
    Tm = Wm @ Pm
    cov = Tm.T @ Sigma.T @ Tm                                                              # :162
    a = (cov[0, 0] + 0.01) / (dist * dist); b = cov[1, 0] / (dist * dist); c = (cov[1, 1] + 0.01) / (dist * dist)   # cov[0][1] = column 0, row 1
    abc = torch.stack([a, b, c])
    return abc, dist, u1, u2, pv / dist, one


# ---- forward, vectorised ------------------------------------------------------------------------------------------------------------
def cov6_of(sm, rots):
    """computeCov3D (R3/cr/forward.cu:216-253) on the MODIFIED scales sm [P,3] and the quaternions as they are (not normalised, :228):
    Sigma = sum_k sm_k^2 r_k r_k^T with r_k the k-th ROW of the GLM matrix; the packed upper triangle [P,6]."""
    r, x, y, z = rots.unbind(-1)
    rows = [torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)], -1),
            torch.stack([2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)], -1),
            torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], -1)]
    S = sum((sm[:, k, None, None] ** 2) * rows[k][:, :, None] * rows[k][:, None, :] for k in range(3))
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1)


def _sym(c6):
    return torch.stack([torch.stack([c6[:, 0], c6[:, 1], c6[:, 2]], -1), torch.stack([c6[:, 1], c6[:, 3], c6[:, 4]], -1),
                        torch.stack([c6[:, 2], c6[:, 4], c6[:, 5]], -1)], 1)


def k1(means, cov6, vm):
    """The vectorised k1_one behind the covariance: means [P,3], cov6 [P,6], vm the 16 floats of the transposed world->lidar matrix.
    -> dict(pv, dist, dir, u1, u2, abc): abc = the 2x2 footprint (a, b, c) in the tangent plane, low-passed and over dist^2."""
    V = vm.reshape(4, 4)
    pv = means @ V[:3, :3] + V[3, :3]                                   # pv[k] = sum_r vm[4 r + k] p[r] + vm[12 + k]
    dist = torch.sqrt((pv * pv).sum(-1))
    d = pv / dist[:, None]
    zero = torch.zeros_like(dist)
    u1 = torch.stack([d[:, 1], -d[:, 0], zero], -1)
    u1 = u1 / torch.sqrt((u1 * u1).sum(-1))[:, None]
    u2 = torch.linalg.cross(d, u1)
    t1, t2 = u1 @ V[:3, :3].T, u2 @ V[:3, :3].T                          # world-space tangents: t[r] = sum_k vm[4 r + k] u[k]
    S = _sym(cov6)
    St1, St2 = torch.einsum("pij,pj->pi", S, t1), torch.einsum("pij,pj->pi", S, t2)
    d2 = dist * dist
    a = ((t1 * St1).sum(-1) + 0.01) / d2; b = (t1 * St2).sum(-1) / d2; c = ((t2 * St2).sum(-1) + 0.01) / d2
    return dict(pv=pv, dist=dist, dir=d, u1=u1, u2=u2, abc=torch.stack([a, b, c], -1))


def record(k, damped=False):
    """What the splat record holds on top of k1: conic (A, B, C) = (c, -b, a) / det and the scaled bases u_i' = u_i / (u_i . u_i).
    damped: the gradient that reaches (a, b, c) through the conic's 1 / det^2 is formed with 1 / (det^2 + 1e-7), the reference's one
    substitution (R3/cr/backward.cu:237) -- a scale on the gradient, the values are unchanged."""
    abc = k["abc"]
    if damped:
        det = abc[:, 0] * abc[:, 2] - abc[:, 1] * abc[:, 1]
        s = (det * det / (det * det + 1e-7)).detach()[:, None]
        abc = abc * s + (abc * (1 - s)).detach()
    a, b, c = abc.unbind(-1)
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], -1)
    u1p = k["u1"] / (k["u1"] * k["u1"]).sum(-1)[:, None]
    u2p = k["u2"] / (k["u2"] * k["u2"]).sum(-1)[:, None]
    return dict(conic=conic, det=det, u1p=u1p, u2p=u2p)


def forward64(means, scales, rots, vm, mod=1.0, cov3D=None):
    """k1 + record in float64 from numpy inputs; numpy float64 outputs."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=F64)
    with np.errstate(all="ignore"):
        c6 = t(cov3D) if cov3D is not None else cov6_of(float(np.float32(mod)) * t(scales), t(rots))
        k = k1(t(means), c6, t(np.asarray(vm).reshape(16)))
        k.update(record(k))
    return {n: v.numpy() for n, v in k.items()}


def steps(W):
    """The column steps a forward derives from the image width (csrc/api.hip preprocess_params), as the float32 values the kernel gets."""
    col_step = np.float32(2) * np.float32(PI_F) / np.float32(W)
    return float(col_step), float(np.float32(math.tan(float(col_step))))


def bisect_beam(beams, alpha):
    """find_closest_label (R3/cr/auxiliary.h:41-63): clamp at the ends, else the first beam >= alpha."""
    H = beams.size
    bi = np.searchsorted(beams, alpha, side="left")
    bi = np.where(alpha >= beams[H - 1], H - 1, np.where(alpha <= beams[0], 0, bi))
    return bi.astype(np.int64)


def _round_half_away(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def geometry(f, beams, W, H, near=0.0, far=80.0, shell=(-np.inf, np.inf), n_valid=None, band=1e-5):
    """From forward64's arrays: the image position, the radii, the reference rect in 16 x 1 tiles (R3/cr/auxiliary.h:80-92) and which
    cull rule removes the Gaussian, in the order the kernel applies them.  `near_boundary` marks Gaussians whose float64 3r/tan,
    (p_c -+ rx) / 16 or p_r -+ ry lie within `band` (relative) of the integer / half-integer their rounding turns at."""
    beams = np.asarray(beams, np.float64)
    P = f["dist"].size
    pv, dist, abc = f["pv"], f["dist"], f["abc"]
    col_step, tan_col = steps(W)
    tiles_x = (W + 15) // 16
    with np.errstate(all="ignore"):
        det = abc[:, 0] * abc[:, 2] - abc[:, 1] * abc[:, 1]
        mid = 0.5 * (abc[:, 0] + abc[:, 2])
        disc = np.sqrt(np.maximum(1e-9, mid * mid - det))                  # :328-330
        lam = np.maximum(mid + disc, mid - disc)
        radius = np.sqrt(np.where(lam > 1e-9, lam, 1e-9))
        p_c = (PI_F - np.arctan2(pv[:, 1], pv[:, 0])) / col_step          # :333-334
        alpha = np.arctan2(pv[:, 2], np.sqrt(pv[:, 0] ** 2 + pv[:, 1] ** 2))
        alpha_s = np.where(np.isfinite(alpha), alpha, 0.0)
        bi = bisect_beam(beams, alpha_s)
        up = bi > 0
        before = np.where(up, beams[np.maximum(bi - 1, 0)], beams[0]); after = np.where(up, beams[bi], beams[1])
        p_r = np.where(up, (bi - 1) + (alpha_s - before) / (after - before), 1 + (alpha_s - after) / (after - before))
        off_fan = np.where(up, alpha_s > after + GUARD, alpha_s < before - GUARD)   # :347, :356
        p_r = H - p_r - 1.0
        qy = 3.0 * radius / np.tan(np.abs(after - before)); qx = 3.0 * radius / tan_col      # :361-362
        ry = np.ceil(qy); rx = np.ceil(qx)
        ex0, ex1 = (p_c - rx) / 16.0, (p_c + rx + 15.0) / 16.0
        ey0, ey1, eyc = p_r - ry, p_r + ry, p_r
        xmin = np.clip(np.trunc(ex0), 0, tiles_x); xmax = np.clip(np.trunc(ex1), 0, tiles_x)
        ymin = np.clip(_round_half_away(ey0), 0, H); ymax = np.clip(np.maximum(_round_half_away(ey1), _round_half_away(eyc) + 1.0), 0, H)
        near_int = lambda v: np.abs(v - np.round(v)) <= band * np.maximum(1.0, np.abs(v))
        near_half = lambda v: near_int(v + 0.5)
        near_boundary = near_int(qx) | near_int(qy) | near_int(ex0) | near_int(ex1) | near_half(ey0) | near_half(ey1) | near_half(eyc)
    cull = np.full(P, CULL_NONE)

    def rule(code, cond):                                                   # the first rule that applies names the cull
        cull[(cull == CULL_NONE) & cond] = code

    if n_valid is not None:
        rule(CULL_PADDING, np.arange(P) >= n_valid)
    rule(CULL_RANGE, ~((dist < far) & (dist > near)))                      # :304 (a NaN range passes the kernel's two tests and fails its shell test)
    rule(CULL_SHELL, ~((dist >= shell[0]) & (dist < shell[1])))
    rule(CULL_DET, det == 0.0)
    rule(CULL_GUARD, off_fan)
    rule(CULL_RECT, ~((xmax - xmin) * (ymax - ymin) > 0))
    live = cull == CULL_NONE
    i = lambda v: np.where(live, np.nan_to_num(v), 0).astype(np.int64)
    return dict(p_c=p_c, p_r=p_r, alpha=alpha, bi=bi, rx=i(rx), ry=i(ry), rect=np.stack([i(xmin), i(ymin), i(xmax), i(ymax)], 1), cull=cull, live=live,
                near_boundary=near_boundary & live, radius=radius)


# ---- takers -------------------------------------------------------------------------------------------------------------------------
def pixel_dirs(W, H, beams):
    """R3/cr/forward.cu:589-591: alp = beams[H-1-y], beta = -(x - W/2)/W * 2 pi, (cos a cos b, cos a sin b, sin a) -> [H, W, 3]."""
    alp = np.asarray(beams, np.float64)[H - 1 - np.arange(H)][:, None]
    beta = (-(np.arange(W, dtype=np.float64) - W / 2.0) / W * 2.0 * PI_F)[None, :]
    return np.stack([np.cos(alp) * np.cos(beta), np.cos(alp) * np.sin(beta), np.sin(alp) * np.ones_like(beta)], -1)


def pair_alpha(f, opacities, dirs, g, xs, ys):
    """power and alpha of Gaussian g at the pixels (xs, ys), as renderCUDA forms them (R3/cr/forward.cu:592-604); a NaN opacity blends at
    0.99 (min(0.99f, NaN))."""
    delta = f["dir"][g] - dirs[ys, xs]
    dx = delta @ f["u1p"][g]; dy = delta @ f["u2p"][g]
    A, B, C = f["conic"][g]
    power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
    op = float(opacities[g])
    alpha = np.full_like(power, 0.99) if math.isnan(op) else op * np.exp(power)
    return power, alpha


def takers(f, geo, opacities, beams, W, H):
    """For every live Gaussian, over every pixel of the 16 x 1 tiles its reference rect touches: how many pixels take it (power <= 0 and
    alpha >= (1/255)(1 + 1e-3)), their bounding box, how many are undecided (alpha within 1e-3 relative of 1/255), and how far the
    farthest taker's column lies from p_c.  -> dict of [P] arrays; box = (x0, y0, x1, y1) inclusive, -1 without takers."""
    P = geo["live"].size
    dirs = pixel_dirs(W, H, beams)
    n = np.zeros(P, np.int64); und = np.zeros(P, np.int64); box = np.full((P, 4), -1, np.int64); far_col = np.zeros(P)
    op = np.asarray(opacities, np.float64).reshape(-1)
    for g in np.nonzero(geo["live"])[0]:
        x0, y0, x1, y1 = geo["rect"][g]
        xs, ys = np.meshgrid(np.arange(16 * x0, min(16 * x1, W)), np.arange(y0, y1))
        xs, ys = xs.ravel(), ys.ravel()
        with np.errstate(all="ignore"):
            power, alpha = pair_alpha(f, op, dirs, g, xs, ys)
        ok = power <= 0.0
        und_m = ok & (np.abs(alpha * 255.0 - 1.0) <= UNDECIDED)
        take = ok & (alpha >= ALPHA_MIN * (1.0 + UNDECIDED)) & ~und_m
        n[g] = take.sum(); und[g] = und_m.sum()
        if n[g]:
            tx, ty = xs[take], ys[take]
            box[g] = (tx.min(), ty.min(), tx.max(), ty.max())
            dcol = np.abs(tx - geo["p_c"][g])
            far_col[g] = np.minimum(dcol, W - dcol).max()                  # (columns apart around the panorama)
    return dict(n=n, undecided=und, box=box, far_col=far_col)


# ---- backward -----------------------------------------------------------------------------------------------------------------------
LINE_SLOTS = dict(gx=0, gy=1, norm=2, gA=3, gB=4, gC=5, gop=6, gcol=(7, 9), gdep=9, G1=(10, 13), G2=(13, 16))


def chain(line, means, scales, rots, vm, mod=1.0, cov3D=None, dtype=F64):
    """What k_gaussian_backward makes of the packed gradient lines `line` [P,16] (slots: LINE_SLOTS), by autograd of k1 + record in
    `dtype`.  The cotangents: (gA, 2 gB, gC) on the conic (the line carries the cross term un-doubled, R3/cr/backward.cu:784, :247),
    gdep on the range, gs = gx u1' + gy u2' on the direction, and on the bases the direct gradients du_i = |u_i'|^2 G_i - 2 u_i' (u_i' . G_i)
    of the moments.  The three substitutions: the damped conic (record), the scale gradient taken with respect to the MODIFIED scale
    (:428-432), no Jacobian of a quaternion normalisation (:440-447: the forward does not normalise either).
    -> dict of numpy arrays named as lidargs_backward's."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dtype)
    line = t(line); vm = t(np.asarray(vm).reshape(16))
    P = line.shape[0]
    means = t(means).requires_grad_(True)
    if cov3D is None:
        sm = (t(np.float32(mod)) * t(scales)).requires_grad_(True)      # the modified scale is the leaf
        q = t(rots).requires_grad_(True)
        c6 = cov6_of(sm, q)
    else:
        c6 = t(cov3D).requires_grad_(True)
    k = k1(means, c6, vm)
    r = record(k, damped=True)
    gx, gy = line[:, 0], line[:, 1]
    G1, G2 = line[:, 10:13], line[:, 13:16]
    with torch.no_grad():
        u1p, u2p = r["u1p"], r["u2p"]
        du1 = (u1p * u1p).sum(-1)[:, None] * G1 - 2 * u1p * (u1p * G1).sum(-1)[:, None]
        du2 = (u2p * u2p).sum(-1)[:, None] * G2 - 2 * u2p * (u2p * G2).sum(-1)[:, None]
        gs = gx[:, None] * u1p + gy[:, None] * u2p
        gcon = torch.stack([line[:, 3], 2 * line[:, 4], line[:, 5]], -1)
    L = (r["conic"] * gcon).sum() + (k["dist"] * line[:, 9]).sum() + (k["u1"] * du1).sum() + (k["u2"] * du2).sum() + (k["dir"] * gs).sum()
    leaves = [means, c6] + ([sm, q] if cov3D is None else [])
    g = torch.autograd.grad(L, leaves)
    z = lambda w: np.zeros((P, w))
    n = lambda v: v.detach().to(F64).numpy()
    return dict(dL_dmean2D=n(torch.stack([gx, gy, line[:, 2], torch.zeros_like(gx)], -1)),
                dL_dconic=n(torch.stack([line[:, 3], line[:, 4], torch.zeros_like(gx), line[:, 5]], -1)),
                dL_dopacity=n(line[:, 6:7]), dL_dcolor=n(line[:, 7:9]), dL_ddepths=n(line[:, 9:10]),
                dL_dmean3D=n(g[0]), dL_dcov3D=n(g[1]), dL_dsphere=n(gs), dL_dbasis_u1=n(du1), dL_dbasis_u2=n(du2),
                dL_dscale=n(g[2]) if cov3D is None else z(3), dL_drot=n(g[3]) if cov3D is None else z(4))


def line_from_oracle(g, u1, u2):
    """The packed gradient lines [P,16] the blend would hand the chain, from the per-Gaussian blend sums of an oracle backward `g`
    (lgo.backward) and the unit bases u1, u2: the moments are recovered from the direct basis gradients by the reflection
    G = du - 2 u (u . du), which is its own inverse."""
    P = g["dL_dmeans2D"].shape[0]
    line = np.zeros((P, 16))
    line[:, 0:3] = g["dL_dmeans2D"][:, :3]
    line[:, 3], line[:, 4], line[:, 5] = g["dL_dconic"][:, 0], g["dL_dconic"][:, 1], g["dL_dconic"][:, 3]
    line[:, 6] = g["dL_dopacity"][:, 0]; line[:, 7:9] = g["dL_dcolors"]; line[:, 9] = g["dL_ddepths"][:, 0]
    for sl, du, u in ((slice(10, 13), g["dL_dbasis_u1"], u1), (slice(13, 16), g["dL_dbasis_u2"], u2)):
        du = du.astype(np.float64)
        line[:, sl] = du - 2.0 * u * (u * du).sum(1, keepdims=True)
    return line


def row_error(got, ref):
    """|x - ref| / (|ref| + 1e-3 max|row|), per entry."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    ref2, got2 = ref.reshape(ref.shape[0], -1), got.reshape(ref.shape[0], -1)
    return np.abs(got2 - ref2) / (np.abs(ref2) + 1e-3 * np.abs(ref2).max(1, keepdims=True) + 1e-300)


def ratios(name, hip, yard, ref, say=print):
    """p99 and worst row_error of `hip` and of the fp32 yardstick `yard`, both against the float64 `ref`, and a sentence naming HIP's worst
    entry (its row is the Gaussian's position in the arrays handed in) -> (p99 hip, p99 yard, worst hip, worst yard, where)."""
    eh, ey = row_error(hip, ref), row_error(yard, ref)
    out = (float(np.quantile(eh, 0.99)), float(np.quantile(ey, 0.99)), float(eh.max()), float(ey.max()))
    g, c = np.unravel_index(int(np.argmax(eh)), eh.shape)
    where = (f"worst entry: Gaussian (row) {g}, column {c}: got {np.asarray(hip).reshape(eh.shape)[g, c]!r}, float64 {np.asarray(ref).reshape(eh.shape)[g, c]!r}, "
             f"yardstick {np.asarray(yard).reshape(eh.shape)[g, c]!r}, error {eh[g, c]:.3e}")
    out = out + (where,)
    say(f"[ratio] {name:14s} p99 {out[0]:.2e} / {out[1]:.2e} = {out[0] / max(out[1], 1e-300):.2f}   worst {out[2]:.2e} / {out[3]:.2e} = {out[2] / max(out[3], 1e-300):.2f}")
    return out
