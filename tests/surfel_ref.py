"""The two per-surfel stages of csrc/surfel.hip restated in float64, vectorised over surfels (torch on the CPU where a VJP is wanted,
numpy for the integers).  tests/test_surfel_preprocess_cpu.py holds this file against the oracle without a GPU;
tests/test_surfel_preprocess_gpu.py holds the HIP kernels against it.  R2 = the surfel submodule of the reference, cr = cuda_rasterizer.

  forward    `forward64`: preprocessCUDA_cylinder's per-surfel values (R2/cr/forward.cu:256-302) and what the surfel record holds on top;
             `geometry`: p_c, p_r through the beam model (:145-174), the +-3 sigma extent (:177-215), the rect (R2/cr/auxiliary.h:99-112)
             and the cull rules in the kernel's order.
  takers     `takers`: the pixels of a surfel's reference rect that blend it (R2/cr/forward.cu:426-486).
  backward   `chain`: what k_sf_gaussian_backward makes of a packed 32-slot line (R2/cr/backward.cu:567-598, :625-692): the true VJP by
             torch.autograd, the reconstructed accumulators by the reference's formulas.  Run in torch.float32 it is the yardstick of the
             HIP chain: a second fp32 evaluation in another operation order.
"""
import math

import numpy as np
import torch

from preprocess_ref import ALPHA_MIN, F64, PI_F, UNDECIDED, bisect_beam, pixel_dirs, ratios, row_error, steps  # noqa: F401 (shared, not copied)

GUARD = float(np.float32(0.006))                        # Ray_Divergence_Angle (R2/cr/forward.cu:18, :163, :169)
NEAR_N = float(np.float32(0.2))                         # near_n (R2/cr/forward.cu:474)
CULL_NONE, CULL_RANGE, CULL_GUARD, CULL_EDGE_ON, CULL_RECT = range(5)

# the packed line of csrc/surfel.hip (enum SFA_*): 23 live slots, nine dead ones
SLOT = dict(COL=(0, 1), OPA=(2,), N=(4, 5, 6), TU=(8, 9, 10), TV=(12, 13, 16), TW=(17, 18, 20), AW=(21, 22, 24), M2X=(25,), M2Y=(26,), M2AX=(28,),
            M2AY=(29,), Z2D=(30,))
DEAD = (3, 7, 11, 14, 15, 19, 23, 27, 31)
LIVE = tuple(k for k in range(32) if k not in DEAD)


def _t(a, dtype=F64):
    return torch.as_tensor(np.asarray(a, np.float64), dtype=dtype)


def quat_cols(q):
    """quat_to_rotmat (R2/cr/auxiliary.h:249-271): the columns of the rotation matrix of q = (w, x, y, z) AS GIVEN (callers normalise)."""
    w, x, y, z = q.unbind(-1)
    c0 = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)], -1)
    c1 = torch.stack([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)], -1)
    c2 = torch.stack([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], -1)
    return c0, c1, c2


def rows_of(means, scales, qn, vm):
    """The rows of T = transpose(splat2world) * world2view (R2/cr/forward.cu:271-295, backward.cu:626-650) and the view-space normal:
    Tu = Rv (c0 s0), Tv = Rv (c1 s1), Tw = p_view, n = Rv c2 (transformVec4x3).  qn is the normalised quaternion."""
    V = vm.reshape(4, 4)
    Rv = V[:3, :3]                                                       # v_view[k] = sum_r vm[4 r + k] v[r]
    c0, c1, c2 = quat_cols(qn)
    Tu = (c0 * scales[:, 0:1]) @ Rv; Tv = (c1 * scales[:, 1:2]) @ Rv
    Tw = means @ Rv + V[3, :3]                                           # transformPoint4x3
    return Tu, Tv, Tw, c2 @ Rv


def forward64(means, scales, rots, vm, mod=1.0, transMat=None):
    """preprocessCUDA_cylinder's values in float64 from numpy inputs -> numpy float64 arrays.
    pv, dist (:259-260); Tu, Tv: the axes with scale_modifier (:272); n: the normal flipped towards the sensor, c = -(pv . n) whose zero
    culls (DUAL_VISIABLE, :297-302); Bu, Bv, Bw: the rows the BLEND uses (transMat_precomp's when given, rasterizer_impl.cu:332 -- the
    rect, the normal and the pixel centre still come from scales / rotations); the record's fields Tup = Bu / (Bu . Bu), Tvp, lam = wn =
    the raw Bw . n, blen = |Bw|."""
    with np.errstate(all="ignore"), torch.no_grad():
        q = _t(rots)
        qn = q / torch.sqrt((q * q).sum(-1, keepdim=True))
        Tu, Tv, pv, n = rows_of(_t(means), float(np.float32(mod)) * _t(scales), qn, _t(np.asarray(vm).reshape(16)))
        c = -(pv * n).sum(-1)
        n = torch.where((c > 0)[:, None], n, -n)                          # :300 (c == 0 culls; a NaN flips, as `cos > 0 ? 1 : -1`)
        Bu, Bv, Bw = Tu, Tv, pv
        if transMat is not None:
            tm = _t(transMat).reshape(-1, 9)
            Bu, Bv, Bw = tm[:, 0:3], tm[:, 3:6], tm[:, 6:9]
        uu, vv = (Bu * Bu).sum(-1, keepdim=True), (Bv * Bv).sum(-1, keepdim=True)
        out = dict(pv=pv, dist=torch.sqrt((pv * pv).sum(-1)), Tu=Tu, Tv=Tv, n=n, c=c, Bu=Bu, Bv=Bv, Bw=Bw, Tup=Bu / uu, Tvp=Bv / vv,
                   wn=(Bw * n).sum(-1), blen=torch.sqrt((Bw * Bw).sum(-1)))
        out["lam"] = out["wn"]                                           # |Tw| cos(phi1), :450-452
    return {k: v.numpy() for k, v in out.items()}


def _pix(p, beams, W, H):
    """cpmpute_pix (R2/cr/forward.cu:145-174) of view-space points p [.., 3] -> p_c, p_r (already H - p_r - 1), off the fan."""
    col_step, _ = steps(W)
    p_c = (PI_F - np.arctan2(p[..., 1], p[..., 0])) / col_step
    alpha = np.arctan2(p[..., 2], np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2))
    a = np.where(np.isfinite(alpha), alpha, 0.0)
    bi = bisect_beam(beams, a)
    up = bi > 0
    before = np.where(up, beams[np.maximum(bi - 1, 0)], beams[0]); after = np.where(up, beams[np.minimum(bi, H - 1)], beams[1])
    p_r = np.where(up, (bi - 1) + (a - before) / (after - before), 1 + (a - after) / (after - before))
    off = np.where(up, a > after + GUARD, a < before - GUARD)
    return p_c, H - p_r - 1.0, off


def _round_half_away(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def geometry(f, beams, W, H, near=0.0, far=80.0, band=1e-5, filter_only=False):
    """From forward64's arrays: the pixel centre, the extent rx, ry (+-3 sigma end points through the beam model, at least one pixel,
    R2/cr/forward.cu:177-215), the rect in 16 x 1 tiles (x and ymin truncate, ymax rounds; `+ 16 - 1` in two steps, auxiliary.h:99-112) and
    the cull rule that removes the surfel, in the kernel's order.  filter_only: K2 (filter_preprocessCUDA, :551-631) has no edge-on rule.
    `near_boundary`: surfels whose float64 extent, (p_c -+ rx) / 16 or p_r -+ ry lie within `band` (relative) of the integer / half-integer
    their rounding turns at -- or one of whose five projected points lies within `band` of the azimuth's branch cut, where the extent jumps."""
    beams = np.asarray(beams, np.float64)
    pv, Tu, Tv = f["pv"], f["Tu"], f["Tv"]
    P = pv.shape[0]
    tiles_x = (W + 15) // 16
    with np.errstate(all="ignore"):
        p_c, p_r, off_fan = _pix(pv, beams, W, H)
        ends = np.stack([pv + 3.0 * Tu, pv - 3.0 * Tu, pv + 3.0 * Tv, pv - 3.0 * Tv], 1)                 # cutoff 3 (:304)
        e_c, e_r, _ = _pix(ends, beams, W, H)
        qx = np.fmax.reduce(np.abs(e_c - p_c[:, None]), 1); qy = np.fmax.reduce(np.abs(e_r - p_r[:, None]), 1)
        rx = np.ceil(np.fmax(qx, 1.0)); ry = np.ceil(np.fmax(qy, 1.0))                                   # :209-212 (max() drops a NaN: at least one pixel)
        # (the extents are differences of pixel coordinates: their rounding error is relative to the coordinates, not to the difference)
        sx_ = np.fmax(np.abs(p_c), np.fmax.reduce(np.abs(e_c), 1)); sy_ = np.fmax(np.abs(p_r), np.fmax.reduce(np.abs(e_r), 1))
        ex0, ex1 = (p_c - rx) / 16.0, (p_c + rx + 15.0) / 16.0
        ey0, ey1 = p_r - ry, p_r + ry
        xmin = np.clip(np.trunc(ex0), 0, tiles_x); xmax = np.clip(np.trunc(ex1), 0, tiles_x)
        ymin = np.clip(np.trunc(ey0), 0, H); ymax = np.clip(_round_half_away(ey1), 0, H)
        near_int = lambda v, s=1.0: np.abs(v - np.round(v)) <= band * np.maximum(np.maximum(1.0, np.abs(v)), s)
        pts = np.concatenate([pv[:, None], ends], 1)
        cut = ((pts[..., 0] < 0) & (np.abs(pts[..., 1]) <= band * np.abs(pts[..., 0]))).any(1)
        near_boundary = ((near_int(qx, sx_) & (qx > 1.0 - band * sx_)) | (near_int(qy, sy_) & (qy > 1.0 - band * sy_)) | near_int(ex0) | near_int(ex1) |
                         near_int(ey0) | near_int(ey1 + 0.5) | cut)
    cull = np.full(P, CULL_NONE)

    def rule(code, cond):                                                   # the first rule that applies names the cull
        cull[(cull == CULL_NONE) & cond] = code

    rule(CULL_RANGE, ~((f["dist"] < far) & (f["dist"] > near)))            # :261
    rule(CULL_GUARD, off_fan)                                               # :266-267
    if not filter_only:
        rule(CULL_EDGE_ON, f["c"] == 0.0)                                   # :299
    rule(CULL_RECT, ~((xmax - xmin) * (ymax - ymin) > 0))                  # :312
    live = cull == CULL_NONE
    i = lambda v: np.where(live, np.nan_to_num(v), 0).astype(np.int64)
    return dict(p_c=p_c, p_r=p_r, rx=i(rx), ry=i(ry), rect=np.stack([i(xmin), i(ymin), i(xmax), i(ymax)], 1), cull=cull, live=live,
                near_boundary=near_boundary & live)


# ---- takers -------------------------------------------------------------------------------------------------------------------------
def pair(f, geo, opacities, dirs, g, xs, ys):
    """Everything up to alpha of surfel g at the pixels (xs, ys), as renderCUDA forms it (R2/cr/forward.cu:426-486)
    -> dict(alpha, lam2, depth, cos2, rho3d, rho2d, skip): skip = the pair is passed over before alpha (:455 cos2 == 0, :474 depth < 0.2)."""
    p = dirs[ys, xs]                                                        # :435-446
    n, Bw = f["n"][g], f["Bw"][g]
    cos2 = p @ n                                                            # :453
    lam2 = f["lam"][g] / cos2                                               # :456
    dp = lam2[:, None] * p - Bw                                             # :460-461
    sx, sy = dp @ f["Tup"][g], dp @ f["Tvp"][g]                            # :462-466
    rho3d = sx * sx + sy * sy
    dx, dy = geo["p_c"][g] - xs, geo["p_r"][g] - ys
    rho2d = 80.0 * dx * dx + 200.0 * dy * dy                                # FilterInvSquare (2) * (40 dx^2 + 100 dy^2), :469
    front = lam2 > 0
    rho = np.where(front, np.fmin(rho3d, rho2d), rho2d)                     # :472
    depth = np.where((rho3d <= rho2d) & front, lam2, f["blen"][g])          # :473
    op = float(opacities[g])
    alpha = np.full_like(rho, 0.99) if math.isnan(op) else np.minimum(0.99, op * np.exp(-0.5 * rho))       # :476-484 (min(0.99f, NaN) is 0.99)
    skip = (cos2 == 0) | (depth < NEAR_N)
    return dict(alpha=alpha, lam2=lam2, depth=depth, cos2=cos2, rho3d=rho3d, rho2d=rho2d, skip=skip)


def pair_undecided(pr, blen):
    """alpha within 1e-3 (relative) of 1/255, lam2 within that band of 0 (on the scale of the range), depth within it of 0.2."""
    return (np.abs(pr["alpha"] * 255.0 - 1.0) <= UNDECIDED) | (np.abs(pr["lam2"]) <= UNDECIDED * blen) | (np.abs(pr["depth"] - NEAR_N) <= UNDECIDED * NEAR_N)


def takers(f, geo, opacities, beams, W, H):
    """For every live surfel, over every pixel of its reference rect (tile columns [xmin, xmax), rows [ymin, ymax)): the pixels that take
    it (not skipped, alpha >= (1/255)(1 + 1e-3), not undecided) as arrays xs[g], ys[g] -- a seam span wraps, so no bounding box -- their
    count n and the count of undecided pixels (any of pair_undecided's three bands, whatever else holds of the pixel)."""
    P = geo["live"].size
    dirs = pixel_dirs(W, H, beams)
    n = np.zeros(P, np.int64); und = np.zeros(P, np.int64)
    none = np.zeros(0, np.int64)
    txs, tys = [none] * P, [none] * P
    op = np.asarray(opacities, np.float64).reshape(-1)
    for g in np.nonzero(geo["live"])[0]:
        x0, y0, x1, y1 = geo["rect"][g]
        xs, ys = np.meshgrid(np.arange(16 * x0, min(16 * x1, W)), np.arange(y0, y1))
        xs, ys = xs.ravel(), ys.ravel()
        with np.errstate(all="ignore"):
            pr = pair(f, geo, op, dirs, g, xs, ys)
            und_m = pair_undecided(pr, f["blen"][g])
            take = ~pr["skip"] & (pr["alpha"] >= ALPHA_MIN * (1.0 + UNDECIDED)) & ~und_m
        n[g] = take.sum(); und[g] = und_m.sum()
        txs[g], tys[g] = xs[take], ys[take]
    return dict(n=n, undecided=und, xs=txs, ys=tys)


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def mean2d_coefficients(Tw, aw, beams, W, H):
    """The 3-D branch's dL/dmean2D statistics, abs-linear in the |dL/dTw| sums aw (R2/cr/backward.cu:567-573, with beta_t / alpha_t the
    centre's angles, :422-425): sin(beta_t) cos(alpha_t) = Tw.y / rho_r, cos(beta_t) cos(alpha_t) = -Tw.x / rho_r, ... -> (mx3, my3)."""
    rho_xy = torch.sqrt(Tw[:, 0] ** 2 + Tw[:, 1] ** 2)
    ga = abs(float(beams[H - 1]) - float(beams[0])) / (float(H) - 1.0)      # grad_alpha, :425
    mx3 = math.pi * (Tw[:, 1].abs() * aw[:, 0] + Tw[:, 0].abs() * aw[:, 1])
    my3 = 0.5 * H * ga * (Tw[:, 2].abs() * Tw[:, 0].abs() / rho_xy * aw[:, 0] + Tw[:, 2].abs() * Tw[:, 1].abs() / rho_xy * aw[:, 1] + rho_xy * aw[:, 2])
    return mx3, my3


def ddel_dTw(Tw, beams, W, H):
    """d(delx)/dTw and d(dely)/dTw of the 2-D branch (R2/cr/backward.cu:590-595) -> two [P,3]."""
    rho_xy2 = Tw[:, 0] ** 2 + Tw[:, 1] ** 2
    rho_xy = torch.sqrt(rho_xy2); rho_r2 = rho_xy2 + Tw[:, 2] ** 2
    ga = abs(float(beams[H - 1]) - float(beams[0])) / (float(H) - 1.0)
    kx = W / (2.0 * math.pi)
    zero = torch.zeros_like(rho_xy)
    ddelx = torch.stack([kx * Tw[:, 1] / rho_xy2, -kx * Tw[:, 0] / rho_xy2, zero], -1)
    ddely = torch.stack([-ga * Tw[:, 2] * Tw[:, 0] / (rho_r2 * rho_xy), -ga * Tw[:, 2] * Tw[:, 1] / (rho_r2 * rho_xy), ga * rho_xy / rho_r2], -1)
    return ddelx, ddely


def chain(line, means, scales, rots, vm, beams, W, H, radii, transMat=None, dtype=F64):
    """What k_sf_gaussian_backward / sf_gb_row make of the packed lines `line` [P,32] (slots: SLOT; the dead slots are not read).
    Reconstructed (R2/cr/backward.cu): dL_dmean2D = (mx3 + M2X W/2, my3 + M2Y H/2, mx3 + M2AX W/2, my3 + M2AY H/2) (:567-585), and the final
    dL/dTw = TW + Z2D Tw / |Tw| + M2X ddelx + M2Y ddely (:590-598), all with the Tw the BLEND saw (transMat_precomp's when given, :267).
    The true VJP, by autograd with cotangents (gTu, gTv, gTw, gn) on rows_of(means3D, scales, q): dL_dscale, dL_drot, dL_dmean3D
    (:625-692), with the reference's deviations: the backward ignores scale_modifier (scale_to_mat(scale, 1.0f), :630); the quaternion
    VJP is taken at the normalised quaternion without the normalisation's own chain (quat_to_rotmat_vjp, auxiliary.h:274-316); the
    normal's cotangent is flipped as the forward flipped the normal (:672-674); the chain runs on p_view whatever the blend used.
    depth = sqrt(px^2 + pz^2) for radii > 0, else 0 (:671).  -> dict of float64 numpy arrays named as lidargs_surfel_backward's."""
    line = _t(line, dtype); vmt = _t(np.asarray(vm).reshape(16), dtype)
    P = line.shape[0]
    sl = lambda k: line[:, list(SLOT[k])]
    means_t = _t(means, dtype).requires_grad_(True)
    scales_t = _t(scales, dtype).requires_grad_(True)
    q = _t(rots, dtype)
    qn = (q / torch.sqrt((q * q).sum(-1, keepdim=True))).detach().requires_grad_(True)
    Tu, Tv, pv, nv = rows_of(means_t, scales_t, qn, vmt)
    with torch.no_grad():
        Tw = _t(transMat, dtype).reshape(P, 9)[:, 6:9] if transMat is not None else pv
        aw = sl("AW")
        mx3, my3 = mean2d_coefficients(Tw, aw, beams, W, H)
        m2x, m2y = sl("M2X")[:, 0], sl("M2Y")[:, 0]
        mean2d = torch.stack([mx3 + m2x * 0.5 * W, my3 + m2y * 0.5 * H, mx3 + sl("M2AX")[:, 0] * 0.5 * W, my3 + sl("M2AY")[:, 0] * 0.5 * H], -1)
        ddelx, ddely = ddel_dTw(Tw, beams, W, H)
        rho_r = torch.sqrt((Tw * Tw).sum(-1, keepdim=True))
        gTw = sl("TW") + sl("Z2D") * Tw / rho_r + m2x[:, None] * ddelx + m2y[:, None] * ddely
        gTu, gTv, gn = sl("TU"), sl("TV"), sl("N")
        flip = torch.where(-(pv * nv).sum(-1) > 0, 1.0, -1.0).to(dtype)[:, None]
        depth = torch.where(torch.as_tensor(np.asarray(radii).reshape(-1) > 0), torch.sqrt(pv[:, 0] ** 2 + pv[:, 2] ** 2), torch.zeros((), dtype=dtype))
    L = (Tu * gTu).sum() + (Tv * gTv).sum() + (pv * gTw).sum() + (nv * (flip * gn)).sum()
    g_mean, g_scale, g_q = torch.autograd.grad(L, [means_t, scales_t, qn])
    n = lambda v: v.detach().to(F64).numpy()
    return dict(dL_dmean2D=n(mean2d), dL_dnormal=n(gn), dL_dopacity=n(sl("OPA")), dL_dcolor=n(sl("COL")), dL_dmean3D=n(g_mean),
                dL_dtransMat=n(torch.cat([gTu, gTv, gTw], -1)), dL_dtransMat_2dtemp=n(aw), dL_dscale=n(g_scale), dL_drot=n(g_q), depth=n(depth[:, None]))


def line_from_oracle(g, Tw, beams, W, H):
    """The packed lines [P,32] of one oracle backward `g` (lgo_surfel.backward) where they are identifiable: COL, OPA, N, AW, TU, TV as
    they are; the four M2 slots from dL_dmeans2D minus the 3-D statistics that follow from AW; TW = the oracle's final dL/dTw minus the
    M2X ddelx + M2Y ddely terms; Z2D = 0 (its term stays inside TW).  What is subtracted here is what `chain` adds back: dL_dmean2D and
    the TW row return by construction, so this pair of functions does not test mean2d_coefficients (tests/test_surfel_preprocess_cpu.py
    holds the derived slots to M2AX >= |M2X|, M2AY >= |M2Y|; beyond that mx3 / my3 rest on whole-frame parity)."""
    P = g["dL_dmeans2D"].shape[0]
    line = np.zeros((P, 32))
    put = lambda k, v: line.__setitem__((slice(None), list(SLOT[k])), np.asarray(v, np.float64).reshape(P, -1))
    tm = g["dL_dtransMat"].astype(np.float64)
    put("COL", g["dL_dcolors"]); put("OPA", g["dL_dopacity"]); put("N", g["dL_dnormal"]); put("AW", g["dL_dtransMat_2dtemp"])
    put("TU", tm[:, 0:3]); put("TV", tm[:, 3:6])
    Twt = _t(Tw)
    with np.errstate(all="ignore"):
        mx3, my3 = (v.numpy() for v in mean2d_coefficients(Twt, _t(g["dL_dtransMat_2dtemp"]), beams, W, H))
        m2 = g["dL_dmeans2D"].astype(np.float64)
        m2x, m2y = (m2[:, 0] - mx3) / (0.5 * W), (m2[:, 1] - my3) / (0.5 * H)
        put("M2X", m2x); put("M2Y", m2y); put("M2AX", (m2[:, 2] - mx3) / (0.5 * W)); put("M2AY", (m2[:, 3] - my3) / (0.5 * H))
        ddelx, ddely = (v.numpy() for v in ddel_dTw(Twt, beams, W, H))
        put("TW", tm[:, 6:9] - m2x[:, None] * ddelx - m2y[:, None] * ddely)
    return np.nan_to_num(line)
