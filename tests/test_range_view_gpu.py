"""GPU tests of the range-view conversion (lidar-gs_amd/range_view.py -> liblidargs_rangeview.so, csrc/range_view.hip).

Projection: on margin-masked points (tests/range_view_ref.decision_margin_mask: no pixel hangs on the last bits of atan2f) both images
must EQUAL the float64 restatement -- no tolerance, no allowance of differing pixels.

Back-projection and the round trip's ranges are float32 evaluations of a float64 formula, and only they get a tolerance: 4x the largest
error of the same formula written as float32 framework ops (range_view_ref.framework_unproject / framework_dirs) against the float64
restatement over the cases of this file, measured on an MI355X (test_framework_error_is_the_measured_one prints and re-checks them):
    back-projected coordinates  framework ops 2.51e-05 m  -> allowed 1.00e-04 m       (ranges up to 78 m; the native result: 2.13e-05 m)
    unit rays                   framework ops 3.97e-07    -> allowed 1.59e-06         (the native result: 2.60e-07)
    round-trip ranges           framework ops 1.53e-05 m  -> allowed 6.10e-05 m       (the native result: 1.53e-05 m, two ulp at 64..78 m)
Count, order and the intensity column of the back-projection are exact.
"""
import ctypes

import numpy as np
import pytest
import torch

import lidargs_scenes as sc
import range_view_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMEWORK_BACK_ERR, FRAMEWORK_DIRS_ERR, FRAMEWORK_ROUND_TRIP_ERR = 2.51e-05, 3.97e-07, 1.53e-05      # measured, see above
BACK_TOL, DIRS_TOL, ROUND_TRIP_TOL = 4 * FRAMEWORK_BACK_ERR, 4 * FRAMEWORK_DIRS_ERR, 4 * FRAMEWORK_ROUND_TRIP_ERR
LIDAR_K = (2.0, 26.9)
TAGS = ("u16", "w16", "n16", "u64", "w64", "n64", "fov")


@pytest.fixture(scope="module")
def rv(hip_lib_built):
    import range_view
    return range_view


@pytest.fixture(scope="module")
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "range_view_device_golden.npz"))


def case(g, tag):
    beams = g[tag + "_beams"] if tag + "_beams" in g else None
    return int(g[tag + "_H"]), int(g[tag + "_W"]), beams, None if beams is not None else tuple(float(v) for v in g["lidar_K"])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def host(t):
    return t.cpu().numpy().astype(np.float64)


def project(rv, pts, H, W, beams=None, K=None, **kw):
    """The device front on device tensors -> two float64 numpy images."""
    p, i = rv.lidar_to_pano_with_intensities(dev(pts), H, W, lidar_K=K, beam_inclinations=dev(beams), **kw)
    assert p.dtype == i.dtype == torch.float32 and p.is_cuda and p.shape == i.shape == (H, W)
    return host(p), host(i)


def assert_projection_exact(rv, pts, H, W, beams=None, K=None, **kw):
    got_p, got_i = project(rv, pts, H, W, beams, K, **kw)
    want_p, want_i = ref.project(pts, H, W, beams, K, **kw)
    bad = int((got_p != want_p).sum()), int((got_i != want_i).sum())
    assert bad == (0, 0), f"{bad} differing pixels (pano, intensity) of {H * W}"
    return got_p, got_i


# ---- projection ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_projection_of_the_fixture_is_exact(rv, golden, tag):
    H, W, beams, K = case(golden, tag)
    p, i = project(rv, golden[tag + "_points"], H, W, beams, K)
    assert np.array_equal(p, golden[tag + "_pano"]) and np.array_equal(i, golden[tag + "_intensities"])


@pytest.mark.parametrize("N", [1, 33, 4099, 70001, 1200001])
def test_projection_sizes_are_exact(rv, N):
    """One point, less than a wave, several workgroups, not a multiple of the workgroup; 1 200 001 is 2.29 times the grid's 2048 x 256 =
    524 288 lanes (RV_PROJECT_MAX_BLOCKS of csrc/range_view.hip), so the grid-stride loop makes two whole rounds and a part of a third, with
    point indices above the grid in the keys (at 70 001 every lane still has at most one point)."""
    H, W = 16, 512
    beams = sc.beam_table(H, "waymo")
    pts = ref.masked_points(np.random.default_rng(N), N + N // 16 + 8, H, W, beams)[:N]
    assert len(pts) == N
    p, _ = assert_projection_exact(rv, pts, H, W, beams)
    assert N < 4099 or (p != 0).mean() > 0.25


def test_projection_fov_mode_and_both_conventions_are_exact(rv):
    H, W = 32, 1080
    pts = ref.masked_points(np.random.default_rng(5), 6000, H, W, lidar_K=LIDAR_K)
    assert_projection_exact(rv, pts, H, W, K=LIDAR_K)
    assert_projection_exact(rv, pts, H, W, K=LIDAR_K, pixel_rows=True)
    beams = sc.beam_table(H, "neartie")
    pts = ref.masked_points(np.random.default_rng(6), 6000, H, W, beams)
    p0, _ = assert_projection_exact(rv, pts, H, W, beams)
    p1, _ = assert_projection_exact(rv, pts, H, W, beams, pixel_rows=True)
    assert not p0[0].any() and p1[0].any() and np.array_equal(p0[1:, 1:], p1[:-1, 1:])      # one row up; column 0 also takes column W


def test_many_contenders_per_pixel_are_exact(rv):
    H, W = 4, 8
    beams = sc.beam_table(H, "waymo")
    pts = ref.masked_points(np.random.default_rng(7), 5200, H, W, beams)[:5000]
    assert len(pts) == 5000
    p, _ = assert_projection_exact(rv, pts, H, W, beams, pixel_rows=True)                   # ~150 contenders for each of the 32 pixels
    assert (p != 0).all()
    assert_projection_exact(rv, pts, H, W, beams)


def test_equal_ranges_the_lowest_index_wins_and_order_does_not_change_the_ranges(rv):
    H, W = 16, 512
    beams = sc.beam_table(H, "uniform")
    pts = ref.masked_points(np.random.default_rng(8), 4000, H, W, beams)
    twin = pts.copy()
    twin[:, 3] += 1.0
    p, i = project(rv, pts, H, W, beams)
    p_ab, i_ab = assert_projection_exact(rv, np.concatenate([pts, twin]), H, W, beams)
    p_ba, i_ba = assert_projection_exact(rv, np.concatenate([twin, pts]), H, W, beams)
    assert np.array_equal(p_ab, p) and np.array_equal(i_ab, i)
    assert np.array_equal(p_ba, p) and np.array_equal(i_ba, np.where(p != 0, i + 1.0, 0.0).astype(np.float32).astype(np.float64))
    perm = np.random.default_rng(9).permutation(len(pts))
    p_perm, i_perm = project(rv, pts[perm], H, W, beams)
    assert np.array_equal(p_perm, p)
    assert np.array_equal(i_perm, i)                                                        # (no two of these points share range and pixel)


def test_max_depth_zero_range_and_non_finite_points_are_dropped(rv):
    H, W = 16, 512
    beams = sc.beam_table(H, "uniform")
    step = 2 * np.pi / W
    at = lambda col, r, inten: [r * np.cos(np.pi - col * step), r * np.sin(np.pi - col * step), 0.0, inten]      # elevation 0: inside the table
    good = np.float32([at(10, 20.0, 0.25), at(300, 79.5, 0.5)])
    on = np.float32([[80.0, 0.0, 0.0, 0.9]])                                               # dist == max_depth exactly, column W / 2
    assert ref.range32(on)[0] == np.float32(80.0)
    want = ref.project(good, H, W, beams)
    assert (want[0] != 0).sum() == 2
    bad = np.float32([[0, 0, 0, 0.7], [np.nan, 1, 0, 0.7], [1, np.inf, 0, 0.7], [1, 1, -np.inf, 0.7], [5, 5, 0, np.nan], [3e38, 3e38, 0, 0.7],
                      [200.0, 0, 0, 0.7]])
    for extra in (on, bad, np.concatenate([bad, on])):
        got = project(rv, np.concatenate([extra, good, extra]), H, W, beams)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    p81, i81 = assert_projection_exact(rv, np.concatenate([on, good]), H, W, beams, max_depth=81)     # the same point below another max_depth: kept
    assert (p81 == 80.0).sum() == 1 and (i81 == np.float32(0.9)).sum() == 1
    p_inf, _ = project(rv, bad, H, W, beams, max_depth=float("inf"))                       # an overflowing range is not finite: dropped
    assert (p_inf != 0).sum() == 1 and (p_inf == 200.0).sum() == 1


def test_row_rule_of_both_conventions_on_hand_placed_points(rv):
    H, W = 16, 512
    beams = sc.beam_table(H, "uniform")
    step = 2 * np.pi / W

    def at(col, elev, r):
        az = np.pi - col * step
        return [r * np.cos(elev) * np.cos(az), r * np.cos(elev) * np.sin(az), r * np.sin(elev), r / 100]
    pts = np.float32([at(100, float(beams[0]), 10.0), at(200, float(beams[-1]), 20.0), at(300, float(beams[-1]) + 0.03, 30.0),
                      at(400, float(beams[0]) - 0.03, 40.0), at(50, float(beams[7]), 50.0)])
    p, i = assert_projection_exact(rv, pts, H, W, beams)
    rows, cols = np.nonzero(p)
    # the reference: row H - label.  Beam 0 (and below it: clamped to 0) falls off the image; the top beam and above it land in row 1
    assert sorted(zip(rows.tolist(), cols.tolist())) == [(1, 200), (1, 300), (H - 7, 50)]
    assert p[1, 200] == np.float32(ref.range32(pts[1:2])[0]) and i[1, 300] == np.float32(0.3)
    p, i = assert_projection_exact(rv, pts, H, W, beams, pixel_rows=True)
    rows, cols = np.nonzero(p)
    assert sorted(zip(rows.tolist(), cols.tolist())) == [(0, 200), (0, 300), (H - 1 - 7, 50), (H - 1, 100), (H - 1, 400)]


def test_column_w_is_dropped_by_the_reference_convention_and_wraps_with_pixel_rows(rv):
    H, W = 16, 512
    beams = sc.beam_table(H, "uniform")
    pts = np.float32([[-10.0, -0.0, 0.5, 0.6]])                                             # atan2(-0, x < 0) = -pi: column position W
    assert np.signbit(pts[0, 1])
    p, _ = assert_projection_exact(rv, pts, H, W, beams)
    assert not p.any()
    p, i = assert_projection_exact(rv, pts, H, W, beams, pixel_rows=True)
    assert (p != 0).sum() == 1 and p[0, 0] == np.float32(ref.range32(pts)[0]) and i[0, 0] == np.float32(0.6)      # above the top beam: row 0
    pts[0, 1] = 0.0                                                                         # +0: azimuth +pi, column 0 either way
    for kw in ({}, {"pixel_rows": True}):
        p, _ = assert_projection_exact(rv, pts, H, W, beams, **kw)
        assert (p != 0).sum() == 1 and p[1 - int(bool(kw)), 0] != 0


def raw_project(rv, pts, H, W, beams, fill_out, fill_scratch, flags=0):
    """The C entry point itself, on outputs and scratch the test filled."""
    nb = rv._lib.lidargs_rv_scratch_bytes(H, W)
    out = torch.full((2, H, W), fill_out, dtype=torch.float32, device=DEV)
    scratch = torch.full((nb,), fill_scratch, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = rv._lib.lidargs_rv_project(len(pts), p(pts), H, W, p(beams), 0.0, 0.0, 80.0, None, flags, p(out[0]), p(out[1]), p(scratch), nb,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rv._lib.lidargs_rv_last_error()
    return host(out[0]), host(out[1])


def test_every_pixel_is_written_no_state_is_assumed_and_runs_are_bit_identical(rv):
    H, W = 16, 512
    beams = sc.beam_table(H, "waymo")
    pts = ref.masked_points(np.random.default_rng(10), 3000, H, W, beams)
    want = ref.project(pts, H, W, beams)
    assert (want[0] == 0).sum() > H * W // 2                                                # most pixels are empty ones
    d_pts, d_beams = dev(pts), dev(beams)
    for fill_scratch in (0xFF, 0x00):
        got = raw_project(rv, d_pts, H, W, d_beams, float("nan"), fill_scratch)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    a = rv.lidar_to_pano_with_intensities(d_pts, H, W, beam_inclinations=d_beams)
    b = rv.lidar_to_pano_with_intensities(d_pts, H, W, beam_inclinations=d_beams)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # N == 0 through the C entry point: an all-empty image, every pixel written
    empty = torch.zeros(0, 4, dtype=torch.float32, device=DEV)
    got = raw_project(rv, empty, H, W, d_beams, float("nan"), 0x5A)
    assert not got[0].any() and not got[1].any()


def rigid(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = q * np.sign(np.linalg.det(q)), rng.uniform(-30, 30, 3)
    return m


def test_projection_with_a_transform_is_exact(rv):
    H, W = 16, 512
    beams = sc.beam_table(H, "waymo")
    w2s = rigid(11)
    local = ref.random_points(np.random.default_rng(12), 4000, beams)
    world = local.copy()
    world[:, :3] = ((local[:, :3].astype(np.float64) - w2s[:3, 3]) @ w2s[:3, :3]).astype(np.float32)      # inverse of x -> R x + t
    world = np.ascontiguousarray(world[ref.decision_margin_mask(world, H, W, beams, transform=w2s)])      # masked AFTER the transform
    assert len(world) > 3700
    p, _ = assert_projection_exact(rv, world, H, W, beams, transform=w2s)
    assert_projection_exact(rv, world, H, W, beams, transform=w2s[:3], pixel_rows=True)
    assert (p != 0).sum() > 1500 and not np.array_equal(p, ref.project(world, H, W, beams)[0])


def test_numpy_in_gives_float64_numpy_out_and_mixing_is_refused(rv):
    H, W = 16, 512
    beams = sc.beam_table(H, "uniform")
    pts = ref.masked_points(np.random.default_rng(13), 2000, H, W, beams)
    p, i = rv.lidar_to_pano_with_intensities(pts.astype(np.float64), H, W, beam_inclinations=list(beams))
    want = ref.project(pts, H, W, beams)
    assert isinstance(p, np.ndarray) and p.dtype == i.dtype == np.float64 and np.array_equal(p, want[0]) and np.array_equal(i, want[1])
    back = rv.pano_to_lidar_with_intensities(p, i, beam_inclinations=beams)
    assert isinstance(back, np.ndarray) and back.dtype == np.float64 and back.shape == (int((p != 0).sum()), 4)
    assert np.abs(back - ref.unproject(p, i, beams)).max() <= BACK_TOL
    xyz = rv.pano_to_lidar(p, beam_inclinations=beams)
    assert xyz.shape == (len(back), 3) and xyz.flags["C_CONTIGUOUS"] and np.array_equal(xyz, back[:, :3])
    with pytest.raises(RuntimeError, match="both be device tensors or both numpy"):
        rv.pano_to_lidar_with_intensities(p, dev(i), beam_inclinations=beams)
    with pytest.raises(RuntimeError, match="all on the host or all on the device"):
        rv.lidar_to_pano_with_intensities(pts, H, W, beam_inclinations=dev(beams))
    with pytest.raises(RuntimeError, match="must be float32"):
        rv.lidar_to_pano_with_intensities(dev(pts).double(), H, W, beam_inclinations=beams)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        rv.pano_to_lidar(torch.from_numpy(p), beam_inclinations=beams)
    e = rv.lidar_to_pano_with_intensities(torch.zeros(0, 4, device=DEV), H, W, lidar_K=LIDAR_K)
    assert e[0].shape == (H, W) and e[0].is_cuda and not e[0].any() and not e[1].any()


# ---- back-projection -------------------------------------------------------------------------------------------------------------------
def random_image(rng, H, W, fill):
    pano = rng.uniform(3.0, 78.0, (H, W)).astype(np.float32)
    pano[rng.uniform(size=(H, W)) >= fill] = 0.0
    inten = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    return pano, inten


def back_cases(golden):
    """name -> (pano, intensities, beams, lidar_K, transform): every back-projection this file checks, and what the tolerances were measured over."""
    cases = {}
    for tag in TAGS:
        H, W, beams, K = case(golden, tag)
        cases["fixture " + tag] = (golden[tag + "_pano"], golden[tag + "_intensities"], beams, K, None)
    rng = np.random.default_rng(14)
    for H, W, kind in ((3, 5, "uniform"), (16, 512, "waymo"), (64, 2650, "neartie")):       # the last two span several scan tiles (1024 pixels each)
        cases[f"random {H}x{W}"] = random_image(rng, H, W, 0.6) + (sc.beam_table(H, kind), None, None)
    cases["random fov 32x1080"] = random_image(rng, 32, 1080, 0.6) + (None, LIDAR_K, None)
    cases["random 16x512 transform"] = random_image(rng, 16, 512, 0.6) + (sc.beam_table(16, "uniform"), None, rigid(15))
    full = random_image(rng, 16, 512, 1.1)
    cases["all full 16x512"] = full + (sc.beam_table(16, "waymo"), None, None)
    for name, (r, c) in (("first", (0, 0)), ("last", (15, 511)), ("tile edge", (2, 0))):     # pixel 1024 opens the second scan tile
        one = np.zeros((16, 512), dtype=np.float32)
        one[r, c] = 42.5
        cases["single pixel " + name] = (one, full[1], sc.beam_table(16, "waymo"), None, None)
    return cases


def unproject(rv, pano, inten, beams, K, transform):
    got = rv.pano_to_lidar_with_intensities(dev(pano), dev(inten), lidar_K=K, beam_inclinations=dev(beams), transform=transform)
    assert got.dtype == torch.float32 and got.is_cuda and got.is_contiguous()
    return got


def test_back_projection_count_and_order_are_exact_and_coordinates_within_tolerance(rv, golden):
    for name, (pano, inten, beams, K, xf) in back_cases(golden).items():
        want = ref.unproject(pano.astype(np.float64), inten.astype(np.float64), beams, K, transform=xf)
        got = unproject(rv, pano, inten, beams, K, xf)
        assert got.shape == want.shape == (int((pano != 0).sum()), 4), name                 # the count; exact size
        got = host(got)
        assert np.array_equal(got[:, 3], want[:, 3]), name                                  # row-major order: every pixel has its own intensity
        err = np.abs(got[:, :3] - want[:, :3]).max()
        print(f"back-projection {name}: {len(want)} points, max error {err:.3e} m (allowed {BACK_TOL:.3e})")
        assert err <= BACK_TOL, name
    H, W, beams, K = case(golden, "w16")
    xyz = rv.pano_to_lidar(dev(golden["w16_pano"]), beam_inclinations=dev(beams))
    assert xyz.shape[1] == 3 and xyz.is_contiguous() and torch.equal(xyz, unproject(rv, golden["w16_pano"], None, beams, None, None)[:, :3])
    assert not unproject(rv, golden["w16_pano"], None, beams, None, None)[:, 3].any()       # no intensities: column 3 is 0


def test_back_projection_of_an_empty_image(rv):
    beams = sc.beam_table(16, "uniform")
    got = rv.pano_to_lidar_with_intensities(torch.zeros(16, 512, device=DEV), torch.ones(16, 512, device=DEV), beam_inclinations=beams)
    assert got.shape == (0, 4) and got.dtype == torch.float32 and got.is_cuda
    assert rv.pano_to_lidar(torch.zeros(3, 5, device=DEV), lidar_K=LIDAR_K).shape == (0, 3)


def test_back_projection_with_poisoned_scratch_and_outputs(rv):
    H, W = 64, 2650
    beams = sc.beam_table(H, "waymo")
    pano, inten = random_image(np.random.default_rng(16), H, W, 0.5)
    want = host(unproject(rv, pano, inten, beams, None, None))
    nb = rv._lib.lidargs_rv_scratch_bytes(H, W)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    d_pano, d_inten, d_beams = dev(pano), dev(inten), dev(beams)
    for fill in (0xFF, 0x00):
        out = torch.full((H * W, 4), float("nan"), dtype=torch.float32, device=DEV)
        count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        scratch = torch.full((nb,), fill, dtype=torch.uint8, device=DEV)
        rc = rv._lib.lidargs_rv_unproject(H, W, p(d_pano), p(d_inten), p(d_beams), 0.0, 0.0, None, p(out), p(count), p(scratch), nb,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0 and int(count.item()) == len(want)
        assert np.array_equal(host(out[:len(want)]), want) and torch.isnan(out[len(want):]).all()      # nothing behind the count is touched


def test_ray_dirs(rv, golden):
    for tag in ("w16", "fov"):
        H, W, beams, K = case(golden, tag)
        got = rv.ray_dirs(H, W, lidar_K=K, beam_inclinations=dev(beams) if beams is not None else None)
        assert got.shape == (H, W, 3) and got.dtype == torch.float32 and got.is_cuda
        err = np.abs(host(got) - ref.pixel_dirs(H, W, beams, K)).max()
        print(f"ray_dirs {tag}: max error {err:.3e} (allowed {DIRS_TOL:.3e})")
        assert err <= DIRS_TOL
        assert np.abs(host(got) - golden[tag + "_dirs"]).max() <= DIRS_TOL + 4.2e-7       # the reference's own float32 table (tests/test_range_view_cpu.py)
    H, W = 64, 2650
    beams = sc.beam_table(H, "neartie")
    got = rv.ray_dirs(H, W, beam_inclinations=beams)                                        # a host table: uploaded
    assert np.abs(host(got) - ref.pixel_dirs(H, W, beams)).max() <= DIRS_TOL
    assert np.abs(np.linalg.norm(host(got), axis=2) - 1).max() <= 2 * DIRS_TOL


# ---- round trip ------------------------------------------------------------------------------------------------------------------------
ROUND_TRIPS = [(16, 512, "uniform"), (16, 512, "neartie"), (64, 2650, "waymo"), (64, 2650, None)]


def round_trip_image(H, W):
    return random_image(np.random.default_rng(H + W), H, W, 0.7)


@pytest.mark.parametrize("H,W,kind", ROUND_TRIPS)
def test_round_trip_returns_to_the_same_pixels(rv, H, W, kind):
    beams = None if kind is None else sc.beam_table(H, kind)
    K = LIDAR_K if kind is None else None
    pano, inten = round_trip_image(H, W)
    pts = unproject(rv, pano, inten, beams, K, None)
    p, i = rv.lidar_to_pano_with_intensities(pts, H, W, lidar_K=K, beam_inclinations=dev(beams), pixel_rows=True)
    p, i = host(p), host(i)
    assert np.array_equal(p != 0, pano != 0)                                                # column 0 (azimuth +-pi) included
    assert np.array_equal(i, np.where(pano != 0, inten, 0).astype(np.float64))
    err = np.abs(p - pano.astype(np.float64)).max()
    print(f"round trip {H}x{W} {kind}: max range error {err:.3e} m (allowed {ROUND_TRIP_TOL:.3e})")
    assert err <= ROUND_TRIP_TOL


# ---- where the tolerances come from ----------------------------------------------------------------------------------------------------
def framework_errors(golden):
    """The largest error of the float32 framework-op form of the back-projection, of the unit rays and of the round trip's ranges against
    float64, over the cases above (transform cases aside: the framework form has no double transform)."""
    back = dirs = trip = 0.0
    for name, (pano, inten, beams, K, xf) in back_cases(golden).items():
        if xf is not None:
            continue
        got = ref.framework_unproject(dev(pano), dev(inten), dev(beams), K)
        want = ref.unproject(pano.astype(np.float64), inten.astype(np.float64), beams, K)
        if len(want):
            back = max(back, float(np.abs(host(got)[:, :3] - want[:, :3]).max()))
    for tag in ("w16", "fov"):
        H, W, beams, K = case(golden, tag)
        dirs = max(dirs, float(np.abs(host(ref.framework_dirs(H, W, dev(beams), K, DEV)) - ref.pixel_dirs(H, W, beams, K)).max()))
    H, W = 64, 2650
    beams = sc.beam_table(H, "neartie")
    dirs = max(dirs, float(np.abs(host(ref.framework_dirs(H, W, dev(beams), None, DEV)) - ref.pixel_dirs(H, W, beams)).max()))
    for H, W, kind in ROUND_TRIPS:
        beams = None if kind is None else sc.beam_table(H, kind)
        pano, inten = round_trip_image(H, W)
        pts = ref.framework_unproject(dev(pano), dev(inten), dev(beams), LIDAR_K if kind is None else None)
        rng_ = torch.sqrt((pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2])
        trip = max(trip, float(np.abs(host(rng_) - pano[pano != 0].astype(np.float64)).max()))
    return back, dirs, trip


def test_framework_error_is_the_measured_one(golden):
    """The three constants of the header are what the framework ops give on this hardware (to the two digits they are quoted with, and
    allowing the framework's kernels to change by a factor of two before the constants are taken again)."""
    back, dirs, trip = framework_errors(golden)
    print(f"framework ops against float64: back-projection {back:.3e} m, unit rays {dirs:.3e}, round-trip ranges {trip:.3e} m")
    for got, const in ((back, FRAMEWORK_BACK_ERR), (dirs, FRAMEWORK_DIRS_ERR), (trip, FRAMEWORK_ROUND_TRIP_ERR)):
        assert const / 2 <= got <= const * 2
