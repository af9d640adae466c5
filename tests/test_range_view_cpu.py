"""CPU tests of the range-view conversion (lidar-gs_amd/range_view.py, liblidargs_rangeview.so, include_rangeview/): the restatement
tests/range_view_ref.py reproduces what the reference's functions gave on the margin-masked fixture (the projection exactly, the
back-projection to 1e-12), its keyed minimum is the sequential loop, the fifth library builds and exports exactly what its header
declares, and the front refuses what it cannot take without needing a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import range_view_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED = {"lidargs_rv_scratch_bytes", "lidargs_rv_project", "lidargs_rv_unproject", "lidargs_rv_ray_dirs", "lidargs_rv_last_error",
            "lidargs_rv_abi_version"}
TAGS = ("u16", "w16", "n16", "u64", "w64", "n64", "fov")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "range_view_device_golden.npz"))


def case(g, tag):
    """(H, W, beams or None, lidar_K or None) of a fixture case; lidar_K as Python floats, which is what the reference was called with."""
    beams = g[tag + "_beams"] if tag + "_beams" in g else None
    return int(g[tag + "_H"]), int(g[tag + "_W"]), beams, None if beams is not None else tuple(float(v) for v in g["lidar_K"])


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_projection_equals_the_reference_exactly(golden, tag):
    H, W, beams, K = case(golden, tag)
    pts = golden[tag + "_points"]
    assert pts.dtype == np.float32 and ref.decision_margin_mask(pts, H, W, beams, K).all()      # the fixture's points are masked ones
    pano, inten = ref.project(pts, H, W, beams, K)
    assert pano.dtype == np.float64 and np.array_equal(pano, golden[tag + "_pano"]) and np.array_equal(inten, golden[tag + "_intensities"])
    assert (pano != 0).sum() > 500
    if beams is not None:
        assert not pano[0].any()                            # the reference's row rule: beam 0 falls off, row 0 is never written


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_back_projection_equals_the_reference(golden, tag):
    H, W, beams, K = case(golden, tag)
    pano, inten = golden[tag + "_pano"].astype(np.float64), golden[tag + "_intensities"].astype(np.float64)
    want = golden[tag + "_back"]
    got = ref.unproject(pano, inten, beams, K, as_reference=True)       # the reference's own mix of float32 angles and float64 ranges
    assert got.shape == want.shape == (int((pano != 0).sum()), 4) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12
    # the float64 form, which the device is measured against: the reference's float32 angles are within float32 rounding of it
    # (beta <= 2 pi: half an ulp 2.4e-7; cos, sin and their product 3 x 6e-8) x the range, below 80
    assert np.abs(ref.unproject(pano, inten, beams, K) - want).max() <= 80 * 4.2e-7
    if tag + "_dirs" in golden:
        assert np.abs(ref.pixel_dirs(H, W, beams, K, as_reference=True) - golden[tag + "_dirs"]).max() <= 1e-12
        assert np.abs(ref.pixel_dirs(H, W, beams, K) - golden[tag + "_dirs"]).max() <= 4.2e-7


@pytest.mark.parametrize("kind,H,W", [("uniform", 16, 512), ("waymo", 16, 512), ("neartie", 16, 512), ("waymo", 4, 8), ("neartie", 64, 2650)])
def test_keyed_minimum_equals_the_sequential_loop(kind, H, W):
    """oracle/range_view.points_to_pano is the reference's loop (float32 throughout on float32 points); on masked points the float64
    keyed minimum gives the same image, ties included."""
    import lidargs_scenes as sc
    from oracle import range_view as loop
    beams = sc.beam_table(H, kind)
    rng = np.random.default_rng(H * 1000 + W)
    pts = ref.masked_points(rng, 1500, H, W, beams)
    pts = np.concatenate([pts, pts[:200] * np.float32([1, 1, 1, 0.5])])                    # equal ranges, other intensities: the first wins
    want_p, want_i = loop.points_to_pano(pts, H, W, beams, 80)
    got_p, got_i = ref.project(pts, H, W, beams)
    assert np.array_equal(got_p, want_p) and np.array_equal(got_i, want_i)


def test_margin_mask_keeps_most_points_and_drops_the_boundary_ones():
    import lidargs_scenes as sc
    H, W = 16, 512
    beams = sc.beam_table(H, "uniform").astype(np.float64)
    pts = ref.random_points(np.random.default_rng(3), 4000, beams)
    assert 0.95 < ref.decision_margin_mask(pts, H, W, beams).mean() < 1.0
    step = 2 * np.pi / W
    el = float(beams[5] + beams[6]) / 2                                                    # a midpoint of two beams
    mk = lambda az, e, r: [r * np.cos(e) * np.cos(az), r * np.cos(e) * np.sin(az), r * np.sin(e), 0.5]
    hand = np.float32([mk(np.pi - 10.5 * step, float(beams[3]), 10.0),                     # half-way between columns 10 and 11
                       mk(np.pi - 10.0 * step, el, 10.0),                                  # half-way between beams 5 and 6
                       mk(np.pi - 10.0 * step, float(beams[3]), 80.0004),                  # 4e-4 from max_depth
                       mk(np.pi - 10.0 * step, float(beams[3]), 10.0),                     # clear of everything
                       [80.0, 0.0, 0.0, 0.5],                                              # exactly max_depth: decided, kept
                       [np.nan, 0.0, 1.0, 0.5]])
    assert ref.decision_margin_mask(hand, H, W, beams).tolist() == [False, False, False, True, True, False]
    K = (2.0, 26.9)
    assert 0.95 < ref.decision_margin_mask(ref.random_points(np.random.default_rng(4), 4000, lidar_K=K), H, W, lidar_K=K).mean() < 1.0


def test_header_parses_and_library_exports_exactly_the_declared_functions(hip_lib_built):
    import build_hip
    import native_lib_checks
    import range_view as rv
    typed = native_lib_checks.check_library(build_hip.TARGETS["rangeview"], DECLARED, rv._lib, hip_lib_built)
    assert build_hip.TARGETS["rangeview"].sources == {"range_view.hip": ["-ffp-contract=off"]}
    i, z, f, p = ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_void_p              # written from the header by eye
    assert typed["lidargs_rv_scratch_bytes"] == (z, (i, i))
    assert typed["lidargs_rv_project"] == (i, (i, p, i, i, p, f, f, f, p, i, p, p, p, z, p))
    assert typed["lidargs_rv_unproject"] == (i, (i, i, p, p, p, f, f, p, p, p, p, z, p))
    assert typed["lidargs_rv_ray_dirs"] == (i, (i, i, p, f, f, p, p))
    assert typed["lidargs_rv_last_error"] == (ctypes.c_char_p, ()) and typed["lidargs_rv_abi_version"] == (i, ())
    assert rv._lib.lidargs_rv_abi_version() == rv.ABI_VERSION == 1 and rv.PIXEL_ROWS == 1


def test_entry_points_validate_before_any_device_work(hip_lib_built):
    import range_view as rv
    lib = rv._lib
    err = lambda: lib.lidargs_rv_last_error().decode()
    buf = (ctypes.c_double * 64)()
    host = ctypes.cast(buf, ctypes.c_void_p)                                               # never dereferenced: every call below is refused
    odd = ctypes.c_void_p(host.value + 4)
    assert lib.lidargs_rv_scratch_bytes(64, 2650) >= 64 * 2650 * 8 and lib.lidargs_rv_scratch_bytes(0, 8) == 0
    assert lib.lidargs_rv_scratch_bytes(1 << 15, 1 << 14) == 0                             # H * W above 2^28
    big = 1 << 30
    assert lib.lidargs_rv_project(4, host, 0, 8, host, 0, 0, 80, None, 0, host, host, host, big, None) == -1 and "bad image size" in err()
    assert lib.lidargs_rv_project(-1, host, 4, 8, host, 0, 0, 80, None, 0, host, host, host, big, None) == -1 and "negative N" in err()
    assert lib.lidargs_rv_project(4, host, 4, 8, None, 2.0, 0.0, 80, None, 0, host, host, host, big, None) == -1 and "fov must be positive" in err()
    assert lib.lidargs_rv_project(4, host, 4, 8, host, 0, 0, 80, None, 2, host, host, host, big, None) == -1 and "unknown flags" in err()
    assert lib.lidargs_rv_project(4, None, 4, 8, host, 0, 0, 80, None, 0, host, host, host, big, None) == -1 and "NULL" in err()
    assert lib.lidargs_rv_project(4, host, 4, 8, host, 0, 0, 80, None, 0, host, None, host, big, None) == -1 and "NULL" in err()
    assert lib.lidargs_rv_project(4, odd, 4, 8, host, 0, 0, 80, None, 0, host, host, host, big, None) == -1 and "16-byte" in err()
    assert lib.lidargs_rv_project(4, host, 4, 8, host, 0, 0, 80, None, 0, host, host, host, 4 * 8 * 8 - 1, None) == -1 and "scratch" in err()
    assert lib.lidargs_rv_project(4, host, 4, 8, host, 0, 0, 80, None, 0, host, host, odd, big, None) == -1 and "scratch" in err()
    assert lib.lidargs_rv_unproject(4, -8, host, None, host, 0, 0, None, host, host, host, big, None) == -1 and "bad image size" in err()
    assert lib.lidargs_rv_unproject(4, 8, None, None, host, 0, 0, None, host, host, host, big, None) == -1 and "NULL" in err()
    assert lib.lidargs_rv_unproject(4, 8, host, None, host, 0, 0, None, host, None, host, big, None) == -1 and "NULL" in err()
    assert lib.lidargs_rv_unproject(4, 8, host, None, host, 0, 0, None, odd, host, host, big, None) == -1 and "16-byte" in err()
    assert lib.lidargs_rv_unproject(4, 8, host, None, host, 0, 0, None, host, host, host, 8, None) == -1 and "scratch" in err()
    assert lib.lidargs_rv_unproject(4, 8, host, None, None, 2.0, -1.0, None, host, host, host, big, None) == -1 and "fov must be positive" in err()
    assert lib.lidargs_rv_ray_dirs(4, 8, host, 0, 0, None, None) == -1 and "NULL" in err()
    assert lib.lidargs_rv_ray_dirs(0, 8, host, 0, 0, host, None) == -1 and "bad image size" in err()
    with pytest.raises(ctypes.ArgumentError):
        lib.lidargs_rv_project(4.0, host, 4, 8, host, 0, 0, 80, None, 0, host, host, host, big, None)


def test_get_beam_inclinations_is_the_reference_table(hip_lib_built):
    import range_view as rv
    from oracle import range_view as loop
    b = rv.get_beam_inclinations(2.4, 20.0, 16)
    assert b.dtype == np.float32 and np.array_equal(b, loop.fov_beam_table(2.4, 20.0, 16)) and np.all(np.diff(b) > 0)


def test_the_front_refuses_loudly_without_a_device(hip_lib_built):
    import range_view as rv
    beams = rv.get_beam_inclinations(2.4, 20.0, 4)
    pts = np.zeros((5, 4), dtype=np.float32)
    pano = np.zeros((4, 8))
    with pytest.raises(RuntimeError, match="CPU tensor"):                                  # no CPU path: a host tensor is refused, never computed in numpy
        rv.lidar_to_pano_with_intensities(torch.zeros(5, 4), 4, 8, beam_inclinations=beams)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        rv.pano_to_lidar(torch.zeros(4, 8), beam_inclinations=beams)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        rv.pano_to_lidar_with_intensities(pano, torch.zeros(4, 8), beam_inclinations=beams)
    with pytest.raises(RuntimeError, match=r"\[N, 4\]"):
        rv.lidar_to_pano_with_intensities(np.zeros((5, 3), dtype=np.float32), 4, 8, beam_inclinations=beams)
    with pytest.raises(RuntimeError, match="floating-point"):
        rv.lidar_to_pano_with_intensities(np.zeros((5, 4), dtype=np.int32), 4, 8, beam_inclinations=beams)
    with pytest.raises(RuntimeError, match="device tensor or a numpy array"):
        rv.lidar_to_pano_with_intensities([[0.0, 0.0, 1.0, 0.0]], 4, 8, beam_inclinations=beams)
    with pytest.raises(RuntimeError, match=r"\[H, W\]"):
        rv.pano_to_lidar(np.zeros((4, 8, 1)), beam_inclinations=beams)
    with pytest.raises(RuntimeError, match="elements"):
        rv.pano_to_lidar_with_intensities(pano, np.zeros((4, 7)), beam_inclinations=beams)
    for call in (lambda **kw: rv.lidar_to_pano_with_intensities(pts, 4, 8, **kw), lambda **kw: rv.pano_to_lidar(pano, **kw),
                 lambda **kw: rv.pano_to_lidar_with_intensities(pano, pano, **kw), lambda **kw: rv.ray_dirs(4, 8, **kw)):
        with pytest.raises(ValueError, match="exactly one of"):
            call()
        with pytest.raises(ValueError, match="exactly one of"):
            call(lidar_K=(2.0, 26.9), beam_inclinations=beams)
        with pytest.raises(ValueError, match="one per image row"):
            call(beam_inclinations=beams[:3])
        with pytest.raises(ValueError, match="ascending"):
            call(beam_inclinations=beams[::-1])
        with pytest.raises(ValueError, match="ascending"):
            call(beam_inclinations=[0.0, 0.1, float("nan"), 0.3])
        with pytest.raises(ValueError, match="fov > 0"):
            call(lidar_K=(2.0, 0.0))
    with pytest.raises(ValueError, match="transform"):
        rv.lidar_to_pano_with_intensities(pts, 4, 8, beam_inclinations=beams, transform=np.eye(3))
    with pytest.raises(ValueError, match="transform"):
        rv.pano_to_lidar(pano, beam_inclinations=beams, transform=np.full((4, 4), 1.0))
    with pytest.raises(ValueError, match="bad image size"):
        rv.lidar_to_pano_with_intensities(pts, 0, 8, beam_inclinations=beams)
    for n in (1 << 31, 1 << 32):                                                           # the C ABI takes N as int: 2^31 is the first N refused
        huge = np.broadcast_to(np.zeros((1, 4), dtype=np.float32), (n, 4))                 # a shape, no memory
        with pytest.raises(ValueError, match=r"N < 2\^31"):
            rv.lidar_to_pano_with_intensities(huge, 4, 8, beam_inclinations=beams)
    # nothing to do: answered without a native call (and so without a device)
    p, i = rv.lidar_to_pano_with_intensities(np.zeros((0, 4), dtype=np.float32), 4, 8, beam_inclinations=beams)
    assert p.shape == i.shape == (4, 8) and p.dtype == np.float64 and not p.any() and not i.any()
    assert rv.pano_to_lidar_with_intensities(pano, pano, beam_inclinations=list(beams)).shape == (0, 4)
    assert rv.pano_to_lidar(pano, lidar_K=(2.0, 26.9)).shape == (0, 3)
