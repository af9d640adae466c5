"""CPU tests of the per-view evaluation (include/lidargs_metrics.h, lidar-gs_amd/view_metrics.py): the numpy restatement
(tests/view_metrics_ref.py) against the fixture made by executing the reference's training_report loop on CPU torch
(tests/golden/make_view_metrics_golden.py), the header against the library's symbols, and the refusal of host tensors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import view_metrics_ref as R
from oracle import points_meter as pm_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lidargs_metrics.h")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "view_metrics_golden.npz"))
TAGS = ["a", "b", "c", "d", "e"]


def _case(tag):
    dmin, dmax = (float(v) for v in GOLD[f"{tag}_depth_range"])
    return GOLD[f"{tag}_render"], GOLD[f"{tag}_depth"], GOLD[f"{tag}_gt"], GOLD[f"{tag}_beams"], dmin, dmax


def close(got, want, slot):
    """The tolerances of the contract: means 2e-6 relative, PSNR 1e-4 dB, SSIM 2e-6, medians exact; NaN where the reference has NaN."""
    if np.isnan(want) or np.isnan(got):
        return np.isnan(want) and np.isnan(got)
    if np.isinf(want) or np.isinf(got):
        return got == want
    if slot in (5, 9):
        return got == want
    if slot == 1:
        return abs(got - want) <= 1e-4
    if slot == 2:
        return abs(got - want) <= 2e-6
    return abs(got - want) <= 2e-6 * abs(want)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_the_reference_fixture(tag):
    render, depth, gt, beams, dmin, dmax = _case(tag)
    pts = lambda dr, gd: pm_oracle.update(dr, gd, beams, 1.0)[:2]
    got = R.view_metrics(render, depth, gt, dmin, dmax, points=pts)
    want = GOLD[f"{tag}_out"]
    bad = [(R.NAMES[k], got[k], want[k]) for k in range(11) if not close(got[k], want[k], k)]
    assert not bad, bad


def test_fixture_pins_the_conventions():
    """What the fixture holds, stated: NaN in render[0] reaches every intensity value; 70 % ties give lower medians of 0; the strict
    > 0.5 and the clamp before the mask change the intensity error of case b."""
    assert np.isnan(GOLD["c_out"][[0, 1, 2, 3, 4, 5]]).all() and np.isfinite(GOLD["c_out"][[8, 9, 10]]).all()
    assert GOLD["d_out"][5] == 0.0 and GOLD["d_out"][9] == 0.0
    render, depth, gt, beams, dmin, dmax = _case("b")
    loose = render.copy(); loose[1][render[1] == 0.5] = 0.50001
    assert R.view_metrics(loose, depth, gt, dmin, dmax)[0] != GOLD["b_out"][0]
    unclamped = R.prepare(render, depth, gt, dmin, dmax)[0]
    assert unclamped.max() <= 1.0 and (render[0] > 1).any()


def test_lower_median_and_ssim_edges():
    assert R.lower_median(np.array([3.0, 1.0, 2.0, 4.0], np.float32)) == 2.0           # even n: the lower of the two middle values
    assert R.lower_median(np.array([3.0, 1.0, 2.0], np.float32)) == 2.0
    t = torch.tensor([3.0, 1.0, 2.0, 4.0])
    assert float(t.median()) == 2.0
    x = np.random.default_rng(0).random((9, 11)).astype(np.float32)
    assert abs(R.ssim(x, x) - 1.0) <= 1e-6
    with pytest.raises(ValueError):
        R.ssim(np.zeros((6, 20), np.float32), np.zeros((6, 20), np.float32))


def test_header_is_plain_c_and_exported(hip_lib_built):
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-x", "c", HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = set(re.findall(r"\b(lidargs_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert names == {"lidargs_view_metrics_scratch_bytes", "lidargs_view_metrics", "lidargs_view_metrics_ex"}
    out = subprocess.run(["nm", "-D", "--defined-only", hip_lib_built], capture_output=True, text=True).stdout
    assert names <= set(re.findall(r" T (lidargs_\w+)", out))


def test_c_abi_validates_before_device_work(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    lib.lidargs_last_error.restype = ctypes.c_char_p
    lib.lidargs_view_metrics_scratch_bytes.restype = ctypes.c_size_t
    ci, cf, cs = ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    call = lambda H, W: lib.lidargs_view_metrics(ci(H), ci(W), None, None, None, cf(5), cf(80), None, cf(0), cf(0), None, None, cs(0), None)
    assert call(6, 100) == -1 and b"H >= 7" in lib.lidargs_last_error()
    assert call(100, 6) == -1
    assert call(7, 7) == -1 and b"NULL" in lib.lidargs_last_error()
    assert lib.lidargs_view_metrics_scratch_bytes(ci(6), ci(100)) == 0
    assert lib.lidargs_view_metrics_scratch_bytes(ci(64), ci(2650)) >= 6 * 4 * 64 * 2650


@pytest.mark.parametrize("which", ["render", "depth", "gt_image"])
def test_host_tensors_are_refused(hip_lib_built, which):
    import view_metrics
    args = {"render": torch.zeros(2, 8, 8), "depth": torch.zeros(1, 8, 8), "gt_image": torch.zeros(3, 8, 8)}
    if torch.cuda.is_available():
        args = {k: (v if k == which else v.cuda()) for k, v in args.items()}
    with pytest.raises(RuntimeError):
        view_metrics.view_metrics(args["render"], args["depth"], args["gt_image"], intrinsics=(2.0, 26.9))
