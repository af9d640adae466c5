"""CPU tests of the simple_knn drop-in and the device voxel sampling (include/lidargs_knn.h): the import path the reference uses, the
argument errors, the C ABI's validation before any device work, and the host restatements (tests/knn_ref.py) the GPU tests compare
against -- distCUDA2's float32 contract against a float64 k-d tree, voxelize_sample's key arithmetic against the reference expression."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import knn_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lidargs_knn.h")


def test_simple_knn_import_path(hip_lib_built):
    """gaussian_model.py:21 of the reference, unchanged."""
    from simple_knn._C import distCUDA2
    assert callable(distCUDA2)
    from anchor_init import voxelize_sample
    assert callable(voxelize_sample)


def test_header_is_plain_c_and_exported(hip_lib_built):
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-x", "c", HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = set(re.findall(r"\b(lidargs_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert names == {"lidargs_knn_scratch_bytes", "lidargs_knn_mean_dist", "lidargs_voxelize_scratch_bytes", "lidargs_voxelize_sample"}
    out = subprocess.run(["nm", "-D", "--defined-only", hip_lib_built], capture_output=True, text=True).stdout
    assert names <= set(re.findall(r" T (lidargs_\w+)", out))


@pytest.mark.parametrize("bad", ["cpu", "shape", "dtype", "dim"])
def test_distcuda2_argument_errors(hip_lib_built, bad):
    from simple_knn._C import distCUDA2
    x = {"cpu": torch.zeros(4, 3), "shape": torch.zeros(4, 2), "dtype": torch.zeros(4, 3, dtype=torch.float64),
         "dim": torch.zeros(4, 3, 1)}[bad]
    if torch.cuda.is_available():
        x = x.cuda() if bad != "cpu" else x
    with pytest.raises(RuntimeError):
        distCUDA2(x)


def test_voxelize_argument_errors(hip_lib_built):
    from anchor_init import voxelize_device
    with pytest.raises(RuntimeError):
        voxelize_device(torch.zeros(4, 3), 0.1)                       # not on a device: no CPU path


def test_c_abi_validates_before_device_work(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    lib.lidargs_last_error.restype = ctypes.c_char_p
    lib.lidargs_knn_scratch_bytes.restype = ctypes.c_size_t
    lib.lidargs_voxelize_scratch_bytes.restype = ctypes.c_size_t
    c_int, c_size, c_dbl = ctypes.c_int, ctypes.c_size_t, ctypes.c_double
    assert lib.lidargs_knn_mean_dist(c_int(-1), None, c_int(3), None, None, c_size(0), None) == -1
    assert lib.lidargs_knn_mean_dist(c_int(10), None, c_int(2), None, None, c_size(0), None) == -1
    assert b"row_stride" in lib.lidargs_last_error()
    assert lib.lidargs_knn_mean_dist(c_int(10), None, c_int(3), None, None, c_size(0), None) == -1       # NULL pointers
    assert lib.lidargs_knn_mean_dist(c_int(0), None, c_int(3), None, None, c_size(0), None) == 0        # P = 0: nothing to do
    assert lib.lidargs_knn_scratch_bytes(c_int(0)) == 0 and lib.lidargs_knn_scratch_bytes(c_int(1000)) >= 1000 * 40
    alloc = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)(lambda u, n: 0)
    for v, dbl in ((0.0, 0), (-1.0, 1), (float("nan"), 0), (float("inf"), 1), (1e-50, 0)):              # 1e-50 is 0 in float32
        assert lib.lidargs_voxelize_sample(c_int(5), None, c_int(dbl), c_dbl(v), None, c_size(0), alloc, None, None) == -1
        assert b"voxel_size" in lib.lidargs_last_error()
    assert lib.lidargs_voxelize_sample(c_int(0), None, c_int(0), c_dbl(0.1), None, c_size(0), alloc, None, None) == 0


# ---- the distCUDA2 restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,P", [(0, 50), (1, 700), (2, 3000)])
def test_restatement_agrees_with_float64_kdtree(seed, P):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(P, 3)) * rng.uniform(0.1, 100.0, (P, 1))).astype(np.float32)
    got = K.dist3_brute(x)
    D, _ = cKDTree(x.astype(np.float64)).query(x.astype(np.float64), k=4)
    ref = (D[:, 1:] ** 2).mean(1)
    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=0)
    kd, n_brute = K.dist3_kdtree(x)
    assert np.array_equal(kd, got)


def test_restatement_sentinels():
    fmax = np.finfo(np.float32).max
    assert np.all(np.isposinf(K.dist3_brute(np.zeros((1, 3), np.float32))))
    assert np.all(np.isposinf(K.dist3_brute(np.array([[0, 0, 0], [1, 2, 3]], np.float32))))
    r3 = K.dist3_brute(np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32))
    assert np.all(np.isfinite(r3)) and np.allclose(r3 / (fmax / 3), 1.0, rtol=1e-6)
    assert r3[0] == np.float32((np.float32(1.0) + np.float32(4.0)) + np.float32(fmax)) / np.float32(3)
    x = np.repeat(np.random.default_rng(3).normal(size=(40, 3)).astype(np.float32), 4, axis=0)     # every point 4 times: 3 copies at 0
    assert np.all(K.dist3_brute(x) == 0.0)
    y = np.random.default_rng(4).normal(size=(30, 3)).astype(np.float32)
    yb = y.copy(); yb[[3, 7]] = np.nan; yb[11, 1] = np.inf; yb[12, 2] = -np.inf
    r = K.dist3_brute(yb)
    assert np.all(np.isposinf(r[[3, 7, 11, 12]]))
    keep = np.setdiff1d(np.arange(30), [3, 7, 11, 12])
    assert np.array_equal(r[keep], K.dist3_brute(y[keep]))               # non-finite rows are nobody's neighbours


def test_accumulated_scan_shape():
    import lidargs_scenes as sc
    x = sc.accumulated_scan(20000, 5)
    assert x.shape == (20000, 3) and x.dtype == np.float32 and np.isfinite(x).all()
    assert np.array_equal(x, sc.accumulated_scan(20000, 5))
    n = np.linalg.norm(x.astype(np.float64), axis=1)
    assert 1 <= int((n > 900).sum()) <= 8
    assert 0.02 * 20000 <= 20000 - np.unique(x, axis=0).shape[0] <= 0.04 * 20000


# ---- the voxelize_sample key arithmetic ------------------------------------------------------------------------------------------

def _voxel_cases():
    rng = np.random.default_rng(11)
    yield "f32", rng.uniform(-50, 50, (5000, 3)).astype(np.float32), 0.37
    yield "f64", rng.uniform(-50, 50, (5000, 3)), 0.37
    h = (np.arange(-8, 9) + 0.5).astype(np.float32) * np.float32(0.25)                     # exact half voxels: half to even
    yield "half", np.stack(np.meshgrid(h, h[::-1], h, indexing="ij"), -1).reshape(-1, 3), 0.25
    yield "neg", -rng.uniform(0, 3, (2000, 3)).astype(np.float32), 0.1
    yield "wide", np.concatenate([rng.uniform(-1, 1, (3000, 3)), [[3e6, -3e6, 2e6]]]).astype(np.float64), 0.5   # > 2^22 voxels per axis
    yield "dup", np.repeat(rng.normal(size=(50, 3)).astype(np.float32), 7, 0), 0.01
    yield "one", np.array([[1.25, -0.75, 3.0]], np.float32), 0.5
    yield "empty", np.zeros((0, 3), np.float32), 0.5
    yield "scan", None, 0.05


@pytest.mark.parametrize("name,data,v", list(_voxel_cases()), ids=[c[0] for c in _voxel_cases()])
def test_voxelize_restatement_matches_reference(name, data, v):
    if data is None:
        import lidargs_scenes as sc
        data = sc.accumulated_scan(20000, 2)
        data = data[np.linalg.norm(data, axis=1) < 500]
    ref = K.voxelize_reference(data, v)
    got, words = K.voxelize_restatement(data, v)
    assert got.dtype == ref.dtype == (np.float32 if data.dtype == np.float32 else np.float64)
    assert np.array_equal(got, ref)
    if name == "wide":
        assert words >= 3                                                  # the key does not fit one 64-bit pack


def test_voxelize_restatement_refuses_non_finite():
    with pytest.raises(RuntimeError):
        K.voxelize_restatement(np.array([[0, 0, np.nan]], np.float32), 0.1)
