"""GPU tests of include/lidargs_knn.h through its Python surface: simple_knn._C.distCUDA2 bit for bit against the float32 restatement
of tests/knn_ref.py, and anchor_init.voxelize_sample against the reference expression (np.array_equal, same dtype, same global-RNG use)."""
import numpy as np
import pytest
import torch

import knn_ref as K
import lidargs_scenes as sc

pytestmark = pytest.mark.gpu


def _dist(x, hip_lib_built):
    from simple_knn._C import distCUDA2
    return distCUDA2(torch.from_numpy(np.ascontiguousarray(x)).cuda()).cpu().numpy()


def _same_bits(a, b):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    diff = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
    assert diff.size == 0, f"{diff.size} of {a.size} differ, first {diff[:5]}: {a[diff[:5]]} vs {b[diff[:5]]}"


def _cloud(kind, P, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return (rng.normal(size=(P, 3)) * 10).astype(np.float32)
    if kind == "identical":
        return np.tile(np.array([[1.5, -2.25, 0.125]], np.float32), (P, 1))
    if kind == "repeat5":
        return np.tile(rng.uniform(-5, 5, (P // 5, 3)).astype(np.float32), (5, 1))
    if kind == "coplanar":
        x = rng.uniform(-20, 20, (P, 3)).astype(np.float32); x[:, 2] = 0
        return x
    if kind == "collinear":
        t = rng.uniform(-100, 100, P)
        return np.stack([t, 0.5 * t + 3, np.full(P, -2.0)], 1).astype(np.float32)
    if kind == "outliers":
        x = rng.normal(size=(P, 3)).astype(np.float32)
        x[rng.choice(P, 6, replace=False)] = rng.choice([-1, 1], (6, 3)) * 1e6 * rng.uniform(0.5, 1, (6, 3))
        return x.astype(np.float32)
    if kind == "nonfinite":
        x = rng.normal(size=(P, 3)).astype(np.float32)
        idx = rng.choice(P, 40, replace=False)
        x[idx[:10], 0] = np.nan; x[idx[10:20]] = np.nan; x[idx[20:30], 1] = np.inf; x[idx[30:], 2] = -np.inf
        return x
    raise KeyError(kind)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 1000])
def test_distcuda2_small_bitwise(hip_lib_built, P):
    x = _cloud("random", P, P)
    _same_bits(_dist(x, hip_lib_built), K.dist3_brute(x))


@pytest.mark.parametrize("kind,P", [("identical", 3000), ("repeat5", 5000), ("coplanar", 6000), ("collinear", 6000), ("outliers", 6000),
                                    ("nonfinite", 4000)])
def test_distcuda2_special_clouds_bitwise(hip_lib_built, kind, P):
    x = _cloud(kind, P, 7)
    _same_bits(_dist(x, hip_lib_built), K.dist3_brute(x))


def test_distcuda2_65537_bitwise(hip_lib_built):
    x = _cloud("random", 65537, 3)
    ref, _ = K.dist3_kdtree(x)
    _same_bits(_dist(x, hip_lib_built), ref)


def test_distcuda2_accumulated_scan_1m_bitwise(hip_lib_built):
    x = sc.accumulated_scan(1_000_000, 1)
    ref, _ = K.dist3_kdtree(x)
    _same_bits(_dist(x, hip_lib_built), ref)


def test_distcuda2_street_scene_2m_bitwise(hip_lib_built):
    x = sc.street_scene(2_000_000, 16, 1)["means3D"]
    ref, _ = K.dist3_kdtree(x)
    _same_bits(_dist(x, hip_lib_built), ref)


def test_distcuda2_permutation_invariant_and_strided(hip_lib_built):
    from simple_knn._C import distCUDA2
    x = torch.from_numpy(sc.accumulated_scan(200_000, 4)).cuda()
    perm = torch.from_numpy(np.random.default_rng(5).permutation(x.shape[0])).cuda()
    a = distCUDA2(x)
    b = distCUDA2(x[perm])
    assert torch.equal(b.view(torch.int32), a[perm].view(torch.int32))
    x4 = torch.cat([x, torch.full_like(x[:, :1], float("nan"))], 1)      # the 4th column must not be read
    v = x4[:, :3]
    assert not v.is_contiguous()
    assert torch.equal(distCUDA2(v).view(torch.int32), a.view(torch.int32))
    assert distCUDA2(torch.empty((0, 3), device="cuda")).shape == (0,)


# ---- voxelize_sample ---------------------------------------------------------------------------------------------------------

def _voxel_numpy_cases():
    rng = np.random.default_rng(21)
    h = (np.arange(-8, 9) + 0.5).astype(np.float32) * np.float32(0.25)
    return [("f32", rng.uniform(-50, 50, (20000, 3)).astype(np.float32), 0.37),
            ("f64", rng.uniform(-50, 50, (20000, 3)), 0.37),
            ("half", np.stack(np.meshgrid(h, h[::-1], h, indexing="ij"), -1).reshape(-1, 3), 0.25),
            ("half64", np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3).astype(np.float64), 0.25),
            ("neg", -rng.uniform(0, 3, (8000, 3)).astype(np.float32), 0.1),
            ("wide", np.concatenate([rng.uniform(-1, 1, (3000, 3)), [[3e6, -3e6, 2e6]]]), 0.5),
            ("wide32", np.concatenate([rng.uniform(-1, 1, (3000, 3)), [[3e6, -3e6, 2e6]]]).astype(np.float32), 0.25),
            ("one", np.array([[1.25, -0.75, 3.0]], np.float32), 0.5),
            ("empty", np.zeros((0, 3), np.float32), 0.5)]


@pytest.mark.parametrize("name,data,v", _voxel_numpy_cases(), ids=[c[0] for c in _voxel_numpy_cases()])
def test_voxelize_sample_numpy_matches_reference(hip_lib_built, name, data, v):
    from anchor_init import voxelize_sample
    a, b = data.copy(), data.copy()
    np.random.seed(123)
    got = voxelize_sample(a, voxel_size=v)
    st_got = np.random.get_state()[1].copy()
    np.random.seed(123)
    np.random.shuffle(b)                                                 # the reference, scene/gaussian_model.py:272-276
    ref = np.unique(np.round(b / v), axis=0) * v
    assert isinstance(got, np.ndarray) and got.dtype == ref.dtype and got.shape == ref.shape
    assert np.array_equal(got, ref)
    assert np.array_equal(a, b) and np.array_equal(st_got, np.random.get_state()[1])     # same shuffle, same RNG stream


def test_voxelize_sample_device_tensor(hip_lib_built):
    from anchor_init import voxelize_sample
    x = sc.accumulated_scan(300_000, 6)
    for dt, v in ((np.float32, 0.05), (np.float64, 0.02)):
        xd = x.astype(dt)
        got = voxelize_sample(torch.from_numpy(xd).cuda(), v)
        assert got.is_cuda and got.dtype == (torch.float32 if dt == np.float32 else torch.float64)
        assert np.array_equal(got.cpu().numpy(), K.voxelize_reference(xd, v))
    with pytest.raises(RuntimeError):
        voxelize_sample(torch.tensor([[0.0, float("nan"), 1.0]], device="cuda"), 0.1)
    with pytest.raises(RuntimeError):
        voxelize_sample(torch.zeros((3, 3), device="cuda"), 0.0)


def test_create_from_pcd_numeric_steps(hip_lib_built):
    """scene/gaussian_model.py:278-305 with the drop-ins against the same steps on the restatements: median voxel size, anchors, scales."""
    from simple_knn._C import distCUDA2
    from anchor_init import voxelize_sample
    points = sc.accumulated_scan(400_000, 8).astype(np.float64)          # pcd.points (float64 in a BasicPointCloud)
    # voxel size (:283-287)
    init_dist = distCUDA2(torch.tensor(points).float().cuda()).float().cuda()
    median, _ = torch.kthvalue(init_dist, int(init_dist.shape[0] * 0.5))
    ref_dist, _ = K.dist3_kdtree(points.astype(np.float32))
    ref_median, _ = torch.kthvalue(torch.from_numpy(ref_dist), int(ref_dist.shape[0] * 0.5))
    voxel_size = median.item()
    assert voxel_size == ref_median.item() and voxel_size > 0
    # anchors (:293)
    p_got, p_ref = points.copy(), points.copy()
    np.random.seed(9)
    anchors = voxelize_sample(p_got, voxel_size=voxel_size)
    np.random.seed(9)
    np.random.shuffle(p_ref)
    anchors_ref = np.unique(np.round(p_ref / voxel_size), axis=0) * voxel_size
    assert anchors.dtype == np.float64 and np.array_equal(anchors, anchors_ref)
    # scales (:300-301)
    fused = torch.tensor(np.asarray(anchors)).float().cuda()
    dist2 = torch.clamp_min(distCUDA2(fused).float().cuda(), 0.0000001)
    scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 6)
    ref2, _ = K.dist3_kdtree(np.asarray(anchors_ref).astype(np.float32))
    ref_scales = torch.log(torch.sqrt(torch.clamp_min(torch.from_numpy(ref2).cuda(), 0.0000001)))[..., None].repeat(1, 6)
    assert torch.equal(scales.view(torch.int32), ref_scales.view(torch.int32))
