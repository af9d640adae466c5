"""CPU tests of the torch_scatter stand-in (lidar-gs_amd/torch_scatter/, liblidargs_scatter.so, include_scatter/): the restatement
tests/scatter_ref.py against cases worked by hand and against torch's CPU scatter_reduce_, the library against its header, the argument
validation of the C ABI (which precedes any device work, so host pointers do), what the Python front refuses, and the build."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scatter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED = {"lidargs_scatter_scratch_bytes", "lidargs_scatter_extreme", "lidargs_scatter_extreme_backward", "lidargs_scatter_last_error",
            "lidargs_scatter_abi_version"}
NAN = float("nan")


def test_restatement_on_a_tie_an_empty_group_and_a_nan():
    f, i = np.float32, np.int64
    # a tie: 3 at positions 1 and 2 of group 0 -> the lower position; the minimum 1 is alone
    v, a = ref.scatter_max(f([1, 3, 3, 2]), i([0, 0, 0, 1]))
    assert v.tolist() == [3, 2] and a.tolist() == [1, 3] and v.dtype == np.float32 and a.dtype == np.int64
    v, a = ref.scatter_min(f([1, 3, 3, 2]), i([0, 0, 0, 1]))
    assert v.tolist() == [1, 2] and a.tolist() == [0, 3]
    # an empty group (1) and trailing empty groups (3, 4): value 0, arg = E = 3
    v, a = ref.scatter_max(f([-5, -7, -6]), i([0, 2, 2]), dim_size=5)
    assert v.tolist() == [-5, 0, -6, 0, 0] and a.tolist() == [0, 3, 2, 3, 3]
    # a NaN makes its group NaN whatever else it holds, and the first NaN is the winner; -0.0 < +0.0
    src = f([1, NAN, 9, NAN, -0.0, 0.0, 0.0])
    for fn, zero_arg in ((ref.scatter_max, 5), (ref.scatter_min, 4)):
        v, a = fn(src, i([0, 0, 0, 0, 1, 1, 1]))
        assert np.isnan(v[0]) and a.tolist() == [1, zero_arg] and v[1] == 0 and bool(np.signbit(v[1])) == (fn is ref.scatter_min)
        assert v[:1].view(np.uint32)[0] == 0x7FC00000
    # out=: the initial value wins (5 > 3), ties (3: kept, arg = E) and loses (1 < 3)
    v, a = ref.scatter_max(f([3, 3, 3]), i([0, 1, 2]), out=f([5, 3, 1]))
    assert v.tolist() == [5, 3, 3] and a.tolist() == [3, 3, 2]
    v, a = ref.scatter_min(f([3, 3, 3]), i([0, 1, 2]), out=f([5, 3, 1]))
    assert v.tolist() == [3, 3, 1] and a.tolist() == [0, 3, 3]
    # a 2-D src with a 1-D index at dim 0, and the gradient: grad_out at the arg positions only
    src = f([[1, 8], [4, 8], [4, 2]])
    v, a = ref.scatter_max(src, i([1, 1, 0]), dim=0)
    assert v.tolist() == [[4, 2], [4, 8]] and a.tolist() == [[2, 2], [1, 0]]
    g = ref.scatter_extreme_grad(f([[10, 20], [30, 40]]), i([1, 1, 0]), a, src.shape, dim=0)
    assert g.tolist() == [[0, 40], [30, 0], [10, 20]]
    v, a = ref.scatter_max(f([1, 2, 3]), i([0, -1, 5]), dim_size=2, skip_bad=True)
    assert v.tolist() == [1, 0] and a.tolist() == [0, 3]
    with pytest.raises(IndexError):
        ref.scatter_max(f([1, 2, 3]), i([0, -1, 5]), dim_size=2)


@pytest.mark.parametrize("shape,dim,G", [((500,), 0, 37), ((300, 7), 0, 50), ((5, 200, 3), 1, 11), ((4, 90), -1, 200)])
def test_restatement_values_equal_torch_cpu_scatter_reduce_bit_for_bit(shape, dim, G):
    rng = np.random.default_rng(sum(shape) + G)
    src = rng.standard_normal(shape).astype(np.float32)
    index = rng.integers(0, G, shape)                       # a full-shape index, as scatter_reduce_ takes it
    out_shape = list(shape)
    out_shape[dim] = G
    for fn, how in ((ref.scatter_max, "amax"), (ref.scatter_min, "amin")):
        want = torch.zeros(out_shape).scatter_reduce_(dim % len(shape), torch.from_numpy(index), torch.from_numpy(src), how, include_self=False)
        got, arg = fn(src, index, dim=dim, dim_size=G)
        assert ref.same_bits(got, want.numpy())
        hit = arg < shape[dim]                              # the arg points at an element of that group with that value
        safe = np.where(hit, arg, 0)
        assert np.array_equal(np.take_along_axis(src, safe, dim % len(shape))[hit], got[hit])
        assert np.array_equal(np.take_along_axis(index, safe, dim % len(shape))[hit], np.indices(out_shape)[dim % len(shape)][hit])
        assert not got[~hit].any()


def test_header_parses_and_library_exports_exactly_the_declared_functions(hip_lib_built):
    import build_hip
    import native_lib_checks
    import torch_scatter as ts
    target = build_hip.TARGETS["scatter"]
    typed = native_lib_checks.check_library(target, DECLARED, ts._lib, hip_lib_built)
    assert target.sources == {"scatter.hip": []} and os.path.exists(os.path.join(build_hip.CSRC, "scatter.hip"))
    assert target.include == os.path.join(ROOT, "include_scatter") and os.listdir(target.include) == ["lidargs_scatter.h"]
    for t in build_hip.TARGETS.values():
        assert t is target or native_lib_checks.exports(t.out).isdisjoint(DECLARED), t.name
    i, z, p = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p                                # written from the header by eye
    assert typed["lidargs_scatter_scratch_bytes"] == (z, (z,))
    assert typed["lidargs_scatter_extreme"] == (i, (i, z, z, z, z, p, p, z, z, z, i, p, p, p, z, p))
    assert typed["lidargs_scatter_extreme_backward"] == (i, (z, z, z, z, p, z, z, z, p, p, p, p))
    assert typed["lidargs_scatter_last_error"] == (ctypes.c_char_p, ()) and typed["lidargs_scatter_abi_version"] == (i, ())
    assert ts._lib.lidargs_scatter_abi_version() == ts.ABI_VERSION == 1 and (ts.MAX, ts.MIN) == (0, 1)
    assert isinstance(ts.__version__, str) and ts.__version__[0].isdigit()


def test_entry_points_validate_before_any_device_work(hip_lib_built):
    import torch_scatter as ts
    lib = ts._lib
    err = lambda: lib.lidargs_scatter_last_error().decode()
    buf = (ctypes.c_double * 64)()
    host = ctypes.cast(buf, ctypes.c_void_p)                                               # never dereferenced: every call below is refused
    odd = ctypes.c_void_p(host.value + 4)
    big = 1 << 40
    assert lib.lidargs_scatter_scratch_bytes(0) == 0 and lib.lidargs_scatter_scratch_bytes(1000) == 8000
    assert lib.lidargs_scatter_scratch_bytes(1 << 61) == 0                                 # more elements than a call takes
    fwd = lambda op=0, A=1, E=4, B=2, G=3, src=host, index=host, init=0, out=host, arg=host, scratch=host, nb=big: \
        lib.lidargs_scatter_extreme(op, A, E, B, G, src, index, 0, 1, 0, init, out, arg, scratch, nb, None)
    assert fwd(op=2) == -1 and "unknown op" in err()
    assert fwd(op=-1) == -1 and "unknown op" in err()
    assert fwd(init=2) == -1 and "use_initial" in err()
    assert fwd(E=1 << 31) == -1 and "below 2^31" in err()
    assert fwd(A=1 << 40, E=1 << 30, B=1 << 20) == -1 and "does not fit" in err()
    assert fwd(A=1 << 40, G=1 << 40, B=1 << 20) == -1 and "does not fit" in err()
    assert fwd(A=1 << 30, E=1 << 30, B=4) == -1 and "does not fit" in err()                 # fits 64 bits, above what a call takes
    for name in ("src", "index", "out", "arg", "scratch"):
        assert fwd(**{name: None}) == -1 and "NULL" in err(), name
    assert fwd(nb=1 * 3 * 2 * 8 - 1) == -1 and "scratch" in err()
    assert fwd(scratch=odd) == -1 and "scratch" in err()
    bwd = lambda A=1, E=4, B=2, G=3, index=host, arg=host, grad_out=host, grad_src=host: \
        lib.lidargs_scatter_extreme_backward(A, E, B, G, index, 0, 1, 0, arg, grad_out, grad_src, None)
    assert bwd(E=1 << 31) == -1 and "below 2^31" in err()
    assert bwd(A=1 << 40, E=1 << 30, B=1 << 20) == -1 and "does not fit" in err()
    for name in ("index", "arg", "grad_out", "grad_src"):
        assert bwd(**{name: None}) == -1 and "NULL" in err(), name
    # nothing to write: 0 at once, whatever the pointers
    assert fwd(A=0) == 0 and fwd(B=0) == 0 and fwd(G=0) == 0 and fwd(E=0, G=0, src=None, index=None, out=None, arg=None, scratch=None, nb=0) == 0
    assert bwd(A=0) == 0 and bwd(E=0) == 0 and bwd(B=0, index=None, arg=None, grad_out=None, grad_src=None) == 0
    with pytest.raises(ctypes.ArgumentError):
        fwd(op=0.0)
    with pytest.raises(ctypes.ArgumentError):
        fwd(E=4.0)


def test_the_front_refuses_loudly_without_a_device(hip_lib_built):
    import torch_scatter as ts
    src, index = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    for fn in (ts.scatter_max, ts.scatter_min, lambda *a, **k: ts.scatter(*a, reduce="max", **k), lambda *a, **k: ts.scatter(*a, reduce="min", **k)):
        with pytest.raises(RuntimeError, match="HIP device"):                              # no CPU path: a host tensor is refused, never computed by torch
            fn(src, index, dim=0)
        with pytest.raises(RuntimeError, match="must be a torch.Tensor"):
            fn(src.numpy(), index, dim=0)
    for fn in (ts.scatter_max, ts.scatter_min):                                            # the dtypes, before the device is looked at
        with pytest.raises(RuntimeError, match=r"`src` must be torch\.float32, got torch\.float16"):
            fn(src.half(), index, dim=0)
        with pytest.raises(RuntimeError, match=r"`src` must be torch\.float32, got torch\.int64"):
            fn(src.long(), index, dim=0)
        with pytest.raises(RuntimeError, match=r"`index` must be torch\.int64, got torch\.int32"):
            fn(src, index.int(), dim=0)
        with pytest.raises(RuntimeError, match=r"`out` must be torch\.float32"):
            fn(src, index, dim=0, out=torch.zeros(2, 3, dtype=torch.float64))
        with pytest.raises(RuntimeError, match="`out` requires grad"):
            fn(src, index, dim=0, out=torch.zeros(2, 3, requires_grad=True))
    for reduce, name in (("sum", "scatter_sum"), ("add", "scatter_add"), ("mean", "scatter_mean"), ("mul", "scatter_mul")):
        with pytest.raises(NotImplementedError, match=name + r"`.*Tensor\.scatter_(add|reduce)_"):
            ts.scatter(src, index, dim=0, reduce=reduce)
    with pytest.raises(NotImplementedError, match="scatter_sum"):                          # torch_scatter's default reduce
        ts.scatter(src, index, dim=0)
    with pytest.raises(ValueError, match="unknown reduce"):
        ts.scatter(src, index, dim=0, reduce="median")
    with pytest.raises(NotImplementedError, match=r"scatter_add`.*Tensor\.scatter_add_"):
        ts.scatter_add
    with pytest.raises(NotImplementedError, match=r"scatter_mean`.*Tensor\.scatter_reduce_"):
        from torch_scatter import scatter_mean  # noqa: F401
    with pytest.raises(NotImplementedError, match="segment_csr"):
        ts.segment_csr
    for name in ("scatter_sum", "scatter_add", "scatter_mean", "scatter_mul", "scatter_softmax", "segment_coo", "segment_csr", "gather_csr"):
        assert name not in vars(ts) and name not in ts.__all__
    with pytest.raises(AttributeError):                                                    # what torch_scatter does not have either stays an AttributeError
        ts.no_such_name
    assert not hasattr(ts, "__wrapped__")
    from torch_scatter import scatter, scatter_max, scatter_min  # noqa: F401  (scene/gaussian_model.py:15)


def test_the_reference_import_resolves_with_only_the_package_directory_on_the_path(hip_lib_built, tmp_path):
    """scene/gaussian_model.py:15 in a fresh interpreter whose only addition to the path is lidar-gs_amd/ (this test is about that process)."""
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "lidar-gs_amd"))
    r = subprocess.run([sys.executable, "-c", "from torch_scatter import scatter_max; import torch_scatter; print(torch_scatter.__file__)"],
                       capture_output=True, text=True, cwd=tmp_path, env=env)
    assert r.returncode == 0, r.stderr
    assert os.path.samefile(r.stdout.strip().splitlines()[-1], os.path.join(ROOT, "lidar-gs_amd", "torch_scatter", "__init__.py"))


def test_the_library_is_rebuilt_for_its_own_files_only_and_builds_once(hip_lib_built):
    import build_hip
    assert list(build_hip.TARGETS) == ["hip", "optim", "decode_options", "tcnn", "rangeview", "scatter"]
    assert build_hip.all_targets() == list(build_hip.TARGETS.values())
    target = build_hip.TARGETS["scatter"]
    source, header = os.path.join(build_hip.CSRC, "scatter.hip"), os.path.join(target.include, "lidargs_scatter.h")
    d = build_hip.deps(target)
    assert all(os.path.exists(f) for f in d)
    assert {source, header, os.path.join(build_hip.CSRC, "lidargs_status.h"), os.path.abspath(build_hip.__file__)} <= set(d)
    assert not any(source in build_hip.deps(t) for t in build_hip.TARGETS.values() if t is not target)
    assert len({t.out for t in build_hip.all_targets()}) == len({t.include for t in build_hip.all_targets()}) == len(build_hip.all_targets())
    assert not build_hip.stale(target)
    before = os.stat(target.out).st_mtime_ns
    assert os.path.abspath(build_hip.build()) == os.path.abspath(hip_lib_built)
    assert os.stat(target.out).st_mtime_ns == before
