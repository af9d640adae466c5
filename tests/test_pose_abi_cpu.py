"""CPU tests of the pose entry points' boundary (include_pose/lidargs_pose.h, prefix `lgpose_`, part of liblidargs_hip.so): the header is
plain C and declares exactly the expected functions, the library exports exactly those under that prefix, the binding's one CDLL types
them from the header, and arguments are refused before any device work.  The `lidargs_*` side of the library is tests/test_abi_cpu.py's."""
import ctypes

import pytest

import build_hip
import lidargs_abi
from native_lib_checks import check_family

DECLARED = {"lgpose_backward_view", "lgpose_view_partial_floats", "lgpose_debug_view_backward"}


def test_header_library_and_binding_agree(hip_lib_built):
    typed = check_family("pose", "lidargs_pose.h", DECLARED, hip_lib_built)
    i, f, z, p = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p   # written from the header by eye
    back = lidargs_abi.signatures()["lidargs_backward"]
    assert typed["lgpose_backward_view"] == (i, back[1] + (p, p, z))       # lidargs_backward's list + three
    assert typed["lgpose_view_partial_floats"] == (z, (i,))
    assert typed["lgpose_debug_view_backward"] == (i, (i, p, p, p, f, p, p, p) + (p,) * 12 + (p, p, p, p, p, p, z, p))


def test_a_declared_function_the_library_lacks_is_an_import_error(hip_lib_built, tmp_path):
    (tmp_path / "x.h").write_text("int lgpose_not_there(int a);\n")
    with pytest.raises(ImportError, match="does not export lgpose_not_there"):
        lidargs_abi.load(hip_lib_built, families=(build_hip.Family("tmp", str(tmp_path), "lgpose"),))


def test_arguments_are_refused_before_any_device_work(hip_lib_built):
    from diff_lidargs_rasterization import _C
    lib = _C._lib
    assert lib.lgpose_view_partial_floats(0) == 0 and lib.lgpose_view_partial_floats(-3) == 0
    assert lib.lgpose_view_partial_floats(1) == 16 and lib.lgpose_view_partial_floats(256) == 16 and lib.lgpose_view_partial_floats(257) == 32
    args = [-1, 0, 0, 0, None, 64, 8] + [None] * 4 + [1.0] + [None] * 6 + [1.0, 1.0] + [None] * 20 + [0, None, None, None, 0]
    assert lib.lgpose_backward_view(*args) == -1 and b"backward_view" in lib.lidargs_last_error()
    args[0] = 4
    assert lib.lgpose_backward_view(*args) == -1 and b"dL_dviewmatrix is NULL" in lib.lidargs_last_error()
    hook = [-1, None, None, None, 1.0] + [None] * 3 + [None] * 12 + [None] * 6 + [0, None]
    assert lib.lgpose_debug_view_backward(*hook) == -1 and b"debug_view_backward" in lib.lidargs_last_error()
    with pytest.raises(ctypes.ArgumentError):
        lib.lgpose_view_partial_floats(1.5)
