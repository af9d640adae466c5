"""CPU tests of the surfel pose entry points' boundary (include_surfel_pose/lidargs_surfel_pose.h, prefix `lgsfpose_`, part of
liblidargs_hip.so): the header is plain C99 and declares exactly the expected functions, the library exports exactly those under that
prefix, the surfel binding types them from the header on the process' one CDLL, and arguments are refused before any device work.
The 3-D form's side is tests/test_pose_abi_cpu.py's, the `lidargs_*` side tests/test_abi_cpu.py's."""
import ctypes

import pytest

import lidargs_abi
from native_lib_checks import check_family

DECLARED = {"lgsfpose_backward_view", "lgsfpose_view_partial_floats", "lgsfpose_debug_view_backward"}
ALIGNED = ctypes.c_void_p(0x1000)                                           # a pointer that passes the checks and is never dereferenced


def test_header_library_and_binding_agree(hip_lib_built):
    typed = check_family("surfel_pose", "lidargs_surfel_pose.h", DECLARED, hip_lib_built)
    i, f, z, p = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p   # written from the header by eye
    back = lidargs_abi.signatures()["lidargs_surfel_backward"]
    assert typed["lgsfpose_backward_view"] == (i, back[1] + (p, p, z))      # lidargs_surfel_backward's list + three
    assert typed["lgsfpose_view_partial_floats"] == (z, (i,))
    assert typed["lgsfpose_debug_view_backward"] == (i, (i, i, i, p, p, p, f, p, p, p, p) + (p,) * 9 + (p, p, p, p, p, z, p))
    from diff_lidargs_surfel_rasterization import _C
    from diff_lidargs_rasterization import _C as base
    assert _C._lib is base._lib                                             # the one CDLL of the process


def _backward_view_args(P=4, transMat=None, out=ALIGNED, partials=ALIGNED, n=None, width=64, height=8, lib=None):
    """lgsfpose_backward_view's 40 arguments with every pointer NULL but the ones named: nothing here can pass lidargs_surfel_backward's
    own checks (the forward buffers are NULL), so no call reaches a launch."""
    n = int(lib.lgsfpose_view_partial_floats(P)) if n is None else n
    return ([P, 0, 0, 0, None, width, height] + [None] * 4 + [1.0, None, transMat] + [None] * 21 +[0, None, out, partials, n])


def test_arguments_are_refused_before_any_device_work(hip_lib_built):
    from diff_lidargs_surfel_rasterization import _C
    lib = _C._lib
    assert lib.lgsfpose_view_partial_floats(0) == 0 and lib.lgsfpose_view_partial_floats(-3) == 0
    assert lib.lgsfpose_view_partial_floats(1) == 16 and lib.lgsfpose_view_partial_floats(256) == 16 and lib.lgsfpose_view_partial_floats(257) == 32
    with pytest.raises(ctypes.ArgumentError):
        lib.lgsfpose_view_partial_floats(1.5)
    view = lambda **kw: lib.lgsfpose_backward_view(*_backward_view_args(lib=lib, **kw))
    assert len(_backward_view_args(lib=lib)) == len(lib.lgsfpose_backward_view.argtypes) == 40
    err = lib.lidargs_last_error
    assert view(P=-1) == -1 and b"surfel backward_view: bad sizes" in err()
    assert view(height=1) == -1 and b"bad sizes" in err()
    assert view(out=None) == -1 and b"dL_dviewmatrix is NULL" in err()
    assert view(transMat=ALIGNED) == -1 and b"transMat_precomp" in err() and b"dL_dviewmatrix" in err()
    assert view(P=0, transMat=ALIGNED, partials=None, n=0) == -1 and b"transMat_precomp" in err()      # also on an empty frame
    assert view(partials=None) == -1 and b"view_partials" in err()
    assert view(partials=ctypes.c_void_p(0x1008)) == -1 and b"16-byte aligned" in err()
    assert view(P=257, n=31) == -1 and b"lgsfpose_view_partial_floats" in err()
    assert view(P=257, n=32) < 0 and b"missing forward buffers" in err()   # past the pose checks: lidargs_surfel_backward's own refusal
    hook = [-1, 64, 8, None, None, None, 1.0] + [None] * 4 + [None] * 9 + [None] * 3 + [ALIGNED, ALIGNED, 16, None]
    assert len(hook) == len(lib.lgsfpose_debug_view_backward.argtypes)
    assert lib.lgsfpose_debug_view_backward(*hook) == -1 and b"debug_surfel_view_backward: bad sizes" in err()
    hook[0] = 4
    assert lib.lgsfpose_debug_view_backward(*hook) == -1 and b"NULL required pointer" in err()
    hook[-2] = 15
    assert lib.lgsfpose_debug_view_backward(*hook) == -1 and b"view_partials" in err()
    hook[-4] = None
    assert lib.lgsfpose_debug_view_backward(*hook) == -1 and b"dL_dviewmatrix is NULL" in err()


def test_the_binding_refuses_a_precomputed_transform_with_the_request(hip_lib_built):
    """Raised by the binding itself, before any tensor is looked at: a RuntimeError that names both."""
    import torch
    from diff_lidargs_surfel_rasterization import _C
    with pytest.raises(RuntimeError, match="transMat_precomp.*viewmatrix"):
        _C.refuse_pose_with_transmat(torch.zeros(2, 9))
    _C.refuse_pose_with_transmat(torch.zeros(0))
    _C.refuse_pose_with_transmat(None)
