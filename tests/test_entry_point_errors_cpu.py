"""CPU tests of what the frame entry points refuse before any device work: the return code and the exact bytes of
lidargs_last_error() for every argument check that comes before the first HIP call and the first allocator call.

The calls go through a plain ctypes.CDLL of the built library.  Arguments are given BY NAME: the parameter lists are read from the
public headers, every pointer defaults to a small host array (never dereferenced by a call that is refused), every size to a valid
one, and a case overrides only what it is about.  No environment variable is used (the switches are parsed once per process), and
no P = 0 call is made to the pose entry point (it enqueues a memset)."""
import ctypes
import os
import re

import pytest

import build_hip

HIP = build_hip.TARGETS["hip"]             # the frame entry points: the primary header and the `pose` family's
HEADERS = [os.path.join(HIP.include, "lidargs_rasterizer.h"),
           os.path.join(next(f.include for f in HIP.families if f.name == "pose"), "lidargs_pose.h")]

INVALID, NO_COLORS, STATE = -1, -2, -5        # LIDARGS_ERR_INVALID_ARGUMENT, _NO_COLORS, _STATE (include/lidargs_rasterizer.h)

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}


def _prototypes():
    """{function: [(parameter name, ctypes scalar type, or None for a pointer)]} of the frame entry points of both headers."""
    protos = {}
    for path in HEADERS:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(path).read(), flags=re.S)
        for m in re.finditer(r"\b(?:int|size_t)\s+(lidargs_(?:surfel_)?(?:forward|backward)\w*|lidargs_render_shell|lidargs_visible_filter|lgpose_\w+)"
                             r"\s*\(([^;{]*)\)\s*;", text):
            params = []
            for decl in m.group(2).split(","):
                words = decl.replace("*", " * ").split()
                if words == ["void"]:
                    continue
                pointer = "*" in words or words[0] == "lidargs_alloc_fn"
                params.append((words[-1], None if pointer else _SCALARS[" ".join(words[:-1])]))
            protos[m.group(1)] = params
    return protos


PROTOS = _prototypes()
_HOST = (ctypes.c_float * 64)()                # what every non-NULL pointer points at
_BASE = ctypes.addressof(_HOST)
PTR = ctypes.c_void_p(_BASE)
ALIGNED = (_BASE + 15) & ~15                   # a 16-byte aligned address inside _HOST
DEFAULTS = {"P": 4, "D": 0, "M": 0, "R": 0, "width": 512, "height": 16, "scale_modifier": 1.0, "cov3D_precomp": None, "transMat_precomp": None,
            "lidar_far": 80, "lidar_near": 0, "prefiltered": 0, "debug": 0, "stream": None, "tan_fovx": 1.0, "tan_fovy": 1.0,
            "shell_lo": 0.0, "shell_hi": 100.0, "transmittance_pass": 0, "T_in": None, "col_lo": 0, "col_hi": 256,
            "instance_capacity": 1024, "tile_rows": 4, "status_host": None, "n_valid": None}


@pytest.fixture(scope="module")
def lib(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    lib.lidargs_last_error.restype = ctypes.c_char_p
    lib.lgpose_view_partial_floats.restype = ctypes.c_size_t
    return lib


def refused(lib, name, code, message, **given):
    """Call `name` with the defaults and `given`; it must return `code` and leave exactly `message` as the thread's last error."""
    unknown = set(given) - {n for n, _ in PROTOS[name]}
    assert not unknown, (name, unknown)         # a case must name parameters the entry point has
    args = []
    for pname, ctype in PROTOS[name]:
        v = given[pname] if pname in given else DEFAULTS.get(pname, PTR if ctype is None else 0)
        args.append(ctype(v) if ctype is not None else (v if v is None or isinstance(v, ctypes.c_void_p) else ctypes.c_void_p(v)))
    rc = getattr(lib, name)(*args)
    print(name, given, "->", rc, lib.lidargs_last_error())
    assert rc == code, (name, given, rc, lib.lidargs_last_error())
    assert lib.lidargs_last_error() == message, (name, given, lib.lidargs_last_error())


def pose_partials(lib, P=DEFAULTS["P"]):
    """(view_partials, view_partial_floats) that lgpose_backward_view accepts for P Gaussians; the buffer is never dereferenced."""
    return {"view_partials": ALIGNED, "view_partial_floats": lib.lgpose_view_partial_floats(ctypes.c_int(P))}


# the 3-D forwards that go through the shared host sequence, with the prefix of the messages only they have
FORWARDS_3D = ["lidargs_forward", "lidargs_forward_enqueue", "lidargs_forward_shell", "lidargs_forward_shell_enqueue", "lidargs_forward_wedge",
               "lidargs_forward_wedge_enqueue"]
ENQUEUE = {"lidargs_forward_enqueue": b"forward_enqueue", "lidargs_forward_shell_enqueue": b"forward_shell_enqueue",
           "lidargs_forward_wedge_enqueue": b"forward_wedge_enqueue"}
WEDGE_COV = b": cov3D_precomp is not supported on the column-wedge path (give scales + rotations)"


def test_the_headers_declare_the_entry_points_this_file_calls():
    for name in FORWARDS_3D + ["lidargs_surfel_forward", "lidargs_visible_filter", "lidargs_backward", "lidargs_backward_shell", "lidargs_backward_wedge",
                               "lgpose_backward_view", "lidargs_surfel_backward", "lidargs_render_shell"]:
        assert name in PROTOS, name
    assert [n for n, _ in PROTOS["lidargs_forward"]][:7] == ["geometry_alloc", "geometry_user", "binning_alloc", "binning_user", "image_alloc",
                                                              "image_user", "P"]
    assert len(PROTOS["lidargs_forward"]) == 34 and len(PROTOS["lidargs_backward"]) == 42 and len(PROTOS["lgpose_backward_view"]) == 45


@pytest.mark.parametrize("name", FORWARDS_3D)
def test_forward_argument_errors(lib, name):
    refused(lib, name, INVALID, b"forward: bad sizes", P=-1)
    refused(lib, name, INVALID, b"forward: need at least 2 beams", height=1)
    refused(lib, name, NO_COLORS, b"For non-RGB, provide precomputed Gaussian colors!", colors_precomp=None)
    for pointer in ("means3D", "opacities", "viewmatrix", "beam_inclinations", "out_color", "out_depth", "out_occ", "radii"):
        refused(lib, name, INVALID, b"forward: NULL required pointer", **{pointer: None})
    refused(lib, name, INVALID, b"forward: need scales+rotations or cov3D_precomp", scales=None)
    for allocator in ("geometry_alloc", "binning_alloc", "image_alloc"):
        refused(lib, name, INVALID, b"forward: NULL allocator", **{allocator: None})


def test_surfel_forward_argument_errors(lib):
    name = "lidargs_surfel_forward"
    refused(lib, name, INVALID, b"surfel forward: bad sizes", P=-1)
    refused(lib, name, INVALID, b"surfel forward: bad sizes", height=1)
    refused(lib, name, NO_COLORS, b"For non-RGB, provide precomputed Gaussian colors!", colors_precomp=None)
    for pointer in ("means3D", "opacities", "scales", "rotations", "viewmatrix", "beam_inclinations", "background", "out_color", "out_others", "radii",
                    "radii_xy"):
        refused(lib, name, INVALID, b"surfel forward: NULL required pointer", **{pointer: None})
    refused(lib, name, INVALID, b"surfel forward: transMat_precomp without scales and rotations (the reference's preprocess reads them even then, "
            b"R2/cr/forward.cu:271-273)", transMat_precomp=PTR, scales=None)
    for allocator in ("geometry_alloc", "binning_alloc", "image_alloc"):
        refused(lib, name, INVALID, b"surfel forward: NULL allocator", **{allocator: None})


def test_visible_filter_argument_errors(lib):
    """It has no colours and uses no allocator (NULL allocators are valid there and the call goes on to the device), so those two cases
    do not exist for it."""
    name = "lidargs_visible_filter"
    refused(lib, name, INVALID, b"visible_filter: bad sizes", P=-1)
    refused(lib, name, INVALID, b"visible_filter: bad sizes", height=1)
    for pointer in ("means3D", "viewmatrix", "beam_inclinations", "radii"):
        refused(lib, name, INVALID, b"visible_filter: NULL required pointer", **{pointer: None})
    refused(lib, name, INVALID, b"visible_filter: need scales+rotations or cov3D_precomp", rotations=None)


@pytest.mark.parametrize("name", sorted(ENQUEUE))
def test_enqueue_forms_check_capacity_and_tile_rows(lib, name):
    refused(lib, name, INVALID, ENQUEUE[name] + b": instance_capacity must be positive", instance_capacity=0)
    refused(lib, name, INVALID, b"forward (enqueue-only): tile_rows must be 4, 8, 16 or 32", instance_capacity=1024, tile_rows=5)
    refused(lib, name, INVALID, b"forward (enqueue-only): tile_rows must be 4, 8, 16 or 32", instance_capacity=1024, tile_rows=5, P=-1)   # (it is the first check)


@pytest.mark.parametrize("name,prefix", [("lidargs_forward_wedge", b"forward_wedge"), ("lidargs_forward_wedge_enqueue", b"forward_wedge"),
                                         ("lidargs_backward_wedge", b"backward_wedge")])
def test_wedge_entry_points_check_the_wedge_first(lib, name, prefix):
    refused(lib, name, INVALID, prefix + b": col_lo < 0", col_lo=-1)
    refused(lib, name, INVALID, prefix + b": col_lo < 0", col_lo=-1, P=-1)
    refused(lib, name, INVALID, prefix + WEDGE_COV, cov3D_precomp=PTR)
    refused(lib, name, INVALID, prefix + b": col_lo < 0", col_lo=-1, cov3D_precomp=PTR)


def test_wedge_enqueue_checks_the_wedge_before_the_capacity(lib):
    refused(lib, "lidargs_forward_wedge_enqueue", INVALID, b"forward_wedge: col_lo < 0", col_lo=-1, instance_capacity=0)
    refused(lib, "lidargs_forward_wedge_enqueue", INVALID, b"forward_wedge" + WEDGE_COV, cov3D_precomp=PTR, instance_capacity=0)


BACKWARDS_3D = ["lidargs_backward", "lidargs_backward_shell", "lidargs_backward_wedge", "lgpose_backward_view"]


@pytest.mark.parametrize("name", BACKWARDS_3D)
def test_backward_argument_errors(lib, name):
    pose = name == "lgpose_backward_view"
    more = pose_partials(lib) if pose else {}
    refused(lib, name, INVALID, b"backward_view: bad sizes" if pose else b"backward: bad sizes", P=-1, **more)
    refused(lib, name, INVALID, b"backward_view: bad sizes" if pose else b"backward: bad sizes", R=-1, **more)
    for buffer in ("geom_buffer", "binning_buffer", "image_buffer"):
        refused(lib, name, STATE, b"backward: missing forward buffers", **{buffer: None}, **more)
    refused(lib, name, STATE, b"backward: missing forward buffers", geom_buffer=None, binning_buffer=None, image_buffer=None, dL_dpix=None, **more)
    required = ["means3D", "viewmatrix", "radii", "dL_dpix", "dL_dout_depth", "dL_dout_occ", "dL_dmean2D", "dL_dopacity", "dL_dcolor", "dL_dmean3D",
                "dL_dscale", "dL_drot"]
    for pointer in required:
        refused(lib, name, INVALID, b"backward: NULL required pointer", **{pointer: None}, **more)
    if name == "lidargs_backward_wedge":       # (refused as a wedge before the rows are looked at)
        refused(lib, name, INVALID, b"backward_wedge" + WEDGE_COV, cov3D_precomp=PTR, dL_dcov3D=None)
    else:
        refused(lib, name, INVALID, b"backward: NULL required pointer", cov3D_precomp=PTR, dL_dcov3D=None, **more)


def test_surfel_backward_argument_errors(lib):
    """(it has neither cov3D_precomp nor dL_dcov3D: that case does not exist for it)"""
    name = "lidargs_surfel_backward"
    refused(lib, name, INVALID, b"surfel backward: bad sizes", P=-1)
    refused(lib, name, INVALID, b"surfel backward: bad sizes", height=1)
    for buffer in ("geom_buffer", "binning_buffer", "image_buffer"):
        refused(lib, name, STATE, b"surfel backward: missing forward buffers", **{buffer: None})
    refused(lib, name, STATE, b"surfel backward: missing forward buffers", geom_buffer=None, binning_buffer=None, image_buffer=None, dL_dpix=None)
    for pointer in ("means3D", "scales", "rotations", "viewmatrix", "beam_inclinations", "background", "radii", "dL_dpix", "dL_depths", "dL_dmean2D",
                    "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dscale", "dL_drot", "depth"):
        refused(lib, name, INVALID, b"surfel backward: NULL required pointer", **{pointer: None})


def test_pose_backward_checks_its_own_arguments_first(lib):
    name = "lgpose_backward_view"
    ok = pose_partials(lib)
    short = b"backward_view: view_partials is NULL, not 16-byte aligned or shorter than lgpose_view_partial_floats(P)"
    refused(lib, name, INVALID, b"backward_view: dL_dviewmatrix is NULL", dL_dviewmatrix=None, **ok)
    refused(lib, name, INVALID, b"backward_view: bad sizes", dL_dviewmatrix=None, width=0, **ok)
    refused(lib, name, INVALID, short, view_partials=None, view_partial_floats=ok["view_partial_floats"])
    refused(lib, name, INVALID, short, view_partials=ALIGNED + 4, view_partial_floats=ok["view_partial_floats"])
    refused(lib, name, INVALID, short, view_partials=ALIGNED, view_partial_floats=ok["view_partial_floats"] - 1)
    refused(lib, name, INVALID, short, view_partials=None, view_partial_floats=ok["view_partial_floats"], geom_buffer=None)   # before the buffers
    assert ok["view_partial_floats"] > 0


def test_render_shell_refuses_an_empty_frame(lib):
    refused(lib, "lidargs_render_shell", STATE, b"render_shell: missing forward buffers", P=0)
    refused(lib, "lidargs_render_shell", STATE, b"render_shell: missing forward buffers", R=-1)
    for buffer in ("geom_buffer", "binning_buffer", "image_buffer"):
        refused(lib, "lidargs_render_shell", STATE, b"render_shell: missing forward buffers", **{buffer: None})
