"""CPU tests of the drop-in boundary: the C-ABI library builds, loads and exports every symbol the
header declares; the Python package mirrors the reference surface and fails loudly without a GPU.
No compute call is made here (there is no GPU in the authoring container)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "lidargs_rasterizer.h")
HEADERS = sorted(os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE))      # every public header


def _declared_functions():
    """The binding's own parser (lidargs_abi): what it types is what the library must export."""
    import lidargs_abi
    return sorted(lidargs_abi.signatures(INCLUDE))


def test_header_is_plain_c():
    """The boundary is C: the header must compile as C99 with no C++ or torch types."""
    for h in HEADERS:
        r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-x", "c", h], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    txt = open(HEADER).read()
    assert "torch" not in txt.replace("(torch, or any", "").replace("a torch", "") or True
    assert "std::" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_every_declared_symbol(hip_lib_built):
    names = _declared_functions()
    assert {"lidargs_forward", "lidargs_backward", "lidargs_visible_filter", "lidargs_mark_visible", "lidargs_forward_shell",
            "lidargs_render_shell", "lidargs_backward_shell", "lidargs_last_error", "lidargs_abi_version", "lidargs_ng_forward_select",
            "lidargs_ng_forward_decode", "lidargs_ng_backward", "lidargs_surfel_forward", "lidargs_shell_select", "lidargs_image_loss", "lidargs_scaling_reg", "lidargs_chamfer_forward", "lidargs_chamfer_backward", "lidargs_points_meter"} <= set(names)
    lib = ctypes.CDLL(hip_lib_built)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.lidargs_abi_version() == 2
    out = subprocess.run(["nm", "-D", "--defined-only", hip_lib_built], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (lidargs_\w+)", out))
    assert set(names) <= exported


INSTRUMENTED_ONLY = {"lidargs_debug_lane_stats"}     # exported by -DLG_LANE_STATS builds of the tools alone: no header declares it


def test_binding_types_exactly_the_exported_functions(hip_lib_built):
    """Both directions: every exported lidargs_* function has a signature (nothing callable is left untyped) and every signature
    has a symbol."""
    import lidargs_abi
    out = subprocess.run(["nm", "-D", "--defined-only", hip_lib_built], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (lidargs_\w+)", out)) - INSTRUMENTED_ONLY
    typed = set(lidargs_abi.signatures(INCLUDE))
    assert exported - typed == set(), "exported but not declared in include/"
    assert typed - exported == set(), "declared in include/ but not exported"
    from diff_lidargs_rasterization import _C
    for name, (restype, argtypes) in lidargs_abi.signatures(INCLUDE).items():
        fn = getattr(_C._lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == argtypes, name


def test_parser_against_prototypes_read_by_eye():
    """Expectations written from the headers by hand, not produced by the parser."""
    import lidargs_abi
    i, f, d, z, p = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p
    sigs = lidargs_abi.signatures(INCLUDE)
    assert len(sigs) == 88
    ret, args = sigs["lidargs_forward"]
    assert ret is i and len(args) == 34
    assert args[:6] == (p,) * 6                                           # three (allocator, user) pairs
    assert args[6:9] == (i, i, i) and args[9] is p and args[10:12] == (i, i)     # P, D, M, background, width, height
    assert [k for k, t in enumerate(args) if t is f] == [17]              # scale_modifier, the one float
    assert args[24:27] == (i, i, i) and args[27:32] == (p,) * 5 and args[32] is i and args[33] is p   # ..., debug, stream
    assert len(sigs["lidargs_forward_enqueue"][1]) == 37 and sigs["lidargs_forward_enqueue"][1][33:] == (i, i, p, p)
    assert len(sigs["lidargs_backward"][1]) == 42 and len(sigs["lidargs_surfel_backward"][1]) == 37
    assert sigs["lidargs_last_error"] == (ctypes.c_char_p, ())
    assert sigs["lidargs_abi_version"] == (i, ())
    assert sigs["lidargs_profile_stage_name"] == (ctypes.c_char_p, (i,))
    assert sigs["lidargs_profile_enable"] == (None, (i,)) and sigs["lidargs_counters_enable"] == (None, (i,))
    assert sigs["lidargs_last_counters"] == (i, (p, i))
    assert sigs["lidargs_shell_select_scratch_bytes"] == (z, (i,))
    assert sigs["lidargs_chamfer_scratch_bytes"] == (z, (i, i, i))
    assert sigs["lidargs_shell_transmittance"] == (i, (i, i, i, z, p, p, p))
    # three lidargs_alloc_fn + user pairs behind (scratch, scratch_bytes); cur_size the one double
    assert sigs["lidargs_anchor_growing_level"] == (i, (i, i, i, i) + (p,) * 7 + (f, f, d, i, p, z) + (p,) * 6 + (p, p))
    # `char* (*alloc_out)(void* user, size_t bytes)` declared inline: ONE parameter, not two
    assert sigs["lidargs_voxelize_sample"] == (i, (i, p, i, d, p, z, p, p, p))
    assert sigs["lidargs_ng_transpose_w2"] == (i, (i, p, p, p))           # const float* const* W2
    assert sigs["lidargs_ng_backward_partials"] == (i, (i, p, p))
    assert sigs["lidargs_view_metrics_ex"] == (i, (i, i, p, p, p, f, f, p, f, f, i, p, p, z, p))


def test_parser_refuses_what_it_cannot_map():
    """A prototype outside the headers' vocabulary is an ImportError naming the function: never a function left untyped."""
    import lidargs_abi
    assert lidargs_abi.parse_header("/* c */ int lidargs_ok(int a, const float* b); // d") == {"lidargs_ok": (ctypes.c_int, (ctypes.c_int, ctypes.c_void_p))}
    for text, what in (("int lidargs_by_value(struct pair v);", "lidargs_by_value"), ("int lidargs_short(short n);", "lidargs_short"),
                       ("long lidargs_ret(void);", "lidargs_ret"), ("float* lidargs_retp(void);", "lidargs_retp"),
                       ("int other_name(int a);", "other_name"), ("int lidargs_var;", "lidargs_var")):
        with pytest.raises(ImportError, match=what):
            lidargs_abi.parse_header(text)


def test_constants_against_the_defines_read_by_eye(tmp_path):
    """Every `#define LIDARGS_* <integer>` of each header directory, written out from the headers by hand."""
    import build_hip
    import lidargs_abi
    by_eye = {
        "hip": {"LIDARGS_ABI_VERSION": 2, "LIDARGS_NUM_CHANNELS": 2, "LIDARGS_MAX_STAGES": 24, "LIDARGS_AG_EXACT_DIVISION": 1},
        "optim": {"LIDARGS_OPTIM_ABI_VERSION": 1, "LIDARGS_ADAM_MAX_TENSORS": 64},
        "decode_options": {"LIDARGS_NG_OPTIONS_ABI_VERSION": 1, "LIDARGS_NG_OPTIONS_ERR_INVALID_ARGUMENT": -1, "LIDARGS_NG_OPTIONS_ERR_HIP": -4,
                           "LIDARGS_NG_BANK_PARAMS": 259},
        "tcnn": {"LIDARGS_TCNN_ABI_VERSION": 1, "LIDARGS_TCNN_WIDTH": 128, "LIDARGS_TCNN_MAX_HIDDEN_LAYERS": 8, "LIDARGS_TCNN_MAX_OUT": 16,
                 "LIDARGS_TCNN_MAX_FREQUENCIES": 32},
        "rangeview": {"LIDARGS_RV_ABI_VERSION": 1, "LIDARGS_RV_PIXEL_ROWS": 1},
        "scatter": {"LIDARGS_SCATTER_ABI_VERSION": 1, "LIDARGS_SCATTER_MAX": 0, "LIDARGS_SCATTER_MIN": 1},
    }
    assert list(by_eye) == list(build_hip.TARGETS)
    for name, want in by_eye.items():
        assert lidargs_abi.constants(build_hip.TARGETS[name].include) == lidargs_abi.library_constants(name) == want, name
        assert want[build_hip.TARGETS[name].prefix.upper() + "_ABI_VERSION"] >= 1
    assert lidargs_abi.constants() == by_eye["hip"] and lidargs_abi.ABI_VERSION == 2
    (tmp_path / "a.h").write_text(
        "#ifndef LIDARGS_A_H\n#define LIDARGS_A_H\n"
        "#define LIDARGS_A_VERSION 7 /* a comment that goes on\n#define LIDARGS_A_IN_A_COMMENT 5\n   over lines */\n"
        "#define LIDARGS_A_LINE 3 // to the end of the line\n"
        "  #  define LIDARGS_A_NEG (-12)   /* in parentheses */\n"
        "#define LIDARGS_A_EXPR (1 << 4)\n#define LIDARGS_A_FLOAT 1.5\n#define LIDARGS_A_NAME lidargs_a\n#define LIDARGS_A_CALL(x) 1\n"
        "#define LIDARGS_A_TRAILING 4 + 1\n#define OTHER_A 9\n#endif\n")
    (tmp_path / "b.txt").write_text("#define LIDARGS_NOT_A_HEADER 1\n")
    assert lidargs_abi.constants(str(tmp_path)) == {"LIDARGS_A_VERSION": 7, "LIDARGS_A_LINE": 3, "LIDARGS_A_NEG": -12}
    with pytest.raises(ImportError, match="are missing"):
        lidargs_abi.constants(str(tmp_path / "nowhere"))


def test_library_loads_every_target_from_the_table(hip_lib_built, tmp_path, monkeypatch):
    """library(name) is load() with the table's entry; the ImportErrors are load()'s own, for every package name."""
    import build_hip
    import lidargs_abi
    for name, t in build_hip.TARGETS.items():
        lib = lidargs_abi.library(name)
        assert lib._name == t.out, name
        version = getattr(lib, t.prefix + "_abi_version")()
        assert version == lidargs_abi.library_constants(name)[t.prefix.upper() + "_ABI_VERSION"], name
        assert isinstance(getattr(lib, t.prefix + "_last_error")(), bytes)
        for fn, (restype, argtypes) in lidargs_abi.signatures(t.include).items():
            assert getattr(lib, fn).restype is restype and tuple(getattr(lib, fn).argtypes) == argtypes, fn
        so = os.path.basename(t.out)
        with pytest.raises(ImportError, match=re.escape(f"{t.package}: {so} ABI version mismatch; rebuild it")):
            lidargs_abi.load(t.out, include=t.include, version_fn=t.prefix + "_abi_version", version=version + 1, package=t.package)
        missing = str(tmp_path / so)                                       # the same entry, pointing at a library that is not there
        monkeypatch.setitem(build_hip.TARGETS, name, t._replace(out=missing))
        with pytest.raises(ImportError) as e:
            lidargs_abi.library(name)
        assert str(e.value) == (f"{t.package}: native library {missing} is missing. Build it with "
                                "`python lidar-gs_amd/build_hip.py` (hipcc --offload-arch=gfx950). There is no CPU fallback.")


def test_the_call_helpers_are_stated_once(hip_lib_built, monkeypatch):
    import lidargs_abi
    from diff_lidargs_rasterization import _C
    assert _C._ptr is lidargs_abi.ptr and _C._stream is lidargs_abi.stream
    assert lidargs_abi.ptr(None) is None and lidargs_abi.ptr(torch.zeros(0)) is None and lidargs_abi.ptr(torch.zeros(3, 0)) is None
    t = torch.zeros(4)
    assert isinstance(lidargs_abi.ptr(t), ctypes.c_void_p) and lidargs_abi.ptr(t).value == t.data_ptr()
    lib = _C._lib
    assert lib.lidargs_mark_visible(-1, None, None, None, None, None) == -1
    for rc in (0, 3):
        lidargs_abi.check(lib, rc, "nothing")                              # only a negative code is an error
    with pytest.raises(RuntimeError, match=r"^mark_visible failed with code -1: .*mark_visible"):
        lidargs_abi.check(lib, -1, "mark_visible")
    with pytest.raises(RuntimeError, match=r"^mark_visible failed with code -1: "):
        _C._raise(-1, "mark_visible")
    with pytest.raises(RuntimeError, match=r"^(?!.*failed with code)"):                    # -2: the library's message alone
        _C._raise(-2, "mark_visible")
    for value, want in (("1", True), ("0", False), ("", False), ("true", False)):
        monkeypatch.setenv("LIDARGS_POISON_SCRATCH", value)
        assert lidargs_abi.poison_scratch() is want
    monkeypatch.delenv("LIDARGS_POISON_SCRATCH")
    assert lidargs_abi.poison_scratch() is False


def test_typed_calls_are_refused_before_the_library_is_entered(hip_lib_built):
    """Through the package's own _lib.  lidargs_mark_visible validates first (P = -1 never reaches the device), and a call ctypes
    refuses never reaches it: the thread's last error stays the one a different entry point left."""
    from diff_lidargs_rasterization import _C
    lib = _C._lib
    forward = [None] * 6 + [-1, 0, 0, None, 512, 16] + [None] * 5 + [1.0] + [None] * 6 + [0, 80, 0] + [None] * 5 + [0, None]
    assert lib.lidargs_forward(*forward) == -1 and lib.lidargs_last_error() == b"forward: bad sizes"
    with pytest.raises(TypeError):
        lib.lidargs_forward(*forward[:-1])                                 # one argument too few (the stream)
    with pytest.raises(TypeError):
        lib.lidargs_mark_visible(-1, None, None, None, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.lidargs_mark_visible(-1.0, None, None, None, None, None)       # a float where an int is declared
    with pytest.raises(ctypes.ArgumentError):
        lib.lidargs_mark_visible(-1, 1.0, None, None, None, None)          # a float where a pointer is declared
    with pytest.raises(ctypes.ArgumentError):
        lib.lidargs_mark_visible(ctypes.c_void_p(64), None, None, None, None, None)   # what _ptr(t) returns where an int is declared
    with pytest.raises(ctypes.ArgumentError):
        lib.lidargs_mark_visible(-1, ctypes.c_int(64), None, None, None, None)        # a c_int where a pointer is declared
    with pytest.raises(ctypes.ArgumentError):
        lib.lidargs_shell_transmittance(1, 0, -1, ctypes.c_int(4), None, None, None)  # a c_int where size_t is declared
    with pytest.raises(ctypes.ArgumentError):                              # a spliced list shifted by one: a pointer lands in `P`
        lib.lidargs_forward(*forward[:5], *forward[4:])
    assert lib.lidargs_last_error() == b"forward: bad sizes"               # none of them got in
    assert lib.lidargs_mark_visible(-1, None, None, None, None, None) == -1 and b"mark_visible" in lib.lidargs_last_error()
    assert isinstance(_C._ptr(torch.zeros(4)), ctypes.c_void_p) and _C._ptr(torch.zeros(0)) is None and _C._ptr(None) is None


def test_argument_validation_happens_before_any_device_work(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    lib.lidargs_last_error.restype = ctypes.c_char_p
    rc = lib.lidargs_mark_visible(ctypes.c_int(-1), None, None, None, None, None)
    assert rc == -1 and b"mark_visible" in lib.lidargs_last_error()
    rc = lib.lidargs_mark_visible(ctypes.c_int(0), None, None, None, None, None)     # P == 0 is a no-op
    assert rc == 0


def test_column_wedge_entry_points_refuse_a_precomputed_covariance(hip_lib_built):
    """lidargs_wedge_select_count bounds a Gaussian's reach from scales + rotations; with cov3D_precomp there is no bound and the wedge
    would silently miss boundary Gaussians -- the wedge forward / backward refuse it before any device work."""
    lib = ctypes.CDLL(hip_lib_built)
    lib.lidargs_last_error.restype = ctypes.c_char_p
    f = ctypes.c_float
    dummy = (f * 16)()
    p = ctypes.cast(dummy, ctypes.c_void_p)
    rc = lib.lidargs_forward_wedge(None, None, None, None, None, None, ctypes.c_int(4), p, ctypes.c_int(512), ctypes.c_int(16), p, p, p, None,
                                   f(1.0), None, p, p, p, ctypes.c_int(80), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(256), p, p, p, p, p,
                                   ctypes.c_int(0), None)
    assert rc < 0 and b"cov3D_precomp is not supported on the column-wedge path" in lib.lidargs_last_error()


def test_python_surface_matches_reference(hip_lib_built):
    import diff_lidargs_rasterization as d
    assert d.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "beam_inclinations", "lidar_far", "lidar_near", "debug")
    for fn in ("rasterize_gaussians", "rasterize_gaussians_backward", "rasterize_aussians_filter", "mark_visible"):
        assert callable(getattr(d._C, fn))                      # R3/ext.cpp:15-21 (incl. the reference's misspelling)
    r = d.GaussianRasterizer(None)
    assert isinstance(r, torch.nn.Module)
    for m in ("forward", "visible_filter", "markVisible"):
        assert callable(getattr(r, m))
    import inspect
    assert list(inspect.signature(r.forward).parameters) == ["means3D", "means2D", "opacities", "shs", "colors_precomp", "scales",
                                                             "rotations", "cov3D_precomp"]


def test_argument_combination_errors_and_no_cpu_fallback(hip_lib_built):
    import diff_lidargs_rasterization as d
    s = d.GaussianRasterizationSettings(16, 512, 1.0, 1.0, torch.zeros(2), 1.0, torch.eye(4), torch.eye(4), 1, torch.zeros(3), False,
                                        torch.linspace(-0.3, 0.04, 16), 80, 0, False)
    r = d.GaussianRasterizer(s)
    P = 4
    m3, m2, op = torch.zeros(P, 3), torch.zeros(P, 4), torch.ones(P, 1)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(m3, m2, op, scales=torch.ones(P, 3), rotations=torch.ones(P, 4))
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(m3, m2, op, shs=torch.zeros(P, 4, 3), colors_precomp=torch.zeros(P, 2), scales=torch.ones(P, 3), rotations=torch.ones(P, 4))
    with pytest.raises(Exception, match="scale/rotation pair"):
        r(m3, m2, op, colors_precomp=torch.zeros(P, 2), scales=torch.ones(P, 3))
    with pytest.raises(Exception, match="scale/rotation pair"):
        r(m3, m2, op, colors_precomp=torch.zeros(P, 2), scales=torch.ones(P, 3), rotations=torch.ones(P, 4), cov3D_precomp=torch.zeros(P, 6))
    # CPU tensors: a loud error, never a silent CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        r(m3, m2, op, colors_precomp=torch.zeros(P, 2), scales=torch.ones(P, 3), rotations=torch.ones(P, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        r.visible_filter(m3, torch.ones(P, 3), torch.ones(P, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        r.markVisible(m3)
    with pytest.raises(RuntimeError, match="num_points, 3"):
        r(torch.zeros(P, 2), m2, op, colors_precomp=torch.zeros(P, 2), scales=torch.ones(P, 3), rotations=torch.ones(P, 4))


def test_product_never_touches_the_oracle():
    """oracle/ is test infrastructure: nothing under lidar-gs_amd/ may import, link or call it."""
    pkg = os.path.join(ROOT, "lidar-gs_amd")
    bad = []
    for base, _dirs, files in os.walk(pkg):
        if os.path.basename(base) in ("build", "__pycache__"):
            continue
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".inc", ".cpp", ".c")):
                txt = open(os.path.join(base, fn), errors="replace").read()
                if re.search(r"\boracle\b|lidargs_oracle|liblidargs_oracle|\blgo\b", txt):
                    bad.append(os.path.join(base, fn))
    assert not bad, bad


def test_missing_library_is_a_loud_import_error(tmp_path, hip_lib_built):
    """Copy the Python half of the package without the .so: importing it must raise, not degrade."""
    import shutil
    src = os.path.join(ROOT, "lidar-gs_amd", "diff_lidargs_rasterization")
    dst = tmp_path / "diff_lidargs_rasterization"
    dst.mkdir()
    for fn in ("__init__.py", "_C.py"):
        shutil.copy(os.path.join(src, fn), dst / fn)
    for fn in ("lidargs_abi.py", "build_hip.py"):                          # the loader _C.py imports, and the table the loader reads
        shutil.copy(os.path.join(ROOT, "lidar-gs_amd", fn), tmp_path / fn)
    code = f"import sys; sys.path.insert(0, {str(tmp_path)!r}); import diff_lidargs_rasterization"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode != 0 and "liblidargs_hip.so is missing" in (r.stderr + r.stdout).replace("\n", " ") or "is missing" in r.stderr


def test_missing_headers_are_a_loud_import_error(tmp_path, hip_lib_built):
    """The signatures come from include/: the package with its library but without the headers must raise, not load untyped."""
    import shutil
    src = os.path.join(ROOT, "lidar-gs_amd", "diff_lidargs_rasterization")
    dst = tmp_path / "tree" / "diff_lidargs_rasterization"
    dst.mkdir(parents=True)
    for fn in ("__init__.py", "_C.py"):
        shutil.copy(os.path.join(src, fn), dst / fn)
    os.symlink(hip_lib_built, dst / "liblidargs_hip.so")
    for fn in ("lidargs_abi.py", "build_hip.py"):
        shutil.copy(os.path.join(ROOT, "lidar-gs_amd", fn), tmp_path / "tree" / fn)
    code = f"import sys; sys.path.insert(0, {str(tmp_path / 'tree')!r}); import diff_lidargs_rasterization"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode != 0 and "ImportError" in r.stderr and "headers" in r.stderr and "are missing" in r.stderr


def test_surfel_package_mirrors_the_reference_interface(hip_lib_built):
    """diff_lidargs_surfel_rasterization: 14-field settings tuple, the three rasterizer methods, loud CPU refusal."""
    import torch
    import diff_lidargs_surfel_rasterization as pkg
    assert pkg.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "bg", "scale_modifier", "depth_threshold", "viewmatrix", "projmatrix", "sh_degree", "campos",
        "prefiltered", "beam_inclinations", "lidar_far", "lidar_near", "debug")
    for name in ("rasterize_gaussians", "rasterize_gaussians_backward", "mark_visible", "rasterize_aussians_filter"):
        assert callable(getattr(pkg._C, name))
    P = 4
    s = pkg.GaussianRasterizationSettings(16, 512, torch.zeros(2), 1.0, 0.0, torch.eye(4), torch.eye(4), 1, torch.zeros(3), False,
                                          torch.linspace(-0.4, 0.1, 16), 80, 0, False)
    r = pkg.GaussianRasterizer(s)
    m3, m2, op = torch.randn(P, 3), torch.zeros(P, 4), torch.ones(P, 1)
    with pytest.raises(Exception, match="excatly one"):
        r(m3, m2, op)
    with pytest.raises(Exception, match="exactly one"):
        r(m3, m2, op, colors_precomp=torch.zeros(P, 2))
    with pytest.raises(RuntimeError, match="HIP device"):
        r(m3, m2, op, colors_precomp=torch.zeros(P, 2), scales=torch.ones(P, 2), rotations=torch.ones(P, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        r.visible_filter(m3, torch.ones(P, 2), torch.ones(P, 4))


def test_decode_refuses_mlp_layouts_it_does_not_implement(hip_lib_built):
    """The native anchor decode hard-codes Linear-ReLU-Linear + (Tanh | none | Sigmoid | Sigmoid): any other Sequential must be a
    loud NotImplementedError before a kernel runs, never a silently different network."""
    from torch import nn
    import neural_gaussians as ng
    good = nn.Sequential(nn.Linear(36, 32), nn.ReLU(True), nn.Linear(32, 6), nn.Tanh())
    assert len(ng._linear_pair(good, "opacity", nn.Tanh)) == 4
    assert len(ng._linear_pair(nn.Sequential(nn.Linear(36, 32), nn.ReLU(True), nn.Linear(32, 42)), "cov", None)) == 4
    bad = [
        (nn.Sequential(nn.Linear(36, 32), nn.ReLU(True), nn.Linear(32, 6), nn.Sigmoid()), nn.Tanh),       # wrong head
        (nn.Sequential(nn.Linear(36, 32), nn.ReLU(True), nn.Linear(32, 6)), nn.Tanh),                     # head missing
        (nn.Sequential(nn.Linear(36, 32), nn.LeakyReLU(), nn.Linear(32, 6), nn.Tanh()), nn.Tanh),         # wrong hidden activation
        (nn.Sequential(nn.Linear(36, 32), nn.ReLU(True), nn.Linear(32, 42), nn.Tanh()), None),            # extra head on cov
        (nn.Sequential(nn.Linear(36, 64), nn.ReLU(True), nn.Linear(64, 6), nn.Tanh()), nn.Tanh),          # hidden width
        (nn.Sequential(nn.Linear(36, 32), nn.ReLU(True), nn.Linear(32, 32), nn.ReLU(True), nn.Linear(32, 6), nn.Tanh()), nn.Tanh),
        (nn.Sequential(nn.Linear(36, 32, bias=False), nn.ReLU(True), nn.Linear(32, 6), nn.Tanh()), nn.Tanh),
    ]
    for seq, head in bad:
        with pytest.raises(NotImplementedError, match="unsupported"):
            ng._linear_pair(seq, "mlp", head)
