"""CPU tests of the decode's two model options (use_feat_bank, appearance_dim > 0): the float64 restatement tests/decode_options_ref.py
equals the fixture made by executing the reference (tests/golden/make_decode_options_golden.py); the new entry points are declared,
exported and typed; the front-end's refusals that happen before any device call."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch
from torch import nn

import decode_options_ref as ref
import lidargs_scenes as sc
from test_neural_gaussians_cpu import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("c", "d", "e", "f")
NEW = {"lidargs_ng_bank_forward", "lidargs_ng_bank_backward", "lidargs_ng_bank_backward_partial_floats", "lidargs_ng_appearance_fold",
       "lidargs_ng_appearance_backward", "lidargs_ng_options_abi_version", "lidargs_ng_options_last_error"}


def test_fixture_holds_the_four_cases_and_stays_small():
    gold = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(gold, "decode_options_golden.npz")) < os.path.getsize(os.path.join(gold, "neural_gaussians_golden.npz"))
    z = np.load(os.path.join(gold, "decode_options_golden.npz"))
    got = {t: (int(z[t + "_N"]), int(z[t + "_k"]), bool(z[t + "_bank"]), int(z[t + "_A"]), tuple(bool(f) for f in z[t + "_flags"]), int(z[t + "_uid"]))
           for t in CASES}
    assert got == {"c": (400, 6, False, 32, (True, True, True), 3), "d": (300, 5, True, 0, (False, True, False), 0),
                   "e": (200, 10, True, 8, (True, False, True), 0), "f": (97, 4, True, 32, (True, True, False), 4)}
    assert z["c_emb_color"].shape == (5, 32) and z["f_emb_raydrop"].shape == (5, 32)
    for t in CASES:
        assert float(np.abs(z[t + "_out_neural_opacity"]).min()) >= 5e-5       # no offset within float32 rounding of the mask's edge


@pytest.mark.parametrize("tag", CASES)
def test_restatement_matches_reference_execution(tag):
    p, cam, vis, uid, exp = ref.load_case(tag)
    r = ref.run(p, cam, vis, uid, [exp["up_" + k] for k in ("xyz", "color", "opacity", "scaling", "rot")])
    assert np.array_equal(r["mask"], exp["out_mask"])
    for k in ref.OUT_KEYS:
        close(k, r[k], exp["out_" + k])
    for k in ref.TENSOR_KEYS:
        close("d" + k, r["g_" + k], exp["g_" + k])
    # parameter gradients are sums over all anchors, taken by a float32 GEMM in the fixture and in float64 here (see test_neural_gaussians_cpu.py)
    for k in ref.param_keys(p):
        close("d" + k, r["g_" + k], exp["g_" + k], rtol=5e-4)
    assert set(exp) == {"out_mask"} | {"out_" + k for k in ref.OUT_KEYS} | {"up_" + k for k in ("xyz", "color", "opacity", "scaling", "rot")} \
        | {"g_" + k for k in ref.TENSOR_KEYS + tuple(ref.param_keys(p))}      # the fixture stores every gradient, the new parameters' included
    if "emb_color" in p:
        for k in ("g_emb_color", "g_emb_raydrop"):
            others = np.delete(exp[k], uid, axis=0)
            assert (others == 0).all() and np.abs(exp[k][uid]).max() > 0 and (np.delete(r[k], uid, axis=0) == 0).all()
        assert exp["g_color_W1"].shape == p["color_W1"].shape == (32, 35 + int(p["add_color_dist"]) + p["emb_color"].shape[1])
    assert (r["g_anchor_feat"][~vis] == 0).all() and (r["g_anchor"][~vis] == 0).all()


def test_new_entry_points_are_declared_exported_and_typed(hip_lib_built):
    """The options' library (liblidargs_decode_options.so, include_decode/) beside the decode's: exactly the declared functions are
    exported, every one typed by lidargs_abi from the header, none of them in liblidargs_hip.so, and the header is plain C."""
    import build_hip
    import native_lib_checks
    import neural_gaussians as prod
    typed = native_lib_checks.check_library(build_hip.TARGETS["decode_options"], NEW, prod._options_lib(), hip_lib_built)
    assert "decode_options.hip" in build_hip.TARGETS["decode_options"].sources
    i, z, p = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p                  # written from the header by eye
    assert typed["lidargs_ng_bank_forward"] == (i, (i,) + (p,) * 10)
    assert typed["lidargs_ng_bank_backward"] == (i, (i,) + (p,) * 13 + (z, p))
    assert typed["lidargs_ng_bank_backward_partial_floats"] == (z, (i,))
    assert typed["lidargs_ng_appearance_fold"] == (i, (i, i) + (p,) * 9)
    assert typed["lidargs_ng_appearance_backward"] == (i, (i, i) + (p,) * 12)
    assert prod._options_lib().lidargs_ng_options_abi_version() == prod.OPTIONS_ABI_VERSION == 1


def test_entry_points_validate_before_any_device_work(hip_lib_built):
    import neural_gaussians as prod
    lib = prod._options_lib()
    err = lambda: lib.lidargs_ng_options_last_error().decode()
    cam = (ctypes.c_float * 3)(0, 0, 0)
    host = ctypes.cast((ctypes.c_float * 512)(), ctypes.c_void_p)             # never dereferenced: every call below is refused or a no-op
    assert lib.lidargs_ng_bank_forward(-1, None, host, host, cam, host, host, host, host, host, None) == -1 and "bad sizes" in err()
    assert lib.lidargs_ng_bank_forward(4, None, host, host, None, host, host, host, host, host, None) == -1 and "NULL" in err()
    assert lib.lidargs_ng_bank_forward(4, None, host, host, cam, host, host, host, host, None, None) == -1 and "NULL" in err()
    assert lib.lidargs_ng_bank_forward(0, None, None, None, cam, host, host, host, host, None, None) == 0          # N == 0: no launch
    assert lib.lidargs_ng_bank_backward(0, None, None, None, cam, host, host, host, host, None, None, None, None, None, 0, None) == 0
    need = lib.lidargs_ng_bank_backward_partial_floats(100)
    assert need == 4 * 259 and lib.lidargs_ng_bank_backward_partial_floats(1) == 259 and lib.lidargs_ng_bank_backward_partial_floats(10 ** 8) == 1024 * 259
    assert lib.lidargs_ng_bank_backward(100, None, host, host, cam, host, host, host, host, host, host, host, host, host, need - 1, None) == -1
    assert "partials too small" in err()
    assert lib.lidargs_ng_bank_backward(100, None, host, host, cam, host, host, host, host, host, host, None, host, host, need, None) == -1 and "NULL" in err()
    assert lib.lidargs_ng_appearance_fold(34, 32, host, host, host, host, host, host, host, host, None) == -1 and "bad sizes" in err()
    assert lib.lidargs_ng_appearance_fold(36, 0, host, host, host, host, host, host, host, host, None) == -1 and "bad sizes" in err()
    assert lib.lidargs_ng_appearance_fold(36, 8, host, host, None, host, host, host, host, host, None) == -1 and "NULL" in err()
    assert lib.lidargs_ng_appearance_backward(37, 8, *([host] * 11), None) == -1 and "bad sizes" in err()
    assert lib.lidargs_ng_appearance_backward(35, 8, *([host] * 10), None, None) == -1 and "NULL" in err()
    with pytest.raises(ctypes.ArgumentError):
        lib.lidargs_ng_bank_forward(4.0, None, host, host, cam, host, host, host, host, host, None)


def _cpu_model(bank=True, A=8, seed=5):
    p, cam, vis, _ = sc.make_anchor_model(64, 6, seed)
    q = ref.random_options(p, seed, bank=bank, A=A)
    return ref.to_torch_model(q, "cpu"), types.SimpleNamespace(camera_center=torch.tensor(cam), uid=0)


def test_front_end_refuses_before_any_device_call(hip_lib_built):
    """Everything here is on the CPU: a refusal must come before a device call, and nothing may fall back to the framework."""
    from neural_gaussians import generate_neural_gaussians
    # the feature bank: a missing MLP and every other layout
    pc, camera = _cpu_model(A=0)
    del pc.get_featurebank_mlp
    with pytest.raises(NotImplementedError, match="feature-bank"):
        generate_neural_gaussians(camera, pc)
    bad_banks = [
        nn.Sequential(nn.Linear(4, 32), nn.ReLU(True), nn.Linear(32, 3)),                                  # no softmax
        nn.Sequential(nn.Linear(4, 32), nn.ReLU(True), nn.Linear(32, 3), nn.Softmax(dim=0)),               # over the anchors
        nn.Sequential(nn.Linear(4, 32), nn.ReLU(True), nn.Linear(32, 3), nn.Sigmoid()),
        nn.Sequential(nn.Linear(4, 32), nn.Tanh(), nn.Linear(32, 3), nn.Softmax(dim=1)),
        nn.Sequential(nn.Linear(4, 64), nn.ReLU(True), nn.Linear(64, 3), nn.Softmax(dim=1)),
        nn.Sequential(nn.Linear(3, 32), nn.ReLU(True), nn.Linear(32, 3), nn.Softmax(dim=1)),
        nn.Sequential(nn.Linear(4, 32), nn.ReLU(True), nn.Linear(32, 4), nn.Softmax(dim=1)),
        nn.Sequential(nn.Linear(4, 32, bias=False), nn.ReLU(True), nn.Linear(32, 3), nn.Softmax(dim=1)),
        nn.Sequential(nn.Linear(4, 32), nn.ReLU(True), nn.Linear(32, 32), nn.ReLU(True), nn.Linear(32, 3), nn.Softmax(dim=1)),
        nn.Linear(4, 3),
    ]
    for seq in bad_banks:
        pc.get_featurebank_mlp = seq
        with pytest.raises(NotImplementedError, match="unsupported feature-bank MLP"):
            generate_neural_gaussians(camera, pc)
    # the appearance modules
    pc, camera = _cpu_model(bank=False)
    good = pc.get_appearance_rd
    for attr in ("get_appearance", "get_appearance_rd"):
        keep = getattr(pc, attr)
        for module in (torch.jit.trace(nn.Embedding(3, 8), (torch.zeros(1, dtype=torch.long),)),       # what load_mlp_checkpoints leaves
                       nn.Linear(3, 8), None, nn.Embedding(3, 8, max_norm=1.0), nn.Embedding(3, 8, padding_idx=0), nn.Embedding(3, 16),
                       types.SimpleNamespace(embedding=nn.Linear(3, 8))):
            setattr(pc, attr, module)
            with pytest.raises(NotImplementedError, match=attr):
                generate_neural_gaussians(camera, pc)
        setattr(pc, attr, keep)
    assert pc.get_appearance_rd is good
    # an object whose .embedding is an nn.Embedding is accepted (scene/embedding.py): the next refusal is the camera's uid
    pc.get_appearance = types.SimpleNamespace(embedding=pc.get_appearance)
    for uid in (3, -1, 100):
        camera.uid = uid
        with pytest.raises(IndexError, match="out of range"):
            generate_neural_gaussians(camera, pc)
    camera.uid = 0
    # first-layer widths: din + A
    pc.appearance_dim = 8
    keep = pc.get_color_mlp
    pc.get_color_mlp = nn.Sequential(nn.Linear(36, 32), nn.ReLU(True), nn.Linear(32, 6), nn.Sigmoid())
    with pytest.raises(NotImplementedError, match="appearance_dim"):
        generate_neural_gaussians(camera, pc)
    pc.get_color_mlp = keep
    # what stays refused
    pc.color_channel = 3
    with pytest.raises(NotImplementedError, match="colour channels"):
        generate_neural_gaussians(camera, pc)
    pc.color_channel = 2
    pc.n_offsets = 7
    with pytest.raises(NotImplementedError, match="n_offsets"):
        generate_neural_gaussians(camera, pc)
    pc.n_offsets = 6
    # nothing on a HIP device: a loud error from the first native step, never a framework path
    with pytest.raises(RuntimeError, match="HIP device"):
        generate_neural_gaussians(camera, pc)
    pc, camera = _cpu_model(A=0)
    with pytest.raises(RuntimeError, match="HIP device"):
        generate_neural_gaussians(camera, pc)
