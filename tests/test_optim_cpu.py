"""CPU tests of the optimizer's boundary (lidargs_optim, liblidargs_optim.so, include_optim/): the second library builds and exports
exactly what its header declares, every function is typed from the header, the main library's export set is untouched, and the
Adam class keeps torch.optim.Adam's surface: options it does not implement are refused, CPU parameters are refused, state_dict()
moves between the two classes in both directions, and the optimizer surgery of the training script (concatenate rows, mask rows out,
replace a tensor) leaves param_groups and state consistent.  No device call is made here."""
import ctypes
import os
import subprocess

import pytest
import torch
from torch import nn

import build_hip

build_hip.build()          # importing lidargs_optim needs its library (a no-op when it is up to date)
import lidargs_abi  # noqa: E402
import lidargs_optim  # noqa: E402
import native_lib_checks  # noqa: E402
from lidargs_optim import Adam  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE_OPTIM = os.path.join(ROOT, "include_optim")
DECLARED = {"lidargs_adam_step", "lidargs_adam_max_tensors", "lidargs_optim_last_error", "lidargs_optim_abi_version"}
K = 6      # offsets per anchor
PER_ANCHOR = {"anchor": (3,), "offset": (K, 3), "anchor_feat": (32,), "opacity": (1,), "scaling": (6,), "rotation": (4,)}


def test_second_library_exports_exactly_its_header(hip_lib_built):
    typed = native_lib_checks.check_library(build_hip.TARGETS["optim"], DECLARED, lidargs_optim._lib, hip_lib_built)
    assert "adam.hip" in build_hip.TARGETS["optim"].sources
    i, d, p = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    assert typed["lidargs_adam_step"] == (i, (i, p, d, d, d, p))          # read from the header by eye
    assert typed["lidargs_optim_last_error"] == (ctypes.c_char_p, ())
    assert lidargs_optim._lib.lidargs_optim_abi_version() == 1 and lidargs_optim.MAX_TENSORS == 64


def test_header_is_plain_c_and_the_struct_mirror_matches_it(tmp_path):     # plain C: check_library compiles it with -Wall -Werror
    src = tmp_path / "layout.c"
    fields = [f for f, _ in lidargs_optim._Tensor._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lidargs_optim.h"\nint main(void) { printf("%zu", sizeof(lidargs_adam_tensor));\n'
                   + "".join(f'printf(" %zu", offsetof(lidargs_adam_tensor, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", INCLUDE_OPTIM, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(lidargs_optim._Tensor)] + [getattr(lidargs_optim._Tensor, f).offset for f in fields]


def test_main_library_is_unchanged_by_the_second(hip_lib_built):
    main = native_lib_checks.exports(hip_lib_built)
    assert main == set(lidargs_abi.signatures()) and len(main) == 88
    assert not any("adam" in n or "optim" in n for n in main)
    assert native_lib_checks.exports(build_hip.TARGETS["optim"].out).isdisjoint(main)
    assert "adam.hip" not in build_hip.SOURCES and os.path.abspath(build_hip.build()) == os.path.abspath(hip_lib_built)
    from diff_lidargs_rasterization import _C
    assert _C._lib.lidargs_abi_version() == lidargs_abi.ABI_VERSION       # load() with today's arguments: as before


def test_arguments_are_validated_before_any_device_work(hip_lib_built):
    lib = lidargs_optim._lib
    err = lambda: lib.lidargs_optim_last_error().decode()
    assert lib.lidargs_adam_step(-1, None, 0.9, 0.999, 1e-15, None) == -1 and "n_tensors" in err()
    assert lib.lidargs_adam_step(65, None, 0.9, 0.999, 1e-15, None) == -1 and "n_tensors" in err()
    assert lib.lidargs_adam_step(1, None, 0.9, 0.999, 1e-15, None) == -1 and "NULL table" in err()
    assert lib.lidargs_adam_step(0, None, 0.9, 0.999, 1e-15, None) == 0
    t = (lidargs_optim._Tensor * 2)()
    t[1].n = -5
    assert lib.lidargs_adam_step(2, t, 0.9, 0.999, 1e-15, None) == -1 and "negative size" in err()
    t[1].n = 8
    assert lib.lidargs_adam_step(2, t, 0.9, 0.999, 1e-15, None) == -1 and "NULL pointer" in err()
    t[1].n = 0
    assert lib.lidargs_adam_step(2, t, 0.9, 0.999, 1e-15, None) == 0      # only empty tensors: nothing is launched
    with pytest.raises(ctypes.ArgumentError):
        lib.lidargs_adam_step(0, None, 0.9, 0.999, None, None)


def test_unsupported_options_raise_and_cpu_parameters_are_refused():
    w = lambda: [nn.Parameter(torch.zeros(4, 3))]
    for kw in (dict(weight_decay=1e-2), dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True),
               dict(decoupled_weight_decay=True), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(NotImplementedError):
            Adam(w(), **kw)
    with pytest.raises(ValueError):
        Adam(w(), lr=-1.0)
    opt = Adam([{"params": w(), "name": "anchor"}], lr=0.0, eps=1e-15)
    assert isinstance(opt, torch.optim.Optimizer) and opt.defaults["eps"] == 1e-15
    opt.step()                                                            # no gradient anywhere: nothing to do, no state
    assert len(opt.state) == 0
    opt.param_groups[0]["params"][0].grad = torch.ones(4, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        opt.step()
    opt.param_groups[0]["amsgrad"] = True                                 # an option switched on later is refused at the step
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.step()
    opt.zero_grad(set_to_none=True)
    assert opt.param_groups[0]["params"][0].grad is None


def _model(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    groups = [{"params": [nn.Parameter(torch.randn((n,) + shape, generator=g))], "lr": 1e-3 * (i + 1), "name": name}
              for i, (name, shape) in enumerate(PER_ANCHOR.items())]
    mlp = nn.Sequential(nn.Linear(35, 32), nn.ReLU(True), nn.Linear(32, K))
    groups.append({"params": list(mlp.parameters()), "lr": 2e-3, "name": "mlp_opacity"})
    return groups


def _torch_steps(opt, steps, seed=1):
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for group in opt.param_groups:
            if group["name"] in ("opacity", "rotation"):                  # never receive a gradient in training
                continue
            for p in group["params"]:
                p.grad = torch.randn(p.shape, generator=g)
        opt.step()


def _assert_same_state_dict(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert list(a["state"][k]) == list(b["state"][k]) == ["step", "exp_avg", "exp_avg_sq"]
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device and torch.equal(x, y), (k, name)


def test_state_dict_round_trip_with_torch_adam():
    ref = torch.optim.Adam(_model(7), lr=0.0, eps=1e-15)
    _torch_steps(ref, 3)
    sd = ref.state_dict()
    assert len(sd["state"]) == 4 + 4                                      # anchor, offset, anchor_feat, scaling + the MLP's four tensors
    ours = Adam(_model(7), lr=0.0, eps=1e-15)
    ours.load_state_dict(sd)
    _assert_same_state_dict(ours.state_dict(), sd)
    for state in ours.state.values():
        assert state["step"].dtype == torch.float32 and state["step"].device.type == "cpu" and state["step"].item() == 3.0
    back = torch.optim.Adam(_model(7), lr=0.0, eps=1e-15)
    back.load_state_dict(ours.state_dict())
    _assert_same_state_dict(back.state_dict(), sd)
    _torch_steps(back, 1)                                                 # and torch continues from it
    assert all(s["step"].item() == 4.0 for s in back.state.values())
    fresh = Adam(_model(7), lr=0.0, eps=1e-15)                            # ours without any state -> torch
    torch.optim.Adam(_model(7), lr=0.0, eps=1e-15).load_state_dict(fresh.state_dict())


# ---- the training script's optimizer surgery, restated: per-anchor groups hold one tensor each ----------------------------------

def _is_per_anchor(group):
    return "mlp" not in group["name"]


def _swap_param(opt, group, new_tensor, moments):
    """Put `new_tensor` in the group's only slot; the old parameter's state moves to the new one with `moments` applied to both moments."""
    old = group["params"][0]
    state = opt.state.get(old, None)
    new = nn.Parameter(new_tensor.requires_grad_(True))
    if state is not None:
        state["exp_avg"], state["exp_avg_sq"] = moments(state["exp_avg"]), moments(state["exp_avg_sq"])
        del opt.state[old]
        opt.state[new] = state
    group["params"][0] = new
    return new


def append_rows(opt, rows):
    return {g["name"]: _swap_param(opt, g, torch.cat((g["params"][0].detach(), rows[g["name"]]), dim=0),
                                   lambda m, e=rows[g["name"]]: torch.cat((m, torch.zeros_like(e)), dim=0))
            for g in opt.param_groups if _is_per_anchor(g)}


def keep_rows(opt, mask):
    return {g["name"]: _swap_param(opt, g, g["params"][0].detach()[mask], lambda m: m[mask]) for g in opt.param_groups if _is_per_anchor(g)}


def replace_tensor(opt, name, tensor):
    return {g["name"]: _swap_param(opt, g, tensor, lambda m: torch.zeros_like(tensor)) for g in opt.param_groups if g["name"] == name}


def _assert_consistent(opt, n, steps):
    """Every per-anchor group holds n rows; a parameter with state has moments of its own shape and the expected step count."""
    for group in opt.param_groups:
        for p in group["params"]:
            if _is_per_anchor(group):
                assert p.shape == (n,) + PER_ANCHOR[group["name"]] and p.requires_grad
            state = opt.state.get(p)
            if group["name"] in ("opacity", "rotation"):
                assert state is None
                continue
            assert list(state) == ["step", "exp_avg", "exp_avg_sq"]
            assert state["exp_avg"].shape == p.shape and state["exp_avg_sq"].shape == p.shape and state["step"].item() == steps
            assert state["exp_avg"].is_contiguous() and state["exp_avg_sq"].is_contiguous()
    live = {p for group in opt.param_groups for p in group["params"]}
    assert set(opt.state) <= live, "state left behind for a parameter no group holds"


def test_surgery_keeps_groups_and_state_consistent():
    warm = torch.optim.Adam(_model(9), lr=0.0, eps=1e-15)
    _torch_steps(warm, 2)
    opt = Adam(_model(9), lr=0.0, eps=1e-15)
    opt.load_state_dict(warm.state_dict())
    _assert_consistent(opt, 9, 2)
    before = {g["name"]: opt.state[g["params"][0]]["exp_avg"].clone() for g in opt.param_groups if g["name"] in ("anchor", "scaling")}
    new = append_rows(opt, {name: torch.full((4,) + shape, 0.5) for name, shape in PER_ANCHOR.items()})
    assert set(new) == set(PER_ANCHOR)
    _assert_consistent(opt, 13, 2)
    for name, m in before.items():
        got = opt.state[new[name]]["exp_avg"]
        assert torch.equal(got[:9], m) and not got[9:].any()              # old rows keep their moments, new rows start at zero
    mask = torch.tensor([True, False] * 6 + [True])
    kept = keep_rows(opt, mask)
    _assert_consistent(opt, 7, 2)
    assert torch.equal(opt.state[kept["anchor"]]["exp_avg"], torch.cat((before["anchor"], torch.zeros(4, 3)))[mask])
    rep = replace_tensor(opt, "scaling", torch.ones(7, 6))
    _assert_consistent(opt, 7, 2)
    assert not opt.state[rep["scaling"]]["exp_avg_sq"].any()
    for group in opt.param_groups:                                        # the schedule writes the learning rate per group by name
        if group["name"] == "offset":
            group["lr"] = 3e-4
    sd = opt.state_dict()                                                 # and the result still moves to torch, which steps on
    cont = torch.optim.Adam(_model(7), lr=0.0, eps=1e-15)
    cont.load_state_dict(sd)
    _torch_steps(cont, 1)
    assert [g["lr"] for g in cont.param_groups if g["name"] == "offset"] == [3e-4]
    assert all(s["step"].item() == 3.0 for s in cont.state.values())
