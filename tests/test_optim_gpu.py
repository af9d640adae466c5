"""GPU tests of lidargs_optim.Adam (csrc/adam.hip): one step from arbitrary state against torch.optim.Adam, and a short trajectory.

The yardstick of the one-step check is torch's own Adam, which is what the training script runs: the same float32 (param, grad,
exp_avg, exp_avg_sq, step, lr) goes through ours, through torch.optim.Adam on the device three ways (foreach=False, foreach=True,
fused=True) and through torch.optim.Adam on float64 CPU copies, which gives the exact value.  For each of param, exp_avg and exp_avg_sq
of each tensor our maximum absolute error against the float64 result, and our 99.9th-percentile relative error of the parameter update,
must each be at most 2 x the largest such error among torch's three float32 paths: room for one differently placed rounding per element
and nothing more.  Every element takes part.  Where a value is not finite, ours and a path's count as equal to the exact one only when
they are the same non-finite value (error 0), otherwise the error is +inf; the NaN / inf pattern is also compared with the
foreach=False path directly.  How many elements differ in bits from the foreach=False path is printed per case, not asserted
(DESIGN.md section "Optimizer step" records it)."""
import math

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

K = 6
MODEL_SHAPES = {"anchor": (3,), "offset": (K, 3), "anchor_feat": (32,), "scaling": (6,)}      # the per-anchor tensors that receive gradients
MLP_SHAPES = [s for dout in (K, 7 * K, K, K) for s in ((32, 36), (32,), (dout, 32), (dout,))]   # sixteen nn.Linear tensors of the four MLPs
FACTOR = 2.0


def _case(shape, step, lr, seed, grad=None, fresh=False, offset_view=False):
    """One tensor's inputs on the CPU in float32; `grad`: None = normal, or a callable that edits the drawn gradient in place."""
    g = torch.Generator().manual_seed(seed)
    c = dict(param=torch.randn(shape, generator=g), grad=0.1 * torch.randn(shape, generator=g) * torch.rand(shape, generator=g) ** 4,
             exp_avg=0.05 * torch.randn(shape, generator=g), exp_avg_sq=(0.05 * torch.randn(shape, generator=g)) ** 2,
             step=float(step - 1), lr=lr, offset_view=offset_view)
    if fresh:
        c["exp_avg"].zero_(); c["exp_avg_sq"].zero_()
    if grad is not None:
        grad(c["grad"])
    return c


def _place(t, device, dtype, offset_view):
    """A copy on `device`; with offset_view a contiguous view that starts 4 bytes into its allocation (never 16-byte aligned)."""
    t = t.to(dtype)
    if not offset_view:
        return t.to(device).clone()
    base = torch.empty(t.numel() + 1, dtype=dtype, device=device)
    view = base[1:].view(t.shape)
    view.copy_(t)
    return view


def _run(cases, make, device, dtype, step_device, chunk=None):
    """One step of `make(groups)` on copies of the cases; returns [(param, exp_avg, exp_avg_sq, step)] on the CPU."""
    params = [nn.Parameter(_place(c["param"], device, dtype, c["offset_view"])) for c in cases]
    opt = make([{"params": [p], "lr": c["lr"]} for p, c in zip(params, cases)])
    for p, c in zip(params, cases):
        p.grad = _place(c["grad"], device, dtype, False)
        opt.state[p] = {"step": torch.tensor(c["step"], dtype=torch.float32, device=step_device),
                        "exp_avg": _place(c["exp_avg"], device, dtype, False), "exp_avg_sq": _place(c["exp_avg_sq"], device, dtype, False)}
    opt.step()
    if device != "cpu":
        torch.cuda.synchronize()
    return [(p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu(), float(opt.state[p]["step"])) for p in params]


def _err(x, exact):
    """|x - exact| per element in float64; equal non-finite values count as 0, any other non-finite difference as +inf."""
    x = x.double()
    e = (x - exact).abs()
    same = (x == exact) | (x.isnan() & exact.isnan())
    e = torch.where(same, torch.zeros_like(e), e)
    return torch.where(e.isnan(), torch.full_like(e, math.inf), e)


def _p999(e):
    if e.numel() == 0:
        return 0.0
    k = max(1, math.ceil(0.999 * e.numel()))
    return float(e.flatten().kthvalue(k).values)


def _metrics(res, exact, p_old):
    p, m, v, _ = res
    pe, me, ve, _ = exact
    mx = lambda e: float(e.max()) if e.numel() else 0.0
    u_exact = pe - p_old.double()
    ue = _err(p.double() - p_old.double(), u_exact)
    rel = torch.where(ue == 0, torch.zeros_like(ue), ue / u_exact.abs())      # a wrong update of an exactly zero one: +inf
    rel = torch.where(rel.isnan(), torch.full_like(rel, math.inf), rel)
    return dict(param=mx(_err(p, pe)), exp_avg=mx(_err(m, me)), exp_avg_sq=mx(_err(v, ve)), update_rel_p999=_p999(rel))


def check_one_step(cases, name, betas=(0.9, 0.999), eps=1e-15):
    from lidargs_optim import Adam
    kw = dict(lr=0.0, betas=betas, eps=eps)
    ours = _run(cases, lambda g: Adam(g, **kw), "cuda", torch.float32, "cpu")
    paths = {"foreach=False": _run(cases, lambda g: torch.optim.Adam(g, foreach=False, fused=False, **kw), "cuda", torch.float32, "cpu"),
             "foreach=True": _run(cases, lambda g: torch.optim.Adam(g, foreach=True, **kw), "cuda", torch.float32, "cpu"),
             "fused=True": _run(cases, lambda g: torch.optim.Adam(g, fused=True, **kw), "cuda", torch.float32, "cuda")}
    exact = _run(cases, lambda g: torch.optim.Adam(g, foreach=False, **kw), "cpu", torch.float64, "cpu")
    failures, differ, total = [], [0, 0, 0], 0
    for i, c in enumerate(cases):
        assert ours[i][3] == exact[i][3] == c["step"] + 1
        got = _metrics(ours[i], exact[i], c["param"])
        ref = {k: _metrics(r[i], exact[i], c["param"]) for k, r in paths.items()}
        for key, val in got.items():
            bound = FACTOR * max(r[key] for r in ref.values())
            if not val <= bound:
                failures.append(f"tensor {i} {list(c['param'].shape)} step {c['step'] + 1:g} lr {c['lr']:g}: {key} ours {val:.3e} > {FACTOR:g} x "
                                f"max({', '.join(f'{k} {r[key]:.3e}' for k, r in ref.items())})")
        base = paths["foreach=False"][i]
        for j in range(3):
            a, b = ours[i][j], base[j]
            assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.isinf(), b.isinf()) and torch.equal(a[a.isinf()], b[b.isinf()]), \
                f"{name}: tensor {i}: the NaN / inf pattern of {('param', 'exp_avg', 'exp_avg_sq')[j]} differs from torch's"
            differ[j] += int(((a.view(torch.int32) != b.view(torch.int32)) & ~(a.isnan() & b.isnan())).sum())
        total += c["param"].numel()
        if c["lr"] == 0:
            assert torch.equal(ours[i][0].view(torch.int32), c["param"].view(torch.int32)), f"{name}: tensor {i}: lr = 0 changed the parameter's bits"
    print(f"\n[adam one-step] {name}: {len(cases)} tensors, {total} elements; bits differing from torch foreach=False: "
          f"param {differ[0]}, exp_avg {differ[1]}, exp_avg_sq {differ[2]}")
    assert not failures, f"{name}:\n" + "\n".join(failures)
    return ours


def _model_cases(N, step, lr, seed, **kw):
    return [_case((N,) + s, step, lr, seed + 17 * i, **kw) for i, s in enumerate(MODEL_SHAPES.values())]


@pytest.mark.parametrize("N", [1, 5, 4099, 333_000])
def test_model_shapes(N):
    """anchor [N, 3] with N odd has N * 3 odd: its tail goes through the 4-byte path; [1, 3] and [5, 3] are tails only."""
    steps, lrs = (1, 2, 1000, 30000), (7.5e-3, 1e-5, 0.0, 7.5e-3)
    cases = [c for j, (s, lr) in enumerate(zip(steps, lrs)) if N <= 4099 or j in (0, 3) for c in _model_cases(N, s, lr, 100 * j + N % 97)]
    check_one_step(cases, f"model shapes N={N}")


@pytest.mark.parametrize("lr", [0.0, 1e-5, 7.5e-3])
@pytest.mark.parametrize("step", [1, 2, 1000, 30000])
def test_steps_and_learning_rates(step, lr):
    check_one_step(_model_cases(4099, step, lr, 7, fresh=(step == 1)), f"step {step} lr {lr:g}")


def test_unaligned_view_takes_the_scalar_path():
    cases = [_case((4099, 3), 5, 1e-3, 3, offset_view=True), _case((9001,), 5, 1e-3, 4, offset_view=True), _case((4099, 3), 5, 1e-3, 3)]
    ours = check_one_step(cases, "4-byte-offset view")
    assert torch.equal(ours[0][0], ours[2][0]) and torch.equal(ours[0][2], ours[2][2])      # the same values on either path


def test_mlp_tensors_and_mixed_steps():
    """The sixteen nn.Linear tensors (32 x 36 weights down to 6-element biases, and a 1-element one), every tensor at a step of its own."""
    steps = [1, 2, 1000, 30000]
    cases = [_case(s, steps[i % 4], (1e-5, 7.5e-3, 2e-3)[i % 3], 40 + i, fresh=(steps[i % 4] == 1)) for i, s in enumerate(MLP_SHAPES + [(1,)])]
    cases += _model_cases(4099, 77, 1e-3, 9)
    check_one_step(cases, "MLP tensors, mixed steps")


@pytest.mark.parametrize("fresh", [True, False])
def test_zero_gradient_rows(fresh):
    def zero_rows(g):
        g[::3] = 0
    cases = _model_cases(4099, 1 if fresh else 500, 7.5e-3, 21, grad=zero_rows, fresh=fresh)
    ours = check_one_step(cases, f"zero gradient rows, {'fresh' if fresh else 'warm'} state")
    if fresh:
        for (p, m, v, _), c in zip(ours, cases):      # 0 / (0 + eps): no update, no NaN
            assert torch.equal(p[::3], c["param"][::3]) and not m[::3].any() and not v[::3].any()


@pytest.mark.parametrize("value", [1e-20, 1e20, float("nan")])
def test_extreme_gradients(value):
    """1e-20: the square underflows; 1e+20: it overflows to inf; NaN: the pattern must be torch's."""
    def edit(g):
        g.view(-1)[::5] = value
        g.view(-1)[2::10] = -value
    for fresh in (True, False):
        check_one_step(_model_cases(1031, 1 if fresh else 300, 1e-3, 33, grad=edit, fresh=fresh), f"gradient {value:g}, {'fresh' if fresh else 'warm'} state")


def test_more_tensors_than_one_call_holds_an_empty_one_and_one_without_gradient():
    from lidargs_optim import Adam, MAX_TENSORS
    n = MAX_TENSORS + 9
    cases = [_case((5 + 13 * i,), 1 + i, 1e-3, 60 + i) for i in range(n)]
    cases.insert(7, _case((0, 3), 4, 1e-3, 1))                            # no anchors left after a prune
    check_one_step(cases, f"{n + 1} tensors")
    p, q = nn.Parameter(torch.randn(100, 3, device="cuda")), nn.Parameter(torch.randn(100, 4, device="cuda"))
    opt = Adam([{"params": [p], "name": "scaling"}, {"params": [q], "name": "rotation"}], lr=1e-2, eps=1e-15)
    p.grad, before = torch.randn_like(p), q.detach().clone()
    opt.step()
    assert list(opt.state) == [p] and torch.equal(q, before) and opt.state[p]["step"].item() == 1.0
    assert opt.state[p]["step"].device.type == "cpu" and opt.state[p]["step"].dtype == torch.float32


def test_refusals_on_the_device():
    from lidargs_optim import Adam
    p = nn.Parameter(torch.randn(8, 3, device="cuda", dtype=torch.float64))
    p.grad = torch.randn_like(p)
    with pytest.raises(RuntimeError, match="group `offset`.*float32"):
        Adam([{"params": [p], "name": "offset"}], lr=1e-3).step()
    q = nn.Parameter(torch.randn(8, 6, device="cuda")[:, :3])
    q.grad = torch.randn(8, 3, device="cuda")
    with pytest.raises(RuntimeError, match="group 0.*contiguous"):
        Adam([q], lr=1e-3).step()


def test_trajectory_with_surgery_then_torch_continues():
    """Twenty steps with a learning rate that changes every step, one row concatenation and one row prune in the middle, then the
    state moves into torch.optim.Adam, which continues.  Structure only (keys, shapes, counters, no NaN): values are the one-step test's."""
    from lidargs_optim import Adam
    torch.manual_seed(5)
    shapes = {"anchor": (3,), "offset": (K, 3), "anchor_feat": (32,), "opacity": (1,), "scaling": (6,), "rotation": (4,)}
    N = 300
    mlp = nn.Sequential(nn.Linear(35, 32), nn.ReLU(True), nn.Linear(32, K)).cuda()
    groups = [{"params": [nn.Parameter(torch.randn((N,) + s, device="cuda"))], "lr": 0.0, "name": n} for n, s in shapes.items()]
    groups.append({"params": list(mlp.parameters()), "lr": 0.0, "name": "mlp_opacity"})
    opt = Adam(groups, lr=0.0, eps=1e-15)
    target = {n: torch.randn(s, device="cuda") for n, s in shapes.items()}

    def backward():
        opt.zero_grad(set_to_none=True)
        loss = sum(((g["params"][0] - target[g["name"]]) ** 2).mean() for g in opt.param_groups if g["name"] in ("anchor", "offset", "anchor_feat", "scaling"))
        x = torch.randn(64, 35, device="cuda")
        (loss + (mlp(x) ** 2).mean()).backward()

    def swap(group, tensor, moments):
        old, new = group["params"][0], nn.Parameter(tensor.requires_grad_(True))
        state = opt.state.pop(old, None)
        if state is not None:
            state["exp_avg"], state["exp_avg_sq"] = moments(state["exp_avg"]), moments(state["exp_avg_sq"])
            opt.state[new] = state
        group["params"][0] = new

    for it in range(20):
        for g in opt.param_groups:
            g["lr"] = 0.0 if g["name"] == "anchor" else 1e-2 * 0.9 ** it
        if it == 8:                                                       # 40 anchors grow
            for g in opt.param_groups[:6]:
                ext = torch.randn((40,) + shapes[g["name"]], device="cuda")
                swap(g, torch.cat((g["params"][0].detach(), ext)), lambda m, e=ext: torch.cat((m, torch.zeros_like(e))))
            N += 40
        if it == 13:                                                      # every fourth is pruned
            mask = torch.arange(N, device="cuda") % 4 != 0
            for g in opt.param_groups[:6]:
                swap(g, g["params"][0].detach()[mask], lambda m: m[mask])
            N = int(mask.sum())
        backward()
        opt.step()
    assert N == 255
    for g in opt.param_groups:
        for p in g["params"]:
            state = opt.state.get(p)
            if g["name"] in ("opacity", "rotation"):
                assert state is None and p.shape[0] == N
                continue
            assert list(state) == ["step", "exp_avg", "exp_avg_sq"] and state["step"].item() == 20.0
            assert state["exp_avg"].shape == p.shape == state["exp_avg_sq"].shape and (g["name"] == "mlp_opacity" or p.shape[0] == N)
            for t in (p, state["exp_avg"], state["exp_avg_sq"]):
                assert torch.isfinite(t).all()
            assert state["exp_avg_sq"].any()
    ref = torch.optim.Adam([{"params": [nn.Parameter(p.detach().clone()) for p in g["params"]], "lr": 0.0, "name": g["name"]} for g in opt.param_groups],
                           lr=0.0, eps=1e-15)
    ref.load_state_dict(opt.state_dict())
    for it in range(5):
        for g in ref.param_groups:
            for p in g["params"]:
                if g["name"] not in ("opacity", "rotation"):
                    p.grad = 0.01 * torch.randn_like(p)
        ref.step()
    for g in ref.param_groups:
        for p in g["params"]:
            if g["name"] not in ("opacity", "rotation"):
                assert ref.state[p]["step"].item() == 25.0 and torch.isfinite(p).all()
