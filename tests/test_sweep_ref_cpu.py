"""CPU tests of tests/sweep_ref.py, the float64 restatement of the sweep-motion compensation (include_sweep/lidargs_sweep.h): that its
closed-form exponential is the matrix exponential of the chart, that the iterates converge as DESIGN.md 4f quotes, that the seam rule
keeps the points next to the image seam on one branch, that one render of the compensated means reproduces a sweep assembled column by
column from renders at each column's own pose, and that autograd's gradients of it are right (gradcheck).  The GPU tests hold the
kernels against this file."""
import numpy as np
import pytest
import torch

import lidargs_scenes as sc
import sweep_ref as R
from util import oracle_forward_backward

F64 = torch.float64
TWIST = torch.tensor(R.TWIST, dtype=F64)


def _vm(seed=7):
    return torch.from_numpy(sc.rigid_viewmatrix(np.random.default_rng(seed))).to(F64)


@pytest.mark.parametrize("xi", [R.TWIST, (0.9, -1.4, 2.0, 1.5, 0.2, 0.05), (0.0, 0.0, 0.0, 1.0, -2.0, 3.0), (1e-9, -2e-9, 0.0, 1.0, -2.0, 3.0),
                                (0.06, 0.05, -0.06, 0.3, 0.0, 0.1)])
def test_closed_form_is_the_matrix_exponential_of_the_chart(xi):
    xi = torch.tensor(xi, dtype=F64)
    p = torch.randn(64, 3, dtype=F64, generator=torch.Generator().manual_seed(1)) * 20
    for t in (1.0, 0.37, -0.5):
        T = torch.matrix_exp(R.generator_matrix(t * xi))
        assert (R.se3_exp(t * xi) - T).abs().max() <= 1e-12
        want = (torch.cat([p, torch.ones(64, 1, dtype=F64)], 1) @ T)[:, :3]
        assert (R.move(p, xi, torch.full((64,), t, dtype=F64)) - want).abs().max() <= 1e-12 * 64


def test_zero_twist_is_the_identity():
    vm = _vm()
    x = R.world_points(R.points(1000, 3), vm)
    for n in (1, 3, 4):
        assert (R.compensate(x, vm, torch.zeros(6, dtype=F64), iterations=n) - x).abs().max() <= 1e-12


def _errors(x, vm, sweep=(-0.5, 0.5)):
    """Per point |x'_n - x'_12| for n = 1..4."""
    conv = R.compensate(x, vm, TWIST, sweep, 12)
    return [(R.compensate(x, vm, TWIST, sweep, n) - conv).norm(dim=1) for n in (1, 2, 3, 4)]


def test_iterates_converge_as_quoted():
    vm = _vm()
    x = R.world_points(R.points(20000, 5), vm)
    e = _errors(x, vm)
    worst = [float(k.max()) for k in e]
    print("max error against 12 iterations, n = 1..4:", worst, "median:", [float(k.median()) for k in e])
    assert worst[0] > worst[1] > worst[2] > worst[3]
    assert worst[2] < 2e-3


def test_seam_scene_stays_on_one_branch():
    vm = _vm()
    p0 = R.points(512, 9, seam=True)
    x = R.world_points(p0, vm)
    s3 = R.iterate(x @ vm[:3, :3] + vm[3, :3], TWIST, (-0.5, 0.5), 3)
    outside = (s3 < 0) | (s3 >= 1)
    print("points whose s_3 left [0, 1):", int(outside.sum()))
    assert int(outside.sum()) >= 20
    e = _errors(x, vm)
    assert float(e[2].max()) < 2e-3 and float(e[2][outside].max()) < 2e-3
    # without the rule those points jump to the other end of the sweep: off by the whole motion
    raw = R.column_fraction(R.move(p0, TWIST, -0.5 + R.column_fraction(p0)))
    assert float((raw - R.column_fraction(p0)).abs().max()) > 0.9


W_COL, H_COL, P_COL, MOD_COL = 128, 16, 20000, 2.0


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_one_compensated_render_against_a_sweep_assembled_column_by_column(seed):
    """Column c of the truth is column c of a render from the pose of column c's time, vm @ T(t_c xi), t_c = t((c + 0.5) / W)."""
    scene = sc.make_scene("street", P_COL, H_COL, seed)
    vm = torch.from_numpy(scene["viewmatrix"]).to(F64)

    def depth(means=None, view=None):
        s = dict(scene)
        if means is not None:
            s["means3D"] = means.to(torch.float32).numpy()
        if view is not None:
            s["viewmatrix"] = view.to(torch.float32).numpy()
        o = oracle_forward_backward(s, W_COL, H_COL, scale_modifier=MOD_COL)
        return o["depth"][0], o["occ"][0]

    truth, truth_occ = np.zeros((H_COL, W_COL), np.float32), np.zeros((H_COL, W_COL), np.float32)
    for c in range(W_COL):
        d, o = depth(view=vm @ R.se3_exp((-0.5 + (c + 0.5) / W_COL) * TWIST))
        truth[:, c], truth_occ[:, c] = d[:, c], o[:, c]
    x = torch.from_numpy(scene["means3D"]).to(F64)
    comp, comp_occ = depth(means=R.compensate(x, vm, TWIST))
    plain, plain_occ = depth()
    both = (truth_occ > 0.5) & (comp_occ > 0.5) & (plain_occ > 0.5)
    e_comp, e_plain = np.median(np.abs(comp - truth)[both]), np.median(np.abs(plain - truth)[both])
    print(f"seed {seed}: {int(both.sum())} pixels, median |d depth| compensated {e_comp:.4f} m, uncompensated {e_plain:.4f} m, ratio {e_plain / e_comp:.1f}")
    assert int(both.sum()) >= 800
    assert e_comp <= e_plain / 5


def test_gradcheck_of_the_restatement():
    vm = _vm().requires_grad_(True)
    x = R.world_points(torch.cat([R.points(6, 21), R.points(4, 22, seam=True)]), vm.detach()).requires_grad_(True)
    for xi, n, sweep in ((TWIST, 3, (-0.5, 0.5)), (torch.tensor((0.9, -1.4, 2.0, 1.5, 0.2, 0.05), dtype=F64), 2, (0.0, 1.0))):
        xi = xi.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda a, b, c: R.compensate(a, b, c, sweep, n), (x, vm, xi), eps=1e-6, atol=1e-6, rtol=1e-5)
