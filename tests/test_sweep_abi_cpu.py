"""CPU tests of the sweep-motion entry points' boundary (include_sweep/lidargs_sweep.h, prefix `lgsweep_`, part of liblidargs_hip.so): the
header is plain C and declares exactly the expected functions, the library exports exactly those under that prefix and nothing new under
`lidargs_`, the binding's one CDLL types them from the header, and arguments are refused before any device work (never-dereferenced
pointers: no device is needed).  The `lidargs_*` side of the library is tests/test_abi_cpu.py's."""
import ctypes

import pytest

import build_hip
from native_lib_checks import check_family

DECLARED = {"lgsweep_partial_floats", "lgsweep_forward", "lgsweep_backward"}


def test_header_library_and_binding_agree(hip_lib_built):
    typed = check_family("sweep", "lidargs_sweep.h", DECLARED, hip_lib_built)
    assert "sweep_motion.hip" in build_hip.SOURCES
    i, f, z, p = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p               # written from the header by eye
    assert typed["lgsweep_partial_floats"] == (z, (i,))
    assert typed["lgsweep_forward"] == (i, (i, p, p, p, f, f, i, p, p))
    assert typed["lgsweep_backward"] == (i, (i, p, p, p, f, f, i, p, p, p, p, p, z, p))
    import sweep_motion
    from diff_lidargs_rasterization import _C
    assert sweep_motion._lib is _C._lib                                                      # the process' one CDLL


def test_arguments_are_refused_before_any_device_work(hip_lib_built):
    import sweep_motion
    lib = sweep_motion._lib
    assert lib.lgsweep_partial_floats(0) == 0 and lib.lgsweep_partial_floats(-3) == 0
    assert lib.lgsweep_partial_floats(1) == 32 and lib.lgsweep_partial_floats(256) == 32 and lib.lgsweep_partial_floats(257) == 64
    err = lambda: lib.lidargs_last_error().decode()
    q = ctypes.c_void_p(4096)                     # never dereferenced: every call below is refused first
    odd = ctypes.c_void_p(4096 + 4)
    inf, nan = float("inf"), float("nan")

    def fwd(P=4, means=q, vm=q, xi=q, t0=-0.5, t1=0.5, n=3, out=q):
        return lib.lgsweep_forward(P, means, vm, xi, t0, t1, n, out, None)

    def bwd(P=4, means=q, vm=q, xi=q, t0=-0.5, t1=0.5, n=3, g=q, gx=q, gxi=q, gvm=q, part=q, nf=32):
        return lib.lgsweep_backward(P, means, vm, xi, t0, t1, n, g, gx, gxi, gvm, part, nf, None)

    for call, name, pointers in ((fwd, "sweep_forward", ("means", "vm", "xi", "out")), (bwd, "sweep_backward", ("means", "vm", "xi", "g", "gx"))):
        assert call(P=-1) == -1 and name in err() and "negative" in err()
        for n in (0, 5, -1):
            assert call(n=n) == -1 and name in err() and "iterations" in err()
        for kw in (dict(t0=inf), dict(t1=-inf), dict(t0=nan), dict(t1=nan)):
            assert call(**kw) == -1 and name in err() and "finite" in err()
        for k in pointers:
            assert call(**{k: None}) == -1 and name in err() and "NULL required pointer" in err(), k
    # the scratch of the reduced gradients: NULL, misaligned, short -- with either gradient asked for
    for want in (dict(gxi=None), dict(gvm=None), {}):
        for bad in (dict(part=None), dict(part=odd), dict(nf=31), dict(P=257, nf=63)):
            assert bwd(**want, **bad) == -1 and "sweep_backward" in err() and "lgsweep_partial_floats" in err(), (want, bad)
    with pytest.raises(ctypes.ArgumentError):
        lib.lgsweep_partial_floats(1.5)
    with pytest.raises(ctypes.ArgumentError):
        fwd(n=3.0)


def test_python_refusals_that_need_no_device(hip_lib_built):
    import torch
    import sweep_motion
    x, vm, xi = torch.zeros(4, 3), torch.eye(4), torch.zeros(6)
    with pytest.raises(RuntimeError, match="HIP device"):
        sweep_motion.compensate(x, vm, xi)
    T = sweep_motion.se3_exp(torch.tensor([0.01, -0.02, 0.05, 1.5, 0.2, 0.05], dtype=torch.float64))
    import sweep_ref
    assert (T - torch.matrix_exp(sweep_ref.generator_matrix(torch.tensor(sweep_ref.TWIST, dtype=torch.float64)))).abs().max() <= 1e-12
    big = torch.tensor([0.9, -1.4, 2.0, 1.5, 0.2, 0.05], dtype=torch.float64, requires_grad=True)
    assert (sweep_motion.se3_exp(big) - torch.matrix_exp(sweep_ref.generator_matrix(big))).abs().max() <= 1e-12
    assert torch.autograd.gradcheck(sweep_motion.se3_exp, (big,)) and sweep_motion.se3_exp(torch.zeros(6)).equal(torch.eye(4))
