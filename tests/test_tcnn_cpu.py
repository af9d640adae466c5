"""CPU tests of the tinycudann stand-in (lidar-gs_amd/tinycudann, liblidargs_tcnn.so, include_tcnn/): the fourth library builds and
exports exactly what its header declares, the restatement tests/tcnn_ref.py has the documented column layout and correct hand-written
gradients, and the config handling (refusals, the `degree` warning, the widths) works without a device."""
import ctypes
import math
import warnings

import pytest
import torch

import tcnn_ref as ref

DECLARED = {"lidargs_tcnn_frequency_forward", "lidargs_tcnn_frequency_backward", "lidargs_tcnn_param_count", "lidargs_tcnn_mlp_forward",
            "lidargs_tcnn_forward_row_tile", "lidargs_tcnn_backward_row_tile", "lidargs_tcnn_backward_blocks",
            "lidargs_tcnn_backward_partial_floats", "lidargs_tcnn_mlp_backward", "lidargs_tcnn_last_error", "lidargs_tcnn_abi_version"}


def test_header_parses_and_library_exports_exactly_the_declared_functions(hip_lib_built):
    import build_hip
    import lidargs_abi
    import native_lib_checks
    import tinycudann as tcnn
    typed = native_lib_checks.check_library(build_hip.TARGETS["tcnn"], DECLARED, tcnn._lib, hip_lib_built)
    assert "raydrop_mlp.hip" in build_hip.TARGETS["tcnn"].sources
    assert len(lidargs_abi.signatures()) == 88                                 # every signature typed from include/: the tcnn library added none to the main header's
    i, z, p = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p                   # written from the header by eye
    assert typed["lidargs_tcnn_frequency_forward"] == (i, (i, i, i, p, p, p))
    assert typed["lidargs_tcnn_frequency_backward"] == (i, (i, i, i, p, p, p, p))
    assert typed["lidargs_tcnn_param_count"] == (z, (i, i, i))
    assert typed["lidargs_tcnn_mlp_forward"] == (i, (i, i, i, i, i, p, p, p, p))
    assert typed["lidargs_tcnn_backward_partial_floats"] == (z, (i, i, i, i))
    assert typed["lidargs_tcnn_mlp_backward"] == (i, (i, i, i, i, i) + (p,) * 6 + (z, p))
    assert tcnn._lib.lidargs_tcnn_abi_version() == tcnn.ABI_VERSION == 1


def test_entry_points_validate_before_any_device_work(hip_lib_built):
    import tinycudann as tcnn
    lib = tcnn._lib
    err = lambda: lib.lidargs_tcnn_last_error().decode()
    host = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)               # never dereferenced: every call below is refused or a no-op
    assert lib.lidargs_tcnn_param_count(120, 4, 1) == 128 * 120 + 3 * 128 * 128 + 128
    assert lib.lidargs_tcnn_param_count(5, 1, 3) == 128 * 5 + 3 * 128
    assert lib.lidargs_tcnn_param_count(129, 4, 1) == 0 and lib.lidargs_tcnn_param_count(120, 9, 1) == 0 and lib.lidargs_tcnn_param_count(120, 4, 17) == 0
    assert lib.lidargs_tcnn_forward_row_tile() == tcnn.FORWARD_ROW_TILE and tcnn.FORWARD_ROW_TILE % 16 == 0
    assert lib.lidargs_tcnn_backward_row_tile() == tcnn.BACKWARD_ROW_TILE and tcnn.BACKWARD_ROW_TILE % 16 == 0
    assert lib.lidargs_tcnn_frequency_forward(-1, 3, 12, host, host, None) == -1 and "bad sizes" in err()
    assert lib.lidargs_tcnn_frequency_forward(4, 3, 33, host, host, None) == -1 and "bad sizes" in err()
    assert lib.lidargs_tcnn_frequency_forward(4, 3, 12, None, host, None) == -1 and "NULL" in err()
    assert lib.lidargs_tcnn_frequency_forward(0, 3, 12, None, None, None) == 0
    assert lib.lidargs_tcnn_frequency_backward(4, 0, 12, host, host, host, None) == -1 and "bad sizes" in err()
    assert lib.lidargs_tcnn_frequency_backward(4, 2, 12, host, host, None, None) == -1 and "NULL" in err()
    assert lib.lidargs_tcnn_mlp_forward(4, 129, 4, 1, 1, host, host, host, None) == -1 and "bad sizes" in err()
    assert lib.lidargs_tcnn_mlp_forward(4, 120, 0, 1, 1, host, host, host, None) == -1 and "bad sizes" in err()
    assert lib.lidargs_tcnn_mlp_forward(4, 120, 4, 1, 2, host, host, host, None) == -1 and "bad sizes" in err()
    assert lib.lidargs_tcnn_mlp_forward(4, 120, 4, 1, 1, host, None, host, None) == -1 and "NULL" in err()
    assert lib.lidargs_tcnn_mlp_forward(0, 120, 4, 1, 1, None, None, None, None) == 0
    assert lib.lidargs_tcnn_mlp_backward(4, 120, 4, 17, 1, host, host, host, host, None, host, 1 << 30, None) == -1 and "bad sizes" in err()
    assert lib.lidargs_tcnn_mlp_backward(4, 120, 4, 1, 1, host, host, None, host, None, host, 1 << 30, None) == -1 and "NULL" in err()
    assert lib.lidargs_tcnn_mlp_backward(4, 120, 4, 1, 1, host, host, host, None, None, host, 1 << 30, None) == -1 and "NULL dparams" in err()
    assert lib.lidargs_tcnn_mlp_backward(4, 120, 4, 1, 1, host, host, host, host, None, host, 0, None) == -1 and "partials too small" in err()
    with pytest.raises(ctypes.ArgumentError):
        lib.lidargs_tcnn_mlp_forward(4.0, 120, 4, 1, 1, host, host, host, None)


@pytest.mark.parametrize("D,F", [(3, 12), (2, 12), (2, 4), (2, 1)])
def test_restatement_has_the_documented_column_layout(D, F):
    g = torch.Generator().manual_seed(D * 100 + F)
    x = (torch.rand(7, D, generator=g, dtype=torch.float64) * 2 - 1) * 3
    x[0, 0], x[1, -1] = 0.0, 80.0
    got = ref.encode(x, F)
    assert got.shape == (7, D * 2 * F) and got.dtype == torch.float64
    for n in range(7):
        for d in range(D):
            for f in range(F):
                for s in range(2):
                    want = math.sin(math.pi * 2 ** f * float(x[n, d]) + s * math.pi / 2)
                    assert abs(float(got[n, d * 2 * F + 2 * f + s]) - want) <= 1e-9, (n, d, f, s)


def test_restatement_gradients_match_float64_autograd():
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(9, 3, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_()
    dout = torch.randn(9, 3 * 2 * 6, generator=g, dtype=torch.float64)
    ref.encode(x, 6).backward(dout)
    torch.testing.assert_close(ref.encode_grad(x.detach(), dout, 6), x.grad, rtol=1e-12, atol=1e-9)
    for n_in, h, n_out, sig in ((120, 4, 1, True), (5, 1, 3, False), (7, 3, 16, False)):
        n_params = sum(r * c for r, c in ref.layer_shapes(n_in, h, n_out))
        params = (torch.randn(n_params, generator=g, dtype=torch.float64) * 0.15).requires_grad_()
        x = (torch.rand(33, n_in, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_()
        dout = torch.randn(33, n_out, generator=g, dtype=torch.float64)
        out = ref.mlp(x, params, h, n_out, sig)
        out.backward(dout)
        o2, dp, dx = ref.mlp_grads(x.detach(), params.detach(), dout, h, n_out, sig)
        torch.testing.assert_close(o2, out.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(dp, params.grad, rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(dx, x.grad, rtol=1e-10, atol=1e-12)


def test_param_layout_is_row_major_out_in_in_network_order():
    mats = ref.split_params(torch.arange(128 * 5 + 128 * 128 + 3 * 128, dtype=torch.float64), 5, 2, 3)
    assert [tuple(m.shape) for m in mats] == [(128, 5), (128, 128), (3, 128)]
    assert float(mats[0][1, 0]) == 5 and float(mats[1][0, 0]) == 640 and float(mats[1][0, 1]) == 641 and float(mats[2][0, 0]) == 640 + 16384
    from tinycudann import _config
    assert _config.layer_shapes(5, 2, 3) == ref.layer_shapes(5, 2, 3)


def test_degree_key_is_ignored_with_a_warning_and_the_widths_are_the_documented_ones(hip_lib_built):
    import tinycudann as tcnn
    with pytest.warns(UserWarning, match=r"'degree'=4.*n_frequencies=12"):
        enc_dir = tcnn.Encoding(n_input_dims=3, encoding_config={"otype": "Frequency", "degree": 4})
    with pytest.warns(UserWarning, match=r"'degree'=6.*n_frequencies=12") as rec:
        enc_i_d = tcnn.Encoding(n_input_dims=2, encoding_config={"otype": "Frequency", "degree": 6})
    assert len(rec) == 1
    assert (enc_dir.n_output_dims, enc_i_d.n_output_dims) == (72, 48) and enc_dir.n_input_dims == 3
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        enc = tcnn.Encoding(2, {"otype": "Frequency", "n_frequencies": 4})
        net = tcnn.Network(n_input_dims=120, n_output_dims=1, network_config={
            "otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": 128, "n_hidden_layers": 4})
    assert enc.n_output_dims == 16 and enc.params.numel() == 0 and enc.params.dtype == torch.float32
    assert (net.n_input_dims, net.n_output_dims) == (120, 1)
    assert list(net.state_dict()) == ["params"] and list(enc.state_dict()) == ["params"]
    assert net.params.shape == (128 * 120 + 3 * 128 * 128 + 128,) and net.params.dtype == torch.float32
    with pytest.warns(UserWarning, match="'foo'='bar'"):
        tcnn.Network(4, 2, {"otype": "CutlassMLP", "foo": "bar", "n_hidden_layers": 2})


def test_weights_are_xavier_uniform_and_a_function_of_the_seed(hip_lib_built):
    import tinycudann as tcnn
    cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 128, "n_hidden_layers": 2}
    a, b, c = tcnn.Network(7, 3, cfg), tcnn.Network(7, 3, cfg, seed=1337), tcnn.Network(7, 3, cfg, seed=1)
    assert torch.equal(a.params, b.params) and not torch.equal(a.params, c.params)
    for m, (fo, fi) in zip(ref.split_params(a.params.detach(), 7, 2, 3), ref.layer_shapes(7, 2, 3)):
        bound = math.sqrt(6.0 / (fi + fo))
        assert float(m.abs().max()) <= bound and float(m.abs().max()) > 0.8 * bound and abs(float(m.mean())) < 0.1 * bound


@pytest.mark.parametrize("make", [
    lambda t: t.Encoding(3, {"otype": "HashGrid"}),
    lambda t: t.Encoding(3, {"otype": "Composite", "nested": [{"otype": "Frequency"}]}),
    lambda t: t.Encoding(3, {"otype": "Frequency", "nested": []}),
    lambda t: t.Encoding(3, {"otype": "Frequency", "n_frequencies": 33}),
    lambda t: t.Encoding(3, {"otype": "Frequency"}, dtype=torch.half),
    lambda t: t.Network(8, 1, {"otype": "FullyFusedMLP", "activation": "Sigmoid"}),
    lambda t: t.Network(8, 1, {"otype": "FullyFusedMLP", "output_activation": "Exponential"}),
    lambda t: t.Network(8, 1, {"otype": "FullyFusedMLP", "n_neurons": 64}),
    lambda t: t.Network(8, 1, {"otype": "FullyFusedMLP", "n_hidden_layers": 9}),
    lambda t: t.Network(8, 1, {"otype": "FullyFusedMLP", "n_hidden_layers": 0}),
    lambda t: t.Network(129, 1, {"otype": "FullyFusedMLP"}),
    lambda t: t.Network(8, 17, {"otype": "FullyFusedMLP"}),
    lambda t: t.Network(8, 1, {"otype": "MegaMLP"}),
    lambda t: t.NetworkWithInputEncoding(3, 1, {"otype": "Frequency"}, {"otype": "FullyFusedMLP"}),
])
def test_what_is_not_implemented_is_refused_with_the_value(make, hip_lib_built):
    import tinycudann as tcnn
    with pytest.raises(NotImplementedError, match="not implemented"):
        make(tcnn)


def test_cpu_tensors_wrong_dtype_and_wrong_width_are_runtime_errors(hip_lib_built):
    import tinycudann as tcnn
    enc = tcnn.Encoding(2, {"otype": "Frequency"})
    net = tcnn.Network(8, 1, {"otype": "FullyFusedMLP", "n_hidden_layers": 1})
    for mod, w in ((enc, 2), (net, 8)):
        with pytest.raises(RuntimeError, match="HIP device"):
            mod(torch.zeros(4, w))
