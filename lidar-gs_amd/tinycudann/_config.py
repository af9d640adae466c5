"""What the stand-in accepts of tinycudann's JSON configs, decided without a device or the native library.

parse_encoding / parse_network return the few numbers the native calls need, or raise NotImplementedError naming the offending value:
nothing outside this list is emulated with framework ops.  Config keys the stand-in does not know are ignored with ONE warning per
constructor that names each key and what is used in its place.
"""
import warnings

import lidargs_abi

CONSTANTS = lidargs_abi.library_constants("tcnn")      # the limits are those of include_tcnn/lidargs_tcnn.h
WIDTH, MAX_HIDDEN_LAYERS, MAX_OUT, MAX_FREQUENCIES = (CONSTANTS["LIDARGS_TCNN_" + k] for k in ("WIDTH", "MAX_HIDDEN_LAYERS", "MAX_OUT", "MAX_FREQUENCIES"))
DEFAULT_FREQUENCIES = 12         # tinycudann's documented default of the Frequency encoding
OUTPUT_ACTIVATIONS = {"None": 0, "Sigmoid": 1}        # out_act of the C ABI
NETWORK_OTYPES = ("FullyFusedMLP", "CutlassMLP")      # one native path for both


def _refuse(what, key, value, supported):
    raise NotImplementedError(f"tinycudann stand-in: {what} {key}={value!r} is not implemented (supported: {supported}); "
                              "there is no fallback to framework ops")


def _count(what, key, value, lo, hi):
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        _refuse(what, key, value, f"an integer in {lo}..{hi}")
    return value


def _warn_unknown(what, config, known, used):
    unknown = [k for k in config if k not in known]
    if unknown:
        warnings.warn(f"tinycudann stand-in: {what} does not know the config key(s) " + ", ".join(f"{k!r}={config[k]!r}" for k in unknown)
                      + f"; ignored, as tinycudann's documentation has no such option. In use: {used}", UserWarning, stacklevel=4)


def parse_encoding(n_input_dims, encoding_config):
    """{'n_frequencies': F, 'n_output_dims': n_input_dims * 2 F} of a Frequency encoding config."""
    if not isinstance(encoding_config, dict):
        _refuse("Encoding", "encoding_config", encoding_config, "a dict with otype 'Frequency'")
    otype = encoding_config.get("otype")
    if otype != "Frequency":
        _refuse("Encoding", "otype", otype, "'Frequency' (composite and every other encoding are not)")
    if "nested" in encoding_config:
        _refuse("Encoding", "nested", encoding_config["nested"], "a single Frequency encoding, no composite")
    n_in = _count("Encoding", "n_input_dims", n_input_dims, 1, WIDTH)
    F = _count("Encoding", "n_frequencies", encoding_config.get("n_frequencies", DEFAULT_FREQUENCIES), 1, MAX_FREQUENCIES)
    _warn_unknown("the Frequency encoding", encoding_config, ("otype", "n_frequencies"), f"n_frequencies={F}")
    return {"n_frequencies": F, "n_output_dims": n_in * 2 * F}


def parse_network(n_input_dims, n_output_dims, network_config):
    """{'n_hidden_layers': h, 'out_act': 0 | 1, 'n_params': floats} of a fused-MLP config."""
    if not isinstance(network_config, dict):
        _refuse("Network", "network_config", network_config, "a dict with otype 'FullyFusedMLP' or 'CutlassMLP'")
    otype = network_config.get("otype")
    if otype not in NETWORK_OTYPES:
        _refuse("Network", "otype", otype, " / ".join(map(repr, NETWORK_OTYPES)))
    activation = network_config.get("activation", "ReLU")
    if activation != "ReLU":
        _refuse("Network", "activation", activation, "'ReLU'")
    output_activation = network_config.get("output_activation", "None")
    if output_activation not in OUTPUT_ACTIVATIONS:
        _refuse("Network", "output_activation", output_activation, "'None' / 'Sigmoid'")
    n_neurons = network_config.get("n_neurons", WIDTH)
    if isinstance(n_neurons, bool) or n_neurons != WIDTH:
        _refuse("Network", "n_neurons", n_neurons, str(WIDTH))
    h = _count("Network", "n_hidden_layers", network_config.get("n_hidden_layers", 5), 1, MAX_HIDDEN_LAYERS)
    n_in = _count("Network", "n_input_dims", n_input_dims, 1, WIDTH)
    n_out = _count("Network", "n_output_dims", n_output_dims, 1, MAX_OUT)
    _warn_unknown("the fused MLP", network_config, ("otype", "activation", "output_activation", "n_neurons", "n_hidden_layers"),
                  f"activation='ReLU', output_activation={output_activation!r}, n_neurons={WIDTH}, n_hidden_layers={h}")
    return {"n_hidden_layers": h, "out_act": OUTPUT_ACTIVATIONS[output_activation],
            "n_params": WIDTH * n_in + (h - 1) * WIDTH * WIDTH + n_out * WIDTH}


def layer_shapes(n_input_dims, n_hidden_layers, n_output_dims):
    """The matrices of `params` in order, each row-major [out, in]."""
    return [(WIDTH, n_input_dims)] + [(WIDTH, WIDTH)] * (n_hidden_layers - 1) + [(n_output_dims, WIDTH)]
