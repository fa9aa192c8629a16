"""Import-name shim: `import tinycudann as tcnn` [REF scene/gaussian_model.py:25] resolves to the MI355X weights model.
`tcnn.NetworkWithInputEncoding(...)` [REF :373-392] returns `gaussianprediction_amd.weights_ops.WeightsModel`, the fused hash-grid
encoding + MLP kernels (gp_weights_forward / gp_weights_backward), which the caller uses through `.parameters()` and `__call__`.

Only the configuration those kernels implement is accepted: a Grid/Hash encoding of 3-D input with 16 levels x 4 features and linear
interpolation, a FullyFusedMLP of 64 neurons x 2 hidden layers, ReLU, no output activation, at most 16 outputs.  Anything else
raises ValueError naming the key.  Parity with the real tinycudann (its hashing, initialisation and half-precision MLP) is unpinned:
the package is absent, so this follows its documented contract and has never been compared against it."""

_ENCODING = {"otype": ("Grid", "HashGrid"), "type": ("Hash",), "n_levels": (16,), "n_features_per_level": (4,),
             "interpolation": ("Linear",)}
_ENCODING_FREE = ("log2_hashmap_size", "base_resolution", "per_level_scale")
_NETWORK = {"otype": ("FullyFusedMLP",), "activation": ("ReLU",), "output_activation": ("None",), "n_neurons": (64,),
            "n_hidden_layers": (2,)}


def _check(section, config, fixed, free):
    for key, value in config.items():
        if key in fixed:
            if value not in fixed[key]:
                raise ValueError(f"tinycudann shim: {section}[{key!r}] = {value!r} is not implemented (supported: {fixed[key]})")
        elif key not in free:
            raise ValueError(f"tinycudann shim: {section}[{key!r}] is not supported")
    for key in fixed:
        if key not in config and key not in ("interpolation", "type"):
            raise ValueError(f"tinycudann shim: {section}[{key!r}] is required")


def NetworkWithInputEncoding(n_input_dims, n_output_dims, encoding_config, network_config, seed=1337):
    """The reference's weights model: a `WeightsModel` (torch.nn.Module) with the same seed-driven initialisation."""
    if n_input_dims != 3:
        raise ValueError(f"tinycudann shim: n_input_dims = {n_input_dims!r} is not implemented (3)")
    if not 1 <= int(n_output_dims) <= 16:
        raise ValueError(f"tinycudann shim: n_output_dims = {n_output_dims!r} is not implemented (1..16)")
    _check("encoding_config", encoding_config, _ENCODING, _ENCODING_FREE)
    _check("network_config", network_config, _NETWORK, ())
    from gaussianprediction_amd.weights_ops import WeightsModel
    kw = {k: encoding_config[k] for k in _ENCODING_FREE if k in encoding_config}
    return WeightsModel(int(n_output_dims), n_levels=16, n_features_per_level=4, seed=seed, **kw)
