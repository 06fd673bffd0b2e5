"""The appearance-embedding route without a GPU: the oracle of the fused MLP against autograd, the configuration dataclasses, the
model's state dict, the plugin's hooks (setup, load_state_dict, optimizers and schedulers), what the fused op refuses, which path the
model takes, the header, and — where the reference tree is present — the torch path against the reference's own `Model`, bit for bit."""
import dataclasses
import os
import types
import warnings

import pytest
import torch
import torch.nn.functional as Fn

import appearance_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(
    not os.path.exists(os.path.join(REF_ROOT, "internal", "renderers", "gsplat_appearance_embedding_renderer.py")), reason="reference tree not present")

# (F, E, H, L, n_out, n_freq, normalize, activation): every option combination tests/test_appearance_mlp.py runs on the GPU
COMBINATIONS = [(64, 32, 64, 3, 3, 0, False, "none"), (64, 32, 64, 3, 4, 0, False, "none"), (4, 5, 32, 2, 3, 0, False, "none"),
                (4, 5, 32, 2, 4, 0, False, "none"), (32, 8, 32, 4, 4, 0, False, "none"), (64, 32, 64, 3, 3, 0, False, "sigmoid"),
                (64, 128, 64, 3, 3, 0, False, "sigmoid"), (64, 32, 64, 3, 3, 4, False, "sigmoid"), (64, 32, 64, 3, 4, 4, True, "sigmoid"),
                (64, 32, 64, 3, 4, 0, True, "sigmoid"), (128, 32, 64, 3, 3, 0, False, "sigmoid"), (128, 16, 32, 4, 4, 4, True, "sigmoid")]


def _restatement(features, weights, biases, embedding, mask, means, camera, n_freq, normalize, activation):
    """The reference's formulation in torch.nn.functional: gather, repeat, concat, Linear / ReLU, scatter."""
    rows = features[mask]
    embeddings = embedding[None].repeat(rows.shape[0], 1)
    if normalize:
        rows, embeddings = Fn.normalize(rows, dim=-1), Fn.normalize(embeddings, dim=-1)
    parts = [rows, embeddings]
    if n_freq:
        parts.append(AO.view_encoding(Fn.normalize(means[mask] - camera, dim=-1), n_freq))
    x = torch.cat(parts, -1)
    for i, (w, b) in enumerate(zip(weights, biases)):
        x = Fn.linear(x, w, b)
        if i < len(weights) - 1:
            x = torch.relu(x)
    if activation == "sigmoid":
        x = torch.sigmoid(x)
    out = torch.zeros((features.shape[0], weights[-1].shape[0]), dtype=features.dtype)
    out[mask] = x
    return out


@pytest.mark.parametrize("combination", COMBINATIONS, ids=lambda c: "F%d_E%d_H%d_L%d_out%d_freq%d_norm%d_%s" % c)
def test_oracle_formulas_are_autograds(combination):
    F, E, H, L, n_out, n_freq, normalize, activation = combination
    g = torch.Generator().manual_seed(F + E + L)
    rand = lambda *shape: torch.randn(shape, generator=g, dtype=torch.float64)
    N, P = 41, 3 * (2 * n_freq + 1) if n_freq else 0
    features, embedding = rand(N, F).requires_grad_(True), rand(E).requires_grad_(True)
    if normalize:
        with torch.no_grad():
            features[7] = 0          # F.normalize below its eps
    widths = [F + E + P] + [H] * (L - 1)
    weights = [(rand(n_out if i == L - 1 else H, w) / w ** 0.5).requires_grad_(True) for i, w in enumerate(widths)]
    biases = [rand(w.shape[0]).requires_grad_(True) for w in weights]
    means, camera, v_out = rand(N, 3), rand(3), rand(N, n_out)
    mask = torch.rand((N,), generator=g) < 0.7
    mask[7] = True
    out, cache = AO.forward(features, weights, biases, embedding, mask, means, camera, n_freq, normalize, activation)
    grads = AO.backward(cache, v_out)
    want = _restatement(features, weights, biases, embedding, mask, means, camera, n_freq, normalize, activation)
    (want * v_out).sum().backward()
    close = lambda a, b: float((a - b).abs().max()) <= 1e-11 * (1 + float(b.abs().max()))
    assert close(out, want.detach())
    assert close(grads["v_features"], features.grad) and close(grads["v_embedding"], embedding.grad)
    assert not bool(grads["v_features"][~mask].any())
    for got, leaf in zip(grads["v_weights"] + grads["v_biases"], weights + biases):
        assert close(got, leaf.grad)


def test_exact_oracle_asserts_its_bound():
    features, weights, biases, embedding, v_out = AO.integer_case(40, 64, 32, 64, 3, 4, seed=1)
    out, grads, bound = AO.exact(features, weights, biases, embedding, v_out)
    assert out.dtype == torch.int64 and 0 < bound < AO.EXACT_LIMIT
    assert not torch.equal(weights[1], weights[1].T) and not torch.equal(weights[1], torch.eye(64))
    with pytest.raises(AssertionError, match="2\\^24"):
        AO.exact(features * 4096, weights, biases, embedding, v_out)


def test_config_defaults_are_the_references():
    from gspl_amd import appearance as A, renderers as R
    field = lambda cls: {f.name: (f.default if f.default is not dataclasses.MISSING else f.default_factory()) for f in dataclasses.fields(cls)}
    assert field(A.ModelConfig) == {"n_gaussian_feature_dims": 64, "n_appearances": -1, "n_appearance_embedding_dims": 32, "is_view_dependent": False,
                                    "n_view_direction_frequencies": 4, "n_neurons": 64, "n_layers": 3, "skip_layers": [], "with_opacity": False,
                                    "normalize": False, "tcnn": False}
    assert field(A.OptimizationConfig) == {"gamma_eps": 1e-6, "embedding_lr_init": 2e-3, "embedding_lr_final_factor": 0.1, "lr_init": 1e-3,
                                           "lr_final_factor": 0.1, "eps": 1e-15, "max_steps": 30_000, "warm_up": 4000}
    config = R.HipGSplatAppearanceEmbeddingRenderer()
    assert isinstance(config, R.HipGSplatV1Renderer) and config.separate_sh is True and config.fused_mlp is True
    assert config.model == A.ModelConfig() and config.optimization == A.OptimizationConfig()
    module = config.instantiate()
    assert isinstance(module, R.HipGSplatAppearanceEmbeddingRendererModule) and isinstance(module, R.HipGSplatV1RendererModule)
    with pytest.raises(ValueError, match="separate_sh"):
        R.HipGSplatAppearanceEmbeddingRenderer(separate_sh=False).instantiate()


def test_state_dict_keys_and_shapes():
    from gspl_amd import appearance as A
    model = A.HipAppearanceModel(A.ModelConfig(n_appearances=5))
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {
        "embedding.weight": (5, 32), "network.output_layers.0.weight": (64, 96), "network.output_layers.0.bias": (64,),
        "network.output_layers.2.weight": (64, 64), "network.output_layers.2.bias": (64,), "network.output_layers.4.weight": (3, 64),
        "network.output_layers.4.bias": (3,)}
    view = A.HipAppearanceModel(A.ModelConfig(n_appearances=2, is_view_dependent=True, with_opacity=True))
    assert view.state_dict()["network.output_layers.0.weight"].shape == (64, 64 + 32 + 27)
    assert view.state_dict()["network.output_layers.4.weight"].shape == (4, 64)
    skips = A.HipAppearanceModel(A.ModelConfig(n_appearances=2, n_layers=4, skip_layers=[2]))
    assert {k: tuple(v.shape) for k, v in skips.state_dict().items()} == {
        "embedding.weight": (2, 32), "network.skip_layers.0.0.weight": (64, 96), "network.skip_layers.0.0.bias": (64,),
        "network.skip_layers.0.2.weight": (64, 64), "network.skip_layers.0.2.bias": (64,), "network.output_layers.0.weight": (64, 160),
        "network.output_layers.0.bias": (64,), "network.output_layers.2.weight": (3, 64), "network.output_layers.2.bias": (3,)}
    assert skips(torch.randn(6, 64), torch.tensor(1)).shape == (6, 3)


def _module(**model):
    from gspl_amd import appearance as A, renderers as R
    return R.HipGSplatAppearanceEmbeddingRenderer(model=A.ModelConfig(**model)).instantiate()


def test_setup_counts_the_appearances_and_load_state_dict_resizes():
    module = _module()
    groups = {"a.jpg": (0, 0.), "b.jpg": (6, 0.5), "c.jpg": (2, 1.)}
    lightning_module = types.SimpleNamespace(trainer=types.SimpleNamespace(datamodule=types.SimpleNamespace(
        dataparser_outputs=types.SimpleNamespace(appearance_group_ids=groups))))
    module.setup("fit", lightning_module=lightning_module)
    assert module.config.model.n_appearances == 7 and module.model.embedding.weight.shape == (7, 32)
    fixed = _module(n_appearances=3)
    fixed.setup("fit", lightning_module=lightning_module)
    assert fixed.model.embedding.weight.shape == (3, 32)
    none = _module()
    none.setup("fit", lightning_module=types.SimpleNamespace(trainer=types.SimpleNamespace(datamodule=types.SimpleNamespace(
        dataparser_outputs=types.SimpleNamespace(appearance_group_ids=None)))))
    assert none.model.embedding.weight.shape == (1, 32)
    # a checkpoint with another number of appearances decides
    other = _module(n_appearances=11)
    other._setup_model()
    state = {k: v.clone() for k, v in other.state_dict().items()}
    assert "model.embedding.weight" in state
    module.load_state_dict(state)
    assert module.config.model.n_appearances == 11 and module.model.embedding.weight.shape == (11, 32)
    assert all(torch.equal(v, state[k]) for k, v in module.state_dict().items())


def test_optimizers_and_warm_up_schedules():
    from gspl_amd import appearance as A, renderers as R
    optimization = A.OptimizationConfig(max_steps=100, warm_up=10)
    module = R.HipGSplatAppearanceEmbeddingRenderer(model=A.ModelConfig(n_appearances=2, with_opacity=True), optimization=optimization).instantiate()
    module._setup_model()
    host = types.SimpleNamespace(extra_train_metrics=[])
    optimizers, schedulers = module.training_setup(host)
    assert [o.param_groups[0]["name"] for o in optimizers] == ["embedding", "embedding_network"]
    assert all(isinstance(o, torch.optim.Adam) and len(o.param_groups) == 1 and o.param_groups[0]["eps"] == 1e-15 for o in optimizers)
    assert optimizers[0].param_groups[0]["lr"] == 2e-3 and optimizers[1].param_groups[0]["lr"] == 1e-3
    assert [id(p) for p in optimizers[0].param_groups[0]["params"]] == [id(module.model.embedding.weight)]
    assert len(optimizers[1].param_groups[0]["params"]) == 6
    assert host.extra_train_metrics == [module.opacity_offset_reg]
    for scheduler in schedulers:
        assert isinstance(scheduler, torch.optim.lr_scheduler.LambdaLR)
        factor = scheduler.lr_lambdas[0]
        for step in (0, 1, 9, 10, 11, 60, 110, 500):
            assert factor(step) == optimization.lr_final_factor ** min(max(step - optimization.warm_up, 0) / optimization.max_steps, 1)
        assert all(factor(step) == 1.0 for step in range(0, 11)) and factor(11) < 1.0 and factor(60) < factor(11) and factor(500) == 0.1
    plain = _module(n_appearances=2)
    plain._setup_model()
    host = types.SimpleNamespace(extra_train_metrics=[])
    plain.training_setup(host)
    assert host.extra_train_metrics == []


def test_training_forward_passes_the_warm_up_flag(monkeypatch):
    from gspl_amd import appearance as A, renderers as R
    module = R.HipGSplatAppearanceEmbeddingRenderer(optimization=A.OptimizationConfig(warm_up=5)).instantiate()
    seen = []
    monkeypatch.setattr(type(module), "forward", lambda self, *a, **kw: seen.append(kw["warm_up"]))
    for step in (0, 4, 5, 6):
        module.training_forward(step, None, None, None, None)
    assert seen == [True, True, False, False]
    assert module.get_rgbs(None, None, None, None, "the colours") == "the colours"


def test_unbuilt_options_are_refused_by_name():
    from gspl_amd import ops
    ok = dict(n_features=64, n_embedding_dims=32, n_neurons=64, n_layers=3, n_out=3)
    ops.appearance_mlp_check(**ok)
    ops.appearance_mlp_check(**dict(ok, n_features=128, n_view_frequencies=8, n_layers=4, n_out=4, n_embedding_dims=256))
    for change, name in ((dict(skip_layers=[1]), "skip_layers"), (dict(n_neurons=128), "n_neurons"), (dict(n_neurons=16), "n_neurons"),
                         (dict(n_layers=1), "n_layers"), (dict(n_layers=5), "n_layers"), (dict(n_out=5), "n_out"),
                         (dict(n_features=66), "n_gaussian_feature_dims"), (dict(n_features=132), "n_gaussian_feature_dims"),
                         (dict(n_embedding_dims=257), "n_appearance_embedding_dims"), (dict(n_view_frequencies=9), "n_view_direction_frequencies"),
                         (dict(output_activation="relu"), "output_activation"), (dict(dtype=torch.float16), "float16"),
                         (dict(dtype=torch.float64), "float64")):
        with pytest.raises(NotImplementedError, match=name):
            ops.appearance_mlp_check(**dict(ok, **change))
    # the op itself: the same refusals, before it looks at the device; then CPU tensors
    features, embedding = torch.zeros(4, 64), torch.zeros(32)
    weights, biases = [torch.zeros(64, 96), torch.zeros(64, 64), torch.zeros(3, 64)], [torch.zeros(64), torch.zeros(64), torch.zeros(3)]
    with pytest.raises(NotImplementedError, match="float16"):
        ops.appearance_mlp(features.half(), weights, biases, embedding)
    with pytest.raises(NotImplementedError, match="n_neurons"):
        ops.appearance_mlp(features, [torch.zeros(48, 96), torch.zeros(48, 48), torch.zeros(3, 48)], [torch.zeros(48), torch.zeros(48), torch.zeros(3)], embedding)
    with pytest.raises(NotImplementedError, match="skip_layers"):
        ops.appearance_mlp(features, [weights[0], torch.zeros(64, 160), weights[2]], biases, embedding)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.appearance_mlp(features, weights, biases, embedding)
    from gspl_amd.ops import appearance as A
    assert (A.ROW_TILE, A.ROWS_PER_PASS, A.GRID_SIZE) == (32, 256, 256)
    assert A.lds_bytes(128, 64, 4, 8, True, 1) <= A.LDS_BYTES < A.lds_bytes(128, 64, 4, 8, True, 4)


def test_fallback_selection():
    from gspl_amd import appearance as A
    on_gpu = types.SimpleNamespace(is_cuda=True)
    built = A.HipAppearanceModel(A.ModelConfig(n_appearances=2))
    assert built.unbuilt_reason() is None and built.uses_fused(on_gpu) and not built.uses_fused(torch.zeros(1, 64))
    assert not A.HipAppearanceModel(A.ModelConfig(n_appearances=2), fused_mlp=False).uses_fused(on_gpu)
    for change, name in ((dict(n_layers=4, skip_layers=[2]), "skip_layers"), (dict(n_neurons=128), "n_neurons"), (dict(n_layers=5), "n_layers"),
                         (dict(n_gaussian_feature_dims=30), "n_gaussian_feature_dims")):
        model = A.HipAppearanceModel(A.ModelConfig(n_appearances=2, **change))
        assert name in model.unbuilt_reason() and not model.uses_fused(on_gpu)
        assert model(torch.randn(3, model.config.n_gaussian_feature_dims), torch.tensor(0)).shape == (3, 3)      # the torch path runs it
    # frequencies only count when the model is view dependent
    assert A.HipAppearanceModel(A.ModelConfig(n_appearances=2, n_view_direction_frequencies=12)).uses_fused(on_gpu)
    assert not A.HipAppearanceModel(A.ModelConfig(n_appearances=2, n_view_direction_frequencies=12, is_view_dependent=True)).uses_fused(on_gpu)
    # a mask on the torch path: zeros and no gradient for the rows it drops
    features = torch.randn(5, 64, requires_grad=True)
    mask = torch.tensor([True, False, True, True, False])
    out = built(features, torch.tensor(1), mask=mask)
    assert not bool(out[~mask].any()) and bool(out[mask].all())
    out.sum().backward()
    assert not bool(features.grad[~mask].any()) and bool(features.grad[mask].any())
    assert built(torch.zeros(0, 64), torch.tensor(1)).shape == (0, 3)


def test_tcnn_is_accepted_with_one_warning():
    from gspl_amd import appearance as A
    A._TCNN_WARNED = False
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        first = A.HipAppearanceModel(A.ModelConfig(n_appearances=2, tcnn=True))
        A.HipAppearanceModel(A.ModelConfig(n_appearances=2, tcnn=True))
    assert len([w for w in caught if "tcnn" in str(w.message)]) == 1
    assert first.unbuilt_reason() is None and list(first.state_dict()) == list(A.HipAppearanceModel(A.ModelConfig(n_appearances=2)).state_dict())


def test_header_declares_the_entry_points():
    from gspl_amd import _lib as L
    text = open(L.HEADER_PATH).read()
    for name in ("gspl_appearance_mlp_fwd", "gspl_appearance_mlp_bwd"):
        assert f"int {name}(" in text and name in L.exported_symbols()
    assert "size_t gspl_appearance_mlp_workspace_bytes(" in text and "gspl_appearance_mlp_workspace_bytes" in L.exported_symbols()
    section = text[text.index(" 21. The per-Gaussian appearance MLP"):]
    assert "PURELY ADDITIVE" in section and "no new struct" in section and L.ABI_VERSION == 39
    assert L._FUNCTIONS["gspl_appearance_mlp_fwd"][2] == (
        "N", "F", "E", "H", "n_layers", "n_out", "n_freq", "flags", "features", "mask", "means", "camera_center", "embedding", "weights", "biases",
        "out", "stream")
    assert L._FUNCTIONS["gspl_appearance_mlp_bwd"][2][-6:] == ("v_out", "v_features", "v_params", "workspace", "workspace_bytes", "stream")
    assert "appearance.hip" in open(os.path.join(ROOT, "gaussian-splatting-lightning_amd", "csrc", "Makefile")).read()


def test_tinycudann_stand_in_is_unchanged():
    from gspl_amd import compat
    compat.install()
    import tinycudann
    if "gspl_amd" not in (tinycudann.__doc__ or ""):
        pytest.skip("a real tinycudann package is installed")
    assert isinstance(tinycudann.Encoding, type) and not hasattr(tinycudann, "NetworkWithInputEncoding")
    with pytest.raises(ImportError):
        from tinycudann import Network  # noqa: F401


@needs_reference
@pytest.mark.parametrize("options", [dict(), dict(is_view_dependent=True), dict(normalize=True), dict(with_opacity=True)],
                         ids=["default", "view_dependent", "normalize", "with_opacity"])
def test_torch_path_is_the_references_model_bit_for_bit(options, monkeypatch):
    import typing
    import gspl_amd.renderers  # noqa: F401   (registers the stand-ins the reference's imports need)
    from gspl_amd import appearance as A
    from test_package_shims import _stubs
    _stubs()
    if not hasattr(torch, "Any"):          # the reference annotates with `torch.Any` (line 347), which newer torch no longer carries
        monkeypatch.setattr(torch, "Any", typing.Any, raising=False)
    from internal.renderers import gsplat_appearance_embedding_renderer as ref
    torch.manual_seed(11)
    theirs = ref.Model(ref.ModelConfig(n_appearances=4, **options))
    ours = A.HipAppearanceModel(A.ModelConfig(n_appearances=4, **options))
    assert {k: v.shape for k, v in theirs.state_dict().items()} == {k: v.shape for k, v in ours.state_dict().items()}
    ours.load_state_dict(theirs.state_dict())
    features = torch.randn(50, 64)
    view_dirs = Fn.normalize(torch.randn(50, 3), dim=-1)
    v_out = torch.randn(50, ours.n_output_dims)
    results = []
    for model in (theirs, ours):
        leaf = features.clone().requires_grad_(True)
        out = model(leaf, torch.tensor(2), view_dirs)
        model.zero_grad()
        out.backward(v_out)
        results.append([out.detach(), leaf.grad] + [p.grad for p in model.parameters()])
    assert len(results[0]) == len(results[1]) == 9
    assert all(torch.equal(a, b) for a, b in zip(*results))
