"""Matcher forward parity (-m gpu): MultiViewMatcher (HIP) vs oracle.matcher (torch CPU)."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("split_always")]

TOL = 1e-4  # north-star: scores within 1e-4 fp32, assignment indices bit-exact


def _randomize_bn(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)


def test_deep_random_network_18_layers(gpu):
    """Full depth (9 x (self, cross)), random weights + random BatchNorm statistics: rounding differences
    accumulate over 18 layers - both arithmetic modes must stay inside the 1e-4 bar with exact indices."""
    for precision in PRECISIONS:
        cfg = {"sinkhorn_iterations": 30, "conf_mlp": True, "match_threshold": 0.0, "mfma_precision": precision}
        out, ref, _ = _run(cfg, dict(batch=1, tuple_size=2, n_kpts=192), gpu, seed=21)
        _compare(out, ref, [(0, 1)])


def _run(cfg, data_kw, gpu, seed=0, w_id=False):
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    from oracle.matcher import matcher_forward
    torch.manual_seed(seed)
    model = MultiViewMatcher(cfg).eval()
    _randomize_bn(model, seed)
    if w_id:
        identity_like_state(model)
    data = make_tuples(seed=seed, **data_kw)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    ocfg = dict(model.config)
    ocfg["full_output"] = True
    ocfg.pop("mfma_precision", None)
    ref = matcher_forward(data, sd, ocfg)
    model = model.to(gpu)
    with torch.no_grad():
        out = model({k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()})
    return out, ref, data


def _compare(out, ref, pairs):
    for i, j in pairs:
        z, zr = out[f"scores_{i}_{j}"].cpu(), ref[f"scores_{i}_{j}"]
        assert float((z - zr).abs().max()) < TOL, (i, j, float((z - zr).abs().max()))
        for key in (f"matches{i}_{i}_{j}", f"matches{j}_{i}_{j}"):
            assert torch.equal(out[key].cpu(), ref[key]), key
        c, cr = out[f"conf_scores_{i}_{j}"].cpu(), ref[f"conf_scores_{i}_{j}"]
        assert c.shape == cr.shape and float((c - cr).abs().max()) < TOL


# "-chain": generation 5 with the GEMM chain forced on; "-r4": a launch per GEMM (the T = 5 path).  The superseded generations
# ("-r2", "-r3") left the product in round 6 (measurement build only); the round-2 kernels (f16x2 on fp32 activations) still
# serve every width other than 256 with 4 heads: test_pair_width_128_two_heads
PRECISIONS = ["f32", "bf16x3", "f16x2", "f16x2-chain", "f16x2-r4"]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("conf_mlp", [False, True])
def test_pair_random_weights(gpu, conf_mlp, precision):
    cfg = {"GNN_layers": ["self", "cross"] * 2, "sinkhorn_iterations": 20, "conf_mlp": conf_mlp, "match_threshold": 0.0,
           "mfma_precision": precision}
    out, ref, _ = _run(cfg, dict(batch=2, tuple_size=2, n_kpts=256), gpu, seed=1)
    _compare(out, ref, [(0, 1)])


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
def test_pair_width_128_two_heads(gpu, precision):
    """D = 128 with 2 heads: the split modes on fp32 activations (f16x2: gemm_h2 + attention_h2f, the plane kernels take only
    D = 256 with 4 heads; bf16x3: gemm_x3 + attention3f), the encoder's layers below fan-in 128 on the fp32 kernel."""
    cfg = {"descriptor_dim": 128, "num_heads": 2, "keypoint_encoder": [32, 64, 128], "GNN_layers": ["self", "cross"] * 2,
           "sinkhorn_iterations": 20, "conf_mlp": True, "match_threshold": 0.0, "mfma_precision": precision}
    out, ref, _ = _run(cfg, dict(batch=2, tuple_size=2, n_kpts=256, desc_dim=128), gpu, seed=6)
    _compare(out, ref, [(0, 1)])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pair_identity_weights_gives_real_matches(gpu, precision):
    cfg = {"GNN_layers": ["self", "cross"] * 2, "sinkhorn_iterations": 50, "conf_mlp": True, "mfma_precision": precision}
    out, ref, data = _run(cfg, dict(batch=2, tuple_size=2, n_kpts=256), gpu, seed=2, w_id=True)
    _compare(out, ref, [(0, 1)])
    m = out["matches0_0_1"].cpu()
    gt = data["gt_matches0_0_1"]
    assert ((m == gt) & (gt >= 0)).sum() > 0.8 * (gt >= 0).sum()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_keypoint_count(gpu, precision):
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 10, "mfma_precision": precision}
    out, ref, _ = _run(cfg, dict(batch=1, tuple_size=2, n_kpts=203), gpu, seed=3, w_id=True)
    _compare(out, ref, [(0, 1)])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_multi_frame_tuple3(gpu, precision):
    cfg = {"GNN_layers": ["self", "cross", "cross"], "sinkhorn_iterations": 10, "multi_frame_matching": True, "tuple_size": 3,
           "mfma_precision": precision}
    out, ref, _ = _run(cfg, dict(batch=2, tuple_size=3, n_kpts=128), gpu, seed=4, w_id=True)
    _compare(out, ref, [(0, 1), (0, 2), (1, 2)])


def test_pairwise_mode_on_tuple3(gpu):
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 10, "multi_frame_matching": False, "tuple_size": 3}
    out, ref, _ = _run(cfg, dict(batch=1, tuple_size=3, n_kpts=128), gpu, seed=5, w_id=True)
    _compare(out, ref, [(0, 1), (0, 2), (1, 2)])


def test_fp16_descriptors_match_fp16_rounded_oracle(gpu):
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 10}
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    from oracle.matcher import matcher_forward
    torch.manual_seed(0)
    model = identity_like_state(MultiViewMatcher(cfg).eval())
    data = make_tuples(batch=1, tuple_size=2, n_kpts=128, seed=9, desc_dtype=torch.float16)
    rounded = {k: (v.float() if torch.is_tensor(v) and v.dtype == torch.float16 else v) for k, v in data.items()}
    ref = matcher_forward(rounded, model.state_dict(), {**model.config, "full_output": True})
    model = model.to(gpu)
    out = model({k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()})
    _compare(out, ref, [(0, 1)])


def test_config_full_output_is_honoured_after_construction(gpu):
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    model = MultiViewMatcher({"GNN_layers": ["self"], "sinkhorn_iterations": 2}).to(gpu).train()
    data = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in make_tuples(batch=1, n_kpts=64).items()}
    model.config["full_output"] = False
    assert set(model(data)) == {"scores_0_1"}
    model.config["full_output"] = True  # helpers.py:245
    assert "matches0_0_1" in model(data) and model(data)["conf_scores_0_1"].shape == (1, 64, 1)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_images_with_different_keypoint_counts(gpu, precision):
    """eval_pairs.py (batch 1) feeds images whose SuperPoint keypoint counts differ: N0 != N1 (and a ragged 3-tuple)."""
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    from oracle.matcher import matcher_forward
    for T, counts, layers in ((2, (203, 150), ["self", "cross"] * 2), (3, (140, 96, 260), ["self", "cross"])):
        torch.manual_seed(5)
        cfg = {"GNN_layers": layers, "sinkhorn_iterations": 15, "conf_mlp": True, "multi_frame_matching": T > 2,
               "tuple_size": T, "mfma_precision": precision}
        model = identity_like_state(MultiViewMatcher(cfg).eval())
        data = make_tuples(batch=2, tuple_size=T, n_kpts=max(counts), seed=17)
        for m, n in enumerate(counts):  # truncate image m to its own keypoint count
            data[f"keypoints{m}"] = data[f"keypoints{m}"][:, :n].contiguous()
            data[f"scores{m}"] = data[f"scores{m}"][:, :n].contiguous()
            data[f"descriptors{m}"] = data[f"descriptors{m}"][:, :, :n].contiguous()
        ocfg = {k: v for k, v in model.config.items() if k != "mfma_precision"}
        ocfg["full_output"] = True
        ref = matcher_forward(data, {k: v.clone() for k, v in model.state_dict().items()}, ocfg)
        model = model.to(gpu)
        out = model({k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()})
        pairs = [(i, j) for j in range(T) for i in range(j)]
        for i, j in pairs:
            assert out[f"scores_{i}_{j}"].shape == (2, counts[i] + 1, counts[j] + 1)
            assert out[f"matches{i}_{i}_{j}"].shape == (2, counts[i]) and out[f"matches{j}_{i}_{j}"].shape == (2, counts[j])
        _compare(out, ref, pairs)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_tuple3_above_the_256_key_switch(gpu, precision):
    """A ragged 3-tuple whose cross layers walk sources of 300, 513 and 64 keypoints: above 256 keys the f16x2 forward runs
    attention_p2w (tile exponents, source-to-source walk) on operands written by the q|k|v GEMM's epilogue - not by the helper
    kernel of the stand-alone attention tests - with a source that ends exactly on a 64-key tile between two that do not."""
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    T, counts = 3, (300, 513, 64)
    torch.manual_seed(5)
    cfg = {"GNN_layers": ["self", "cross", "cross"], "sinkhorn_iterations": 15, "conf_mlp": True, "multi_frame_matching": True,
           "tuple_size": T, "mfma_precision": precision}
    model = identity_like_state(MultiViewMatcher(cfg).eval())
    data = make_tuples(batch=1, tuple_size=T, n_kpts=max(counts), seed=19)
    for m, n in enumerate(counts):  # truncate image m to its own keypoint count
        data[f"keypoints{m}"] = data[f"keypoints{m}"][:, :n].contiguous()
        data[f"scores{m}"] = data[f"scores{m}"][:, :n].contiguous()
        data[f"descriptors{m}"] = data[f"descriptors{m}"][:, :, :n].contiguous()
    ocfg = {k: v for k, v in model.config.items() if k != "mfma_precision"}
    ocfg["full_output"] = True
    ref = _ragged3_reference(data, {k: v.clone() for k, v in model.state_dict().items()}, ocfg)
    model = model.to(gpu)
    with torch.no_grad():
        out = model({k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()})
    pairs = [(0, 1), (0, 2), (1, 2)]
    for i, j in pairs:
        assert out[f"scores_{i}_{j}"].shape == (1, counts[i] + 1, counts[j] + 1)
    _compare(out, ref, pairs)


_RAGGED3_REF = []


def _ragged3_reference(data, sd, ocfg):
    """The oracle's forward of the case above: seconds on the CPU, the same for every precision - computed once."""
    from oracle.matcher import matcher_forward
    if not _RAGGED3_REF:
        _RAGGED3_REF.append(matcher_forward(data, sd, ocfg))
    return _RAGGED3_REF[0]


def test_maximum_size_2048_keypoints_fp16_multi_frame(gpu):
    """BASELINE configs[4] shape at the library's maximum keypoint count: T = 3 joint matching, 2048 keypoints per image,
    fp16 descriptors, (self, cross, cross) schedule, both arithmetic modes - against the oracle fed the same fp16-rounded
    descriptors; identity-like weights so the assignment is a real (non-degenerate) matching."""
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    from oracle.matcher import matcher_forward
    torch.manual_seed(3)
    cfg = {"GNN_layers": ["self", "cross", "cross"], "sinkhorn_iterations": 20, "multi_frame_matching": True, "tuple_size": 3, "conf_mlp": True}
    model = identity_like_state(MultiViewMatcher(cfg).eval())
    _randomize_bn(model, 3)
    data = make_tuples(batch=1, tuple_size=3, n_kpts=2048, seed=31, desc_dtype=torch.float16)
    rounded = {k: (v.float() if torch.is_tensor(v) and v.dtype == torch.float16 else v) for k, v in data.items()}
    ref = matcher_forward(rounded, model.state_dict(), {**model.config, "full_output": True})
    model = model.to(gpu)
    dev = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()}
    for precision in PRECISIONS:
        model.config["mfma_precision"] = precision
        with torch.no_grad():
            out = model(dev)
        _compare(out, ref, [(0, 1), (0, 2), (1, 2)])
        assert float((out["matches0_0_1"] >= 0).float().mean()) > 0.5


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_pair_at_configs1_exactly(gpu, precision):
    """BASELINE.json configs[1] as the north star states it - N = 1024 keypoints, D = 256, 18 layers, 100 Sinkhorn
    iterations, conf_mlp, tuple_size 2 - on one pair (the oracle needs seconds for it), random weights and BatchNorm
    statistics: scores within 1e-4, assignment indices bit-exact, in every arithmetic mode."""
    cfg = {"sinkhorn_iterations": 100, "conf_mlp": True, "match_threshold": 0.2, "mfma_precision": precision}
    out, ref, _ = _run(cfg, dict(batch=1, tuple_size=2, n_kpts=1024), gpu, seed=33)
    assert out["scores_0_1"].shape == (1, 1025, 1025)
    _compare(out, ref, [(0, 1)])
