"""CPU: batch-statistics BatchNorm on the training path - the reference the GPU tests use, the mode switch, the argument
checks and the new C entries.

The GPU tests (test_gpu_batchnorm_train.py) compute their reference by replacing ``oracle.matcher.batchnorm_eval`` with
torch's training-mode ``F.batch_norm`` on clones of the running buffers.  Here that patched oracle is pinned against torch
itself: the model's own containers (``kenc.encoder``, ``gnn.layers[l].mlp``, ``conf_mlp``) are real ``nn.Sequential`` stacks of
Conv1d, BatchNorm1d and ReLU, run in training mode once per image (per pair for ``conf_mlp``).
"""
import ctypes
import os
import re
from collections import Counter

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("e2emv_train_set_batchnorm", "e2emv_train_running_update")


class BatchStatBN:
    """Drop-in for oracle.matcher.batchnorm_eval: torch's training-mode batch_norm on clones of the running buffers
    (keyed by BatchNorm prefix), counting the calls per prefix."""

    def __init__(self, sd, momentum=0.1):
        self.momentum = momentum
        self.running = {k[:-len(".running_mean")]: [sd[k].detach().clone(), sd[k[:-len("mean")] + "var"].detach().clone()]
                        for k in sd if k.endswith(".running_mean")}
        self.calls = Counter()

    def __call__(self, x, sd, prefix):
        rm, rv = self.running[prefix]
        self.calls[prefix] += 1
        return F.batch_norm(x, rm, rv, sd[prefix + ".weight"], sd[prefix + ".bias"], training=True, momentum=self.momentum, eps=1e-5)


def _randomize(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)


def test_patched_oracle_is_torch_training_mode_batchnorm(monkeypatch):
    from e2e_multi_view_matching_amd import MultiViewMatcher
    import oracle.matcher as OM
    torch.manual_seed(0)
    D, B, N, T = 64, 2, 37, 3
    model = MultiViewMatcher({"descriptor_dim": D, "num_heads": 1, "keypoint_encoder": [16, 32], "GNN_layers": ["self", "cross"],
                              "conf_mlp": True})
    _randomize(model, 1)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    bn = BatchStatBN(sd, momentum=0.1)
    monkeypatch.setattr(OM, "batchnorm_eval", bn)
    model.train()
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for t in range(T):  # encoder and every GNN MLP: one call per image, image order
            x = torch.randn(B, 3, N, generator=g)
            assert torch.allclose(model.kenc.encoder(x), OM.mlp(x, sd, "kenc.encoder", 3), rtol=1e-5, atol=1e-5)
            for l in range(2):
                x = torch.randn(B, 2 * D, N, generator=g)
                assert torch.allclose(model.gnn.layers[l].mlp(x), OM.mlp(x, sd, f"gnn.layers.{l}.mlp", 2), rtol=1e-5, atol=1e-5)
        for _ in range(T * (T - 1) // 2):  # conf head: one call per pair
            x = torch.randn(B, 2 * D, N, generator=g)
            assert torch.allclose(model.conf_mlp(x), OM.mlp(x, sd, "conf_mlp", 2), rtol=1e-5, atol=1e-5)
    for k, m in model.named_modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            rm, rv = bn.running[k]
            assert torch.allclose(m.running_mean, rm, rtol=1e-6, atol=1e-7), k
            assert torch.allclose(m.running_var, rv, rtol=1e-6, atol=1e-7), k
            assert int(m.num_batches_tracked) == bn.calls[k] == T, k
            assert not torch.equal(rm, sd[k + ".running_mean"]), k  # (the buffers did move)


def test_mode_resolution(monkeypatch):
    from e2e_multi_view_matching_amd import MultiViewMatcher, _lib
    model = MultiViewMatcher({"GNN_layers": ["self"]})
    monkeypatch.delenv("E2EMV_TRAIN_BATCHNORM", raising=False)
    assert model._batchnorm_mode() == _lib.BN_FROZEN  # the default: unchanged behaviour (with the warning)
    monkeypatch.setenv("E2EMV_TRAIN_BATCHNORM", "batch")
    assert model._batchnorm_mode() == _lib.BN_BATCH
    monkeypatch.setenv("E2EMV_TRAIN_BATCHNORM", "frozen")
    assert model._batchnorm_mode() == _lib.BN_FROZEN
    monkeypatch.setenv("E2EMV_TRAIN_BATCHNORM", "batch")
    model.config["frozen_batchnorm"] = True  # the key wins over the variable
    assert model._batchnorm_mode() == _lib.BN_FROZEN
    model.config["frozen_batchnorm"] = False
    monkeypatch.setenv("E2EMV_TRAIN_BATCHNORM", "frozen")
    assert model._batchnorm_mode() == _lib.BN_BATCH
    model.config["frozen_batchnorm"] = None
    monkeypatch.setenv("E2EMV_TRAIN_BATCHNORM", "sometimes")
    with pytest.raises(ValueError, match="E2EMV_TRAIN_BATCHNORM"):
        model._batchnorm_mode()


def test_unsupported_batchnorm_settings_are_named():
    from e2e_multi_view_matching_amd import MultiViewMatcher
    cfg = {"GNN_layers": ["self", "cross"], "conf_mlp": True}
    bns, m = MultiViewMatcher(cfg)._batch_norms()
    assert m == 0.1 and [k for k, _ in bns] == ["kenc.encoder.1", "kenc.encoder.4", "kenc.encoder.7", "kenc.encoder.10",
                                                "gnn.layers.0.mlp.1", "gnn.layers.1.mlp.1", "conf_mlp.1"]
    model = MultiViewMatcher(cfg)
    for mod in model.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.momentum = 0.3
    assert model._batch_norms()[1] == pytest.approx(0.3)
    for edit, msg in ((lambda mm: setattr(mm.gnn.layers[1].mlp[1], "momentum", None), "momentum"),
                      (lambda mm: setattr(mm.kenc.encoder[4], "momentum", 0.2), "same momentum"),
                      (lambda mm: setattr(mm.conf_mlp[1], "eps", 1e-3), "eps"),
                      (lambda mm: setattr(mm.kenc.encoder[1], "track_running_stats", False), "track_running_stats")):
        model = MultiViewMatcher(cfg)
        edit(model)
        with pytest.raises(ValueError, match=msg):
            model._batch_norms()


def test_header_declares_and_library_exports_the_batchnorm_entries(lib_built):
    from e2e_multi_view_matching_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "e2emv.h")).read()
    declared = set(re.findall(r"\b(e2emv_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(lib_built)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define E2EMV_BN_FROZEN 0\b", hdr) and re.search(r"#define E2EMV_BN_BATCH 1\b", hdr)
    assert (_lib.BN_FROZEN, _lib.BN_BATCH) == (0, 1)
