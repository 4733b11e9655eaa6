"""Training path (-m gpu): parameter gradients of the match loss and of the pose loss through MultiViewMatcher's HIP backward
(csrc/train.hip behind torch.autograd) against torch.autograd over the CPU oracle (oracle.matcher with grad = True).

Bar (VERDICT r2, row g): every parameter's gradient within 1e-3 relative (||g - g_ref|| / ||g_ref||), fp32 arithmetic,
and the reference's ``has_finite_gradients`` check (/root/reference/helpers.py:284-288) holds.
The loss is the reference's match loss (helpers.py:228-241): the negative log assignment at the ground-truth partner
(or dustbin) of every keypoint of both images, weighted, summed, divided by the batch size.
"""
import pytest
import torch

pytestmark = [pytest.mark.gpu]

REL = 1e-3


def _randomize_bn(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)


def _targets(B, N, seed):
    """Random ground truth in the reference's layout: indices [B][2][N+1] (partner in the other image, N = dustbin; the
    last entry belongs to the dustbin row and carries weight 0), weights [B][2][N+1]."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.full((B, 2, N + 1), N, dtype=torch.int64)
    w = torch.zeros((B, 2, N + 1))
    for b in range(B):
        perm = torch.randperm(N, generator=g)
        matched = torch.rand(N, generator=g) < 0.6
        idx[b, 0, :N] = torch.where(matched, perm, torch.full((N,), N))
        inv = torch.full((N,), N)
        inv[perm[matched]] = torch.arange(N)[matched]
        idx[b, 1, :N] = inv
        w[b, :, :N] = torch.rand(2, N, generator=g) + 0.5
    return idx, w


def _match_loss(log_p, idx, w):
    B = log_p.shape[0]
    rows = -torch.gather(log_p, 2, idx[:, 0, :, None])[..., 0]                  # [B][N+1]: -log_p[b, i, idx0[i]]
    cols = -torch.gather(log_p.transpose(1, 2), 2, idx[:, 1, :, None])[..., 0]  # [B][N+1]: -log_p[b, idx1[j], j]
    return ((rows * w[:, 0]).sum() + (cols * w[:, 1]).sum()) / B


def _has_finite_gradients(net):
    return all(p.grad is None or bool(p.grad.isfinite().all()) for p in net.parameters())


def _grads(cfg, data_kw, gpu, seed):
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    from oracle.matcher import matcher_forward
    torch.manual_seed(seed)
    model = MultiViewMatcher(cfg)
    _randomize_bn(model, seed)
    with torch.no_grad():  # away from the initial values (bin_score = 1, zero biases behind the two MLPs)
        model.bin_score.fill_(0.7)
        for prm in [model.kenc.encoder[-1].bias] + [l.mlp[-1].bias for l in model.gnn.layers]:
            prm.normal_(0.0, 0.05)
    data = make_tuples(seed=seed, **data_kw)
    T, B, N = data_kw["tuple_size"], data_kw["batch"], data_kw["n_kpts"]
    pairs = [(i, j) for j in range(T) for i in range(j)]
    targets = {p: _targets(B, N, seed * 100 + n) for n, p in enumerate(pairs)}

    # ---- oracle: torch.autograd over the CPU restatement ----
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    leaves = {k: sd[k].requires_grad_(True) for k, _ in model.named_parameters()}
    ocfg = dict(model.config)
    ocfg.update(full_output=False, grad=True)
    for k in ("mfma_precision", "autograd", "check_finite"):
        ocfg.pop(k, None)
    ref = matcher_forward(data, sd, ocfg)
    loss_ref = sum(_match_loss(ref[f"scores_{i}_{j}"], *targets[(i, j)]) for i, j in pairs)
    loss_ref.backward()

    # ---- product: HIP forward with a tape + HIP backward ----
    model = model.to(gpu).train()
    out = model({k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()})
    loss = sum(_match_loss(out[f"scores_{i}_{j}"], targets[(i, j)][0].to(gpu), targets[(i, j)][1].to(gpu)) for i, j in pairs)
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) < 1e-3 * abs(loss_ref.item()), (loss.item(), loss_ref.item())
    return model, leaves, out, ref, pairs


def _check(model, leaves, conf_too=False, free=()):
    assert _has_finite_gradients(model)
    worst = {}
    for k, p in model.named_parameters():
        if k.startswith("conf_mlp.") and not conf_too:
            continue
        assert p.grad is not None, k
        g, gr = p.grad.cpu().double(), leaves[k].grad.double()
        assert g.shape == gr.shape, k
        if k.endswith("attn.proj.1.bias") or k in free:
            # a bias on the keys shifts every logit of a query alike: the softmax, hence the loss, does not depend on it (`free`: nor
            # on these biases, which a batch-statistics BatchNorm subtracts again - test_gpu_batchnorm_train._loss_free_biases).
            # Both gradients are rounding noise around zero - compare them with the scale of the weight's gradient instead.
            scale = float(leaves[k.replace(".bias", ".weight")].grad.double().norm())
            assert float(g.norm()) < REL * scale and float(gr.norm()) < REL * scale, k
            worst[k] = 0.0
            continue
        denom = float(gr.norm())
        assert denom > 0, k
        worst[k] = float((g - gr).norm()) / denom
    bad = {k: v for k, v in worst.items() if not v < REL}
    assert not bad, bad
    return worst


def test_pair_two_layers_parameter_gradients(gpu):
    """The VERDICT's case: 2 layers (self, cross), N = 256, T = 2."""
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 50}
    model, leaves, out, ref, pairs = _grads(cfg, dict(batch=2, tuple_size=2, n_kpts=256), gpu, seed=3)
    z, zr = out["scores_0_1"].detach().cpu(), ref["scores_0_1"].detach()
    assert float((z - zr).abs().max()) < 1e-4
    worst = _check(model, leaves)
    assert len(worst) == sum(1 for _ in model.parameters())


def test_full_depth_1024_keypoints_one_pair(gpu):
    """The shape a training step really has (train.py:406-425 at the reference's defaults): 18 layers, 1024 keypoints, 100
    Sinkhorn iterations, one pair - every parameter gradient against torch.autograd over the oracle (the oracle's backward
    costs a few seconds on the host cores)."""
    cfg = {"GNN_layers": ["self", "cross"] * 9, "sinkhorn_iterations": 100, "frozen_batchnorm": True}
    model, leaves, out, ref, pairs = _grads(cfg, dict(batch=1, tuple_size=2, n_kpts=1024), gpu, seed=11)
    z, zr = out["scores_0_1"].detach().cpu(), ref["scores_0_1"].detach()
    assert float((z - zr).abs().max()) < 1e-4
    worst = _check(model, leaves)
    assert len(worst) == sum(1 for _ in model.parameters())


def test_ragged_rows_and_four_layers(gpu):
    """N = 200 (rows padded to 256 inside the library: padded rows must not leak into any weight gradient), 4 layers."""
    cfg = {"GNN_layers": ["self", "cross"] * 2, "sinkhorn_iterations": 20}
    model, leaves, *_ = _grads(cfg, dict(batch=1, tuple_size=2, n_kpts=200), gpu, seed=4)
    _check(model, leaves)


def test_triplet_multi_frame(gpu):
    """T = 3, joint GNN: a cross layer attends to the concatenated keypoints of the two other images; three score matrices
    feed the loss."""
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20, "multi_frame_matching": True, "tuple_size": 3}
    model, leaves, *_ = _grads(cfg, dict(batch=1, tuple_size=3, n_kpts=128), gpu, seed=5)
    _check(model, leaves)


def test_optimizer_step_is_seen_by_the_next_forward(gpu):
    """Two SGD steps on a fixed batch: the loss goes down and the second forward runs on the updated weights (the library
    re-folds them), i.e. the reference's `optimizer.step()` loop (train.py:421-425) works on this module."""
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    torch.manual_seed(7)
    model = MultiViewMatcher({"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20}).to(gpu).train()
    data = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in make_tuples(batch=1, tuple_size=2, n_kpts=128, seed=7).items()}
    idx, w = _targets(1, 128, 70)
    idx, w = idx.to(gpu), w.to(gpu)
    opt = torch.optim.SGD(model.parameters(), lr=1e-4)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = _match_loss(model(data)["scores_0_1"], idx, w)
        loss.backward()
        assert _has_finite_gradients(model)
        opt.step()
        losses.append(loss.item())
    assert losses[2] < losses[1] < losses[0], losses


def test_device_side_weight_update_equals_the_host_commit(gpu):
    """After an optimiser step the parameters go device-to-device into the training arena (e2emv_train_update: folds as
    kernels); the host path (e2emv_set_weight + e2emv_train_commit) on the same values must give the SAME scores and gradients,
    the scores bit for bit - BatchNorm with non-trivial statistics, conf_mlp, and the inference forward afterwards sees the new weights."""
    from e2e_multi_view_matching_amd import MultiViewMatcher, _lib
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    torch.manual_seed(11)
    model = MultiViewMatcher({"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20, "conf_mlp": True, "frozen_batchnorm": True})
    _randomize_bn(model, 5)
    model = model.to(gpu).train()
    data = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in make_tuples(batch=2, tuple_size=2, n_kpts=128, seed=11).items()}
    idx, w = _targets(2, 128, 71)
    idx, w = idx.to(gpu), w.to(gpu)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    ctx = _lib.context(gpu)

    def run():
        opt.zero_grad()
        scores = model(data)["scores_0_1"]
        _match_loss(scores, idx, w).backward()
        return scores.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}

    run()
    opt.step()                       # new values: the next forward takes the device path (the context trains this module)
    assert ctx.train_owner is not None and ctx.train_owner[0] == model._token
    s_dev, g_dev = run()
    assert ctx.sent_owner != ctx.train_owner, "the device path must not have gone through e2emv_set_weight"
    ctx.train_owner = None           # the same values through the host commit
    s_host, g_host = run()
    assert ctx.sent_owner == ctx.train_owner
    assert torch.equal(s_dev, s_host)
    assert g_dev.keys() == g_host.keys()
    scale = max(float(g.norm()) for g in g_host.values())
    for k in g_dev:  # (weight gradients are sums of atomics: equal up to their order; the key bias has a zero gradient - noise)
        d = float((g_dev[k] - g_host[k]).norm()) / max(float(g_host[k].norm()), 1e-4 * scale)
        assert d < 1e-4, (k, d)
    with torch.no_grad():            # and the inference path re-commits from the updated tensors
        inf = model.eval()(data)["scores_0_1"]
    assert float((inf - s_host).abs().max()) < 1e-3


def test_stale_tape_raises(gpu):
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    model = MultiViewMatcher({"GNN_layers": ["self"], "sinkhorn_iterations": 5}).to(gpu).train()
    data = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in make_tuples(batch=1, tuple_size=2, n_kpts=128, seed=1).items()}
    first = model(data)["scores_0_1"].sum()
    model(data)
    with pytest.raises(RuntimeError, match="one tape per context"):
        first.backward()


def test_eval_mode_and_no_grad_stay_on_the_inference_path(gpu):
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    model = MultiViewMatcher({"GNN_layers": ["self"], "sinkhorn_iterations": 5}).to(gpu)
    data = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in make_tuples(batch=1, tuple_size=2, n_kpts=128, seed=1).items()}
    assert not model.eval()(data)["scores_0_1"].requires_grad
    with torch.no_grad():
        assert not model.train()(data)["scores_0_1"].requires_grad
    assert model.train()(data)["scores_0_1"].requires_grad
    model.config["autograd"] = False
    assert not model(data)["scores_0_1"].requires_grad


# ------------------------------------------------------------------------------------------------- pose loss, second slice
def _two_view_scene(B, N, seed, noise_px=0.5):
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[600.0, 0, 320, 0], [0, 600.0, 240, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    k0, k1, Ts = [], [], []
    for _ in range(B):
        axis = torch.randn(3, generator=g)
        axis = axis / axis.norm()
        ang = 0.1 + 0.2 * float(torch.rand(1, generator=g))
        Kx = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = torch.eye(3) + torch.sin(torch.tensor(ang)) * Kx + (1 - torch.cos(torch.tensor(ang))) * (Kx @ Kx)
        t = torch.randn(3, generator=g) * 0.5
        X = torch.stack([torch.rand(N, generator=g) * 4 - 2, torch.rand(N, generator=g) * 3 - 1.5, torch.rand(N, generator=g) * 4 + 3], 1)
        X1 = X @ R.T + t
        p0 = X / X[:, 2:] @ K[:3, :3].T
        p1 = X1 / X1[:, 2:] @ K[:3, :3].T
        k0.append(p0[:, :2] + noise_px * torch.randn(N, 2, generator=g))
        k1.append(p1[:, :2] + noise_px * torch.randn(N, 2, generator=g))
        T = torch.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        Ts.append(T)
    conf = torch.rand(B, N, 1, generator=g) * 0.8 + 0.2
    conf[:, ::7] = 0.0  # unmatched keypoints carry weight 0
    return torch.stack(k0), torch.stack(k1), K.unsqueeze(0).repeat(B, 1, 1), torch.stack(Ts), conf, g


@pytest.mark.parametrize("choose_closest", [True, False])
def test_w8pt_pose_gradient_wrt_confidence(gpu, choose_closest):
    """dLoss/dconfidence through the weighted 8-point solve (e2emv_w8pt_backward: analytic eigenvector derivative + central
    differences of the rank-2 / decomposition tail) against torch.autograd through the fp64 oracle (library SVD backward).
    Loss = a random linear + quadratic functional of the 3 x 4 pose (exercises the whole Jacobian with a pose-dependent dL/dT).
    The reference's own angle losses (compute_pose_error.py:3-22) are NOT the comparison: d arccos = -1 / sqrt(1 - cos^2) with
    1 - cos ~ 1e-6 at these pose errors resolves to a few per cent on an fp32 pose - the conditioning of that loss, on either
    side (measured: every entry of dT/dconfidence matches the oracle to 5e-8); they are checked for finite gradients below."""
    import e2e_multi_view_matching_amd as E
    from oracle import w8pt as OW
    B, N = 3, 300
    k0, k1, Kc, Tgt, conf, g = _two_view_scene(B, N, seed=11 + int(choose_closest))
    # both sides get the SAME fp32 numbers: camera coordinates made once in fp32, identity intrinsics from there on (the gradient
    # divides by the gap between the two smallest eigenvalues: an input rounded differently on the two sides shows up 1e3 x)
    k0 = (k0 - Kc[:, None, :2, 2]) / torch.stack([Kc[:, 0, 0], Kc[:, 1, 1]], -1)[:, None]
    k1 = (k1 - Kc[:, None, :2, 2]) / torch.stack([Kc[:, 0, 0], Kc[:, 1, 1]], -1)[:, None]
    Kc = torch.eye(4).unsqueeze(0).repeat(B, 1, 1)
    Wr = torch.randn(B, 3, 4, generator=g)
    c_ref = conf.double().clone().requires_grad_(True)
    T_ref, _ = OW.estimate_relative_pose_w8pt(k0.double(), k1.double(), Kc.double(), Kc.double(), c_ref, choose_closest=choose_closest,
                                              T_021=Tgt.double())
    loss_ref = (T_ref[:, :3, :] * Wr.double()).sum() + ((T_ref[:, :3, :] - 0.3) ** 2 * Wr.double().flip(1)).sum()
    loss_ref.backward()
    c = conf.to(gpu).clone().requires_grad_(True)
    T, info = E.estimate_relative_pose_w8pt(k0.to(gpu), k1.to(gpu), Kc.to(gpu), Kc.to(gpu), c, choose_closest=choose_closest,
                                            T_021=Tgt.to(gpu))
    assert T.requires_grad and float((T.detach().cpu().double() - T_ref.detach()).abs().max()) < 1e-4
    Td = T.double()
    loss = (Td[:, :3, :] * Wr.to(gpu).double()).sum() + ((Td[:, :3, :] - 0.3) ** 2 * Wr.to(gpu).double().flip(1)).sum()
    assert abs(loss.item() - loss_ref.item()) < 1e-4 * max(1.0, abs(loss_ref.item()))
    loss.backward()
    gp, gr = c.grad.cpu().double(), c_ref.grad
    assert bool(gp.isfinite().all())
    for b in range(B):  # (a correspondence of weight 0 still has a gradient: dL/dc_m carries the normalisation term)
        rel = float((gp[b] - gr[b]).norm() / gr[b].norm())
        assert rel < REL, (b, rel)
    # the reference's pose losses on the same graph: finite gradients (has_finite_gradients, helpers.py:284-288)
    c2 = conf.to(gpu).clone().requires_grad_(True)
    T2, _ = E.estimate_relative_pose_w8pt(k0.to(gpu), k1.to(gpu), Kc.to(gpu), Kc.to(gpu), c2, choose_closest=choose_closest, T_021=Tgt.to(gpu))
    (E.compute_rotation_error(T2, Tgt.to(gpu)) + E.compute_translation_error_as_angle(T2, Tgt.to(gpu))).backward()
    assert c2.grad is not None and bool(c2.grad.isfinite().all()) and float(c2.grad.abs().max()) > 0


def test_pose_error_gradients(gpu):
    """compute_rotation_error / compute_translation_error_as_angle as losses: gradients w.r.t. the predicted pose against
    autograd through the oracle's restatement of compute_pose_error.py:3-22 (moderate angles: the arccos is well conditioned)."""
    import e2e_multi_view_matching_amd as E
    from oracle import w8pt as OW
    _, _, _, Ta, _, _ = _two_view_scene(6, 8, seed=5)
    _, _, _, Tb, _, _ = _two_view_scene(6, 8, seed=6)
    Tb[2, :3, 3] = 0.0  # an entry the translation error leaves out (norm product <= 1e-6)
    for reduce in (True, False):
        a_ref = Ta.double().clone().requires_grad_(True)
        lr = OW.compute_rotation_error(a_ref, Tb.double(), reduce=reduce).sum() * 1.5 + \
            OW.compute_translation_error_as_angle(a_ref, Tb.double(), reduce=reduce).sum() * 0.7
        lr.backward()
        a = Ta.to(gpu).clone().requires_grad_(True)
        lp = E.compute_rotation_error(a, Tb.to(gpu), reduce=reduce).sum() * 1.5 + E.compute_translation_error_as_angle(a, Tb.to(gpu), reduce=reduce).sum() * 0.7
        lp.backward()
        assert abs(lp.item() - lr.item()) < 1e-5
        assert float((a.grad.cpu().double() - a_ref.grad).abs().max()) < 1e-5 * float(a_ref.grad.abs().max())


def _pose_loss_reference(B, N, data_seed=9, dtype=torch.float32):
    """The CPU half of the stage-2 step below (no GPU needed): model, inputs and the oracle's loss and gradients, the matcher in
    `dtype` (fp32: the reference the device is held to; fp64: what that reference is itself measured against), the weighted
    8-point solve in fp64."""
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    from oracle.matcher import matcher_forward
    from oracle import w8pt as OW
    torch.manual_seed(21)
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 30, "conf_mlp": True, "match_threshold": 0.2, "full_output": True}
    model = MultiViewMatcher(cfg)
    _randomize_bn(model, 21)
    identity_like_state(model)
    with torch.no_grad():
        g = torch.Generator().manual_seed(22)
        for _, prm in model.named_parameters():
            prm.add_(torch.randn(prm.shape, generator=g) * (0.01 if prm.dim() > 1 else 0.005))
    data = make_tuples(batch=B, tuple_size=2, n_kpts=N, seed=data_seed)
    idx, w = _targets(B, N, 900)
    Wr = torch.randn(B, 3, 4, generator=torch.Generator().manual_seed(23))
    # the 8-point solve sees camera coordinates made ONCE in fp32 (identical numbers on both sides) and identity intrinsics
    Kc = data["intr0"]
    eye = torch.eye(4).unsqueeze(0).repeat(B, 1, 1)
    pose_in = {"intr0": eye, "intr1": eye}
    for m in range(2):
        pose_in[f"keypoints{m}"] = (data[f"keypoints{m}"] - Kc[:, None, :2, 2]) / torch.stack([Kc[:, 0, 0], Kc[:, 1, 1]], -1)[:, None]
    Tgt = data["T_0to1"]

    def pose_term(T):
        T = T.double()
        W = Wr.to(T.device).double()
        return (T[:, :3, :] * W).sum() + ((T[:, :3, :] - 0.3) ** 2 * W.flip(1)).sum()

    cast = lambda v: v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v
    sd = {k: cast(v.clone()) for k, v in model.state_dict().items()}
    leaves = {k: sd[k].requires_grad_(True) for k, _ in model.named_parameters()}
    ocfg = dict(model.config)
    ocfg.update(full_output=True, grad=True)
    for k in ("mfma_precision", "autograd", "check_finite"):
        ocfg.pop(k, None)
    ref = matcher_forward({k: cast(v) for k, v in data.items()}, sd, ocfg)
    res64 = {"matches0_0_1": ref["matches0_0_1"], "conf_scores_0_1": ref["conf_scores_0_1"].double()}
    T_ref, _ = OW.run_weighted_8_point({k: (v.double() if torch.is_tensor(v) else v) for k, v in pose_in.items()}, res64, 0, 1,
                                       choose_closest=True, target_T_021=Tgt.double())
    loss_ref = _match_loss(ref["scores_0_1"], idx, w).double() + 5.0 * pose_term(T_ref)
    loss_ref.backward()
    return dict(model=model, data=data, idx=idx, w=w, pose_in=pose_in, Tgt=Tgt, pose_term=pose_term, leaves=leaves, ref=ref, T_ref=T_ref,
                loss_ref=loss_ref)


def _pose_loss_end_to_end(gpu, B, N, data_seed=9):
    """Stage-2 training step (helpers.run_matcher with opt.pose_loss, helpers.py:243-260): match loss on the scores + a pose loss
    on run_weighted_8_point's pose, whose confidences come from conf_mlp on the matched descriptors.  Gradients of EVERY
    parameter (conf_mlp included) against autograd through the oracle (matcher in fp32, weighted 8-point in fp64).
    Weights: identity-like (real matches, a well-posed 8-point problem) plus a perturbation so that no gradient vanishes.
    B tuples of N keypoints per image from make_tuples(seed=data_seed) (tests/test_gpu_train_blocks.py runs it at a keypoint count
    that is no multiple of 128)."""
    import e2e_multi_view_matching_amd as E
    r = _pose_loss_reference(B, N, data_seed)
    model, data, idx, w, pose_in, Tgt, pose_term = (r[k] for k in ("model", "data", "idx", "w", "pose_in", "Tgt", "pose_term"))
    leaves, ref, T_ref, loss_ref = (r[k] for k in ("leaves", "ref", "T_ref", "loss_ref"))
    model = model.to(gpu).train()
    out = model({k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()})
    assert torch.equal(out["matches0_0_1"].cpu(), ref["matches0_0_1"]) and int((ref["matches0_0_1"] >= 0).sum()) > 0.3 * B * N
    assert out["conf_scores_0_1"].requires_grad and out["scores_0_1"].requires_grad
    assert float((out["conf_scores_0_1"].detach().cpu() - ref["conf_scores_0_1"].detach()).abs().max()) < 1e-5
    T, _ = E.run_weighted_8_point({k: v.to(gpu) for k, v in pose_in.items()}, out, 0, 1, choose_closest=True, target_T_021=Tgt.to(gpu))
    assert float((T.detach().cpu().double() - T_ref.detach()).abs().max()) < 1e-4
    loss = _match_loss(out["scores_0_1"], idx.to(gpu), w.to(gpu)).double() + 5.0 * pose_term(T)
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) < 1e-3 * abs(loss_ref.item())
    worst = _check(model, leaves, conf_too=True)
    assert any(k.startswith("conf_mlp.") for k in worst)
    # the pose term reached the network: without it the conf head gets exactly zero
    assert all(float(p.grad.abs().max()) > 0 for k, p in model.named_parameters() if k.startswith("conf_mlp."))
    return out, ref


def test_pose_loss_gradients_end_to_end(gpu):
    """The stage-2 step at two pairs of 256 keypoints."""
    _pose_loss_end_to_end(gpu, B=2, N=256)


def test_stage2_step_the_way_run_matcher_drives_it(gpu):
    """The reference's loop body (helpers.py:243-260, train.py:406-425) spelled out on this package's callables: a DataParallel-
    wrapped matcher, `matcher.module.config["full_output"] = True`, match loss over the scores, pose = run_weighted_8_point(...,
    choose_closest=True, target_T_021=inv(pose1) @ pose0 ...), rotation + translation-angle losses, backward, the
    has_finite_gradients gate, two optimiser groups (conf_mlp apart, helpers.get_parameters), step - twice."""
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    torch.manual_seed(3)
    model = MultiViewMatcher({"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20, "conf_mlp": True})
    identity_like_state(model)
    matcher = torch.nn.DataParallel(model.to(gpu), device_ids=[gpu.index or 0]).train()
    conf_params = [p for k, p in matcher.named_parameters() if "conf_mlp" in k]
    other = [p for k, p in matcher.named_parameters() if "conf_mlp" not in k]
    opt = torch.optim.Adam([{"params": other, "lr": 1e-5}, {"params": conf_params, "lr": 1e-4}])
    B, N = 2, 256
    data = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in make_tuples(batch=B, tuple_size=2, n_kpts=N, seed=14).items()}
    gt = data["gt_matches0_0_1"]
    idx = torch.full((B, 2, N + 1), N, dtype=torch.int64, device=gpu)
    idx[:, 0, :N] = torch.where(gt >= 0, gt, torch.full_like(gt, N))
    for b in range(B):
        has = gt[b] >= 0
        idx[b, 1, gt[b][has]] = torch.arange(N, device=gpu)[has]
    w = torch.ones((B, 2, N + 1), device=gpu)
    w[:, :, N] = 0
    before = [p.detach().clone() for p in conf_params]
    for _ in range(2):
        opt.zero_grad()
        matcher.module.config["full_output"] = True
        result = matcher(data)
        match_loss = _match_loss(result["scores_0_1"], idx, w)
        target = data["T_0to1"]
        pred, _ = E.run_weighted_8_point(data, result, 0, 1, choose_closest=True, target_T_021=target)
        rot_loss = E.compute_rotation_error(pred, target)
        transl_loss = E.compute_translation_error_as_angle(pred, target)
        train_loss = match_loss + 100.0 * (rot_loss + transl_loss)
        assert bool(torch.isfinite(train_loss))
        train_loss.backward()
        assert _has_finite_gradients(matcher)
        assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in conf_params)
        opt.step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, conf_params))


# ------------------------------------------------------------------------------------------ every region of the tape at once
# A triplet (three score matrices, three conf heads), conf_mlp, batch-statistics BatchNorm, two layers (self, cross), B = 2 and
# N = 129: n_rows = 256 != N, the score stride 132 != N, the tape holds every region it can hold and no two of a kind with
# another kind's size - a region carved too short, or over its neighbour, is a wrong gradient.  The data seed is chosen on the CPU,
# from the oracle alone (tests/test_train_blocks.py::test_reference_of_the_all_regions_case_is_well_conditioned).
TAPE_CASE = dict(B=2, N=129, T=3, iters=3, data_seed=1)


def _all_regions_reference(data_seed, dtype=torch.float64):
    """The CPU half (no GPU needed): model, inputs and the oracle's loss and gradients, the oracle in `dtype` with torch's
    training-mode batch_norm (fp64: what the device is held to; fp32: how well the problem is conditioned in the device's own
    precision).  Loss: the match loss of the three score matrices + a fixed random linear functional of the three conf_scores."""
    import oracle.matcher as OM
    import test_gpu_batchnorm_train as BT
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    B, N, T = TAPE_CASE["B"], TAPE_CASE["N"], TAPE_CASE["T"]
    torch.manual_seed(31)
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": TAPE_CASE["iters"], "conf_mlp": True, "match_threshold": 0.2,
           "full_output": True, "multi_frame_matching": True, "tuple_size": T, "frozen_batchnorm": False}
    model = MultiViewMatcher(cfg)
    _randomize_bn(model, 31)
    identity_like_state(model)
    with torch.no_grad():  # (as test_gpu_batchnorm_train's stage-2 case: the descriptors, not the perturbation, decide the matches)
        g = torch.Generator().manual_seed(32)
        for k, prm in model.named_parameters():
            res = k.endswith("mlp.3.weight") or k == "kenc.encoder.12.weight"
            prm.add_(torch.randn(prm.shape, generator=g) * (0.001 if res else 0.01 if prm.dim() > 1 else 0.005))
    data = make_tuples(batch=B, tuple_size=T, n_kpts=N, seed=data_seed)
    pairs = [(i, j) for j in range(T) for i in range(j)]
    targets = {p: _targets(B, N, 3100 + n) for n, p in enumerate(pairs)}
    Wc = {p: torch.randn(B, N, 1, generator=torch.Generator().manual_seed(3200 + n)) for n, p in enumerate(pairs)}

    def loss_of(out):
        dev = out["scores_0_1"].device
        match = sum(_match_loss(out[f"scores_{i}_{j}"], targets[(i, j)][0].to(dev), targets[(i, j)][1].to(dev)) for i, j in pairs)
        return match.double() + 5.0 * sum((out[f"conf_scores_{i}_{j}"].double() * Wc[(i, j)].to(dev).double()).sum() for i, j in pairs)

    cast = lambda v: v.detach().to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v
    sd = {k: cast(v.clone()) for k, v in model.state_dict().items()}
    leaves = {k: sd[k].requires_grad_(True) for k, _ in model.named_parameters()}
    ocfg = dict(model.config)
    ocfg.update(full_output=True, grad=True)
    for k in ("mfma_precision", "autograd", "check_finite", "frozen_batchnorm"):
        ocfg.pop(k, None)
    eval_bn, OM.batchnorm_eval = OM.batchnorm_eval, BT.BatchStatBN(sd)
    try:
        ref = OM.matcher_forward({k: cast(v) for k, v in data.items()}, sd, ocfg)
    finally:
        OM.batchnorm_eval = eval_bn
    loss_ref = loss_of(ref)
    loss_ref.backward()
    return dict(model=model, data=data, pairs=pairs, loss_of=loss_of, leaves=leaves, ref=ref, loss_ref=loss_ref, free=BT._loss_free_biases(model))


def test_every_tape_region_at_once(gpu):
    r = _all_regions_reference(TAPE_CASE["data_seed"])
    pairs, ref = r["pairs"], r["ref"]
    model = r["model"].to(gpu).train()
    out = model({k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in r["data"].items()})
    for i, j in pairs:
        assert torch.equal(out[f"matches{i}_{i}_{j}"].cpu(), ref[f"matches{i}_{i}_{j}"]), (i, j)
        assert float((out[f"scores_{i}_{j}"].detach().cpu() - ref[f"scores_{i}_{j}"].detach()).abs().max()) < 1e-4, (i, j)
        assert out[f"conf_scores_{i}_{j}"].requires_grad
        assert float((out[f"conf_scores_{i}_{j}"].detach().cpu() - ref[f"conf_scores_{i}_{j}"].detach()).abs().max()) < 1e-5, (i, j)
    loss = r["loss_of"](out)
    loss.backward()
    assert abs(loss.item() - r["loss_ref"].item()) < 1e-3 * abs(r["loss_ref"].item()), (loss.item(), r["loss_ref"].item())
    worst = _check(model, r["leaves"], conf_too=True, free=r["free"])
    print("worst relative gradient error per parameter:", {k: f"{v:.1e}" for k, v in worst.items() if v > 1e-5})
    assert len(worst) == sum(1 for _ in model.parameters())
