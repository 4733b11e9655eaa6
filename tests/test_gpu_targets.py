"""Validation targets + match loss parity (-m gpu): HIP (csrc/gtmatch.hip) vs the oracle / the reference golden."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _assert_flips_on_a_boundary(name, d, T01, mm, mu, idx, ref):
    """Every index of `idx` that differs from `ref` belongs to a row (keypoint of image 0) or column (image 1) that sits ON a
    decision boundary of the fp64 oracle - or whose arg-min partner does: its selected error within delta of a threshold,
    its two smallest errors within delta of each other, or a relative depth within delta of 0.1.  delta = 4 x the largest
    difference between the fp32 and the fp64 oracle's reprojection errors on this scene (from the oracle alone, never from
    the device).  The rows so excused stay below 1 % of the scene: the excuse cannot swallow the test."""
    from oracle import gt_matches as OG
    args = [d["keypoints0"], d["keypoints1"], d["intr0"], d["intr1"], T01, d["depth0"], d["depth1"]]
    args64 = [a.double() for a in args]
    e32, e64 = OG.reprojection_errors(*args)[0], OG.reprojection_errors(*args64)[0]
    fin = e32.isfinite() & e64.isfinite()
    delta = 4.0 * float((e32.double() - e64)[fin].abs().max())
    m = OG.decision_margins(*args64, mm, mu)
    exc0 = (m["row_thr"] < delta) | (m["row_gap"] < delta) | (m["row_rel"] < delta)  # (NaN / inf margins compare false)
    exc1 = (m["col_thr"] < delta) | (m["col_gap"] < delta)
    row_ok = exc0 | exc1.gather(1, m["row_min"])
    col_ok = exc1 | exc0.gather(1, m["col_min"])
    share = float(row_ok.sum() + col_ok.sum()) / (2 * row_ok.numel())
    diff = idx.cpu() != ref.cpu()
    N = row_ok.shape[1]
    bad = int((diff[:, 0, :N] & ~row_ok).sum()) + int((diff[:, 1, :N] & ~col_ok).sum()) + int(diff[:, :, N].sum())
    print(f"{name}: delta {delta:.3e} px, excusable share {share:.4%}, {int(diff.sum())} differing indices, {bad} of them off every boundary")
    assert share < 0.01, (name, share)
    assert bad == 0, (name, bad, int(diff.sum()))


def test_gt_matches_vs_reference_golden(gpu):
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd.synthetic import make_depth_pairs
    z = np.load(os.path.join(G, "gt_matches_reference.npz"))
    for name in [str(n) for n in z["names"]]:
        B, N, seed, mm, mu = z[f"{name}/args"]
        B, N, seed = int(B), int(N), int(seed)
        d = _to(make_depth_pairs(B, N, seed=seed, height=240, width=320), gpu)
        idx, w = E.compute_gt_matches_of_image_pair(d["keypoints0"], d["keypoints1"], d["intr0"], d["intr1"], d["T_0to1"],
                                                    d["depth0"], d["depth1"], float(mm), float(mu))
        ri, rw = torch.from_numpy(z[f"{name}/indices"]), torch.from_numpy(z[f"{name}/weights"])
        assert idx.dtype == torch.int64
        # the reprojection runs in fp64 here and in fp32 in the reference: a target may flip only where an error sits on a threshold
        assert int((idx.cpu() != ri).sum()) <= 2, name
        _assert_flips_on_a_boundary(name, {k: v.cpu() for k, v in d.items()}, d["T_0to1"].cpu(), float(mm), float(mu), idx, ri)
        if torch.equal(idx.cpu(), ri):
            assert float((w.cpu() - rw).abs().max()) < 1e-6
        lp = torch.log_softmax(torch.randn(B, N + 1, N + 1, generator=torch.Generator().manual_seed(seed)), -1)
        loss = E.compute_match_loss(lp.to(gpu), ri.to(gpu), rw.to(gpu))
        assert abs(float(loss) - float(z[f"{name}/loss"])) < 1e-3 * abs(float(z[f"{name}/loss"]))


def test_gt_matches_larger_and_loss_vs_oracle(gpu):
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd.synthetic import make_depth_pairs
    from oracle import gt_matches as OG
    d = make_depth_pairs(4, 1024, seed=9)
    oi, ow = OG.compute_gt_matches_of_image_pair(d["keypoints0"], d["keypoints1"], d["intr0"], d["intr1"], d["T_0to1"],
                                                 d["depth0"], d["depth1"], 5.0, 15.0)
    dg = _to(d, gpu)
    idx, w = E.compute_gt_matches_of_image_pair(dg["keypoints0"], dg["keypoints1"], dg["intr0"], dg["intr1"], dg["T_0to1"],
                                                dg["depth0"], dg["depth1"], 5.0, 15.0)
    assert int((idx.cpu() != oi).sum()) <= 4 and int((oi[:, 0] >= 0).sum()) > 800
    _assert_flips_on_a_boundary("B4_N1024_s9", d, d["T_0to1"], 5.0, 15.0, idx, oi)
    lp = torch.log_softmax(torch.randn(4, 1025, 1025, generator=torch.Generator().manual_seed(0)), -1)
    lo = float(OG.compute_match_loss(lp, oi, ow))
    lh = float(E.compute_match_loss(lp.to(gpu), oi.to(gpu), ow.to(gpu)))
    assert abs(lh - lo) < 1e-4 * abs(lo)


def test_validation_step_pieces_as_the_reference_caller_uses_them(gpu):
    """What helpers.run_matcher (helpers.py:243-260, the unchanged caller) asks of the package per validation step: the
    matcher wrapped in DataParallel, the match loss per pair, the relative target pose and the choose_closest pose losses."""
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    from oracle import gt_matches as OG, w8pt as OW
    from oracle.matcher import matcher_forward
    torch.manual_seed(0)
    cfg = {"GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20, "conf_mlp": True}
    shell = identity_like_state(E.MultiViewMatcher(cfg).eval())
    sd = {k: v.clone() for k, v in shell.state_dict().items()}
    d = make_tuples(batch=2, tuple_size=2, n_kpts=128, seed=3)
    gt = d["gt_matches0_0_1"]
    idx = torch.full((2, 2, 129), -1, dtype=torch.int64)
    idx[:, 0, :128] = gt
    for b in range(2):
        v = gt[b] >= 0
        idx[b, 1, gt[b][v]] = torch.nonzero(v)[:, 0]
    w = torch.rand(2, 2, 129, generator=torch.Generator().manual_seed(1))
    # the reference's dataset stores camera-to-world poses (target = inv(pose1) @ pose0); the generator world-to-camera
    c2w0, c2w1 = torch.linalg.inv(d["pose0"]), torch.linalg.inv(d["pose1"])
    model = torch.nn.DataParallel(shell.to(gpu), device_ids=[0]) if torch.cuda.device_count() == 1 else shell.to(gpu)
    getattr(model, "module", model).config["full_output"] = True
    dg = _to(d, gpu)
    result = model(dg)
    ref = matcher_forward(d, sd, {**cfg, "full_output": True})
    lh = E.compute_match_loss(result["scores_0_1"], idx.to(gpu), w.to(gpu))
    lo = OG.compute_match_loss(ref["scores_0_1"], idx, w)
    assert abs(float(lh) - float(lo)) < 1e-3 * abs(float(lo))
    target = E.relative_pose(c2w0.to(gpu), c2w1.to(gpu))
    assert float((target.cpu() - d["T_0to1"]).abs().max()) < 1e-5
    pred, _ = E.run_weighted_8_point(dg, result, 0, 1, choose_closest=True, target_T_021=target)
    Tr, _ = OW.run_weighted_8_point(d, ref, 0, 1, choose_closest=True, target_T_021=d["T_0to1"])
    rot = E.compute_rotation_error(pred, target)
    tra = E.compute_translation_error_as_angle(pred, target)
    assert rot.dim() == 0 and tra.dim() == 0 and rot.is_cuda
    assert abs(float(rot) - float(OW.compute_rotation_error(Tr, d["T_0to1"]))) < 2e-3
    assert abs(float(tra) - float(OW.compute_translation_error_as_angle(Tr, d["T_0to1"]))) < 2e-3
    assert "matches0_0_1" in result


def test_gt_matches_for_tuple_equals_the_pair_loop(gpu):
    """The batched stand-in for helpers.compute_gt_matches' pair loop: relative poses on the device + one call per pair."""
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd.synthetic import make_depth_pairs
    d = make_depth_pairs(3, 256, seed=4, height=240, width=320)
    # camera-to-world poses as the dataset stores them
    data = {"ids": [0, 1], "pose0": torch.linalg.inv(d["pose0"]), "pose1": torch.linalg.inv(d["pose1"])}
    for k in ("keypoints0", "keypoints1", "intr0", "intr1", "depth0", "depth1"):
        data[k] = d[k]
    dg = _to(data, gpu)
    out = E.gt_matches_for_tuple(dg, 5.0, 15.0)
    assert set(out) == {(0, 1)} and "depth0" in dg
    T01 = torch.linalg.inv(data["pose1"]) @ data["pose0"]
    assert float((E.relative_pose(dg["pose0"], dg["pose1"]).cpu() - T01).abs().max()) < 1e-5
    idx, w = E.compute_gt_matches_of_image_pair(dg["keypoints0"], dg["keypoints1"], dg["intr0"], dg["intr1"], T01.to(gpu),
                                                dg["depth0"], dg["depth1"], 5.0, 15.0)
    assert int((out[(0, 1)][0] != idx).sum()) <= 2  # fp64 vs fp32 relative pose: flips only on a threshold
    _assert_flips_on_a_boundary("B3_N256_s4", d, T01, 5.0, 15.0, out[(0, 1)][0], idx)
    assert int((idx[:, 0] >= 0).sum()) > 100
