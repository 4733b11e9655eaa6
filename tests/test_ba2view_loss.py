"""The robust losses of the two-view bundle adjustment, as far as they can be checked without a GPU.

tests/ba2view_loss_restatement.py is the fp64 oracle of ``e2emv_ba_2view_loss``.  Here: without a loss it IS the pinned oracle
(oracle/ba2view.py), trajectory included; its corrected system has the gradient of ``1/2 sum rho``; the premises every device case
of tests/test_gpu_ba2view_loss.py rests on hold (both sign runs decide alike, no decision on a tie, rejected steps followed by
accepted ones occur, both Huber branches occur); the Cauchy loss pays on a scene with planted wrong matches; and the Python
keywords and the C entry are declared, bound, exported and refuse what they must on the host, before any device call.

The cases are the smallest sizes at which ``ba2view_kernel`` changes path (one wave, two waves, a second stride trip, the largest
row stride of the back-end), with the masks of tests/test_gpu_ba_steps.py, the scene with 10 % wrong matches where the losses act
for all ten iterations, and the confidence clamp.  Every case runs at ``loss_scale`` = one pixel at f = 600 except the clamp case,
whose confidences are ~3e-9: its scale is 3e-11, so that ``confidence x residual`` straddles it there as well."""
import ctypes
import functools
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ba2view_loss_restatement as rs
from test_gpu_ba_steps import DELTA_CAP, N_MAX, TIE_GAP, _mask_rows, _scale_conf, _scattered, make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL = 1.0 / 600.0
LOSSES = ["huber", "cauchy"]

# name -> (scene builder, relative loss scale).  Seeds and starts are chosen so that the premise test holds (see there).
CASES = {
    "a_n7": (lambda: make_scene(7, 101), PIXEL),                                                         # smallest valid problem
    "b_n8_hole0": (lambda: _mask_rows(make_scene(8, 102), np.arange(1, 8), 0), PIXEL),                    # masked row 0
    "c_n65": (lambda: make_scene(65, 103), PIXEL),                                                       # one row in the second wave
    # 100 valid rows of 257, row 256 (alone in the second stride trip) among them; the others NaN / inf behind 0, -0.0, -1, NaN
    "f_n257_garbage": (lambda: _mask_rows(make_scene(257, 106), np.union1d(_scattered(257, 100, 6), [256]), 60, garbage=True), PIXEL),
    # 10 % wrong matches and a far start: the losses act in every evaluation, steps get rejected and accepted again
    "j_n257_outliers": (lambda: make_scene(257, 120, rot_pert=0.45, t_pert=0.3, noise=3e-4, outliers=0.10), PIXEL),
    "h_n2048": (lambda: _mask_rows(make_scene(2048, 108), _scattered(2048, 520, 8), 0), PIXEL),           # largest row stride
    "k_n65_clamp": (lambda: _scale_conf(make_scene(65, 103), 2e-7), 3e-11),                              # cden is the 1e-6 clamp
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return CASES[name][0]()


def scale_of(name):
    return CASES[name][1]


def _restated(s, sign, loss, scale, n=N_MAX):
    T, valid, traj, summary = rs.run_bundle_adjust_2_view(s["k0"].double(), s["k1"].double(), s["conf"].double(), s["T_init"].double(), n,
                                                          homogeneous_sign=sign, loss=loss, loss_scale=scale if loss else None)
    assert bool(valid.all())
    return dict(traj[0], summary=summary[0])


@functools.lru_cache(maxsize=None)
def trajectories(name, loss):
    """(T+ trajectory, T- trajectory) of a case under a loss: two 10-iteration runs of the restatement, shared by every test,
    never modified.  Each carries its ``summary``."""
    s = scene(name)
    return _restated(s, +1, loss, scale_of(name)), _restated(s, -1, loss, scale_of(name))


def delta(tp, tm, n):
    return float((tp["best"][n] - tm["best"][n]).abs().max())


def pattern(tr):
    return "".join("A" if a else "r" for a in tr["accepted"][1:].tolist())


# ------------------------------------------------------------------------------------------------ the restatement


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_without_a_loss_is_the_pinned_oracle_exactly(name):
    from oracle import ba2view as OB
    s = scene(name)
    a = [s[k].double() for k in ("k0", "k1", "conf", "T_init")]
    for sign in (+1, None):
        T, valid, traj = OB.run_bundle_adjust_2_view(*a, N_MAX, homogeneous_sign=sign, return_trajectory=True)
        T2, valid2, traj2, summary = rs.run_bundle_adjust_2_view(*a, N_MAX, homogeneous_sign=sign)
        assert torch.equal(T, T2) and torch.equal(valid, valid2) and len(traj) == len(traj2) == 1
        want, got = traj[0], traj2[0]
        assert torch.equal(want["best"], got["best"]) and torch.equal(want["rn"], got["cost"]) and torch.equal(want["accepted"], got["accepted"])
        assert bool(got["best_cost"][0].isnan()) and torch.equal(want["best_r"][1:], got["best_cost"][1:])
        assert float(summary[0, 0]) == float(want["rn"][0]) and float(summary[0, 1]) == float(want["rn"][want["accepted"]].min())
        assert float(summary[0, 2]) == float(want["accepted"][1:].sum()) and float(summary[0, 3]) == 0.0


def test_restatement_returns_nothing_for_an_invalid_sample():
    s = make_scene(8, 301)
    s["conf"][0, 6:] = 0.0
    T, valid, traj, summary = rs.run_bundle_adjust_2_view(s["k0"].double(), s["k1"].double(), s["conf"].double(), s["T_init"].double(), 3,
                                                          loss="cauchy", loss_scale=PIXEL)
    assert valid.tolist() == [False] and T.shape == (0, 4, 4) and traj == [] and summary.shape == (0, 4)


def test_rho_follows_the_operation_order_of_the_kernel():
    a = 0.02
    a2 = a * a
    s = torch.tensor([0.0, 1e-300, a2 * (1 - 1e-15), a2, a2 * (1 + 1e-15), 1.0, float("nan")], dtype=torch.float64)
    rho, sq = rs.rho_sq("huber", a, s)
    assert bool((sq[s <= a2] == 1.0).all()) and torch.equal(rho[s <= a2], s[s <= a2]) and int((s <= a2).sum()) == 4
    assert float(sq[5]) == np.sqrt(a / 1.0) and float(rho[5]) == 2.0 * a * 1.0 - a2
    assert bool(rho[6].isnan()) and bool(sq[6].isnan())
    rho, sq = rs.rho_sq("cauchy", a, s)
    assert float(rho[0]) == 0.0 and float(sq[0]) == 1.0
    assert float(rho[5]) == a2 * np.log1p(1.0 / a2) and float(sq[5]) == np.sqrt(1.0 / (1.0 + 1.0 / a2))
    assert bool(rho[6].isnan()) and bool(sq[6].isnan())


def _exp_left(extr1, d6):
    """exp of ONE se(3) coordinate applied on the left, exactly (Rodrigues): what the Jacobian ``[I | -hat(Ap)]`` linearises."""
    v, w = d6[:3], d6[3:]
    th = float(w.norm())
    R = torch.eye(3, dtype=torch.float64)
    if th > 0.0:
        k = w / th
        Kx = torch.tensor([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]], dtype=torch.float64)
        R = R + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)
    D = torch.eye(4, dtype=torch.float64)
    D[:3, :3], D[:3, 3] = R, v
    return D @ extr1


@pytest.mark.parametrize("loss", LOSSES)
def test_corrected_gradient_is_the_central_difference_of_the_robust_cost(loss):
    """The 7-match scene at its start, all 6 + 3 * 7 unknowns one at a time: ``J^T r`` of the corrected system against
    ``D(h) = (F(x + h e) - F(x - h e)) / 2h`` of ``F = 1/2 sum rho``, h = 1e-6.  The scale lies midway between the two middle block norms, so
    that seven blocks take each Huber branch and none sits at the branch point (where F'' jumps).  The bar is derived, not tuned:
    * truncation: ``D(h) - F' = h^2 F''' / 6 + ...``, so ``(D(2h) - D(h)) / 3`` estimates it; allowed is 3 x that, ``|D(2h) - D(h)|``
      (an observation within h of Huber's branch point adds O(h) x its share, which the same estimate sees);
    * rounding: every coordinate entering a weighted residual component is at most 1 in magnitude here (asserted) and goes through
      fewer than 16 fp64 roundings (rigid motion, division, subtraction), so the component is off by at most 16 eps c_i; with
      ``|dF / dr_k| = rho' |r_k| <= |r_k|`` F is off by at most ``E = 16 eps sum_k c_k |r_k|``, and D(h), a difference of two such
      values over 2h, by ``E / h``."""
    from oracle import kornia_fns as K
    s = scene("a_n7")
    x0, x1, conf = s["k0"][0].double(), s["k1"][0].double(), s["conf"][0].double()
    c = conf / (0.5 * (2 * conf.sum()).clamp(min=1e-6))
    extr1 = s["T_init"][0].double()
    pts = K.triangulate_points(torch.eye(4, dtype=torch.float64)[None, :3], extr1[None, :3], x0[None], x1[None])[0]
    M = 7
    _, r_plain, _, s_blocks = rs.corrected_system(extr1, pts, x0, x1, c)
    norms = s_blocks.sqrt().sort().values
    a = 0.5 * float(norms[M - 1] + norms[M])
    assert int((s_blocks <= a * a).sum()) == M and float(norms[M] / norms[M - 1]) > 1.01  # seven blocks on each branch, none at the branch point
    assert float(x0.abs().max()) <= 1.0 and float(x1.abs().max()) <= 1.0 and float(pts[:, :2].abs().max() / pts[:, 2].min()) <= 1.0
    J, r, _, _ = rs.corrected_system(extr1, pts, x0, x1, c, loss, a)
    g = J.T @ r

    def F(dx):
        return 0.5 * float(rs.corrected_system(_exp_left(extr1, dx[:6]), pts + dx[6:].view(-1, 3), x0, x1, c, loss, a)[2])

    def D(k, h):
        e = torch.zeros(6 + 3 * M, dtype=torch.float64)
        e[k] = h
        return (F(e) - F(-e)) / (2.0 * h)

    h = 1e-6
    eps = 2.0 ** -52
    rounding = 16.0 * eps * float((r_plain.abs() * c.repeat_interleave(2).repeat(2)).sum()) / h
    worst = 0.0
    for k in range(6 + 3 * M):
        d1, d2 = D(k, h), D(k, 2.0 * h)
        tol = abs(d2 - d1) + rounding
        worst = max(worst, abs(float(g[k]) - d1) / tol)
        assert abs(float(g[k]) - d1) <= tol, (loss, k, float(g[k]), d1, tol)
    print(loss, "largest |J^T r - D(h)| / bar", worst, "largest gradient entry", float(g.abs().max()), "rounding term", rounding)


# ------------------------------------------------------------------------------------------------ premises of the device tests


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", list(CASES))
def test_premise_both_signs_decide_alike_and_never_on_a_tie(name, loss):
    s = scene(name)
    tp, tm = trajectories(name, loss)
    print(f"{name} {loss}: pattern {pattern(tp)}  delta(1,3,10) = {delta(tp, tm, 1):.2e} {delta(tp, tm, 3):.2e} {delta(tp, tm, 10):.2e}  "
          f"huber branches {tp['inliers'].tolist()} / {tp['outliers'].tolist()}")
    assert pattern(tp) == pattern(tm), (name, loss, pattern(tp), pattern(tm))
    for tr in (tp, tm):
        gap = (tr["cost"][1:] - tr["best_cost"][1:]).abs() / tr["best_cost"][1:].abs()
        assert bool(tr["cost"].isfinite().all()) and float(gap.min()) >= TIE_GAP, (name, loss, gap.tolist())
        assert bool(tr["best"].isfinite().all())
    # the bracket is as tight as on the loss-free scenes of tests/test_gpu_ba_steps.py: the bar of the device tests stays a bar
    for n in range(1, N_MAX + 1):
        assert delta(tp, tm, n) <= DELTA_CAP, (name, loss, n, delta(tp, tm, n))
    assert delta(tp, tm, 0) == 0.0 and torch.equal(tp["best"][0], s["T_init"][0].double())
    # the scale reaches the device as one division by the kernel's own denominator; the confidences are fp32 within a few
    # binades, so their fp64 sum is exact in ANY order (fewer than 2^11 terms, all multiples of one 2^-k more than 40 bits below
    # 2^53 x the smallest) and a_b is ONE number
    conf = s["conf"][0][s["conf"][0] > 0].double()
    cden = 0.5 * max(2.0 * float(conf.sum()), 1e-6)
    assert float(conf.sum()) == float(conf.flip(0).sum()) == float(conf[torch.randperm(len(conf), generator=torch.Generator().manual_seed(1))].sum())
    assert float(tp["summary"][3]) == float(tm["summary"][3]) == scale_of(name) / cden
    if loss == "huber":  # both branches among the observations of the run
        assert int(tp["inliers"].sum()) > 0 and int(tp["outliers"].sum()) > 0, (name, tp["inliers"].tolist(), tp["outliers"].tolist())
    if name.startswith("k_"):
        assert cden == 5e-7 and float(tp["summary"][3]) == scale_of(name) / 5e-7
    if name.startswith("j_"):  # the losses act throughout, and steps are rejected and accepted again
        assert "rA" in pattern(tp) and int(tp["outliers"].min()) > 0, (name, loss, pattern(tp))
    if name.startswith("f_"):
        off = torch.ones(257, dtype=torch.bool)
        off[s["keep"]] = False
        cf, k = s["conf"][0, off], torch.cat([s["k0"][0, off], s["k1"][0, off]], 1)
        assert int((s["conf"] > 0).sum()) == len(s["keep"]) == 100 and float(s["conf"][0, 256]) > 0
        assert bool(cf.isnan().any()) and bool((cf == -1).any()) and bool(torch.signbit(cf[cf == 0]).any())
        assert bool(k.isnan().any()) and bool((k == float("inf")).any()) and bool((k == float("-inf")).any())
    if name.startswith("h_"):
        assert int((s["conf"] > 0).sum()) == 520
    if name.startswith("b_"):
        assert int((s["conf"] > 0).sum()) == 7 and float(s["conf"][0, 0]) == 0.0


def test_premise_a_rejected_step_is_followed_by_an_accepted_one_somewhere():
    hit = [(n, loss) for n in CASES for loss in LOSSES if "rA" in pattern(trajectories(n, loss)[0])]
    assert ("j_n257_outliers", "huber") in hit and ("j_n257_outliers", "cauchy") in hit, hit


def test_premise_trajectory_is_a_prefix():
    """best[n] of one 10-iteration run IS the result of n_iterations = n, summary included."""
    tp, _ = trajectories("c_n65", "cauchy")
    for n in (0, 2, 5):
        tr = _restated(scene("c_n65"), +1, "cauchy", PIXEL, n)
        assert torch.equal(tr["best"], tp["best"][:n + 1]) and torch.equal(tr["cost"], tp["cost"][:n + 1])
        assert float(tr["summary"][1]) == float(tp["best_cost_after"][n]) and float(tr["summary"][2]) == float(tp["accepted"][1:n + 1].sum())


# ------------------------------------------------------------------------------------------------ benefit


def _rotation_error_deg(T, T_true):
    R = T[:3, :3].double() @ T_true[:3, :3].double().T
    return float(torch.rad2deg(torch.arccos(((torch.trace(R) - 1.0) / 2.0).clamp(-1.0, 1.0))))


def test_cauchy_halves_the_rotation_error_under_planted_wrong_matches():
    """257 matches, 10 % of them wrong (``make_scene(257, 118, ..., outliers=0.10)``, the outlier scene of
    tests/test_gpu_ba_steps.py, started 1.7 degrees off), 10 iterations, on the restatement alone: the squared loss is pulled to 7.0
    degrees, Cauchy at one pixel (f = 600) ends at 0.03 degrees.  The first seed tried; seeds 119, 120, 121 give ratios of 0.03,
    0.008 and 0 the same way.  Asserted is the ratio the issue asks for: at most one half."""
    s = make_scene(257, 118, rot_pert=0.03, t_pert=0.05, noise=3e-4, outliers=0.10)
    err = {}
    for loss in (None, "cauchy"):
        T = _restated(s, +1, loss, PIXEL)["best"][N_MAX]
        err[loss] = _rotation_error_deg(T, s["T_true"])
    print("rotation error (degrees): start", _rotation_error_deg(s["T_init"][0], s["T_true"]), err)
    assert err["cauchy"] <= 0.5 * err[None], err


# ------------------------------------------------------------------------------------------------ C ABI and Python keywords

NAME, BASE = "e2emv_ba_2view_loss", "e2emv_ba_2view"


def test_header_declares_and_library_exports_the_entry(lib_built):
    from e2e_multi_view_matching_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "e2emv.h")).read()
    assert NAME in set(re.findall(r"\b(e2emv_[a-z0-9_]+)\s*\(", hdr))
    assert NAME in _lib.SIGNATURES and hasattr(ctypes.CDLL(lib_built), NAME) and hasattr(ctypes.CDLL(lib_built), BASE)
    norm = lambda t: [" ".join(x.split()) for x in t.split(",")]  # noqa: E731
    decl = norm(re.search(r"int %s\((.*?)\);" % NAME, hdr, re.S).group(1))
    old = norm(re.search(r"int %s\((.*?)\);" % BASE, hdr, re.S).group(1))
    # the counterpart's arguments, then the loss and the summary, then the stream
    assert decl == old[:-1] + ["int loss", "double loss_scale", "double* d_summary", "void* stream"]
    sig, sig_old = _lib.SIGNATURES[NAME], _lib.SIGNATURES[BASE]
    assert sig[0] is ctypes.c_int and len(sig[1]) == len(decl)
    assert sig[1] == sig_old[1][:-1] + [ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]


def test_null_context_is_rejected(lib_built):
    from e2e_multi_view_matching_amd import _lib
    lib = _lib.load_library()
    assert lib.e2emv_ba_2view_loss(None, 1, 8, None, None, None, None, 1, None, None, 2, 1.0, None, None) == _lib.EINVAL


def test_keywords_default_to_no_loss_and_share_one_check():
    from e2e_multi_view_matching_amd import multi_view, pose
    assert multi_view._check_loss is pose._check_loss and multi_view.LOSSES is pose.LOSSES
    for fn in (pose.run_bundle_adjust_2_view, multi_view.relative_poses_w8pt_ba, multi_view.relative_poses_ransac, multi_view._w8pt_ba_on_device,
               multi_view._ransac_on_device):
        p = inspect.signature(fn).parameters
        assert p["loss"].default is None and p["loss_scale"].default is None, fn
    assert inspect.signature(pose.run_bundle_adjust_2_view).parameters["return_summary"].default is False
    for fn in (multi_view.solve_tuple_poses_batch, multi_view.eval_bundle_adjust_batch):
        p = inspect.signature(fn).parameters
        assert p["pair_loss"].default is None and p["pair_loss_scale"].default is None, fn


def test_dropin_reexports_the_function_with_its_keywords():
    import e2e_multi_view_matching_amd as E
    spec = importlib.util.spec_from_file_location("dropin_estimate_relative_pose", os.path.join(
        ROOT, "dropin", "pose_optimization", "two_view", "estimate_relative_pose.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run_bundle_adjust_2_view is E.run_bundle_adjust_2_view is E.pose.run_bundle_adjust_2_view
    assert {"loss", "loss_scale", "return_summary"} <= set(inspect.signature(mod.run_bundle_adjust_2_view).parameters)


BAD = [("l2", 1.0, "loss must be"), ("Cauchy", 1.0, "loss must be"), (2, 1.0, "loss must be"), (["huber"], 1.0, "loss must be"),
       ("huber", None, "needs a loss_scale"), ("cauchy", None, "needs a loss_scale"), (None, 1.0, "needs a loss"),
       ("huber", 0.0, "finite positive"), ("cauchy", -1.0, "finite positive"), ("huber", float("nan"), "finite positive"),
       ("cauchy", float("inf"), "finite positive"), ("huber", "1", "finite positive"), ("cauchy", True, "finite positive")]


def _no_device(monkeypatch):
    """No device exists where this runs, and none may be asked for: every route to the library raises."""
    from e2e_multi_view_matching_amd import _lib, multi_view, pose

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "context", no_device)
    monkeypatch.setattr(multi_view, "_dev", no_device)
    monkeypatch.setattr(pose, "_dev_of", no_device)
    monkeypatch.setattr(multi_view, "estimate_poses_ransac", no_device)
    monkeypatch.setattr(multi_view, "_collect_matches_batch", no_device)


def _per_image(T=3, N=4):
    return {f"keypoints{t}": torch.zeros(1, N, 2) for t in range(T)}


@pytest.mark.parametrize("loss,scale,match", BAD)
def test_bad_loss_arguments_are_value_errors_before_any_device_call(loss, scale, match, monkeypatch):
    from e2e_multi_view_matching_amd import multi_view, pose
    _no_device(monkeypatch)
    z = torch.zeros(1, 8, 2)
    with pytest.raises(ValueError, match=match):
        pose.run_bundle_adjust_2_view(z, z, torch.ones(1, 8), torch.eye(4)[None], 3, loss=loss, loss_scale=scale)
    with pytest.raises(ValueError, match=match):
        pose.run_bundle_adjust_2_view(z, z, torch.ones(1, 8), torch.eye(4)[None], 3, loss=loss, loss_scale=scale, return_summary=True)
    problem = (np.eye(3), np.eye(3), np.zeros((8, 2), np.float32), np.zeros((8, 2), np.float32), np.ones((8, 1), np.float32))
    with pytest.raises(ValueError, match=match):
        multi_view.relative_poses_w8pt_ba([problem], loss=loss, loss_scale=scale)
    with pytest.raises(ValueError, match=match):
        multi_view.relative_poses_w8pt_ba([], loss=loss, loss_scale=scale)
    for ba in (False, True):
        with pytest.raises(ValueError, match=match):
            multi_view.relative_poses_ransac([problem], ba=ba, loss=loss, loss_scale=scale)
    with pytest.raises(ValueError, match=match):
        multi_view._w8pt_ba_on_device(None, None, None, None, None, None, None, loss=loss, loss_scale=scale)
    with pytest.raises(ValueError, match=match):
        multi_view._ransac_on_device(3, None, None, 3, 1, ba=True, loss=loss, loss_scale=scale)
    for method in ("w8pt_ba", "ransac_ba", "ransac"):
        for init in ("host", "device"):
            for tracks in (False, True):
                with pytest.raises(ValueError, match=match):
                    multi_view.solve_tuple_poses_batch(3, _per_image(), {}, init=init, rel_pose_method=method, tracks=tracks and method == "w8pt_ba",
                                                       pair_loss=loss, pair_loss_scale=scale)
        with pytest.raises(ValueError, match=match):
            multi_view.eval_bundle_adjust_batch(3, _per_image(), {}, [[], [], []], rel_pose_method=method, pair_loss=loss, pair_loss_scale=scale)


@pytest.mark.parametrize("loss", LOSSES)
def test_a_pair_loss_needs_a_two_view_stage(loss, monkeypatch):
    """"ransac" has no two-view bundle adjustment; neither has ``relative_poses_ransac`` without ``ba``."""
    from e2e_multi_view_matching_amd import multi_view
    _no_device(monkeypatch)
    for init in ("host", "device"):
        with pytest.raises(ValueError, match="no two-view bundle"):
            multi_view.solve_tuple_poses_batch(3, _per_image(), {}, init=init, rel_pose_method="ransac", pair_loss=loss, pair_loss_scale=PIXEL)
        # ... whatever the last stage's loss is
        with pytest.raises(ValueError, match="no two-view bundle"):
            multi_view.solve_tuple_poses_batch(3, _per_image(), {}, init=init, rel_pose_method="ransac", loss="huber", loss_scale=PIXEL,
                                               pair_loss=loss, pair_loss_scale=PIXEL)
    with pytest.raises(ValueError, match="no two-view bundle"):
        multi_view.eval_bundle_adjust_batch(3, _per_image(), {}, [[], [], []], rel_pose_method="ransac", pair_loss=loss, pair_loss_scale=PIXEL)
    problem = (np.eye(3), np.eye(3), np.zeros((8, 2), np.float32), np.zeros((8, 2), np.float32), np.ones((8, 1), np.float32))
    with pytest.raises(ValueError, match="no two-view bundle"):
        multi_view.relative_poses_ransac([problem], ba=False, loss=loss, loss_scale=PIXEL)
    with pytest.raises(ValueError, match="no two-view bundle"):
        multi_view._ransac_on_device(3, None, None, 3, 1, ba=False, loss=loss, loss_scale=PIXEL)


def test_a_good_pair_loss_passes_the_host_checks(monkeypatch):
    """... and only then reaches for the device: the first device-side step is what raises here."""
    from e2e_multi_view_matching_amd import multi_view
    _no_device(monkeypatch)
    for method in ("w8pt_ba", "ransac_ba"):
        with pytest.raises(AssertionError, match="a device call was made"):
            multi_view.solve_tuple_poses_batch(3, _per_image(), {}, rel_pose_method=method, pair_loss="cauchy", pair_loss_scale=PIXEL)
