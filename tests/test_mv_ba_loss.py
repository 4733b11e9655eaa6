"""The robust losses of the multi-view bundle adjustment, as far as they can be checked without a GPU: the fp64 restatement
(tests/mvba_loss_restatement.py) is ``oracle.mvba.solve`` without a loss and with a Huber scale no residual reaches, its corrected
system has the gradient of ``1/2 sum rho(s)``, the new C entry points are declared, bound and exported, and what the Python
keywords refuse is refused on the host before any device call."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mvba_loss_restatement as rs
from oracle import mvba
from test_gpu_mv_ba_steps import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"e2emv_mv_bundle_adjust_batch_loss": ("e2emv_mv_bundle_adjust_batch", 2), "e2emv_mv_tuple_ba_loss": ("e2emv_mv_tuple_ba", 3),
       "e2emv_mv_tuple_ba_tracks_loss": ("e2emv_mv_tuple_ba_tracks", 3)}


def _same_trajectory(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for key in x:
            if isinstance(x[key], np.ndarray):
                assert x[key].tobytes() == y[key].tobytes(), key
            elif isinstance(x[key], float) and np.isnan(x[key]):
                assert np.isnan(y[key]), key
            else:
                assert x[key] == y[key], (key, x[key], y[key])


@pytest.mark.parametrize("name", ["minimal", "fixed_mid", "far_start", "exact", "nan_obs", "strides_o513"])
def test_restatement_without_a_loss_is_the_oracle_record_for_record(name):
    p = scene(name)
    want = mvba.solve(p, max_iterations=50, return_trajectory=True)
    got = rs.solve(p, max_iterations=50, return_trajectory=True)
    assert want[0].tobytes() == got[0].tobytes() and want[1].tobytes() == got[1].tobytes()
    assert {k: v for k, v in want[2].items() if v == v} == {k: v for k, v in got[2].items() if v == v} and want[2].keys() == got[2].keys()
    _same_trajectory(want[3], got[3])


def test_restatement_without_a_loss_is_the_oracle_in_long_double_too():
    p = scene("fixed_mid")
    _same_trajectory(mvba.solve(p, max_iterations=50, return_trajectory=True, dtype=np.longdouble)[3],
                     rs.solve(p, max_iterations=50, return_trajectory=True, dtype=np.longdouble)[3])


@pytest.mark.parametrize("name", ["minimal", "fixed_mid", "far_start", "exact", "nan_obs", "strides_o513"])
def test_huber_above_every_residual_is_the_loss_free_run_bit_for_bit(name):
    """sqrt(1) = 1, rho = s, the same sums."""
    p = scene(name)
    stats = {}
    free = rs.solve(p, max_iterations=50, return_trajectory=True)[3]
    rs.solve(p, max_iterations=50, loss="huber", loss_scale=1e30, stats=stats)
    big = 2.0 * np.sqrt(stats["max_s"])  # above every residual of every iterate and candidate
    stats = {}
    _same_trajectory(free, rs.solve(p, max_iterations=50, loss="huber", loss_scale=big, return_trajectory=True, stats=stats)[3])
    assert stats["outliers"] == 0 and stats["inliers"] > 0


@pytest.mark.parametrize("loss,a", [("huber", 0.02), ("cauchy", 0.02)])
def test_corrected_gradient_is_the_central_difference_of_the_robust_cost(loss, a):
    """At three random iterates, ``J^T r`` of the corrected system against the central difference ``D(h) = (F(x + h e) - F(x -
    h e)) / 2h`` of ``F = 1/2 sum rho(s)`` in every free parameter, evaluated in long double so that rounding stays out of the
    way (h = 1e-5: rounding ~ 1e-19 F / h).  The bar is the difference's OWN truncation error: ``D(h) - F' = h^2 F''' / 6 + ...``,
    so ``(D(2h) - D(h)) / 3`` estimates it; allowed are 3 x that estimate plus 1e-12 x the largest gradient entry (where F'''
    vanishes the estimate does, and F'' of Huber jumps at s = a^2: an observation within h of the branch adds O(h) x its own
    share, which the same estimate sees)."""
    p = scene("fixed_mid")
    ld = np.longdouble
    wide = dict(p, intr=np.asarray(p["intr"], ld), obs=np.asarray(p["obs"], ld), wts=np.asarray(p["wts"], ld))
    rng = np.random.default_rng(5)
    h = ld(1e-5)
    for it in range(3):
        cams = (p["cams"] + rng.normal(0, 0.02, p["cams"].shape)).astype(ld)
        pts = (p["pts"] + rng.normal(0, 0.02, p["pts"].shape)).astype(ld)
        stats = {}
        rs.corrected(wide, cams, pts, loss, a, stats)
        assert stats["inliers"] > 0 and stats["outliers"] > 0  # both branches at this iterate
        gc, gp = rs.gradient(wide, cams, pts, loss, a)
        assert not gc[p["fixed"]].any()

        def diff(arr, idx, step):
            lo, hi = arr.copy(), arr.copy()
            lo[idx] -= step; hi[idx] += step
            f = lambda x: rs.objective(wide, x if arr is cams else cams, x if arr is pts else pts, loss, a)  # noqa: E731
            return (f(hi) - f(lo)) / (2 * step)

        worst = 0.0
        gscale = max(np.abs(gc).max(), np.abs(gp).max())
        for arr, g in ((cams, gc), (pts, gp)):
            for idx in np.ndindex(arr.shape):
                if arr is cams and idx[0] == p["fixed"]:
                    continue
                d1, d2 = diff(arr, idx, h), diff(arr, idx, 2 * h)
                tol = abs(d2 - d1) + 1e-12 * gscale
                worst = max(worst, float(abs(g[idx] - d1) / tol))
                assert abs(g[idx] - d1) <= tol, (loss, it, idx, float(g[idx]), float(d1), float(tol))
        print(loss, "iterate", it, "largest |J^T r - D(h)| / bar", worst, "largest gradient entry", float(gscale))


def test_rho_and_its_derivative_at_the_edges():
    s = np.array([0.0, 1e-300, 4e-4 * (1 - 1e-15), 4e-4, 4e-4 * (1 + 1e-15), 1.0, np.nan])
    a = 0.02
    rho, sq = rs.rho_sq("huber", a, s)
    a2 = a * a
    assert rho[0] == 0.0 and sq[0] == 1.0 and rho[1] == s[1] and sq[1] == 1.0
    assert (sq[s <= a2] == 1.0).all() and (rho[s <= a2] == s[s <= a2]).all()
    assert sq[5] == np.sqrt(a / 1.0) and rho[5] == 2 * a * 1.0 - a2
    assert np.isnan(rho[6]) and np.isnan(sq[6])
    assert abs(rho[4] - s[4]) < 1e-18 and abs(sq[4] - 1.0) < 1e-15  # continuous across the branch
    rho, sq = rs.rho_sq("cauchy", a, s)
    assert rho[0] == 0.0 and sq[0] == 1.0 and rho[5] == a2 * np.log1p(1.0 / a2) and sq[5] == np.sqrt(1 / (1 + 1.0 / a2))
    assert np.isnan(rho[6]) and np.isnan(sq[6])


# ------------------------------------------------------------------------------------------------ C ABI and Python keywords


@pytest.mark.parametrize("name", list(NEW))
def test_header_declares_and_library_exports_the_loss_entries(lib_built, name):
    from e2e_multi_view_matching_amd import _lib
    base, extra = NEW[name]
    hdr = open(os.path.join(ROOT, "include", "e2emv.h")).read()
    assert name in set(re.findall(r"\b(e2emv_[a-z0-9_]+)\s*\(", hdr))
    assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(lib_built), name)
    decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1)
    old = re.search(r"int %s\((.*?)\);" % base, hdr, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[base][1]) + extra
    # the counterpart's arguments, then the loss, then the stream
    norm = lambda t: [" ".join(x.split()) for x in t.split(",")]  # noqa: E731
    assert norm(decl)[:len(norm(old)) - 1] == norm(old)[:-1] and norm(decl)[-1] == norm(old)[-1] == "void* stream"
    assert norm(decl)[len(norm(old)) - 1:-1] == ["int loss", "double loss_scale"] + (["double* loss_a_out"] if extra == 3 else [])
    assert _lib.SIGNATURES[name][1][:len(_lib.SIGNATURES[base][1]) - 1] == _lib.SIGNATURES[base][1][:-1]
    assert _lib.SIGNATURES[name][1][len(_lib.SIGNATURES[base][1]) - 1:][:2] == [ctypes.c_int, ctypes.c_double]
    assert [int(re.search(r"#define E2EMV_LOSS_%s (\d)" % n, hdr).group(1)) for n in ("NONE", "HUBER", "CAUCHY")] == [0, 1, 2]


def test_null_context_is_rejected(lib_built):
    from e2e_multi_view_matching_amd import _lib
    lib = _lib.load_library()
    assert lib.e2emv_mv_bundle_adjust_batch_loss(None, 1, None, None, None, None, None, None, None, None, None, None, None, 1, None, 1, 1.0, None) == _lib.EINVAL
    assert lib.e2emv_mv_tuple_ba_loss(None, 1, 3, 4, None, None, None, None, None, 3, 1, None, 1, None, None, 1, 1.0, None, None) == _lib.EINVAL
    assert lib.e2emv_mv_tuple_ba_tracks_loss(None, 1, 3, 4, 4, None, None, None, None, None, None, 1, 0.0, None, 3, 1, None, 1, None, None, 1, 1.0,
                                             None, None) == _lib.EINVAL


@pytest.mark.parametrize("name", ["bundle_adjust", "bundle_adjust_batch", "solve_tuple_poses_batch", "eval_bundle_adjust_batch"])
def test_loss_defaults_to_none(name):
    from e2e_multi_view_matching_amd import multi_view
    sig = inspect.signature(getattr(multi_view, name))
    assert sig.parameters["loss"].default is None and sig.parameters["loss_scale"].default is None


def _per_image(T=3, N=4):
    return {f"keypoints{t}": torch.zeros(1, N, 2) for t in range(T)}


BAD = [("l2", 1.0, "loss must be"), ("Huber", 1.0, "loss must be"), (1, 1.0, "loss must be"), (["huber"], 1.0, "loss must be"),  # an unknown name
       ("huber", None, "needs a loss_scale"), ("cauchy", None, "needs a loss_scale"),                                          # a loss without a scale
       (None, 1.0, "needs a loss"),                                                                                              # a scale without a loss
       ("huber", 0.0, "finite positive"), ("cauchy", -1.0, "finite positive"), ("huber", float("nan"), "finite positive"),
       ("cauchy", float("inf"), "finite positive"), ("huber", "1", "finite positive"), ("huber", True, "finite positive")]


@pytest.mark.parametrize("loss,scale,match", BAD)
def test_bad_loss_arguments_are_value_errors_before_any_device_call(loss, scale, match, monkeypatch):
    """No device exists where this runs, and none may be asked for: every route to the library raises here."""
    from e2e_multi_view_matching_amd import _lib, multi_view

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "context", no_device)
    monkeypatch.setattr(multi_view, "_dev", no_device)
    p = scene("minimal")
    args = (p["n_cams"], p["fixed"], p["intr"], p["cam_idx"], p["pt_idx"], p["obs"], p["wts"], p["cams"], p["pts"])
    with pytest.raises(ValueError, match=match):
        multi_view.bundle_adjust(*args, loss=loss, loss_scale=scale)
    with pytest.raises(ValueError, match=match):
        multi_view.bundle_adjust_batch([args], loss=loss, loss_scale=scale)
    with pytest.raises(ValueError, match=match):
        multi_view.bundle_adjust_batch([], loss=loss, loss_scale=scale)
    for init in ("host", "device"):
        for tracks in (False, True):
            with pytest.raises(ValueError, match=match):
                multi_view.solve_tuple_poses_batch(3, _per_image(), {}, init=init, tracks=tracks, loss=loss, loss_scale=scale)
    with pytest.raises(ValueError, match=match):
        multi_view.eval_bundle_adjust_batch(3, _per_image(), {}, [[], [], []], loss=loss, loss_scale=scale)


def test_good_loss_arguments_pass_the_check():
    from e2e_multi_view_matching_amd import multi_view
    assert multi_view._check_loss(None, None) == 0
    assert multi_view._check_loss("huber", 1) == 1 and multi_view._check_loss("cauchy", np.float32(0.5)) == 2
    assert multi_view._check_loss("cauchy", 1.0 / 600.0) == 2
