"""The robust losses of the two-view bundle adjustment on the device (csrc/ba2view.hip: ``ba2view_kernel<LOSS>`` through
``e2emv_ba_2view_loss``), against tests/ba2view_loss_restatement.py.

Method and bar are those of tests/test_gpu_ba_steps.py: the restatement runs with the sign of the triangulation's null vector
forced to + and to -, ``delta(n) = max |T+(n) - T-(n)|`` brackets that one legitimate freedom, and at every ``n_iterations`` of
``N_ITERS`` the device is within ``2^-23 max(1, |T|) + 4 delta(n)`` of the midpoint, elementwise.  The summary's costs are within
four times their own bracket plus ``N 2^-52 |cost|`` (the kernel sums N matches in another order than the restatement); the
number of improving evaluations and the scale ``a_b`` - one fp64 division by a sum that is exact in any order - are exact.  The
premises (same decisions under either sign, none on a tie, tight brackets, both Huber branches, rejected steps) are checked without
a GPU in tests/test_ba2view_loss.py, which also defines the cases."""
import numpy as np
import pytest
import torch

from test_ba2view_loss import CASES, LOSSES, PIXEL, delta, pattern, scale_of, scene, trajectories
from test_gpu_ba_steps import EPS32, N_ITERS, make_scene
from test_gpu_mv_tracks import _to, planted_scene

CODES = {None: 0, "huber": 1, "cauchy": 2}


def _device(gpu, s, n, loss=None, scale=None, summary=True):
    """-> (T [n_valid,4,4], valid [B], summary [B,4] or None) on the host."""
    import e2e_multi_view_matching_amd as E
    out = E.run_bundle_adjust_2_view(s["k0"].to(gpu), s["k1"].to(gpu), s["conf"].to(gpu), s["T_init"].to(gpu), n_iterations=n, loss=loss,
                                     loss_scale=scale, return_summary=summary)
    return out[0].cpu(), out[1].cpu(), (out[2].cpu() if summary else None)


def _raw(gpu, s, n, code, scale, want_summary):
    """``e2emv_ba_2view_loss`` itself, also with arguments the Python layer never sends.  -> (T [B,4,4], valid [B], summary)."""
    from e2e_multi_view_matching_amd import _lib
    P = _lib.ptr
    k0, k1, cf, Ti = (s[k].to(gpu).contiguous() for k in ("k0", "k1", "conf", "T_init"))
    B, N = cf.shape
    To = torch.empty((B, 4, 4), dtype=torch.float32, device=gpu)
    valid = torch.empty((B,), dtype=torch.uint8, device=gpu)
    sm = torch.full((B, 4), -1.0, dtype=torch.float64, device=gpu) if want_summary else None
    with torch.cuda.device(gpu):
        _lib.context(gpu).call("e2emv_ba_2view_loss", B, N, P(k0), P(k1), P(cf), P(Ti), int(n), P(To), P(valid), int(code), float(scale), P(sm),
                               _lib.stream_ptr(gpu))
    return To.cpu(), valid.cpu(), (sm.cpu() if want_summary else None)


def _cat(batch):
    return {k: torch.cat([s[k] for s in batch]) for k in ("k0", "k1", "conf", "T_init")}


def _padded(s, N):
    """The scene with zero-confidence rows behind its own: another match count in the same row stride."""
    n = s["conf"].shape[1]
    z = lambda t, shape: torch.cat([t, torch.zeros(shape, dtype=t.dtype)], 1)  # noqa: E731
    return dict(s, k0=z(s["k0"], (1, N - n, 2)), k1=z(s["k1"], (1, N - n, 2)), conf=z(s["conf"], (1, N - n)))


# ------------------------------------------------------------------------------------------------ bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c_n65", "f_n257_garbage", "j_n257_outliers"])
def test_loss_none_through_the_new_entry_is_the_old_entry_bit_for_bit(gpu, name):
    s = scene(name)
    for n in (0, 3, 10):
        T, valid, _ = _device(gpu, s, n, summary=False)  # e2emv_ba_2view
        for want_summary in (False, True):
            T2, valid2, sm = _raw(gpu, s, n, 0, 123.0, want_summary)  # the scale is ignored without a loss
            assert valid2.tolist() == [1] and valid.tolist() == [True] and torch.equal(T, T2), (name, n, want_summary)
        assert float(sm[0, 3]) == 0.0 and float(sm[0, 1]) <= float(sm[0, 0]) and 0 <= float(sm[0, 2]) <= n and float(sm[0, 2]) == int(sm[0, 2])
        T3, valid3, sm3 = _device(gpu, s, n)  # the Python route to the same call
        assert torch.equal(T, T3) and torch.equal(sm, sm3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c_n65", "f_n257_garbage", "j_n257_outliers"])
def test_huber_above_every_residual_is_the_loss_free_run_bit_for_bit(gpu, name):
    """Every observation takes the ``sqrt(rho') = 1`` branch: a product with 1.0 is exact, the poses are the same bits."""
    s = scene(name)
    for n in (1, 3, 10):
        T, valid, _ = _device(gpu, s, n, summary=False)
        T2, valid2, sm = _device(gpu, s, n, "huber", 1e12)
        assert torch.equal(valid, valid2) and torch.equal(T, T2), (name, n, float((T - T2).abs().max()))
        assert float(sm[0, 3]) > 1e9


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
def test_a_pair_of_a_batch_is_the_pair_alone_bit_for_bit(gpu, loss):
    """B = 3 at N = 257: [257 matches with wrong ones, six positive confidences (invalid), 65 matches + padding].  Pose, validity
    and summary of every pair are the bits of the pair run alone; the invalid pair returns its start and a zero summary; the
    scale ``a_b`` is the pair's own, whatever its position."""
    six = make_scene(257, 302)
    six["conf"][0, np.setdiff1d(np.arange(257), [0, 17, 63, 64, 255, 256])] = 0.0
    assert int((six["conf"] > 0).sum()) == 6
    batch = [scene("j_n257_outliers"), six, _padded(scene("c_n65"), 257)]
    for n in (3, 10):
        T, valid, sm = _device(gpu, _cat(batch), n, loss, PIXEL)
        assert valid.tolist() == [True, False, True] and T.shape == (2, 4, 4) and bool(T.isfinite().all())
        assert not sm[1].any()
        raw_T = _raw(gpu, _cat(batch), n, CODES[loss], PIXEL, False)[0]
        assert torch.equal(raw_T[1], six["T_init"][0]) and torch.equal(raw_T[[0, 2]], T)
        for i, (b, s) in enumerate(((0, batch[0]), (2, batch[2]))):
            Ta, va, sa = _device(gpu, s, n, loss, PIXEL)
            assert va.tolist() == [True] and torch.equal(Ta[0], T[i]) and torch.equal(sa[0], sm[b]), (loss, n, b)
        Ts, vs, ss = _device(gpu, six, n, loss, PIXEL)
        assert vs.tolist() == [False] and Ts.shape == (0, 4, 4) and not ss.any()
        # the same pair at another position: the same scale, the same everything
        T2, _, sm2 = _device(gpu, _cat(batch[::-1]), n, loss, PIXEL)
        assert torch.equal(sm2[2], sm[0]) and torch.equal(sm2[0], sm[2]) and torch.equal(T2[[1, 0]], T)
        for b in (0, 2):
            conf = batch[b]["conf"][0][batch[b]["conf"][0] > 0].double()
            assert float(sm[b, 3]) == PIXEL / (0.5 * max(2.0 * float(conf.sum()), 1e-6)), (loss, n, b)
    # the padded pair is the pair: the rows behind it reach nothing
    Tp, _, sp = _device(gpu, batch[2], 10, loss, PIXEL)
    Tc, _, sc = _device(gpu, scene("c_n65"), 10, loss, PIXEL)
    assert torch.equal(Tp, Tc) and torch.equal(sp, sc)


@pytest.mark.gpu
def test_the_c_entry_validates_its_arguments(gpu):
    from e2e_multi_view_matching_amd import _lib
    s = scene("a_n7")
    for code, a in ((3, 1.0), (-1, 1.0), (1, 0.0), (1, -1.0), (2, float("nan")), (2, float("inf"))):
        with pytest.raises(_lib.E2EMVError) as e:
            _raw(gpu, s, 1, code, a, True)
        assert e.value.code == _lib.EINVAL and "loss" in str(e.value), (code, a, e.value)
    with pytest.raises(_lib.E2EMVError) as e:  # shape errors as in e2emv_ba_2view
        _raw(gpu, s, -1, 2, PIXEL, False)
    assert e.value.code == _lib.ESHAPE
    T, valid, sm = _raw(gpu, s, 1, 0, float("nan"), True)  # without a loss the scale is not looked at
    assert valid.tolist() == [1] and bool(T.isfinite().all()) and float(sm[0, 3]) == 0.0


# ------------------------------------------------------------------------------------------------ parity per LM step


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", list(CASES))
def test_every_lm_step_matches_the_restatement(gpu, name, loss):
    s = scene(name)
    scale = scale_of(name)
    tp, tm = trajectories(name, loss)
    N = s["conf"].shape[1]
    for n in N_ITERS:
        T, valid, sm = _device(gpu, s, n, loss, scale)
        assert valid.tolist() == [True] and T.dtype == torch.float32 and T.shape == (1, 4, 4) and sm.shape == (1, 4), (name, n)
        sm = sm[0]
        # exact: the scale (one division) and the number of evaluations that improved
        assert float(sm[3]) == float(tp["summary"][3]), (name, loss, n, float(sm[3]), float(tp["summary"][3]))
        assert float(sm[2]) == float(tp["accepted"][1:n + 1].sum()), (name, loss, n, float(sm[2]), pattern(tp)[:n])
        # costs: four brackets plus the summation order
        for k, key in ((0, "cost"), (1, "best_cost_after")):
            p, m = float(tp[key][0 if k == 0 else n]), float(tm[key][0 if k == 0 else n])
            bar = 4.0 * abs(p - m) + N * 2.0 ** -52 * abs(0.5 * (p + m))
            got = float(sm[k])
            print(f"{name} {loss} n={n}: summary[{k}] = {got:.6e}  |got - mid| = {abs(got - 0.5 * (p + m)):.3e}  bar = {bar:.3e}")
            assert np.isfinite(got) and abs(got - 0.5 * (p + m)) <= bar, (name, loss, n, k, got, p, m, bar)
        if n == 0:
            assert torch.equal(T, s["T_init"]) and float(sm[0]) == float(sm[1]), (name, "n_iterations = 0 must return T_init bit for bit")
            continue
        T = T[0].double()
        mid = 0.5 * (tp["best"][n] + tm["best"][n])
        d = delta(tp, tm, n)
        bar = EPS32 * T.abs().clamp(min=1.0) + 4.0 * d
        dist = (T - mid).abs()
        print(f"{name} {loss} n={n}: |T - mid| = {float(dist.max()):.3e}  delta = {d:.3e}  bar = {float(bar.min()):.3e}  [{pattern(tp)[:n]}]")
        assert bool(T.isfinite().all()), (name, loss, n)
        assert bool((dist <= bar).all()), (name, loss, n, float(dist.max()), float(bar.min()), d)


# ------------------------------------------------------------------------------------------------ the batched path


def _planted(gpu, n_kpts):
    data, result, gt, _ = planted_scene(21, wrong=0.1, n_kpts=n_kpts)
    return data, _to(result, gpu), gt


def _record_calls(monkeypatch):
    from e2e_multi_view_matching_amd import _lib
    called = []
    real = _lib.Context.call
    monkeypatch.setattr(_lib.Context, "call", lambda self, name, *a: (called.append(name), real(self, name, *a))[1])
    return called


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["w8pt_ba", "ransac_ba"])
def test_no_pair_loss_is_todays_path_bit_for_bit(gpu, method, monkeypatch):
    from e2e_multi_view_matching_amd import multi_view
    data, result, _ = _planted(gpu, 64)
    today = multi_view.solve_tuple_poses_batch(5, data, result, rel_pose_method=method)
    called = _record_calls(monkeypatch)
    none = multi_view.solve_tuple_poses_batch(5, data, result, rel_pose_method=method, pair_loss=None, pair_loss_scale=None)
    assert np.array_equal(none, today) and np.isfinite(today).all()
    assert "e2emv_ba_2view" in called and "e2emv_ba_2view_loss" not in called, called


@pytest.mark.gpu
@pytest.mark.parametrize("method,init", [("w8pt_ba", "host"), ("w8pt_ba", "device"), ("ransac_ba", "host")])
def test_whole_path_with_a_pair_loss(gpu, method, init, monkeypatch):
    """One planted 5-tuple at 256 keypoints, 10 % wrong matches, Cauchy at one pixel in the pairwise stage: finite, camera 0 the
    identity, ``e2emv_ba_2view_loss`` in place of ``e2emv_ba_2view``, and the relative poses that the initialisation gets are
    ``run_bundle_adjust_2_view(..., loss="cauchy", loss_scale=1/600)`` of every pair alone, bit for bit."""
    from e2e_multi_view_matching_amd import multi_view, pose
    data, result, gt = _planted(gpu, 256)
    plain = multi_view.solve_tuple_poses_batch(5, data, result, init=init, rel_pose_method=method)
    called = _record_calls(monkeypatch)
    seen = {}
    if method == "w8pt_ba":
        real_ba = multi_view.run_bundle_adjust_2_view

        def ba(*a, **k):
            seen["args"], seen["kwargs"] = tuple(x.clone() for x in a), k  # the caller writes the refined poses into its start
            return real_ba(*a, **k)

        monkeypatch.setattr(multi_view, "run_bundle_adjust_2_view", ba)
    real_stage = getattr(multi_view, "_w8pt_ba_on_device" if method == "w8pt_ba" else "_ransac_on_device")

    def stage(*a, **k):
        seen["stage"] = real_stage(*a, **k)
        return seen["stage"]

    monkeypatch.setattr(multi_view, real_stage.__name__, stage)
    out = multi_view.solve_tuple_poses_batch(5, data, result, init=init, rel_pose_method=method, pair_loss="cauchy", pair_loss_scale=PIXEL)
    assert out.shape == (1, 5, 4, 4) and np.isfinite(out).all() and np.array_equal(out[0, 0], np.eye(4))
    assert "e2emv_ba_2view_loss" in called and "e2emv_ba_2view" not in called, called
    assert not np.array_equal(out, plain) and np.isfinite(plain).all()
    err_t, err_R = multi_view.tuple_pose_errors(out[0], np.linalg.inv(gt))
    print(method, init, "pose errors (degrees) with the pair loss: max", max(err_t.max(), err_R.max()))
    if method == "w8pt_ba":
        T_d = seen["stage"][0].cpu()
        k0n, k1n, cf, T0 = seen["args"][:4]
        assert seen["kwargs"]["loss"] == "cauchy" and seen["kwargs"]["loss_scale"] == PIXEL and T_d.shape == (10, 4, 4)
        for q in range(10):
            refined, ok = pose.run_bundle_adjust_2_view(k0n[q:q + 1], k1n[q:q + 1], cf[q:q + 1], T0[q:q + 1], 10, loss="cauchy", loss_scale=PIXEL)
            assert ok.tolist() == [True] and torch.equal(refined[0].cpu(), T_d[q]), q
    else:
        T_d = seen["stage"]["T"].cpu().numpy()
        pw = multi_view._collect_matches(5, data, {k: v.cpu() for k, v in result.items()}, 0.)
        pairs = multi_view._pairs(5)
        problems = [(pw[f"intr{i}"], pw[f"intr{j}"], pw[f"mkpts{i}_{i}_{j}"], pw[f"mkpts{j}_{i}_{j}"], pw[f"conf{i}_{i}_{j}"]) for i, j in pairs]
        host = multi_view.relative_poses_ransac(problems, ba=True, loss="cauchy", loss_scale=PIXEL)
        plain = multi_view.relative_poses_ransac(problems, ba=True)
        assert any(ok and not np.array_equal(R, Rp) for (ok, R, _, _), (_, Rp, _, _) in zip(host, plain))
        for q, (ok, R, t, _) in enumerate(host):
            assert ok and np.array_equal(T_d[q, :3, :3], R) and np.array_equal(T_d[q, :3, 3], t), q


@pytest.mark.gpu
def test_relative_poses_take_the_loss(gpu):
    """``relative_poses_w8pt_ba`` passes the loss on: with it the result differs from the one without, and is repeatable."""
    from e2e_multi_view_matching_amd import multi_view
    data, result, _ = _planted(gpu, 256)
    pw = multi_view._collect_matches(5, data, {k: v.cpu() for k, v in result.items()}, 0.)
    problems = [(pw[f"intr{i}"], pw[f"intr{j}"], pw[f"mkpts{i}_{i}_{j}"], pw[f"mkpts{j}_{i}_{j}"], pw[f"conf{i}_{i}_{j}"]) for i, j in [(0, 1), (1, 3)]]
    plain = multi_view.relative_poses_w8pt_ba(problems)
    robust = multi_view.relative_poses_w8pt_ba(problems, loss="cauchy", loss_scale=PIXEL)
    again = multi_view.relative_poses_w8pt_ba(problems, loss="cauchy", loss_scale=PIXEL)
    for (ok, R, t, _), (ok2, R2, t2, _), (_, R3, t3, _) in zip(plain, robust, again):
        assert ok and ok2 and np.isfinite(R2).all() and not np.array_equal(R, R2) and np.array_equal(R2, R3) and np.array_equal(t2, t3)
