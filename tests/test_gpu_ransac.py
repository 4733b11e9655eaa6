"""GPU: the RANSAC essential-matrix baseline (csrc/ransac.hip, ransac.py, multi_view ransac / ransac_ba) against an
independent numpy restatement kept in this file: Stewenius' action-matrix 5-point solver (np.linalg.eig), the Sampson
test, OpenCV's sequential RANSAC rule on the documented sample stream, and recoverPose (SVD + DLT + depth tests)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ransac_host import draw_sample  # noqa: E402

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------
# numpy restatement
# ---------------------------------------------------------------------------------------------------------------------
_GREVLEX = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
            (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _lin(c):
    p = np.zeros((4, 4, 4))
    p[1, 0, 0], p[0, 1, 0], p[0, 0, 1], p[0, 0, 0] = c
    return p


def _pmul(p, q):
    out = np.zeros((4, 4, 4))
    for a, b, c in zip(*np.nonzero(q)):
        out[a:, b:, c:] += p[:4 - a, :4 - b, :4 - c] * q[a, b, c]
    return out


def np_five_point(x0, x1):
    """Stewenius: null space by SVD, the 10 cubics in grevlex order, action matrix of x on the quotient basis
    (x^2, xy, xz, y^2, yz, z^2, x, y, z, 1), eigenvectors -> (x, y, z).  Returns (E [n,9] unit norm, ambiguous) where
    ambiguous flags an eigenvalue too close to the real axis to classify."""
    h0, h1 = np.c_[x0, np.ones(5)], np.c_[x1, np.ones(5)]
    A = np.einsum("ni,nj->nij", h1, h0).reshape(5, 9)
    N = np.linalg.svd(A)[2][5:]
    e = [[_lin(N[:, 3 * i + j]) for j in range(3)] for i in range(3)]
    det = (_pmul(e[0][0], _pmul(e[1][1], e[2][2]) - _pmul(e[1][2], e[2][1]))
           - _pmul(e[0][1], _pmul(e[1][0], e[2][2]) - _pmul(e[1][2], e[2][0]))
           + _pmul(e[0][2], _pmul(e[1][0], e[2][1]) - _pmul(e[1][1], e[2][0])))
    EEt = [[sum(_pmul(e[i][k], e[j][k]) for k in range(3)) for j in range(3)] for i in range(3)]
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    eqs = [det] + [2 * sum(_pmul(EEt[i][k], e[k][j]) for k in range(3)) - _pmul(tr, e[i][j]) for i in range(3) for j in range(3)]
    C = np.array([[q[m] for m in _GREVLEX] for q in eqs])
    G = np.linalg.solve(C[:, :10], C[:, 10:])
    At = np.zeros((10, 10))
    for j in range(6):
        At[j] = -G[j]
    At[6, 0] = At[7, 1] = At[8, 2] = At[9, 6] = 1.0
    _, V = np.linalg.eig(At)
    sols, amb = [], False
    for k in range(10):
        v = V[:, k] / V[9, k]
        im = np.abs(v.imag).max() / max(1.0, np.abs(v.real).max())
        if im > 1e-9:
            amb |= im < 1e-4
            continue
        E = v.real[6] * N[0] + v.real[7] * N[1] + v.real[8] * N[2] + N[3]
        sols.append(E / np.linalg.norm(E))
    return np.array(sols).reshape(-1, 9), amb


def canon(E):
    E = E.reshape(-1, 9) / np.linalg.norm(E.reshape(-1, 9), axis=1, keepdims=True)
    return E * np.sign(E[np.arange(len(E)), np.abs(E).argmax(1)])[:, None]


def essential_residual(E):
    E = E.reshape(3, 3)
    return max(abs(np.linalg.det(E)), np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max())


def sampson(E, k0, k1):
    E = E.reshape(3, 3)
    h0, h1 = np.c_[k0, np.ones(len(k0))], np.c_[k1, np.ones(len(k1))]
    a, b = h0 @ E.T, h1 @ E
    num = np.einsum("ni,ni->n", h1, a)
    den = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return num * num / den


def update_num_iters(p, ep, max_iters):
    num = np.log(max(1.0 - p, np.finfo(float).tiny))
    denom = 1.0 - (1.0 - ep) ** 5
    if denom < np.finfo(float).tiny:
        return 0
    denom = np.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * -denom) else int(np.rint(num / denom))


def np_ransac(k0, k1, thr, hyps, conf=0.99999, max_iters=1000, margin=1e-5):
    """OpenCV's loop on the given hypotheses per iteration (hyps[it] = [n,9]); returns (iters, best count, E, clean) where
    clean = no hypothesis has a match within `margin` relative of the threshold that could change its outcome."""
    M, t2 = len(k0), thr * thr
    niters, best, bestE, clean, it = max_iters, 0, None, True, 0
    while it < niters:
        for E in hyps[it]:
            err = sampson(E, k0, k1)
            good = int(np.sum(err <= t2))
            lo, hi = int(np.sum(err <= t2 * (1 - margin))), int(np.sum(err <= t2 * (1 + margin)))
            # a match inside the margin matters only where it could change a decision or a new best's count
            clean &= lo == hi or (hi <= max(best, 4) and lo <= max(best, 4))
            if good > max(best, 4):
                best, bestE = good, E
                niters = update_num_iters(conf, (M - good) / M, niters)
        it += 1
    return it, best, bestE, clean


def np_recover_pose(E, k0, k1, mask, dist=1e9):
    U, _, Vt = np.linalg.svd(E.reshape(3, 3))
    U = U * (-1 if np.linalg.det(U) < 0 else 1)
    Vt = Vt * (-1 if np.linalg.det(Vt) < 0 else 1)
    W = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    best = None
    for R, tt in ((R1, t), (R2, t), (R1, -t), (R2, -t)):
        P1 = np.c_[R, tt]
        rows = np.zeros((len(k0), 4, 4))
        rows[:, 0] = np.c_[-np.ones(len(k0)), np.zeros(len(k0)), k0[:, 0], np.zeros(len(k0))]
        rows[:, 1] = np.c_[np.zeros(len(k0)), -np.ones(len(k0)), k0[:, 1], np.zeros(len(k0))]
        rows[:, 2] = k1[:, :1] * P1[2] - P1[0]
        rows[:, 3] = k1[:, 1:] * P1[2] - P1[1]
        X = np.linalg.svd(rows)[2][:, -1]
        with np.errstate(divide="ignore", invalid="ignore"):
            ok = X[:, 2] * X[:, 3] > 0
            Xd = X[:, :3] / X[:, 3:]
            z2 = Xd @ R[2] + tt[2]
            ok &= (Xd[:, 2] < dist) & (z2 > 0) & (z2 < dist) & mask
        n = int(ok.sum())
        if best is None or n > best[0]:
            best = (n, R, tt)
    return best


# ---------------------------------------------------------------------------------------------------------------------
# synthetic scenes
# ---------------------------------------------------------------------------------------------------------------------
def rotation(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def scene(rng, M, outliers, noise=0.5):
    R = rotation(rng.normal(size=3) * 0.15)
    t = np.r_[rng.normal(size=2), 0.3 * rng.normal()]
    t /= np.linalg.norm(t)
    K0 = np.array([[520.0, 0, 320], [0, 515.0, 240], [0, 0, 1]])
    K1 = np.array([[610.0, 0, 300], [0, 600.0, 250], [0, 0, 1]])
    X = np.c_[rng.uniform(-2, 2, (M, 2)), rng.uniform(2.5, 5, M)]  # depth / baseline 2.5..5
    Y = X @ R.T + t
    p0 = (X[:, :2] / X[:, 2:]) * K0[[0, 1], [0, 1]] + K0[:2, 2] + rng.normal(size=(M, 2)) * noise
    p1 = (Y[:, :2] / Y[:, 2:]) * K1[[0, 1], [0, 1]] + K1[:2, 2] + rng.normal(size=(M, 2)) * noise
    n_out = int(round(outliers * M))
    p1[:n_out] = rng.uniform([0, 0], [640, 480], (n_out, 2))
    return p0, p1, K0, K1, R, t


def angle_errors(R, t, Rg, tg):
    cos_r = np.clip((np.trace(R.T @ Rg) - 1) / 2, -1, 1)
    cos_t = np.clip(t @ tg / np.linalg.norm(t) / np.linalg.norm(tg), -1, 1)
    return np.degrees(np.arccos(cos_r)), np.degrees(np.arccos(cos_t))


# ---------------------------------------------------------------------------------------------------------------------
def test_minimal_solver_matches_action_matrix_solver(gpu):
    from e2e_multi_view_matching_amd.ransac import essential_5pt
    rng = np.random.default_rng(0)
    x0s, x1s, Ets = [], [], []
    while len(x0s) < 300:
        R, t = rotation(rng.normal(size=3) * 0.3), rng.normal(size=3)
        t /= np.linalg.norm(t)
        X = np.c_[rng.uniform(-1, 1, (5, 2)), rng.uniform(2, 6, 5)]
        Y = X @ R.T + t
        if Y[:, 2].min() < 0.5:
            continue
        x0s.append(X[:, :2] / X[:, 2:])
        x1s.append(Y[:, :2] / Y[:, 2:])
        Ets.append((skew(t) @ R).ravel())
    Ed, nd = essential_5pt(np.array(x0s), np.array(x1s))
    checked = matched = 0
    for k in range(len(x0s)):
        En, amb = np_five_point(x0s[k], x1s[k])
        # well-conditioned: numpy classifies every root clearly and its own solutions satisfy the constraints
        if amb or any(essential_residual(E) > 1e-12 for E in En):
            continue
        checked += 1
        dev = Ed[k, :nd[k]].reshape(-1, 9)
        for E in dev:  # every device solution is an essential matrix
            assert essential_residual(E) <= 1e-10, essential_residual(E)
        assert np.abs(canon(dev) - canon(Ets[k][None])).max(-1).min() < 1e-8  # the true E is in the set
        if len(En) == len(dev):
            d = np.abs(canon(En)[:, None] - canon(dev)[None]).max(-1)
            matched += int(d.min(1).max() < 1e-8 and d.min(0).max() < 1e-8)
    assert checked >= 200, checked
    # the same solution set within 1e-8 (one problem in ~2000 loses digits in the w = 1 parametrisation: see DESIGN.md §8)
    assert matched >= checked - 2, (matched, checked)


SIZES = (5, 6, 50, 500, 2048, 4096)
OUTLIERS = (0.0, 0.3, 0.6)


@pytest.fixture(scope="module")
def batch(gpu):
    from e2e_multi_view_matching_amd.ransac import essential_ransac, normalize_keypoints
    rng = np.random.default_rng(1)
    probs = []
    for rep in range(2):
        for M in SIZES:
            for o in OUTLIERS:
                probs.append(scene(rng, M, o if M >= 50 else 0.0))
    k0n = [normalize_keypoints(p[0], p[2]) for p in probs]
    k1n = [normalize_keypoints(p[1], p[3]) for p in probs]
    th = [1.0 / np.mean([p[2][0, 0], p[3][1, 1], p[2][0, 0], p[3][1, 1]]) for p in probs]
    out = essential_ransac(k0n, k1n, th, seed=0)
    return probs, k0n, k1n, th, out


def test_estimator_poses_masks_and_counts(batch):
    probs, k0n, k1n, th, out = batch
    assert len(probs) >= 32
    for q, (p0, p1, K0, K1, Rg, tg) in enumerate(probs):
        M = len(p0)
        assert out["status"][q] == 0, (q, M, out["status"][q])
        E, R, t, mask = out["E"][q], out["R"][q], out["t"][q], out["mask"][q]
        assert np.all(np.isfinite(R)) and np.all(np.isfinite(t))
        if M >= 500:  # the pose is the best minimal-sample model, unrefined (as OpenCV's); at 50 matches and 60 % outliers
            er, et = angle_errors(R, t, Rg, tg)  # (20 inliers) it was seen 1.6 deg off, so the bar starts at 500
            assert er < 1.0 and et < 2.0, (q, M, er, et)
        if M > 5:
            err, t2 = sampson(E, k0n[q], k1n[q]), th[q] ** 2
            near = np.abs(err - t2) <= 1e-5 * t2
            assert np.array_equal(mask[~near], (err <= t2)[~near]), q
            Eg = skew(tg) @ Rg
            n_gt = int(np.sum(sampson(Eg / np.linalg.norm(Eg), k0n[q], k1n[q]) <= t2))
            # (the loop stops once a model's count makes niters small: with no outliers the first ~88 % model ends it;
            # at 50 matches a model from ~10 clean samples of 20 inliers was seen at 13 / 19, so the bar starts at 500)
            assert M < 500 or out["n_inliers"][q] >= 0.8 * n_gt, (q, out["n_inliers"][q], n_gt)
            assert out["n_inliers"][q] == mask.sum()
        else:
            assert mask.all() and out["iters"][q] == 1
        n, Rn, tn = np_recover_pose(E, k0n[q], k1n[q], mask)
        assert n == out["n_cheiral"][q], (q, n, out["n_cheiral"][q])
        assert np.abs(Rn - R).max() < 1e-6 and np.abs(tn - t).max() < 1e-6, q


def test_estimator_follows_the_sequential_rule(batch):
    """iters and the best count equal OpenCV's loop run in numpy on the same sample stream (hypotheses from the device's
    minimal solver, checked on its own above) wherever no scored match lies within 1e-5 relative of the threshold."""
    from e2e_multi_view_matching_amd.ransac import essential_5pt
    probs, k0n, k1n, th, out = batch
    qualifying = compared = 0
    for q in range(len(probs)):
        M = len(k0n[q])
        if M <= 5:
            continue
        compared += 1
        n_it = int(out["iters"][q])
        samples = [draw_sample(0, it, M) for it in range(n_it + 1)]
        x0 = np.array([k0n[q][s] for s in samples])
        x1 = np.array([k1n[q][s] for s in samples])
        Es, ns = essential_5pt(x0, x1)
        hyps = [Es[i, :ns[i]].reshape(-1, 9) for i in range(len(samples))] + [np.zeros((0, 9))] * (1000 - len(samples))
        it, best, _, clean = np_ransac(k0n[q], k1n[q], th[q], hyps)
        if not clean:
            continue
        qualifying += 1
        assert (it, best) == (n_it, int(out["n_inliers"][q])), (q, M, it, best, n_it, out["n_inliers"][q])
    assert qualifying >= 0.9 * compared, (qualifying, compared)


def test_contract_few_degenerate_deterministic(gpu):
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd.ransac import estimate_poses_ransac
    rng = np.random.default_rng(2)
    p0, p1, K0, K1, _, _ = scene(rng, 300, 0.3)
    assert E.estimate_pose(p0[:4], p1[:4], K0, K1, 1.0) is None
    assert E.estimate_pose(p0[:0], p1[:0], K0, K1, 1.0) is None
    # degenerate: every point the same; points on one plane through the baseline (all epipolar lines coincide)
    same0, same1 = np.tile(p0[:1], (100, 1)), np.tile(p1[:1], (100, 1))
    X = np.c_[rng.uniform(-2, 2, 100), np.zeros(100), rng.uniform(4, 8, 100)]
    Kn = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    Y = X + np.array([1.0, 0, 0])
    q0 = X[:, :2] / X[:, 2:] * 500 + [320, 240]
    q1 = Y[:, :2] / Y[:, 2:] * 500 + [320, 240]
    for r in estimate_poses_ransac([(same0, same1, K0, K1), (q0, q1, Kn, Kn)]):
        assert r is None or (np.all(np.isfinite(r[0])) and np.all(np.isfinite(r[1])))
    # bit-identical: two runs; alone vs inside a batch (any position)
    others = [scene(rng, m, 0.3)[:4] for m in (50, 700, 2000)]
    target = (p0, p1, K0, K1)
    alone = estimate_poses_ransac([target], seed=5)[0]
    again = estimate_poses_ransac([target], seed=5)[0]
    inside = estimate_poses_ransac(others[:2] + [target] + others[2:], seed=5)[2]
    for a, b in ((alone, again), (alone, inside)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_estimate_pose_threshold_follows_f_mean(gpu):
    import e2e_multi_view_matching_amd as E
    from e2e_multi_view_matching_amd.ransac import essential_ransac, normalize_keypoints
    rng = np.random.default_rng(3)
    p0, p1, K0, K1, _, _ = scene(rng, 500, 0.3, noise=1.0)
    K1 = K1.copy()
    K1[1, 1] = 900.0  # upstream's f_mean = mean(K0[0,0], K1[1,1], K0[0,0], K1[1,1])
    R, t, mask = E.estimate_pose(p0, p1, K0, K1, 2.0)
    f_mean = (2 * K0[0, 0] + 2 * K1[1, 1]) / 4
    r = essential_ransac([normalize_keypoints(p0, K0)], [normalize_keypoints(p1, K1)], [2.0 / f_mean])
    assert np.array_equal(mask, r["mask"][0]) and np.array_equal(R, r["R"][0]) and np.array_equal(t, r["t"][0])
    other = essential_ransac([normalize_keypoints(p0, K0)], [normalize_keypoints(p1, K1)], [2.0 / K0[0, 0]])
    assert other["n_inliers"][0] != r["n_inliers"][0]


# ---------------------------------------------------------------------------------------------------------------------
def _tuple(rng, T=5, N=400, noise=1.0, outliers=0.2):
    X = np.c_[rng.uniform(-3, 3, (N, 2)), rng.uniform(6, 12, N)]
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]], np.float32)
    data, result, c2w = {}, {}, []
    for v in range(T):
        R = rotation(np.r_[0.0, 0.08 * v + 1e-9, 0.0])
        C = np.r_[1.5 * v, 0.3 * v, 0.2 * v]  # camera centre
        W = np.eye(4)
        W[:3, :3], W[:3, 3] = R, -R @ C
        c2w.append(np.linalg.inv(W))
        Y = X @ R.T + W[:3, 3]
        kp = Y[:, :2] / Y[:, 2:] * 500 + [320, 240] + rng.normal(size=(N, 2)) * noise
        data["keypoints" + str(v)] = torch.from_numpy(kp.astype(np.float32))[None]
        data["intr" + str(v)] = torch.from_numpy(K)[None]
        data["pose" + str(v)] = torch.from_numpy(c2w[-1].astype(np.float32))[None]
    for j in range(T):
        for i in range(j):
            m = np.arange(N)
            bad = rng.choice(N, int(outliers * N), replace=False)
            m[bad] = rng.permutation(m[bad])
            result["matches{}_{}_{}".format(i, i, j)] = torch.from_numpy(m)[None].cuda()
            result["conf_scores_{}_{}".format(i, j)] = torch.from_numpy(rng.uniform(0.5, 1.0, (N, 1)).astype(np.float32))[None].cuda()
    return data, result, np.array(c2w)


def test_initialize_bundle_adjust_ransac_and_ransac_ba(gpu, tmp_path):
    from e2e_multi_view_matching_amd import multi_view
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("dropin_bundle_adjust_io", os.path.join(
        root, "dropin", "pose_optimization", "multi_view", "bundle_adjust_io.py"))
    dropin_io = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dropin_io)
    assert dropin_io.estimate_relative_pose_ransac is multi_view.estimate_relative_pose_ransac
    assert dropin_io.estimate_relative_pose_ransac_ba is multi_view.estimate_relative_pose_ransac_ba
    rng = np.random.default_rng(4)
    T = 5
    data, result, c2w = _tuple(rng, T)
    errs = {}
    for method in ("ransac", "ransac_ba"):
        path = tmp_path / (method + ".csv")
        pw = multi_view.initialize_bundle_adjust(T, data, result, str(path), rel_pose_method=method)
        assert path.exists() and len(open(path).read().splitlines()) >= T
        e = []
        for j in range(T):
            for i in range(j):
                for v in (i, j):
                    for kind in ("mkpts", "conf"):
                        assert "{}{}_{}_{}".format(kind, v, i, j) in pw
                n_in = pw["inlier_count{}_{}".format(i, j)]
                assert len(pw["mkpts{}_{}_{}".format(i, i, j)]) == n_in == len(pw["conf{}_{}_{}".format(j, i, j)])
                assert n_in >= 0.4 * 400  # 1 px noise against a 1 px Sampson threshold
                Tg = np.linalg.inv(c2w[j]) @ c2w[i]
                Tp = pw["rel_pose{}_{}".format(i, j)]
                er, et = angle_errors(Tp[:3, :3], Tp[:3, 3], Tg[:3, :3], Tg[:3, 3])
                assert er < 2.0 and et < 5.0, (method, i, j, er, et)
                e.append(er + et)
        for v in range(T):
            assert "abs_init_pose" + str(v) in pw and "intr" + str(v) in pw
        errs[method] = np.mean(e)
    assert errs["ransac_ba"] <= errs["ransac"] + 1e-3, errs
    # the one-pair forms agree with the batched path
    pw = multi_view._collect_matches(T, data, result, 0.0)
    args = (pw["intr0"], pw["intr1"], pw["mkpts0_0_1"], pw["mkpts1_0_1"])
    ok, R, t, inl = multi_view.estimate_relative_pose_ransac(*args)
    okb, Rb, tb, inlb = multi_view.estimate_relative_pose_ransac_ba(*args, pw["conf0_0_1"])
    assert ok and okb and np.array_equal(inl, inlb) and inl.dtype == bool
