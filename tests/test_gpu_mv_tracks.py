"""GPU: track merging of the batched multi-view back-end (``multi_view.match_tracks``, ``solve_tuple_poses_batch(...,
tracks=True)``; csrc/mvtracks.hip) against a numpy union-find and a numpy problem builder that live in this file."""
import numpy as np
import pytest
import torch

from test_gpu_mv_batch import T5_CFG, _random_match_inputs, _slice

pytestmark = pytest.mark.gpu


# ---- the host restatement ------------------------------------------------------------------------------------------------
def _pairs(T):
    return [(i, j) for j in range(T) for i in range(j)]


def host_edges(T, data, result, b, conf_thresh):
    """Kept edges of batch element ``b``: ``{(node_i, node_j): confidence of channel 0}``, node = ``t * Nmax + n``."""
    n_img = [data[f"keypoints{t}"].shape[1] for t in range(T)]
    Nmax = max(n_img)
    edges = {}
    for i, j in _pairs(T):
        if f"matches{i}_{i}_{j}" not in result:
            continue
        m = result[f"matches{i}_{i}_{j}"][b].cpu().numpy()
        c = result[f"conf_scores_{i}_{j}"][b].cpu().numpy().astype(np.float32).reshape(len(m), -1)
        keep = (m >= 0) & (m < n_img[j]) & (c > np.float32(conf_thresh)).all(1)
        for n in np.nonzero(keep)[0]:
            edges[(i * Nmax + int(n), j * Nmax + int(m[n]))] = c[n, 0]
    return edges, Nmax


def host_labels(T, Nmax, edges):
    """Union-find: ``(label [T, Nmax] int32, stats [4])`` with the semantics of ``e2emv_mv_tracks``."""
    parent = np.arange(T * Nmax)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in edges:
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    root = np.array([find(x) for x in range(T * Nmax)])
    label = np.full(T * Nmax, -1, np.int32)
    tracks = obs = conflicts = 0
    order = np.argsort(root, kind="stable")
    uniq, first, size = np.unique(root[order], return_index=True, return_counts=True)
    for r, f, k in zip(uniq, first, size):
        if k < 2:
            continue
        nodes = order[f:f + k]
        images = nodes // Nmax
        if len(np.unique(images)) < len(images):
            conflicts += 1
        elif len(nodes) >= 2:
            label[nodes] = r
            tracks += 1
            obs += len(nodes)
    return label.reshape(T, Nmax), np.array([tracks, obs, conflicts, len(edges)], np.int32)


def host_problem(T, data, b, label, edges, extr, svd_points=True):
    """The track problem of batch element ``b`` from its labels: the argument tuple of ``bundle_adjust``; points by numpy's SVD."""
    Nmax = label.shape[1]
    cam_idx, pt_idx, obs, conf, pts = [], [], [], [], []
    for p, r in enumerate(np.unique(label[label >= 0])):
        nodes = np.nonzero(label.reshape(-1) == r)[0]  # ascending id = ascending image
        rows = []
        for x in nodes:
            t, n = divmod(int(x), Nmax)
            K = data[f"intr{t}"].cpu().numpy().astype(np.float32)
            K = K[b] if K.ndim == 3 else K
            kp = data[f"keypoints{t}"][b, n].cpu().numpy().astype(np.float32)
            xy = (kp - np.array([K[0, 2], K[1, 2]], np.float32)) / np.array([K[0, 0], K[1, 1]], np.float32)
            assert xy.dtype == np.float32
            s, k = 0.0, 0
            for y in nodes:  # other image ascending
                c = edges.get((min(x, y), max(x, y))) if y != x else None
                if c is not None:
                    s, k = s + float(c), k + 1
            cam_idx.append(t); pt_idx.append(p); obs.append(xy.astype(np.float64)); conf.append(s / k)
            rows += [xy[0].astype(np.float64) * extr[t, 2] - extr[t, 0], xy[1].astype(np.float64) * extr[t, 2] - extr[t, 1]]
        if svd_points:
            X = np.linalg.svd(np.array(rows))[2][-1]
            pts.append(X[:3] / X[3])
    conf = np.array(conf, np.float64)
    w = conf / (0.5 * (conf.sum() + 1e-3)) if len(conf) else conf
    return (np.array(cam_idx, np.int32), np.array(pt_idx, np.int32), np.array(obs, np.float64).reshape(-1, 2), np.stack([w, w], 1).reshape(-1, 2),
            np.array(pts, np.float64).reshape(-1, 3))


def _rodrigues(aa):
    th = np.linalg.norm(aa)
    if th < 1e-12:
        return np.eye(3)
    k = aa / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _perturbed_start(gt, rng, rot=0.02, tr=0.05):
    """Ground-truth world -> camera extrinsics [T,4,4] perturbed by N(0, rot) rad and N(0, tr) per camera; camera 0 is the gauge."""
    out = gt.copy()
    for t in range(1, len(gt)):
        out[t, :3, :3] = _rodrigues(rng.normal(0, rot, 3)) @ gt[t, :3, :3]
        out[t, :3, 3] = gt[t, :3, 3] + rng.normal(0, tr, 3)
    return out


def planted_scene(seed, wrong=0.0, drop=0.0, T=5, n_kpts=256):
    """The scenes of the table in DESIGN.md section 1: ``make_tuples`` 5-tuple, matches = ``gt_matches``, confidences U(0.5, 1)
    per keypoint; with ``wrong`` each matched keypoint is replaced with that probability by a uniform random target of confidence
    U(0, 0.5) (all drawn from ``default_rng(1000 + seed)``, pairs in ``_pairs`` order); with ``drop`` matches are removed instead
    (tracks of every length without conflicts).  Returns ``(data, result, gt extrinsics [T,4,4], start [T,4,4])``, the start
    drawn from ``default_rng(7 + seed)``."""
    from e2e_multi_view_matching_amd.synthetic import make_tuples
    data = make_tuples(batch=1, tuple_size=T, n_kpts=n_kpts, seed=seed, noise_px=0.5, max_angle=0.25, transl_sigma=0.4)
    rng = np.random.default_rng(1000 + seed)
    result = {}
    for i, j in _pairs(T):
        m = data[f"gt_matches{i}_{i}_{j}"][0].numpy().copy()
        conf = rng.uniform(0.5, 1.0, n_kpts)
        hit = (m >= 0) & (rng.uniform(size=n_kpts) < max(wrong, drop))
        if wrong:
            m[hit] = rng.integers(0, n_kpts, int(hit.sum()))
            conf[hit] = rng.uniform(0.0, 0.5, int(hit.sum()))
        elif drop:
            m[hit] = -1
        result[f"matches{i}_{i}_{j}"] = torch.from_numpy(m[None])
        result[f"conf_scores_{i}_{j}"] = torch.from_numpy(conf.astype(np.float32)[None, :, None])
    gt = np.stack([data[f"pose{t}"][0].numpy().astype(np.float64) for t in range(T)])
    return data, result, gt, _perturbed_start(gt, np.random.default_rng(7 + seed))


def _to(result, gpu):
    return {k: v.to(gpu) for k, v in result.items()}


def _device_tracks(T, data, result, conf_thresh, gpu):
    from e2e_multi_view_matching_amd import multi_view
    label, stats = multi_view.match_tracks(T, data, _to(result, gpu), conf_thresh)
    assert label.dtype == torch.int32 and stats.dtype == torch.int32 and label.device.type == "cuda"
    return label.cpu().numpy(), stats.cpu().numpy()


def _device_problems(T, data, result, conf_thresh, extr, gpu):
    from e2e_multi_view_matching_amd import multi_view
    intr, kdim, nb = multi_view._tuple_intrinsics(T, data, gpu, len(extr))
    return multi_view._tuple_problems_tracks(T, data, _to(result, gpu), conf_thresh, intr, kdim, nb, extr)


# ---- labels --------------------------------------------------------------------------------------------------------------
def _random_inputs():
    """B = 3, T = 4, N = 70 (two waves, no multiple of 64), the last image 50 keypoints, 40 % unmatched; element 1 has pair (0, 2)
    at -1 throughout and the ``matches`` entry of pair (1, 3) is absent."""
    B, T, N = 3, 4, 70
    data, result = _random_match_inputs(B, T, N, seed=11)
    data[f"keypoints{T - 1}"] = data[f"keypoints{T - 1}"][:, :50].contiguous()
    result["matches0_0_2"][1] = -1
    del result["matches1_1_3"]
    return B, T, N, data, result


@pytest.mark.parametrize("conf_thresh", [0.0, 0.3])
def test_labels_are_the_union_find(gpu, conf_thresh):
    """Labels and stats of random planted matches, exactly; tracks of every length 2 .. T and conflicts both occur; targets beyond
    the 50 keypoints of the last image are no edges; the batch is each element alone, and run to run."""
    B, T, N, data, result = _random_inputs()
    label, stats = _device_tracks(T, data, result, conf_thresh, gpu)
    assert label.shape == (B, T, N) and stats.shape == (B, 4)
    lengths = set()
    for b in range(B):
        edges, Nmax = host_edges(T, data, result, b, conf_thresh)
        want, want_stats = host_labels(T, Nmax, edges)
        assert np.array_equal(label[b], want), (b, np.nonzero(label[b] != want))
        assert np.array_equal(stats[b], want_stats), (b, stats[b], want_stats)
        lengths |= set(np.unique(np.unique(want[want >= 0], return_counts=True)[1]))
        assert (label[b][T - 1, 50:] == -1).all()
        alone = _device_tracks(T, _slice(data, b), _slice(result, b), conf_thresh, gpu)
        assert np.array_equal(alone[0][0], label[b]) and np.array_equal(alone[1][0], stats[b])
    assert lengths == set(range(2, T + 1)) and (stats[:, 2] > 0).all() and (stats[:, 0] > 0).all(), (lengths, stats)
    again = _device_tracks(T, data, result, conf_thresh, gpu)
    assert np.array_equal(again[0], label) and np.array_equal(again[1], stats)


def test_two_images_give_stars(gpu):
    """T = 2: components are stars around the keypoints of image 1; the tracks are the one-to-one pairs."""
    data, result = _random_match_inputs(2, 2, 70, seed=3)
    label, stats = _device_tracks(2, data, result, 0.0, gpu)
    for b in range(2):
        m = result["matches0_0_1"][b].numpy()
        hits = np.bincount(m[m >= 0], minlength=70)
        one_to_one = np.array([m[n] >= 0 and hits[m[n]] == 1 for n in range(70)])
        assert one_to_one.any() and (hits > 1).any()
        assert np.array_equal(label[b, 0], np.where(one_to_one, np.arange(70), -1))
        assert np.array_equal(stats[b], [one_to_one.sum(), 2 * one_to_one.sum(), (hits > 1).sum(), (m >= 0).sum()])
        edges, Nmax = host_edges(2, data, result, b, 0.0)
        assert np.array_equal(label[b], host_labels(2, Nmax, edges)[0])


def test_zigzag_through_three_images(gpu):
    """One component threaded through every keypoint of three images by the pairs (0,1), (1,2), (0,2) alternately: the path
    (0,0) (1,0) (2,0) (0,1) (1,1) (2,1) ... - the input that needs the most sweeps and the one a wrong sweep bound breaks.  It is a
    conflict, so every node reads -1; that node 0 became the label of all 210 nodes shows in the stats: ONE conflict component
    (a propagation that stopped early leaves several), no track, no observation."""
    T, N = 3, 70
    data, _ = _random_match_inputs(1, T, N, seed=1)
    n = np.arange(N)
    m01, m12 = n.copy(), n.copy()                   # (0,n) - (1,n), (1,n) - (2,n)
    m02 = np.where(n >= 1, n - 1, -1)               # (0,n) - (2,n-1) closes (2,n-1) -> (0,n)
    result = {"matches0_0_1": m01, "matches0_0_2": m02, "matches1_1_2": m12}
    result = {k: torch.from_numpy(v.astype(np.int64)[None]) for k, v in result.items()}
    for i, j in _pairs(T):
        result[f"conf_scores_{i}_{j}"] = torch.full((1, N, 1), 0.5)
    edges, Nmax = host_edges(T, data, result, 0, 0.0)
    want, want_stats = host_labels(T, Nmax, edges)
    assert (want == -1).all() and list(want_stats) == [0, 0, 1, 3 * N - 1]
    label, stats = _device_tracks(T, data, result, 0.0, gpu)
    assert (label == -1).all() and list(stats[0]) == [0, 0, 1, 3 * N - 1]


def test_long_chain_label_is_node_zero(gpu):
    """A chain through 8 images with one keypoint each (a track): its far end, 7 hops away, gets label 0; with the threshold at the
    edges' confidence nothing is kept (the comparison is strict)."""
    T, N = 8, 70
    data, _ = _random_match_inputs(1, T, N, seed=2)
    result = {}
    for i, j in _pairs(T):
        m = np.full(N, -1, np.int64)
        if j == i + 1:
            m[0] = 0  # (i,0) - (i+1,0)
        result[f"matches{i}_{i}_{j}"] = torch.from_numpy(m[None])
        result[f"conf_scores_{i}_{j}"] = torch.full((1, N, 1), 0.25)
    label, stats = _device_tracks(T, data, result, 0.0, gpu)
    assert list(stats[0]) == [1, 8, 0, 7] and (label[0, :, 0] == 0).all() and (label[0, :, 1:] == -1).all()
    assert _device_tracks(T, data, result, 0.25, gpu)[1][0].tolist() == [0, 0, 0, 0]  # the threshold is strict


def test_a_tuple_without_matches(gpu):
    """All -1: no track, stats 0, and the solve returns its start extrinsics."""
    from e2e_multi_view_matching_amd import multi_view
    T, N = 3, 70
    data, result = _random_match_inputs(2, T, N, seed=4)
    for k in result:
        if k.startswith("matches"):
            result[k][:] = -1
    label, stats = _device_tracks(T, data, result, 0.0, gpu)
    assert (label == -1).all() and not stats.any()
    start = np.stack([_perturbed_start(np.tile(np.eye(4), (T, 1, 1)), np.random.default_rng(b), rot=0.3, tr=1.0) for b in range(2)])
    intr, kdim, nb = multi_view._tuple_intrinsics(T, data, gpu, 2)
    out, summary = np.zeros((2, T, 4, 4)), np.ones((2, 4))
    multi_view._tracks_ba_call("e2emv_mv_tuple_ba_tracks", T, data, _to(result, gpu), 0.0, intr, kdim, nb, start, 50,
                               multi_view._p(out), multi_view._p(summary))
    assert np.abs(out - start).max() < 1e-14 and np.array_equal(out[:, :, :3, 3], start[:, :, :3, 3]) and not summary[:, :3].any()
    for init in ("host", "device"):
        whole = multi_view.solve_tuple_poses_batch(T, data, _to(result, gpu), init=init, tracks=True)
        assert np.array_equal(whole, multi_view.solve_tuple_poses_batch(T, data, _to(result, gpu), init=init))  # both return the start
        assert np.isfinite(whole).all()


def test_the_node_limit(gpu):
    """T = 8 images of 2048 keypoints = 16384 nodes, the documented limit, against the union-find; one keypoint more is
    ``E2EMV_ESHAPE`` before any launch."""
    from e2e_multi_view_matching_amd import _lib
    T, N = 8, 2048
    rng = np.random.default_rng(6)
    data = {f"keypoints{t}": torch.zeros(1, N, 2) for t in range(T)}
    result = {}
    for i, j in _pairs(T):
        m = rng.integers(0, N, N)
        m[rng.uniform(size=N) < 0.93] = -1  # sparse enough for tracks beside the conflicts
        result[f"matches{i}_{i}_{j}"] = torch.from_numpy(m[None])
        result[f"conf_scores_{i}_{j}"] = torch.from_numpy(rng.uniform(0, 1, (1, N, 1)).astype(np.float32))
    label, stats = _device_tracks(T, data, result, 0.1, gpu)
    edges, Nmax = host_edges(T, data, result, 0, 0.1)
    want, want_stats = host_labels(T, Nmax, edges)
    assert Nmax == N and np.array_equal(label[0], want) and np.array_equal(stats[0], want_stats)
    assert want_stats[0] > 100 and want_stats[2] > 100 and (want[T - 1] >= 0).any(), want_stats
    data[f"keypoints{T - 1}"] = torch.zeros(1, N + 1, 2)
    with pytest.raises(_lib.E2EMVError) as err:
        _device_tracks(T, data, result, 0.1, gpu)
    assert err.value.code == _lib.ESHAPE and "16384" in str(err.value)


# ---- problem build ---------------------------------------------------------------------------------------------------------
def _check_problem(T, data, result, conf_thresh, extr, gpu, points):
    """Device problems of every batch element against ``host_problem``: indices, counts, observations exactly; weights within
    1e-12 relative (fp64 sums of at most a few thousand fp32 values in different orders, n * eps ~ 5e-13).  Returns the device
    problems, labels and the host points."""
    problems, label, stats = _device_problems(T, data, result, conf_thresh, extr, gpu)
    label = label.cpu().numpy()
    host_pts = []
    for b, prob in enumerate(problems):
        edges, Nmax = host_edges(T, data, result, b, conf_thresh)
        want_label, want_stats = host_labels(T, Nmax, edges)
        assert np.array_equal(label[b], want_label) and np.array_equal(stats[b], want_stats)
        cam_idx, pt_idx, obs, wts, pts = host_problem(T, data, b, want_label, edges, extr[b], svd_points=points)
        n_cams, fixed, intr4, d_cam, d_pt, d_obs, d_w, d_cams, d_pts = prob
        assert (n_cams, fixed, list(intr4)) == (T, 0, [1.0, 1.0, 0.0, 0.0])
        assert len(d_pts) == want_stats[0] and len(d_cam) == want_stats[1] == len(cam_idx)
        assert np.array_equal(d_cam, cam_idx) and np.array_equal(d_pt, pt_idx)
        assert np.array_equal(d_obs, obs)
        assert np.array_equal(d_w[:, 0], d_w[:, 1])
        if len(wts):
            rel = (np.abs(d_w - wts) / wts).max()
            print("tuple", b, ":", want_stats, "weights: max relative difference", rel)
            assert (np.abs(d_w - wts) <= 1e-12 * np.abs(wts)).all() and abs(d_w[:, 0].sum() - 2.0) < 1e-3
        assert np.abs(d_cams[:, 3:] - extr[b][:, :3, 3]).max() == 0.0
        host_pts.append(pts)
    return problems, label, host_pts


def test_problem_build_on_random_matches(gpu):
    """The random inputs of the label test with both thresholds and random start extrinsics: everything but the points (random
    matches have no geometry, their null vectors are ill-conditioned)."""
    B, T, N, data, result = _random_inputs()
    extr = np.stack([_perturbed_start(np.tile(np.eye(4), (T, 1, 1)), np.random.default_rng(b), rot=0.2, tr=0.5) for b in range(B)])
    for conf_thresh in (0.0, 0.3):
        problems, _, _ = _check_problem(T, data, result, conf_thresh, extr, gpu, points=False)
        for b in range(B):  # each element alone builds the same bits
            alone = _device_problems(T, _slice(data, b), _slice(result, b), conf_thresh, extr[b:b + 1], gpu)[0][0]
            for x, y in zip(alone[3:], problems[b][3:]):
                assert np.array_equal(x, y, equal_nan=True)


@pytest.fixture(scope="module")
def thinned_scene(gpu):
    """Planted 5-tuple (seed 20) with 60 % of the matches removed: tracks of every length 2 .. 5, no wrong match."""
    data, result, gt, start = planted_scene(20, drop=0.6)
    return data, result, gt, start


def test_problem_build_and_points_on_a_planted_scene(gpu, thinned_scene):
    """Indices, observations, weights as above.  Points: a two-view track equals ``e2emv_mv_triangulate`` on its views EXACTLY; a
    track of k >= 3 views against numpy's SVD null vector, relative to max(1, |X|), at most 10 x the error the two-view routine
    shows against the same SVD on the two-view sub-tracks (all view pairs) of the same tracks (the margin is for the longer sums
    in the normal matrix)."""
    from e2e_multi_view_matching_amd import multi_view
    T = 5
    data, result, gt, start = thinned_scene
    (prob,), label, (svd_pts,) = _check_problem(T, data, result, 0.0, start[None], gpu, points=True)
    _, _, _, cam_idx, pt_idx, obs, _, _, pts = prob
    views = np.bincount(pt_idx)
    assert set(views) == {2, 3, 4, 5} and (label[0] >= 0).sum() == len(cam_idx)
    rel = np.abs(pts - svd_pts).max(1) / np.maximum(1.0, np.abs(svd_pts).max(1))
    # two-view tracks, and the two-view sub-tracks of the longer ones, through the existing routine, grouped by image pair
    first = np.concatenate([[0], np.cumsum(views)])
    two_view_err = 0.0
    for i, j in _pairs(T):
        rows = [(p, first[p] + list(cam_idx[first[p]:first[p + 1]]).index(i), first[p] + list(cam_idx[first[p]:first[p + 1]]).index(j))
                for p in range(len(views)) if i in cam_idx[first[p]:first[p + 1]] and j in cam_idx[first[p]:first[p + 1]]]
        if not rows:
            continue
        p_ids, oi, oj = (np.array(c) for c in zip(*rows))
        X = multi_view.triangulate_points(start[i, :3], start[j, :3], obs[oi], obs[oj])
        exact = views[p_ids] == 2
        assert np.array_equal(X[exact], pts[p_ids[exact]]), (i, j)
        for k in np.nonzero(~exact)[0]:
            A = np.array([obs[oi[k], 0] * start[i, 2] - start[i, 0], obs[oi[k], 1] * start[i, 2] - start[i, 1],
                          obs[oj[k], 0] * start[j, 2] - start[j, 0], obs[oj[k], 1] * start[j, 2] - start[j, 1]])
            Y = np.linalg.svd(A)[2][-1]
            Y = Y[:3] / Y[3]
            two_view_err = max(two_view_err, np.abs(X[k] - Y).max() / max(1.0, np.abs(Y).max()))
    k_view_err = rel[views >= 3].max()
    print("DLT against numpy SVD, relative to max(1, |X|): two-view routine on sub-tracks", two_view_err, " k-view (k >= 3)", k_view_err,
          " two-view tracks", rel[views == 2].max())
    assert (views == 2).sum() > 5 and two_view_err > 0.0
    assert k_view_err <= 10 * two_view_err, (k_view_err, two_view_err)


def test_two_images_give_todays_problem(gpu):
    """T = 2 with one-to-one matches: the track problem is today's ``_tuple_problems`` problem after sorting today's observations
    (image 0 block, image 1 block) into point order: points and observations exactly, weights within 1e-12."""
    from e2e_multi_view_matching_amd import multi_view
    data, result, gt, start = planted_scene(23, drop=0.2, T=2)
    dres = _to(result, gpu)
    (prob,), _, stats = _device_problems(2, data, result, 0.6, start[None], gpu)
    collected = multi_view._collect_matches_batch(2, data, dres, 0.6)
    counts = collected[3].cpu().numpy()
    intr, kdim, nb = multi_view._tuple_intrinsics(2, data, gpu, 1)
    (old,) = multi_view._tuple_problems(2, collected, counts, intr, kdim, nb, start[None])
    n = int(counts[0])
    assert 20 < n < 179 and list(stats[0][:2]) == [n, 2 * n]
    order = np.stack([np.arange(n), n + np.arange(n)], 1).reshape(-1)  # point p: its image-0 then its image-1 observation
    assert np.array_equal(prob[3], old[3][order]) and np.array_equal(prob[4], old[4][order])
    assert np.array_equal(prob[5], old[5][order]) and np.array_equal(prob[8], old[8]) and np.array_equal(prob[7], old[7])
    assert (np.abs(prob[6] - old[6][order]) <= 1e-12 * old[6][order]).all()


# ---- solve -----------------------------------------------------------------------------------------------------------------
def _extrinsics(cams):
    E = np.tile(np.eye(4), (len(cams), 1, 1))
    for c, cam in enumerate(cams):
        E[c, :3, :3], E[c, :3, 3] = _rodrigues(cam[:3]), cam[3:]
    return E


def _solve_tracks(T, data, result, conf_thresh, start, gpu):
    from e2e_multi_view_matching_amd import multi_view
    intr, kdim, nb = multi_view._tuple_intrinsics(T, data, gpu, len(start))
    out, summary = np.zeros((len(start), T, 4, 4)), np.zeros((len(start), 4))
    _, stats = multi_view._tracks_ba_call("e2emv_mv_tuple_ba_tracks", T, data, _to(result, gpu), conf_thresh, intr, kdim, nb, start, 50,
                                          multi_view._p(out), multi_view._p(summary))
    return out, summary, stats


def test_solve_is_the_solver_on_the_copied_out_problem(gpu, thinned_scene):
    """``e2emv_mv_tuple_ba_tracks`` = ``bundle_adjust(*problem)`` on the problem ``e2emv_mv_tuple_problem_tracks`` copies out: the
    same solver on the same inputs, so the device-built index lists are the host-built ones.  Bit for bit in what both return
    unconverted (translations, costs, iterations); the rotations went through the library's angle-axis -> matrix code on one
    side and numpy's on the other (1e-14).  Tuple 0 also against ``oracle.mvba.solve`` at the bars of
    ``test_batched_bundle_adjustment_is_the_single_one_bit_for_bit``."""
    from e2e_multi_view_matching_amd import multi_view
    from oracle import mvba
    T = 5
    d0, r0, _, s0 = thinned_scene
    d1, r1, _, s1 = planted_scene(21, wrong=0.1)
    data = {k: (torch.cat([d0[k], d1[k]], 0) if torch.is_tensor(v) else v) for k, v in d0.items()}
    result = {k: torch.cat([r0[k], r1[k]], 0) for k in r0}
    start = np.stack([s0, s1])
    out, summary, stats = _solve_tracks(T, data, result, 0.0, start, gpu)
    problems, _, _ = _device_problems(T, data, result, 0.0, start, gpu)
    assert stats[0][0] > stats[1][0] > 0
    for b, prob in enumerate(problems):
        cams, pts, sm = multi_view.bundle_adjust(*prob)
        assert np.array_equal(out[b, :, :3, 3], cams[:, 3:]), b
        assert np.abs(out[b] - _extrinsics(cams)).max() < 1e-14
        assert (sm["initial_cost"], sm["final_cost"], sm["iterations"]) == (summary[b, 0], summary[b, 1], int(summary[b, 2])), (sm, summary[b])
        assert sm["final_cost"] < sm["initial_cost"] and sm["iterations"] >= 1
    n_cams, fixed, intr4, cam_idx, pt_idx, obs, wts, cams0, pts0 = problems[0]
    oc, op, osum = mvba.solve(dict(n_cams=n_cams, fixed=fixed, intr=intr4, cam_idx=cam_idx, pt_idx=pt_idx, obs=obs, wts=wts, cams=cams0, pts=pts0))
    gc, gp, gsum = multi_view.bundle_adjust(*problems[0])
    assert gsum["iterations"] == osum["iterations"] and gsum["termination"] == osum["termination"], (gsum, osum)
    assert abs(gsum["initial_cost"] - osum["initial_cost"]) <= 1e-10 * osum["initial_cost"]
    assert abs(gsum["final_cost"] - osum["final_cost"]) <= 1e-8 * osum["final_cost"]
    assert np.abs(gc - oc).max() < 1e-7 and np.abs(gp - op).max() < 1e-6


@pytest.mark.parametrize("seed", [21, 22])
def test_planted_scenes_with_wrong_matches(gpu, seed):
    """The scenes of DESIGN.md section 1 with 10 % wrong matches: the wrong matches turn their components into conflicts, which
    are dropped; at least 25 tracks survive and the solved track problem has pose errors below 2.0 degrees on every pair.
    Measured on an MI355X with this file's draw order: 35 and 39 of 179 tracks, 24 and 31 conflicts, 4 and 3 LM iterations, max
    error 1.76 and 0.79 degrees - the figures ``oracle.mvba.solve`` gives on the numpy-built problem (1.7596, 0.7913)."""
    from e2e_multi_view_matching_amd import multi_view
    T = 5
    data, result, gt, start = planted_scene(seed, wrong=0.1)
    out, summary, stats = _solve_tracks(T, data, result, 0.0, start[None], gpu)
    err_t, err_R = multi_view.tuple_pose_errors(out[0], np.linalg.inv(gt))
    print("seed", seed, "stats", stats[0], "iterations", int(summary[0, 2]), "max pose error", max(err_t.max(), err_R.max()),
          "mean", np.maximum(err_t, err_R).mean())
    assert stats[0][0] >= 25 and stats[0][2] > 0
    assert max(err_t.max(), err_R.max()) < 2.0, (err_t, err_R)


# ---- whole path ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_tuples(gpu):
    """The ``two_tuples`` recipe of tests/test_gpu_mv_batch_ransac.py: B = 2 five-tuples (seeds 20, 21) at 256 keypoints through the
    identity-like matcher; two pairs of element 1 keep 3 matches each."""
    from e2e_multi_view_matching_amd import MultiViewMatcher
    from e2e_multi_view_matching_amd.synthetic import identity_like_state, make_tuples
    T = 5
    model = identity_like_state(MultiViewMatcher(T5_CFG).eval()).to(gpu)
    parts = [make_tuples(batch=1, tuple_size=T, n_kpts=256, seed=s, noise_px=0.5, max_angle=0.25, transl_sigma=0.4) for s in (20, 21)]
    data = {k: (torch.cat([p[k] for p in parts], 0) if torch.is_tensor(v) else v) for k, v in parts[0].items()}
    dev = {k: (v.to(gpu) if torch.is_tensor(v) else v) for k, v in data.items()}
    for m in range(T):  # the reference's pose{m} are camera -> world
        dev[f"pose{m}"] = torch.linalg.inv(data[f"pose{m}"])
        dev[f"intr{m}"] = data[f"intr{m}"]
    with torch.no_grad():
        result = model(dev)
    result = {k: v.clone() for k, v in result.items()}
    for i, j in ((0, 4), (1, 3)):
        m = result[f"matches{i}_{i}_{j}"]
        matched = torch.nonzero(m[1] >= 0)[:, 0]
        assert len(matched) > 8
        m[1, matched[3:]] = -1
    return dev, result


@pytest.mark.parametrize("init", ["host", "device"])
def test_whole_path_with_tracks(gpu, two_tuples, init):
    """``solve_tuple_poses_batch(5, ..., tracks=True)``: finite [2, 5, 4, 4]; the batch is each element alone, bit for bit, and
    equal run to run; fewer observations than the pairwise problem; pose errors against ground truth through
    ``eval_bundle_adjust_batch(..., tracks=True)`` at the bars of the existing whole-path tests (max below 2.0 degrees, AUC@5
    above 0.8), the figures of ``tracks=False`` printed beside them."""
    from e2e_multi_view_matching_amd import multi_view, pose_auc
    dev, result = two_tuples
    tm = {}
    whole = multi_view.solve_tuple_poses_batch(5, dev, result, init=init, tracks=True, timings=tm)
    assert sorted(tm) == ["build_and_bundle_adjust", "collect", "initialisation", "relative_poses"]
    assert whole.shape == (2, 5, 4, 4) and whole.dtype == np.float64 and np.isfinite(whole).all()
    assert np.array_equal(whole, multi_view.solve_tuple_poses_batch(5, dev, result, init=init, tracks=True))  # run to run
    for b in range(2):
        alone = multi_view.solve_tuple_poses_batch(5, _slice(dev, b), _slice(result, b), init=init, tracks=True)
        assert np.array_equal(alone[0], whole[b]), (b, np.abs(alone[0] - whole[b]).max())
    stats = multi_view.match_tracks(5, dev, result)[1].cpu().numpy()
    counts = multi_view._collect_matches_batch(5, dev, result, 0.)[3].cpu().numpy().reshape(2, 10)
    print("tracks / observations / conflicts / edges per tuple:", stats.tolist(), " pairwise observations:", (2 * counts.sum(1)).tolist())
    assert (stats[:, 3] == counts.sum(1)).all() and (stats[:, 1] < 2 * counts.sum(1)).all() and (stats[:, 0] > 0).all()
    assert not np.array_equal(whole, multi_view.solve_tuple_poses_batch(5, dev, result, init=init))
    figures = {}
    for tracks in (False, True):
        e = np.array(multi_view.eval_bundle_adjust_batch(5, dev, result, [[], [], []], init=init, tracks=tracks)[0])
        figures[tracks] = (e, pose_auc(e, [5, 10, 20]))
        print("init", init, "tracks", tracks, "pose errors (degrees): max", e.max(), "mean", e.mean(), "auc", figures[tracks][1])
    e, auc = figures[True]
    assert len(e) == 2 * 10 and e.max() < 2.0 and auc[0] > 0.8, (e, auc)
