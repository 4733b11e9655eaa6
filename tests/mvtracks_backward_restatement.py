"""TEST INFRASTRUCTURE: torch fp64 restatement of the weights the track route hands the solver (mv_tracks_emit_kernel, csrc/mvtracks.hip),
differentiable by autograd, and the closed form of its adjoint that mv_tracks_weights_backward_kernel implements.  Shared by
tests/test_mv_tracks_backward.py (CPU) and tests/test_gpu_mv_tracks_backward.py (device).  The solver itself is
tests/mvba_backward_restatement.py, imported by the tests and not copied.

Order and arithmetic are those of ``host_problem`` in tests/test_gpu_mv_tracks.py: points = tracks in ascending label, the observations
of a point in ascending node id (= ascending image); the confidence of a node = the fp64 mean of the kept ORIGINAL edges between it and
the other members of its track, other member ascending; weights = confidence / (0.5 (sum + 1e-3)), both components.

Everything discrete is an INPUT and carries no gradient: the labels (of ``host_labels``, ``host_repair`` or the device), the edge list
(the keep rule already applied) and which edges were cut (the weights do not see the cuts: labels are the only interface)."""
import numpy as np
import torch

from test_gpu_mv_tracks import _pairs, host_edges


def kept_edges(T, data, result, b, conf_thresh):
    """Kept edges of batch element ``b`` as a list ``(q, n, x, y)``: row ``n`` of pair ``q`` (``_pairs`` order) joins nodes ``x < y``
    (node = ``t * Nmax + n``); and ``Nmax``.  The keep rule of ``mv_edge``: ``0 <= match < n_kpts_j`` and every confidence channel
    ``> conf_thresh`` as floats.  The selection is that of ``host_edges`` (asserted)."""
    n_img = [data[f"keypoints{t}"].shape[1] for t in range(T)]
    Nmax = max(n_img)
    edges = []
    for q, (i, j) in enumerate(_pairs(T)):
        if f"matches{i}_{i}_{j}" not in result:
            continue
        m = result[f"matches{i}_{i}_{j}"][b].cpu().numpy()
        c = result[f"conf_scores_{i}_{j}"][b].detach().cpu().numpy().astype(np.float32).reshape(len(m), -1)
        keep = (m >= 0) & (m < n_img[j]) & (c > np.float32(conf_thresh)).all(1)
        edges += [(q, int(n), i * Nmax + int(n), j * Nmax + int(m[n])) for n in np.nonzero(keep)[0]]
    want, want_Nmax = host_edges(T, data, {k: v.detach() for k, v in result.items()}, b, conf_thresh)
    assert want_Nmax == Nmax and sorted(want) == sorted((x, y) for _, _, x, y in edges)
    return edges, Nmax


def confidences(T, result, b):
    """Per pair (``_pairs`` order) the confidences of element ``b`` as fp64 LEAF tensors [N, channels] (the fp32 values widened), ``None``
    for a pair without a ``matches`` entry."""
    out = []
    for i, j in _pairs(T):
        if f"matches{i}_{i}_{j}" not in result:
            out.append(None)
            continue
        c = result[f"conf_scores_{i}_{j}"][b].detach().cpu().float()
        out.append(c.reshape(c.shape[0], -1).double().requires_grad_())
    return out


def track_observations(label):
    """The observations in the order the emit kernel writes them: ``[(node, point)]``."""
    lab = np.asarray(label).reshape(-1)
    obs = []
    for p, r in enumerate(np.unique(lab[lab >= 0])):
        obs += [(int(x), p) for x in np.nonzero(lab == r)[0]]
    return obs


def observation_edges(label, edges):
    """Per observation the indices (into ``edges``) of E(o): the kept edges between its node and the other members of its track, other
    member ascending."""
    lab = np.asarray(label).reshape(-1)
    by_nodes = {(x, y): k for k, (_, _, x, y) in enumerate(edges)}
    assert len(by_nodes) == len(edges)
    out = []
    for x, _ in track_observations(label):
        members = np.nonzero(lab == lab[x])[0]
        out.append([by_nodes[(min(x, int(y)), max(x, int(y)))] for y in members if y != x and (min(x, int(y)), max(x, int(y))) in by_nodes])
    return out


def restated_weights(label, edges, conf):
    """labels [T, Nmax], the edge list and the confidence tensors -> ``obs_w [O, 2]`` fp64 (a graph to ``conf`` where it requires grad)."""
    E = observation_edges(label, edges)
    if not E:
        return torch.zeros(0, 2, dtype=torch.float64)
    c = []
    for ks in E:
        assert ks, "a node of a track has at least one kept edge inside it"
        s = 0.0
        for k in ks:
            q, n = edges[k][:2]
            s = s + conf[q][n, 0]
        c.append(s / len(ks))
    c = torch.stack(c)
    w = c / (0.5 * (c.sum() + 1e-3))
    return torch.stack([w, w], 1)


def closed_form(label, edges, conf, g_w):
    """The adjoint the device implements: ``g_w [O, 2]`` = dLoss/d(obs_w) -> per pair dLoss/d(conf) as numpy [N, channels] (``None`` for a
    pair without matches).  G_o = g_w[o].sum(), D = sum G_o w_o, cbar_o = (G_o - D / 2) / H, an edge gets cbar_o / e_o from each end."""
    E = observation_edges(label, edges)
    out = [None if c is None else np.zeros(tuple(c.shape)) for c in conf]
    if not E:
        return out
    val = [c.detach().numpy() if c is not None else None for c in conf]
    c_o = np.array([sum(float(val[edges[k][0]][edges[k][1], 0]) for k in ks) / len(ks) for ks in E])
    H = 0.5 * (c_o.sum() + 1e-3)
    w = c_o / H
    G = np.asarray(g_w, np.float64).sum(1)
    D = float((G * w).sum())
    cbar = (G - 0.5 * D) / H
    for o, ks in enumerate(E):
        for k in ks:
            q, n = edges[k][:2]
            out[q][n, 0] += cbar[o] / len(ks)
    return out


def autograd_form(label, edges, conf, g_w):
    """The same gradient by autograd through ``restated_weights``; a tensor the weights do not touch gets zeros."""
    w = restated_weights(label, edges, conf)
    have = [c for c in conf if c is not None]
    if not len(w):
        grads = [None] * len(have)
    else:
        grads = torch.autograd.grad((w * torch.as_tensor(np.asarray(g_w, np.float64))).sum(), have, allow_unused=True)
    it = iter(grads)
    return [None if c is None else (lambda g: np.zeros(tuple(c.shape)) if g is None else g.numpy())(next(it)) for c in conf]


def inside_tracks(label, edges):
    """Boolean per edge: both nodes carry the same label >= 0."""
    lab = np.asarray(label).reshape(-1)
    return np.array([lab[x] >= 0 and lab[x] == lab[y] for _, _, x, y in edges], bool)


# the graph of test_a_cut_edge_inside_its_final_track_still_weighs (tests/test_gpu_mv_track_repair.py) as (i, j, n, m, confidence)
CUT_GRAPH = [(0, 1, 0, 0, 0.9), (1, 2, 0, 0, 0.8), (0, 2, 0, 0, 0.1), (0, 1, 1, 0, 0.5)]
WRONG_SEED, WRONG_DROP = 38, 0.4


def wrong_and_thinned_scene(seed=WRONG_SEED, drop=WRONG_DROP):
    """``planted_scene(seed, wrong=0.1, T=5, n_kpts=24)`` with ``drop`` of each pair's rows then set to -1 (``default_rng(2000 + seed)``,
    pairs in ``_pairs`` order).  The planted scene alone joins every scene point through all ten pairs, so its tracks all have 5 views
    whatever the seed; thinned, it holds tracks of 2, 3, 4 and 5 views beside the conflicts of its wrong matches.  Seed 38 is chosen on
    the CPU (tests/test_mv_tracks_backward.py asserts it): without repair tracks of 2 .. 5 views and 4 dropped conflicts; after 4 rounds
    tracks of 2 .. 5 views, a cut edge inside its final track and cut edges between two tracks."""
    from test_gpu_mv_tracks import planted_scene
    data, result, gt, start = planted_scene(seed, wrong=0.1, T=5, n_kpts=24)
    rng = np.random.default_rng(2000 + seed)
    for i, j in _pairs(5):
        result[f"matches{i}_{i}_{j}"][0, torch.from_numpy(rng.uniform(size=24) < drop)] = -1
    return data, result, gt, start
