"""CPU: what ``tracks=True`` refuses is refused on the host, before any device call (so also on a machine without a GPU)."""
import pytest
import torch


def _per_image(T=3, N=4):
    return {f"keypoints{t}": torch.zeros(1, N, 2) for t in range(T)}


@pytest.mark.parametrize("method", ["ransac", "ransac_ba"])
def test_tracks_need_the_w8pt_ba_relative_poses(method):
    """The RANSAC methods filter compacted rows that no longer carry keypoint indices."""
    from e2e_multi_view_matching_amd import multi_view
    with pytest.raises(ValueError, match="w8pt_ba"):
        multi_view.solve_tuple_poses_batch(3, _per_image(), {}, rel_pose_method=method, tracks=True)
    with pytest.raises(ValueError, match="w8pt_ba"):
        multi_view.eval_bundle_adjust_batch(3, _per_image(), {}, [[], [], []], rel_pose_method=method, tracks=True)


def test_tracks_need_per_image_keypoints():
    """With per-pair ``keypoints{i}_{i}_{j}`` entries only, a keypoint has no identity across pairs."""
    from e2e_multi_view_matching_amd import multi_view
    data = {}
    for j in range(3):
        for i in range(j):
            data[f"keypoints{i}_{i}_{j}"] = torch.zeros(1, 4, 2)
            data[f"keypoints{j}_{i}_{j}"] = torch.zeros(1, 4, 2)
    result = {f"matches{i}_{i}_{j}": torch.zeros(1, 4, dtype=torch.int64) for j in range(3) for i in range(j)}
    for init in ("host", "device"):
        with pytest.raises(ValueError, match="per-image"):
            multi_view.solve_tuple_poses_batch(3, data, result, init=init, tracks=True)
    with pytest.raises(ValueError, match="per-image"):
        multi_view.eval_bundle_adjust_batch(3, data, result, [[], [], []], tracks=True)
    with pytest.raises(ValueError, match="per-image"):
        multi_view.match_tracks(3, data, result)
    partly = dict(data, keypoints0=torch.zeros(1, 4, 2))  # one image is not enough
    with pytest.raises(ValueError, match=r"images \[1, 2\]"):
        multi_view.solve_tuple_poses_batch(3, partly, result, tracks=True)
