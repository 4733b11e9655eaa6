"""The repair stage of the track merging, as far as it can be checked without a GPU: the C entry point is declared, bound and
exported with matching argument counts, the ``repair_rounds`` keyword exists with the default 0 on every function that takes it,
and what it refuses is refused on the host before any device call."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "e2emv_mv_tracks_repair"


def _per_image(T=3, N=4):
    return {f"keypoints{t}": torch.zeros(1, N, 2) for t in range(T)}


def test_header_declares_and_library_exports_the_repair_entry(lib_built):
    from e2e_multi_view_matching_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "e2emv.h")).read()
    assert NAME in set(re.findall(r"\b(e2emv_[a-z0-9_]+)\s*\(", hdr))
    assert NAME in _lib.SIGNATURES and hasattr(ctypes.CDLL(lib_built), NAME)
    decl = re.search(r"int %s\((.*?)\);" % NAME, hdr, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[NAME][1]) == len(_lib.SIGNATURES["e2emv_mv_tracks"][1]) + 1
    assert re.search(r"\bint rounds\b", decl)


def test_null_context_is_rejected(lib_built):
    from e2e_multi_view_matching_amd import _lib
    assert _lib.load_library().e2emv_mv_tracks_repair(None, 1, 3, 4, None, None, None, 1, 0.0, 1, None, None, None) == _lib.EINVAL


@pytest.mark.parametrize("name", ["match_tracks", "_tracks_ba_call", "_tuple_problems_tracks", "solve_tuple_poses_batch", "eval_bundle_adjust_batch"])
def test_repair_rounds_defaults_to_no_repair(name):
    from e2e_multi_view_matching_amd import multi_view
    sig = inspect.signature(getattr(multi_view, name))
    assert "repair_rounds" in sig.parameters and sig.parameters["repair_rounds"].default == 0


@pytest.mark.parametrize("rounds", [-1, 65, 1.5, True, "2", None])
def test_repair_rounds_outside_0_to_64_is_a_value_error_before_any_device_call(rounds):
    """Empty ``result``: a call that got past the check would fail on the missing matches with another message."""
    from e2e_multi_view_matching_amd import multi_view
    data = _per_image()
    with pytest.raises(ValueError, match="repair_rounds"):
        multi_view.match_tracks(3, data, {}, repair_rounds=rounds)
    with pytest.raises(ValueError, match="repair_rounds"):
        multi_view._tracks_ba_call("e2emv_mv_tuple_ba_tracks", 3, data, {}, 0.0, None, 3, 1, None, repair_rounds=rounds)
    with pytest.raises(ValueError, match="repair_rounds"):
        multi_view._tuple_problems_tracks(3, data, {}, 0.0, None, 3, 1, None, repair_rounds=rounds)
    for init in ("host", "device"):
        with pytest.raises(ValueError, match="repair_rounds"):
            multi_view.solve_tuple_poses_batch(3, data, {}, init=init, tracks=True, repair_rounds=rounds)
    with pytest.raises(ValueError, match="repair_rounds"):
        multi_view.eval_bundle_adjust_batch(3, data, {}, [[], [], []], tracks=True, repair_rounds=rounds)


def test_repair_needs_tracks():
    from e2e_multi_view_matching_amd import multi_view
    with pytest.raises(ValueError, match="tracks=True"):
        multi_view.solve_tuple_poses_batch(3, _per_image(), {}, repair_rounds=2)
    with pytest.raises(ValueError, match="tracks=True"):
        multi_view.eval_bundle_adjust_batch(3, _per_image(), {}, [[], [], []], tracks=False, repair_rounds=2)
