"""The device form of the multi-view global initialisation, as far as it can be checked without a GPU: the two C entry points
are declared, bound and exported with matching argument counts, and the ``init`` switch of the batched path exists, defaults
to the host code and rejects anything but "host" / "device" before any device work."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("e2emv_mv_init_batch", "e2emv_mv_tuple_init")


def test_header_declares_and_library_exports_the_device_initialisation(lib_built):
    from e2e_multi_view_matching_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "e2emv.h")).read()
    declared = set(re.findall(r"\b(e2emv_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(lib_built)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    from e2e_multi_view_matching_amd import build
    assert "mvinit_device.hip" in build.SOURCES


def test_null_context_is_rejected(lib_built):
    from e2e_multi_view_matching_amd import _lib
    lib = _lib.load_library()
    assert lib.e2emv_mv_init_batch(None, 1, None, None, None, None, None, None, None, None, None, None) == _lib.EINVAL
    assert lib.e2emv_mv_tuple_init(None, 1, 5, None, None, None, 8, 20, None, None, None) == _lib.EINVAL


@pytest.mark.parametrize("name", ["solve_tuple_poses_batch", "eval_bundle_adjust_batch"])
def test_init_parameter_defaults_to_the_host_path(name):
    from e2e_multi_view_matching_amd import multi_view
    sig = inspect.signature(getattr(multi_view, name))
    assert "init" in sig.parameters and sig.parameters["init"].default == "host"


def test_unknown_init_is_a_value_error_before_any_device_work():
    from e2e_multi_view_matching_amd import multi_view
    with pytest.raises(ValueError, match="init"):
        multi_view.solve_tuple_poses_batch(5, {}, {}, init="nonsense")
    with pytest.raises(ValueError, match="init"):
        multi_view.eval_bundle_adjust_batch(5, {}, {}, [[], [], []], init="nonsense")
    assert callable(multi_view.averaged_extrinsics_batch)
