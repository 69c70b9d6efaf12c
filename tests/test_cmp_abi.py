"""The names he_cmp / he_cmppt add to the C ABI are declared where they belong, exported and bound: tests/test_abi.py's checks for
include/gpqhe_hip_algo.h's and include/gpqhe_hip_compat.h's new names.  No device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_names_are_declared_exported_and_bound():
    """tests/test_abi.py's checks for the names this surface adds (they fail where the library does not have them)"""
    import ctypes as C
    from gpqhe_amd import _native
    header = open(os.path.join(ROOT, "include", "gpqhe_hip_compat.h")).read()
    algo = open(os.path.join(ROOT, "include", "gpqhe_hip_algo.h")).read()
    lib = C.CDLL(_native.LIB_PATH)
    for name in ("gpq_shim_he_cmp", "gpq_shim_he_cmppt"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert hasattr(lib, name) and name in _native.EXPORTED_ONLY, name
    for name in ("gpq_he_lin_pt", "gpq_he_cmp_rounds", "gpq_he_cmp_depth", "gpq_he_cmp_workspace_bytes", "gpq_he_cmp", "gpq_he_cmppt"):
        assert re.search(r"^(int|size_t) %s\(" % name, algo, re.M), name
        assert hasattr(lib, name) and name in _native.SIGNATURES, name
    core = open(os.path.join(ROOT, "include", "gpqhe_hip.h")).read()
    assert "gpq_he_cmp" not in core and "gpq_he_lin_pt" not in core      # the pinned set of `void *stream` functions there stays as it is
