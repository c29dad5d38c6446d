"""CPU: the entry points of the pair marginals and the closure gate (added without an ABI bump) are exported by the built library,
declared in include/gpslam_hip.h, listed in its "added since without a bump" note and wrapped by the Python binding; the library
still reports ABI 2.4; a NULL handle answers GPSLAM_E_INVALID without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gpslam_hip_marginals_keep_pair_terms", "gpslam_hip_get_state_pair_marginals", "gpslam_hip_gate_between_pairs"]
WRAPPERS = ["marginals_keep_pair_terms", "get_state_pair_marginals", "gate_between_pairs"]


def test_library_header_and_binding_agree_on_the_new_entry_points():
    import gpslam_amd
    from gpslam_amd import chain
    lib = gpslam_amd.load_library()
    with open(os.path.join(ROOT, "include", "gpslam_hip.h")) as f:
        header = f.read()
    for s, w in zip(SYMBOLS, WRAPPERS):
        assert hasattr(lib, s), s
        assert re.search(r"^int %s\(gpslam_hip_handle \*h," % s, header, re.M), s
        assert s in chain.ABI_SYMBOLS, s
        assert callable(getattr(chain.ChainSolver, w, None)), w
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)
    assert (chain.ABI_MAJOR, chain.ABI_MINOR) == (2, 4)
    assert "#define GPSLAM_HIP_ABI_MINOR 4" in header
    m = re.search(r"added since without a bump,(.*?)\)\.", header, re.S)
    assert m and all(s in m.group(1) for s in SYMBOLS)
    assert "N * b * m doubles" in header          # the opt-in states what it costs


def test_null_handle_is_invalid():
    import gpslam_amd
    lib = gpslam_amd.load_library()
    assert lib.gpslam_hip_marginals_keep_pair_terms(None, 1) == -1
    assert lib.gpslam_hip_get_state_pair_marginals(None, 0, None, None, None) == -1
    assert lib.gpslam_hip_gate_between_pairs(None, 0, None, None, None, None, None, None, None) == -1
