"""CPU: the entry points of the marginals on the segmented landmark path (added without an ABI bump) are exported by the built library,
declared in include/gpslam_hip.h and wrapped by the Python binding; the library still reports ABI 2.4."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gpslam_hip_marginals_on_segments", "gpslam_hip_get_landmark_marginals", "gpslam_hip_get_state_landmark_marginals",
           "gpslam_hip_get_landmark_pair_marginals"]
WRAPPERS = ["marginals_on_segments", "get_landmark_marginals", "get_state_landmark_marginals", "get_landmark_pair_marginals"]


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
    m = re.search(r"added since without a bump,(.*?)\)\.", header, re.S)
    assert m and all(s in m.group(1) for s in SYMBOLS)
