"""The entry points of fixed-lag smoothing with landmarks exist in the library, the header and the Python binding, and the ABI version
has not moved: CPU only."""
import ctypes as C
import os

import gpslam_amd as gp
from gpslam_amd import build as B
from gpslam_amd import chain

NAMES = ["gpslam_hip_add_border_gaussians", "gpslam_hip_get_border_gaussians", "gpslam_hip_marginalize_head_onto_landmarks",
         "gpslam_hip_get_head_prior_border"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_in_library_header_and_binding():
    lib = C.CDLL(B.build())
    header = open(os.path.join(ROOT, "include", "gpslam_hip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert "int %s(gpslam_hip_handle *h" % n in header, n
        assert n in chain.ABI_SYMBOLS, n
    par = header[header.index("added since without a bump"):header.index("A MAJOR bump")]
    for n in NAMES:
        assert n in par, n
    flat = header.replace("\n * ", " ").replace("\n", " ")
    assert "Border Gaussians (gpslam_hip_add_border_gaussians) have no rows here" in flat      # said at get_rows
    assert "gpslam_hip_marginalize_head_onto_landmarks (below) lifts it" in flat               # ... and at marginalize_head


def test_wrappers_are_callable():
    for m in ("add_border_gaussians", "get_border_gaussians", "marginalize_head_onto_landmarks", "get_head_prior_border"):
        assert callable(getattr(gp.ChainSolver, m)), m


def test_abi_version_is_still_2_4():
    lib = C.CDLL(B.build())
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)
    assert (chain.ABI_MAJOR, chain.ABI_MINOR) == (2, 4)


def test_null_handle_is_invalid():
    lib = C.CDLL(B.build())
    assert lib.gpslam_hip_add_border_gaussians(None, 0, None, None, None, None, None, None) == -1
    assert lib.gpslam_hip_get_border_gaussians(None, None, None, None, None, None, None) == -1
    assert lib.gpslam_hip_marginalize_head_onto_landmarks(None, 1) == -1
    assert lib.gpslam_hip_get_head_prior_border(None, None, None, None) == -1
