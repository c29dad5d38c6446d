"""CPU guard on which translation unit compiles which kernel, and on what the build believes each unit is made from.  Reads the
objects build() leaves under gpslam_amd/lib/obj with the LLVM tools next to hipcc (scripts/code_objects.py; without them this fails,
it does not skip) and the dependency lists build.py records from the compiler's depfiles.  A launcher of the level-0 forms that finds
its way back into a shared header puts them into every object again, and fails here."""
import importlib.util
import os

import pytest

import test_gpu_forms as F
from gpslam_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = {"_ZN3gps14k_fused_level0ILi%dE%sLi%dELb%dEEEvNS_9FusedArgsIdT0_EE" % (sv, tr[0], b, dg) for sv, tr, b, dg in F.FUSED_FORMS}
ROWS = {"_ZN3gps20k_chunk_forward_rowsILi%dEEEvNS_7FwdArgsIdEE" % b for b in (4, 6, 12)} | {"_ZN3gps21k_chunk_backward_rowsILi%dEEEvNS_7BwdArgsIdEE" % b for b in (4, 6, 12)}
LINES = {"_ZN3gps11k_gps_linesILi2ELb%dEEEvNS_8MeasArgsIdEE" % aux for aux in (0, 1)}


@pytest.fixture(scope="module")
def homes(tmp_path_factory):
    """{kernel: the objects that hold it} of the product build"""
    B.build()
    spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = {}
    for r in tool.dump(B.OBJDIR, str(tmp_path_factory.mktemp("co"))):
        out.setdefault(r["kernel"], set()).add(r["object"])
    return out


def deps(src):
    B.build()
    return B._deps(B._obj(src))


def test_the_level0_forms_are_compiled_by_level0_alone(homes):
    assert len(FUSED) == 12 and len(ROWS) == 6
    named = {k for k in homes if "k_fused_level0" in k or "k_chunk_forward_rows" in k or "k_chunk_backward_rows" in k}
    assert named == FUSED | ROWS, sorted(named ^ (FUSED | ROWS))
    assert {k: homes[k] for k in named} == {k: {"level0.o"} for k in named}


def test_the_gps_lines_are_compiled_by_the_fp64_half_alone(homes):
    named = {k for k in homes if "k_gps_lines" in k}
    assert named == LINES, sorted(named ^ LINES)
    assert {k: homes[k] for k in named} == {k: {"api_impl64.o"} for k in named}


def test_upper_is_made_from_its_own_five_files():
    assert deps("upper.hip") == sorted("gpslam_amd/csrc/" + f for f in ("upper.hip", "upper.hpp", "dpp.hpp", "cr_step.hpp", "cr_quad.hpp"))


def test_level0_hpp_is_read_by_level0_hip_alone():
    assert [s for s in B.SOURCES if "gpslam_amd/csrc/level0.hpp" in deps(s)] == ["level0.hip"]


def test_the_depfile_reader_keeps_the_project_files_normalised():
    text = ("/r/gpslam_amd/lib/obj/api.o.tmp7: /r/gpslam_amd/csrc/api.hip \\\n"
            "  /opt/rocm/lib/llvm/lib/clang/19/include/__clang_hip_runtime_wrapper.h \\\n"
            "  api_common.hpp /r/gpslam_amd/csrc/../../include/gpslam_hip.h \\\n"
            "  ../../include/gpslam_hip_qc.h /usr/include/c++/13/vector kernels.hpp \\\n"
            "  /r/gpslam_amd/csrc/api_common.hpp /r-elsewhere/x.hpp\n")
    assert B.read_depfile(text, cwd="/r/gpslam_amd/csrc", root="/r") == [
        "gpslam_amd/csrc/api.hip", "gpslam_amd/csrc/api_common.hpp", "gpslam_amd/csrc/kernels.hpp", "include/gpslam_hip.h", "include/gpslam_hip_qc.h"]
