"""CPU guard on which translation unit compiles which kernel, and on what the build believes each unit is made from.  Reads the
objects build() leaves under gpslam_amd/lib/obj with the LLVM tools next to hipcc (scripts/code_objects.py; without them this fails,
it does not skip) and the dependency lists build.py records from the compiler's depfiles.  A launcher of the level-0 forms that finds
its way back into a shared header puts them into every object again, and fails here."""
import importlib.util
import os
import re

import pytest

import test_gpu_forms as F
from gpslam_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = {"_ZN3gps14k_fused_level0ILi%dE%sLi%dELb%dEEEvNS_9FusedArgsIdT0_EE" % (sv, tr[0], b, dg) for sv, tr, b, dg in F.FUSED_FORMS}
ROWS = {"_ZN3gps20k_chunk_forward_rowsILi%dEEEvNS_7FwdArgsIdEE" % b for b in (4, 6, 12)} | {"_ZN3gps21k_chunk_backward_rowsILi%dEEEvNS_7BwdArgsIdEE" % b for b in (4, 6, 12)}
LINES = {"_ZN3gps11k_gps_linesILi2ELb%dEEEvNS_8MeasArgsIdEE" % aux for aux in (0, 1)}


# every kernel of the segmented landmark elimination (fatsep.hpp), as the two precision halves held them before fatsep.hip existed: the
# names of api_impl64.o and api_impl32.o, taken once from that build -- k_fs_factor_rows6 under the name it has as a plain kernel
FATSEP = {
    "_ZN3gps10k_fs_sweepIdLi12EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps10k_fs_sweepIdLi12EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps10k_fs_sweepIdLi4EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps10k_fs_sweepIdLi4EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps10k_fs_sweepIdLi6EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps10k_fs_sweepIdLi6EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_factorIdLi12EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_factorIdLi12EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_factorIdLi4EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_factorIdLi4EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_factorIdLi6EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_factorIdLi6EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_solve1IdLi12EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_solve1IdLi12EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_solve1IdLi4EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_solve1IdLi4EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_solve1IdLi6EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps11k_fs_solve1IdLi6EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps12k_fat_updateIddEEvNS_6FsArgsIT_T0_EENS_8FatLevelE",
    "_ZN3gps12k_fat_updateIdfEEvNS_6FsArgsIT_T0_EENS_8FatLevelE",
    "_ZN3gps12k_fs_scatterIddEEvNS_6FsArgsIT_T0_EE",
    "_ZN3gps12k_fs_scatterIdfEEvNS_6FsArgsIT_T0_EE",
    "_ZN3gps13k_fat_back_w4IdEEvNS_6FsArgsIdT_EENS_8FatLevelE",
    "_ZN3gps13k_fat_back_w4IfEEvNS_6FsArgsIdT_EENS_8FatLevelE",
    "_ZN3gps13k_fs_lm_termsIddEEvNS_6FsArgsIT_T0_EE",
    "_ZN3gps13k_fs_lm_termsIdfEEvNS_6FsArgsIT_T0_EE",
    "_ZN3gps13k_fs_mask_mulIdEEvPKT_PKiiiPS1_",
    "_ZN3gps13k_fs_max_intoIdEEvPKT_iPd",
    "_ZN3gps13k_fs_top_takeIddEEvNS_6FsArgsIT_T0_EEPKS2_ii",
    "_ZN3gps13k_fs_top_takeIdfEEvNS_6FsArgsIT_T0_EEPKS2_ii",
    "_ZN3gps14k_fs_lm_updateIdEEvPdPKT_iPKiPS2_",
    "_ZN3gps14k_fs_top_buildIdEEvPKT_iiPS1_S4_S4_",
    "_ZN3gps15k_fat_back_rowsILi16EdEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_back_rowsILi16EfEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_back_rowsILi24EdEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_back_rowsILi24EfEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_back_rowsILi32EdEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_back_rowsILi32EfEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_back_rowsILi40EdEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_back_rowsILi40EfEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_back_rowsILi48EdEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_back_rowsILi48EfEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_mfmaIdEEvNS_6FsArgsIdT_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_mfmaIfEEvNS_6FsArgsIdT_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi16EdEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi16EfEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi24EdEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi24EfEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi32EdEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi32EfEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi40EdEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi40EfEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi48EdEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi48EfEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi8EdEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fat_elim_rowsILi8EfEEvNS_6FsArgsIdT0_EENS_8FatLevelE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi2EdEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi2EfEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi3EdEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi3EfEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi4EdEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi4EfEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi5EdEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi5EfEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi6EdEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi6EfEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi7EdEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps15k_fs_sweep_syrkILi6ELi7EfEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps16k_fs_lmprior_errIdEEvPKdPKiS2_S2_iiPT_",
    "_ZN3gps16k_fs_lmprior_errIfEEvPKdPKiS2_S2_iiPT_",
    "_ZN3gps16k_fs_pack_recordIddEEvNS_6FsArgsIT_T0_EEiiPS2_",
    "_ZN3gps16k_fs_pack_recordIdfEEvNS_6FsArgsIT_T0_EEiiPS2_",
    "_ZN3gps17k_fs_factor_rows6ENS_6FsArgsIddEE",
    "_ZN3gps17k_fs_fat_assembleIddEEvNS_6FsArgsIT_T0_EE",
    "_ZN3gps17k_fs_fat_assembleIdfEEvNS_6FsArgsIT_T0_EE",
    "_ZN3gps20k_fat_elim_wide_mfmaIdEEvNS_6FsArgsIdT_EENS_8FatLevelEi",
    "_ZN3gps20k_fat_elim_wide_mfmaIfEEvNS_6FsArgsIdT_EENS_8FatLevelEi",
    "_ZN3gps8k_fs_gevIdLi12EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps8k_fs_gevIdLi12EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps8k_fs_gevIdLi4EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps8k_fs_gevIdLi4EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps8k_fs_gevIdLi6EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps8k_fs_gevIdLi6EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps8k_fs_rhsIdLi12EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps8k_fs_rhsIdLi12EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps8k_fs_rhsIdLi4EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps8k_fs_rhsIdLi4EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps8k_fs_rhsIdLi6EdEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps8k_fs_rhsIdLi6EfEEvNS_6FsArgsIT_T1_EE",
    "_ZN3gps9k_fat_topIddEEvNS_6FsArgsIT_T0_EEi",
    "_ZN3gps9k_fat_topIdfEEvNS_6FsArgsIT_T0_EEi",
    "_ZN3gps9k_fs_syrkILi12ELi144EdEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps9k_fs_syrkILi12ELi144EfEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps9k_fs_syrkILi17ELi176EdEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps9k_fs_syrkILi17ELi176EfEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps9k_fs_syrkILi20ELi272EdEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps9k_fs_syrkILi20ELi272EfEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps9k_fs_syrkILi7ELi112EdEEvNS_6FsArgsIdT1_EE",
    "_ZN3gps9k_fs_syrkILi7ELi112EfEEvNS_6FsArgsIdT1_EE",
}


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


def test_the_segmented_path_is_compiled_by_fatsep_alone(homes):
    named = {k for k in homes if "k_fs_" in k or "k_fat_" in k}
    assert {k: homes[k] for k in named} == {k: {"fatsep.o"} for k in named}


def test_the_segmented_path_has_the_kernels_the_precision_halves_had(homes):
    assert len(FATSEP) == 99
    named = {k for k in homes if "k_fs_" in k or "k_fat_" in k}
    assert named == FATSEP, sorted(named ^ FATSEP)


def test_fatsep_hpp_is_read_by_fatsep_hip_alone():
    assert [s for s in B.SOURCES if "gpslam_amd/csrc/fatsep.hpp" in deps(s)] == ["fatsep.hip"]


def test_the_precision_halves_launch_no_kernel_of_the_segmented_path():
    """read as text: a launch statement names its kernel in front of <<< (comments may speak of the kernels)"""
    for inc in ("api_impl.inc", "api_iterate.inc"):
        with open(os.path.join(B.CSRC, inc)) as f:
            code = [line.split("//")[0] for line in f]
        assert [line for line in code if re.search(r"\bk_(fs|fat)_[^;]*<<<", line)] == [], inc
