"""CPU guard on the table of k_fused_level0 instantiations: the launch statements of launch_fused_k (level0.hip), the list
tests/test_gpu_forms.py keeps (FUSED_FORMS) and the forms its rows expect must be the same set.  A thirteenth instantiation without a
row, a dropped one, or a row that goes missing fails here, without a GPU."""
import os
import re

import test_gpu_forms as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch_statements():
    """(SV, TR, B, DG) of every GPS_FUSED_LAUNCH(k_fused_level0<...>) statement, the template's defaults (level0.hpp:
    template <int SV, typename TR = double, int B = 12, bool DG = false>) filled in where a statement leaves them out"""
    with open(os.path.join(ROOT, "gpslam_amd", "csrc", "level0.hip")) as f:
        src = f.read()
    found = []
    for args in re.findall(r"GPS_FUSED_LAUNCH\(\s*k_fused_level0<([^>]*)>\s*\)", src):
        a = [x.strip() for x in args.split(",")]
        assert 1 <= len(a) <= 4, args
        a += ["double", "12", "false"][len(a) - 1:]
        assert a[1] in ("double", "float") and a[3] in ("true", "false"), args
        found.append((int(a[0]), a[1], int(a[2]), a[3] == "true"))
    return found


def test_the_template_defaults_are_the_ones_this_file_fills_in():
    with open(os.path.join(ROOT, "gpslam_amd", "csrc", "level0.hpp")) as f:
        src = f.read()
    assert re.search(r"template <int SV, typename TR = double, int B = 12, bool DG = false>\s*\n__global__ void __launch_bounds__\([^)]*\) k_fused_level0\(", src)


def test_launch_statements_table_and_rows_are_one_set():
    found = launch_statements()
    assert len(found) == len(set(found)) == 12, sorted(found)          # no instantiation is launched from two statements
    assert len(F.FUSED_FORMS) == len(set(F.FUSED_FORMS))
    assert set(found) == set(F.FUSED_FORMS), (sorted(set(found) ^ set(F.FUSED_FORMS)))
    assert F.expected_forms() == set(F.FUSED_FORMS), sorted(F.expected_forms() ^ set(F.FUSED_FORMS))


def test_every_row_that_expects_a_fused_launch_names_its_form_consistently():
    for r in F.ROWS + F.FP32_ROWS:
        e = r.expect
        if e.get("l0_fused"):
            assert r.form == (e["sv"], "float" if e["fp32"] else "double", e["block"], bool(e["dg"])), r.id
        else:
            assert r.form is None and e.get("sv", -1) == -1, r.id
    ids = [r.id for r in F.ROWS + F.FP32_ROWS]
    assert len(ids) == len(set(ids))
