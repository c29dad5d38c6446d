"""tests/cpp/d3_branch_host_tests.cpp: lie.hpp / factors.hpp compiled by hipcc's host pass, the d = 3 GP prior, interpolator and
prior / between factors evaluated on every case of tests/golden/d3_branch_pins.json within its tolerance.  Runs on the CPU: a wrong
branch or sign in the device source shows here before any GPU run."""
import os
import subprocess

import d3_branch_refs as D

ROOT = os.path.dirname(D.HERE)
WHAT = {"gp": 0, "interp": 1, "prior": 2, "between": 3}
INPUTS = {"gp": ("p1", "v1", "p2", "v2", "dt"), "interp": ("p1", "v1", "p2", "v2", "dt", "tau"), "prior": ("m", "x"),
          "between": ("m", "x1", "x2")}


def case_lines(pins):
    for fam, cases in pins["families"].items():
        kind, what, chart = D.FAMILIES[fam]
        for c in cases:
            x = [v for key in INPUTS[what] for v in (c["inputs"][key] if isinstance(c["inputs"][key], list) else [c["inputs"][key]])]
            pin, tol = D.pin_of(c), D.tol_of(c)
            yield " ".join([str(kind), str(WHAT[what]), str(chart), str(len(x))] + [repr(float(v)) for v in x] + [str(len(pin))] +
                           [repr(float(v)) for v in pin] + [repr(float(v)) for v in tol])


def test_device_source_in_the_host_pass_meets_every_pin(tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "d3_branch_host_tests")
    src = exe + ".cpp"
    deps = [src] + [os.path.join(ROOT, "gpslam_amd", "csrc", h) for h in ("factors.hpp", "lie.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", src, "-o", exe])
    pins = D.load_pins()
    lines = list(case_lines(pins))
    assert len(lines) == sum(len(c) for c in pins["families"].values())
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr
    assert "all d3 branch host tests passed (%d cases)" % len(lines) in out.stdout
