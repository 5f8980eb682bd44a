"""What the observation-table stages decide on the host before they enqueue anything (cv_amd/csrc/rs_table_host.h: the overlap
rule, the view-list check, the scratch plan) is host code without a HIP type in it: tests/cpp/table_host.cpp, a stand-alone
program built with a plain C++ compiler and -fsanitize=address,undefined, holds it to its properties."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_overlap_rule_view_list_and_scratch_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "table_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "table_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "the table stages' host half holds" and not any(l.startswith("FAILED") for l in lines)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    assert lines[0].startswith("overlap: 900 pairs, ")
