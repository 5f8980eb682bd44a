"""The rival bound of a symmetric match (cv_amd/csrc/hm_rule.h: the one text the decision kernel, the verification kernel and
the dispatcher share) is host arithmetic: tests/cpp/hm_rule.cpp, a stand-alone program, holds it to the reverse check it stands
in for, over every rule, forward distance and rival distance, without a GPU — plain, and under the address and
undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_rival_bound(tmp_path, sanitize):
    cxx = shutil.which("g++")
    assert cxx, "the bound's test needs a host C++ compiler"
    exe = str(tmp_path / "hm_rule")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    # the header alone: no HIP include path, no library
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra +
                          [os.path.join(ROOT, "tests", "cpp", "hm_rule.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "all bounds hold" and not any(l.startswith("FAILED") for l in lines)
    assert lines[-2].startswith("checked ") and int(lines[-2].split()[1]) > 5_000_000
