"""The matcher's recoding plan (cv_amd/csrc/hm_plan.h: which descriptor blocks a k-NN call recodes, and where every problem
finds them) is host arithmetic that enqueues nothing: tests/cpp/hm_plan.cpp, a stand-alone program, holds it to its
properties without a GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_recoding_plan(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "the plan's test needs a host C++ compiler"
    exe = str(tmp_path / "hm_plan")
    # the header alone: no HIP include path, no library
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "hm_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "all plans hold" and not any(l.startswith("FAILED") for l in lines)
    for case, jobs in (("no problems", 0), ("n problems over one block pair", 2), ("one buffer, same count and capacity", 1),
                       ("one buffer, another count", 2), ("one buffer, another capacity", 2), ("symmetric pairs", 2),
                       ("window of 64 x 32 problems over 96 blocks", 96)):
        hits = [l for l in lines if l.startswith(f"ok {case}:")]
        assert hits and all(f" {jobs} jobs," in l for l in hits), (case, hits)
