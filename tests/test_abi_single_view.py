"""The C ABI of the single-view refinement (include/akz.h): struct size, defaults, enum values and limits agree between akz.h,
cv_amd/_lib.py, include/akaze.hpp, the Rust text and the math header; the ABI number stays 11, since the entry points are pure
additions; the parameter refusals come back before any launch.  No GPU needed: the parameters are checked before anything
else, so the refusals are visible without a context."""
import ctypes as C
import os
import re
import subprocess

import pytest

from cv_amd import _lib
from cv_amd.single_view import VERDICTS, SingleViewRefiner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_single_view_params_default", "rs_refine_poses_batch_device", "hm_landmark_original_matches_batch_device")
CONSTANTS = ("RS_SV_OK", "RS_SV_NO_MODEL", "RS_SV_FEW_LANDMARKS", "RS_SV_LOST_HALF", "RS_SV_FEW_ROBUST", "RS_SV_BAD_INDEX", "RS_SV_MAX_MATCHES",
             "RS_SV_MAX_RUNS", "RS_SV_S_INLIERS", "RS_SV_S_RUN_MATCHES", "RS_SV_S_RUN_STOP", "RS_SV_S_ROBUST", "RS_SV_S_NO_OTHER", "RS_SV_S_STAGE",
             "RS_SV_STATS")


@pytest.fixture(scope="module")
def lib():
    from cv_amd.build import build
    build()
    return _lib.lib()


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def call(lib, prm):
    """rs_refine_poses_batch_device with no context and null buffers: only the parameter checks can answer"""
    return lib.rs_refine_poses_batch_device(None, None, 8, 1, None, None, None, None, 0, 0, None, 0, None, None, None, None, None, None, None,
                                            None, 1, C.byref(prm) if prm is not None else None, *([None] * 6))


def test_abi_number_stays_11(lib):
    hdr = read("include", "akz.h")
    assert int(re.search(r"#define\s+AKZ_ABI_VERSION\s+(\d+)u", hdr).group(1)) == 11
    assert lib.akz_abi_version() == 11 == _lib.ABI_VERSION
    rust = read("rust", "akaze-mi355x", "src", "lib.rs")
    assert re.search(r"ABI_VERSION: u32 = 11\b", rust)
    for name in NAMES:
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"fn %s\(" % name, rust), name
    hpp = read("include", "akaze.hpp")
    assert "class SingleViewRefiner" in hpp and "rs_refine_poses_batch_device(" in hpp


def test_the_ctypes_declarations_have_the_headers_argument_counts(lib):
    hdr = read("include", "akz.h")
    rust = read("rust", "akaze-mi355x", "src", "lib.rs")
    for name in NAMES:
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S).group(1).split(",")
        kinds = [bool(re.match(r"\s*uint32_t\s+\w+$", a)) for a in args]
        declared = getattr(lib, name).argtypes
        assert len(declared) == len(kinds), name
        assert [t is C.c_uint32 for t in declared] == kinds, name
        rargs = re.search(r"fn %s\(([^;]*?)\)\s*->\s*i32;" % name, rust, re.S).group(1).split(",")
        assert [bool(re.search(r":\s*u32$", a.strip())) for a in rargs] == kinds, name


def test_header_constants_are_the_bindings():
    hdr, math, rust = read("include", "akz.h"), read("include", "akz_single_view_math.h"), read("rust", "akaze-mi355x", "src", "lib.rs")
    for name in CONSTANTS:
        value = int(re.search(r"\b%s = (\d+)" % name, hdr).group(1))
        assert value == getattr(_lib, name), name
        assert int(re.search(r"\bAKZ_SV_%s = (\d+)" % name[6:], math).group(1)) == value, name
    assert re.search(r"RS_SV_MAX_ITERATIONS = 1 << 20", hdr) and _lib.RS_SV_MAX_ITERATIONS == 1 << 20
    for name in ("RS_SV_MAX_MATCHES", "RS_SV_MAX_RUNS", "RS_SV_STATS", "RS_SV_S_INLIERS", "RS_SV_S_RUN_MATCHES", "RS_SV_S_RUN_STOP", "RS_SV_S_ROBUST",
                 "RS_SV_S_NO_OTHER", "RS_SV_S_STAGE"):
        assert int(re.search(r"pub const %s: \w+ = (\d+);" % name, rust).group(1)) == getattr(_lib, name), name
    verdicts = re.search(r"pub enum SingleViewVerdict \{(.*?)\}", rust, re.S).group(1)
    assert [int(v) for v in re.findall(r"= (\d+)", verdicts)] == list(range(6)) == [getattr(_lib, n) for n in CONSTANTS[:6]]
    assert len(VERDICTS) == 6
    hpp = read("include", "akaze.hpp")
    for cpp, c in (("Ok", "RS_SV_OK"), ("NoModel", "RS_SV_NO_MODEL"), ("FewLandmarks", "RS_SV_FEW_LANDMARKS"), ("LostHalf", "RS_SV_LOST_HALF"),
                   ("FewRobust", "RS_SV_FEW_ROBUST"), ("BadIndex", "RS_SV_BAD_INDEX")):
        assert re.search(r"\b%s = %s\b" % (cpp, c), hpp), cpp


def test_defaults_are_the_references(lib):
    p = _lib.SingleViewParams()
    assert lib.rs_single_view_params_default(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(_lib.SingleViewParams) == 80
    assert p.single_view_optimization_num_matches == 2048 == _lib.RS_SV_MAX_MATCHES      # settings.rs:357-359
    assert p.single_view_filter_loop_iterations == 5                                     # settings.rs:361-363
    assert p.single_view_patience == 100000                                              # settings.rs:365-367
    assert p.single_view_optimization_rate == 1e-3                                       # settings.rs:373-375
    assert p.single_view_minimum_landmarks == 32 and p.single_view_minimum_robust_landmarks == 64   # settings.rs:377-383
    assert p.maximum_cosine_distance == 1e-5 and p.maximum_sine_distance == 1e-1         # settings.rs:324-330
    t = p.triangulate
    assert t.struct_size == C.sizeof(_lib.TriangulateParams) and t.max_sweeps == 1000 and t.eps == 1e-12
    assert lib.rs_single_view_params_default(None) == -1
    # the Rust struct has the same fields in the same order
    rust = re.search(r"pub struct RsSingleViewParams \{(.*?)\}", read("rust", "akaze-mi355x", "src", "lib.rs"), re.S).group(1)
    assert re.findall(r"(\w+): \w+,", rust) == [n for n, _ in _lib.SingleViewParams._fields_]
    fields = re.search(r"typedef struct rs_single_view_params \{(.*?)\} rs_single_view_params;", read("include", "akz.h"), re.S).group(1)
    assert re.findall(r"^\s*\w+ (\w+);", fields, re.M) == [n for n, _ in _lib.SingleViewParams._fields_]
    q = SingleViewRefiner.params(single_view_patience=7)
    assert q.single_view_patience == 7 and q.maximum_cosine_distance == 1e-5
    with pytest.raises(TypeError):
        SingleViewRefiner.params(patience=7)
    with pytest.raises(TypeError):
        SingleViewRefiner.params(struct_size=8)


def test_refusals_come_before_the_device(lib):
    assert call(lib, None) == -1                                        # AKZ_E_INVALID
    p = SingleViewRefiner.params()
    p.struct_size -= 4
    assert call(lib, p) == -1
    for kw in (dict(maximum_cosine_distance=float("nan")), dict(maximum_sine_distance=float("nan")),
               dict(single_view_optimization_rate=float("nan"))):
        assert call(lib, SingleViewRefiner.params(**kw)) == -1
    p = SingleViewRefiner.params()
    p.triangulate.max_sweeps = 0
    assert call(lib, p) == -1
    p = SingleViewRefiner.params()
    p.triangulate.struct_size = 8
    assert call(lib, p) == -1
    assert call(lib, SingleViewRefiner.params(single_view_optimization_num_matches=_lib.RS_SV_MAX_MATCHES + 1)) == -6     # AKZ_E_TOO_LARGE
    assert call(lib, SingleViewRefiner.params(single_view_filter_loop_iterations=_lib.RS_SV_MAX_RUNS)) == -6
    # valid parameters get as far as the context, and there is none here; thresholds of any sign are the caller's business
    for kw in (dict(), dict(maximum_cosine_distance=-1.0), dict(maximum_sine_distance=float("inf")), dict(single_view_minimum_landmarks=0),
               dict(single_view_filter_loop_iterations=_lib.RS_SV_MAX_RUNS - 1), dict(single_view_patience=0xFFFFFFFF)):
        assert call(lib, SingleViewRefiner.params(**kw)) == -1
    # the new matcher entry point checks its arguments like its sibling
    assert lib.hm_landmark_original_matches_batch_device(None, None, None, None, None, None, None, 8, 1, 8, None, None, None) == -1


def test_the_cpp_mirror_compiles(lib, tmp_path):
    import host_build
    exe = host_build.native(tmp_path, "single_view.cpp", hip=True)
    assert os.path.exists(exe)
    import torch
    if not torch.cuda.is_available():
        # without a batch file the program leaves before its first device call
        r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
        assert r.returncode == 2
