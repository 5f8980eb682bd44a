"""The C ABI of the covisibility search, its record and the rows of the pose graph (include/akz.h): defaults, struct size,
constants, early refusals; the ABI number stays 11, since the entry points are pure additions.  No GPU needed: the parameters
are checked before anything else, so the refusals are visible without a context."""
import ctypes as C
import os
import re
import subprocess

import pytest

from cv_amd import _lib
from cv_amd.covisibility import VERDICTS, Covisibility

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_covisibility_params_default", "rs_covisibility_candidates_device", "rs_covisibility_record_device", "rs_pose_graph_rows_device")
CONSTANTS = ("RS_CV_OK", "RS_CV_FEW_CONSTRAINTS", "RS_CV_BAD_INDEX", "RS_CV_NO_GRAPH", "RS_CV_NOT_RECORDED", "RS_CV_MAX_CANDIDATE_VIEWS",
             "RS_CV_MAX_SLOTS", "RS_CV_MAX_FEATURES", "RS_CV_S_ROBUST", "RS_CV_S_CANDIDATES", "RS_CV_S_PAIRS", "RS_CV_S_UNIQUE", "RS_CV_S_EMITTED",
             "RS_CV_S_FLAGS", "RS_CV_S_RECORDED", "RS_CV_STATS", "RS_CV_F_CANDIDATES_CAPPED", "RS_CV_F_LIMIT_REACHED")


@pytest.fixture(scope="module")
def lib():
    from cv_amd.build import build
    build()
    return _lib.lib()


def call(lib, prm):
    """rs_covisibility_candidates_device with no context and null buffers: only the parameter checks can answer"""
    return lib.rs_covisibility_candidates_device(None, None, None, 0, 0, 8, 1, None, None, 0, C.byref(prm) if prm is not None else None,
                                                 *([None] * 7))


def record(lib, prm):
    return lib.rs_covisibility_record_device(None, None, None, 0, None, 0, C.byref(prm) if prm is not None else None, None, None, None, None)


def test_abi_number_stays_11(lib):
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    assert int(re.search(r"#define\s+AKZ_ABI_VERSION\s+(\d+)u", hdr).group(1)) == 11
    assert lib.akz_abi_version() == 11 == _lib.ABI_VERSION
    rust = open(os.path.join(ROOT, "rust", "akaze-mi355x", "src", "lib.rs")).read()
    assert re.search(r"ABI_VERSION: u32 = 11\b", rust)
    hpp = open(os.path.join(ROOT, "include", "akaze.hpp")).read()
    for name in NAMES:
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"fn %s\(" % name, rust), name
        assert re.search(r"\b%s\(" % name, hpp), name
    assert "class ViewConstraints" in hpp and re.search(r"void rows\(const void\* d_views", hpp)
    assert "pub struct ViewConstraints" in rust


def test_the_ctypes_declarations_have_the_headers_argument_counts(lib):
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    rust = open(os.path.join(ROOT, "rust", "akaze-mi355x", "src", "lib.rs")).read()
    for name in NAMES:
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S).group(1)
        kinds = [C.c_uint32 if re.match(r"\s*uint32_t\s+\w+$", a) else None for a in args.split(",")]
        declared = getattr(lib, name).argtypes
        assert len(declared) == len(kinds), name
        for k, (want, got) in enumerate(zip(kinds, declared)):
            assert (got is C.c_uint32) == (want is C.c_uint32), (name, k)
        rargs = re.search(r"fn %s\(([^;]*?)\)\s*->\s*i32;" % name, rust, re.S).group(1).split(",")
        assert [bool(re.search(r":\s*u32$", a.strip())) for a in rargs] == [k is C.c_uint32 for k in kinds], name


def test_header_constants_are_the_bindings():
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    math = open(os.path.join(ROOT, "include", "akz_covisibility_math.h")).read()
    rust = open(os.path.join(ROOT, "rust", "akaze-mi355x", "src", "lib.rs")).read()
    for name in CONSTANTS:
        value = int(re.search(r"\b%s = (\d+)" % name, hdr).group(1))
        assert value == getattr(_lib, name), name
        assert int(re.search(r"\bAKZ_CV_%s = (\d+)" % name[6:], math).group(1)) == value, name
        r = re.search(r"pub const %s: \w+ = (\d+);" % name, rust)
        assert r is None or int(r.group(1)) == value, name
    for name in ("RS_CV_NOT_RECORDED", "RS_CV_MAX_CANDIDATE_VIEWS", "RS_CV_MAX_SLOTS", "RS_CV_MAX_FEATURES", "RS_CV_STATS"):
        assert re.search(r"pub const %s: \w+ = \d+;" % name, rust), name
    assert [int(x) for x in re.search(r"pub enum CovisibilityVerdict \{(.*?)\}", rust, re.S).group(1).replace(",", " ").split() if x.isdigit()] == [0, 1, 2, 3]
    assert len(VERDICTS) == 4
    # the pair keys of one target fit the sort's LDS, the landmark cap is the constraint stage's
    assert _lib.RS_CV_MAX_CANDIDATE_VIEWS * (_lib.RS_CV_MAX_CANDIDATE_VIEWS - 1) // 2 <= 8192
    assert int(re.search(r"AKZ_CV_MAX_LANDMARKS = (\d+)", math).group(1)) == _lib.RS_TVC_MAX_LANDMARKS


def test_defaults_are_the_references(lib):
    p = _lib.CovisibilityParams()
    assert lib.rs_covisibility_params_default(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(_lib.CovisibilityParams) == 32
    assert p.optimization_robust_covisibility_minimum_landmarks == 16     # cv-sfm/src/settings.rs:473-475
    assert p.optimization_maximum_three_view_constraints == 64           # settings.rs:453-455
    assert p.optimization_minimum_new_constraints == 4                   # settings.rs:457-459
    assert p.optimization_minimum_landmarks == 24                        # settings.rs:465-467
    assert p.optimization_maximum_landmarks == 64                        # settings.rs:469-471
    assert p.candidate_limit == 0 and p.shuffle_seed == 0
    assert lib.rs_covisibility_params_default(None) == -1
    t = _lib.ThreeViewConstraintParams()
    lib.rs_three_view_constraint_params_default(C.byref(t))
    assert (t.optimization_minimum_landmarks, t.optimization_maximum_landmarks) == (p.optimization_minimum_landmarks, p.optimization_maximum_landmarks)
    q = Covisibility.params(candidate_limit=7)
    assert q.candidate_limit == 7 and Covisibility.limit(q) == 7 and Covisibility.limit(p) == 64
    with pytest.raises(TypeError):
        Covisibility.params(limit=7)
    with pytest.raises(TypeError):
        Covisibility.params(struct_size=8)


def test_refusals_come_before_the_device(lib):
    for f in (call, record):
        assert f(lib, None) == -1                                                                 # AKZ_E_INVALID
        for size in (0, 28):
            p = Covisibility.params()
            p.struct_size = size
            assert f(lib, p) == -1
        assert f(lib, Covisibility.params(optimization_maximum_landmarks=_lib.RS_TVC_MAX_LANDMARKS + 1,
                                          optimization_minimum_landmarks=0)) == -6                # AKZ_E_TOO_LARGE
        assert f(lib, Covisibility.params(optimization_minimum_landmarks=65)) == -1
        assert f(lib, Covisibility.params(candidate_limit=_lib.RS_CV_MAX_SLOTS + 1)) == -6
        assert f(lib, Covisibility.params(optimization_maximum_three_view_constraints=_lib.RS_CV_MAX_SLOTS + 1)) == -6
        # valid parameters get as far as the context, and there is none here
        for kw in (dict(), dict(candidate_limit=_lib.RS_CV_MAX_SLOTS), dict(optimization_maximum_landmarks=_lib.RS_TVC_MAX_LANDMARKS),
                   dict(optimization_maximum_three_view_constraints=1000, candidate_limit=5), dict(shuffle_seed=0xFFFFFFFF),
                   dict(optimization_minimum_landmarks=64)):
            assert f(lib, Covisibility.params(**kw)) == -1
    assert lib.rs_pose_graph_rows_device(None, None, 0, 3, None, None, None, None) == -1


def test_the_cpp_mirror_compiles(lib, tmp_path):
    import host_build
    exe = host_build.native(tmp_path, "covisibility.cpp", hip=True)
    assert os.path.exists(exe)
    import torch
    if not torch.cuda.is_available():
        # without a device the program's first call fails cleanly
        r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
        assert r.returncode == 2
