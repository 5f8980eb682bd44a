"""The C ABI of the observation filter and of optimize_reconstruction (include/akz.h): defaults, struct size, constants, early
refusals; the ABI number stays 11, since the entry points are pure additions.  No GPU needed: the parameters are checked before
anything else, so the refusals are visible without a context."""
import ctypes as C
import os
import re
import subprocess

import pytest

from cv_amd import _lib
from cv_amd.pose_graph import PoseGraph
from cv_amd.reconstruction import LANDMARK_STATES, VERDICTS, ObservationFilter, ReconstructionOptimizer, stopped_at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_observation_filter_params_default", "rs_filter_observations_device", "rs_optimize_reconstruction_batch_device")


@pytest.fixture(scope="module")
def lib():
    from cv_amd.build import build
    build()
    return _lib.lib()


def call(lib, prm, ctx=None):
    """rs_filter_observations_device with no context and null buffers: only the parameter checks can answer"""
    return lib.rs_filter_observations_device(ctx, None, 8, 1, None, None, None, None, 0, 0, None, None, 0, None,
                                             C.byref(prm) if prm is not None else None, *([None] * 11))


def chain(lib, prm, pg):
    return lib.rs_optimize_reconstruction_batch_device(None, None, 3, None, 1, None, None, 0, None, None, None, 0,
                                                       C.byref(pg) if pg is not None else None, None, 8, None, None, None, 0, 0, None,
                                                       C.byref(prm) if prm is not None else None, *([None] * 17))


def test_abi_number_stays_11(lib):
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    assert int(re.search(r"#define\s+AKZ_ABI_VERSION\s+(\d+)u", hdr).group(1)) == 11
    assert lib.akz_abi_version() == 11 == _lib.ABI_VERSION
    for name in NAMES:
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    rust = open(os.path.join(ROOT, "rust", "akaze-mi355x", "src", "lib.rs")).read()
    assert re.search(r"ABI_VERSION: u32 = 11\b", rust)
    for name in NAMES:
        assert re.search(r"fn %s\(" % name, rust), name
    hpp = open(os.path.join(ROOT, "include", "akaze.hpp")).read()
    assert "class ObservationFilter" in hpp and "inline void optimize_reconstruction(" in hpp


def test_the_ctypes_declarations_have_the_headers_argument_counts(lib):
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    for name in NAMES:
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S).group(1)
        kinds = [C.c_uint32 if re.match(r"\s*uint32_t\s+\w+$", a) else None for a in args.split(",")]
        declared = getattr(lib, name).argtypes
        assert len(declared) == len(kinds), name
        for k, (want, got) in enumerate(zip(kinds, declared)):
            assert (got is C.c_uint32) == (want is C.c_uint32), (name, k)


def test_header_constants_are_the_bindings():
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    names = ("RS_OF_KEPT", "RS_OF_SINGLE", "RS_OF_PAIR_SPLIT", "RS_OF_NO_POINT", "RS_OF_KICKED", "RS_OF_BAD_INDEX", "RS_OF_SKIPPED", "RS_OF_OK",
             "RS_OF_FEW_LANDMARKS", "RS_OF_BAD_RANGE", "RS_OF_RECON_SKIPPED", "RS_OF_NO_SOLVE", "RS_OF_ROBUST_BEFORE", "RS_OF_ROBUST_AFTER",
             "RS_OF_S_LANDMARKS", "RS_OF_S_ROBUST_BEFORE", "RS_OF_S_ROBUST_AFTER", "RS_OF_S_OBS_SPLIT", "RS_OF_S_PAIR_SPLIT", "RS_OF_S_NO_POINT",
             "RS_OF_S_KICKED", "RS_OF_STATS", "RS_OF_MAX_ITERATIONS", "RS_OR_OK", "RS_OR_STAGE_RELAX", "RS_OR_STAGE_FILTER")
    for name in names:
        assert int(re.search(r"\b%s = (\d+)" % name, hdr).group(1)) == getattr(_lib, name), name
    assert re.search(r"RS_OR_STOPPED = 1 << 30", hdr) and _lib.RS_OR_STOPPED == 1 << 30
    assert len(LANDMARK_STATES) == 7 and len(VERDICTS) == 4
    # the math header's own copies
    math = open(os.path.join(ROOT, "include", "akz_observation_filter_math.h")).read()
    for name in names:
        if name.startswith("RS_OF_") and name != "RS_OF_MAX_ITERATIONS":
            assert int(re.search(r"\bAKZ_OF_%s = (\d+)" % name[6:], math).group(1)) == getattr(_lib, name), name
    assert stopped_at(0) is None and stopped_at(_lib.RS_OR_STOPPED | 1 << 16 | 2 << 8 | 1) == (1, "filter", 1)
    assert stopped_at(_lib.RS_OR_STOPPED | 1 << 8 | 2) == (0, "relax", 2)


def test_defaults_are_the_references(lib):
    p = _lib.ObservationFilterParams()
    assert lib.rs_observation_filter_params_default(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(_lib.ObservationFilterParams) == 64
    assert p.maximum_cosine_distance == 1e-5                     # settings.rs:324-326
    assert p.maximum_sine_distance == 1e-1                       # settings.rs:328-330
    assert p.minimum_robust_landmarks == 32                      # settings.rs:340-342
    assert p.reconstruction_optimization_iterations == 1         # settings.rs:429-431
    assert p.reserved == 0
    t = p.triangulate
    assert t.struct_size == C.sizeof(_lib.TriangulateParams) and t.robust_minimum_observations == 3 and t.incidence_minimum_cosine_distance == 1e-3
    assert t.max_sweeps == 1000 and t.eps == 1e-12
    assert lib.rs_observation_filter_params_default(None) == -1
    q = ObservationFilter.params(minimum_robust_landmarks=7)
    assert q.minimum_robust_landmarks == 7 and q.maximum_cosine_distance == 1e-5
    assert ReconstructionOptimizer.params(reconstruction_optimization_iterations=3).reconstruction_optimization_iterations == 3
    with pytest.raises(TypeError):
        ObservationFilter.params(minimum=7)
    with pytest.raises(TypeError):
        ObservationFilter.params(struct_size=8)


def test_refusals_come_before_the_device(lib):
    assert call(lib, None) == -1                                        # AKZ_E_INVALID
    p = ObservationFilter.params()
    p.struct_size -= 4
    assert call(lib, p) == -1
    for kw in (dict(maximum_cosine_distance=float("nan")), dict(maximum_sine_distance=float("nan")), dict(reserved=1)):
        assert call(lib, ObservationFilter.params(**kw)) == -1
    p = ObservationFilter.params()
    p.triangulate.max_sweeps = 0
    assert call(lib, p) == -1
    p = ObservationFilter.params()
    p.triangulate.struct_size = 8
    assert call(lib, p) == -1
    assert call(lib, ObservationFilter.params(reconstruction_optimization_iterations=_lib.RS_OF_MAX_ITERATIONS + 1)) == -6   # AKZ_E_TOO_LARGE
    # valid parameters get as far as the context, and there is none here; thresholds of any sign are the caller's business
    for kw in (dict(), dict(maximum_cosine_distance=-1.0), dict(maximum_sine_distance=float("inf")), dict(minimum_robust_landmarks=0),
               dict(reconstruction_optimization_iterations=_lib.RS_OF_MAX_ITERATIONS)):
        assert call(lib, ObservationFilter.params(**kw)) == -1
    # the chain checks both parameter structs first
    pg = PoseGraph.params()
    assert chain(lib, None, pg) == -1 and chain(lib, ObservationFilter.params(), None) == -1
    assert chain(lib, ObservationFilter.params(), PoseGraph.params(graph_optimization_rate=float("nan"))) == -1
    assert chain(lib, ObservationFilter.params(reconstruction_optimization_iterations=65), pg) == -6
    assert chain(lib, ObservationFilter.params(), pg) == -1


def test_the_cpp_mirror_compiles(lib, tmp_path):
    import host_build
    exe = host_build.native(tmp_path, "observation_filter.cpp", hip=True)
    assert os.path.exists(exe)
    import torch
    if not torch.cuda.is_available():
        # without a device the program's first call fails cleanly
        r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
        assert r.returncode == 2
