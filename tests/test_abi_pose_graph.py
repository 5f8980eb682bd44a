"""The C ABI of the pose-graph relaxation (include/akz.h): defaults, struct size, constants, early refusals, flatten's order;
the ABI number stays 11, since the entry points are pure additions.  No GPU needed: the parameters are checked before anything
else, so the refusals are visible without a context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cv_amd import _lib
from cv_amd.pose_graph import SLOT_OTHER, SLOT_TARGET, PoseGraph, flatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_pose_graph_params_default", "rs_pose_graph_edges_device", "rs_pose_graph_relax_batch_device",
         "rs_pose_graph_debug_resident_views")


@pytest.fixture(scope="module")
def lib():
    from cv_amd.build import build
    build()
    return _lib.lib()


def call(lib, prm, ctx=None):
    """rs_pose_graph_relax_batch_device with no context and null buffers: only the parameter checks can answer"""
    return lib.rs_pose_graph_relax_batch_device(ctx, None, 3, None, 1, None, None, 0, None, None, None, 0,
                                                C.byref(prm) if prm is not None else None, None, None, None, None)


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
    assert "class PoseGraph" in hpp


def test_header_constants_are_the_bindings():
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    for name in ("RS_PG_OK", "RS_PG_FEW_VIEWS", "RS_PG_NONFINITE", "RS_PG_BAD_INDEX", "RS_PG_VIEW_UPDATED", "RS_PG_VIEW_NO_CONSTRAINT",
                 "RS_PG_VIEW_NONFINITE", "RS_PG_RESIDENT_VIEWS", "RS_PG_DEFAULT_RESIDENT_VIEWS", "RS_PG_S_VIEWS", "RS_PG_S_UPDATED", "RS_PG_S_EDGES", "RS_PG_S_ROUNDS",
                 "RS_PG_S_STAGE", "RS_PG_S_FIRST_BAD_VIEW", "RS_PG_STATS"):
        assert int(re.search(r"\b%s = (\d+)" % name, hdr).group(1)) == getattr(_lib, name), name
    assert re.search(r"RS_PG_MAX_ITERATIONS = 1 << 20", hdr) and _lib.RS_PG_MAX_ITERATIONS == 1 << 20
    assert (_lib.RS_PG_OK, _lib.RS_PG_FEW_VIEWS, _lib.RS_PG_NONFINITE, _lib.RS_PG_BAD_INDEX) == (0, 1, 2, 3)
    assert _lib.RS_PG_RESIDENT_VIEWS == 256 and _lib.RS_PG_DEFAULT_RESIDENT_VIEWS == 8 and _lib.RS_PG_STATS == 8
    # the math header's own copies
    math = open(os.path.join(ROOT, "include", "akz_pose_graph_math.h")).read()
    for name in ("OK", "FEW_VIEWS", "NONFINITE", "BAD_INDEX", "VIEW_UPDATED", "VIEW_NO_CONSTRAINT", "VIEW_NONFINITE", "RESIDENT_VIEWS",
                 "S_VIEWS", "S_UPDATED", "S_EDGES", "S_ROUNDS", "S_STAGE", "S_FIRST_BAD_VIEW", "STATS"):
        assert int(re.search(r"\bAKZ_PG_%s = (\d+)" % name, math).group(1)) == getattr(_lib, "RS_PG_" + name), name


def test_defaults_are_the_references(lib):
    p = _lib.PoseGraphParams()
    assert lib.rs_pose_graph_params_default(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(_lib.PoseGraphParams) == 16
    assert p.optimization_iterations == 1024               # settings.rs:461-463
    assert p.graph_optimization_rate == 1e-3               # settings.rs:477-479
    assert lib.rs_pose_graph_params_default(None) == -1
    q = PoseGraph.params(optimization_iterations=7)
    assert q.optimization_iterations == 7 and q.graph_optimization_rate == 1e-3
    with pytest.raises(TypeError):
        PoseGraph.params(iterations=7)
    with pytest.raises(TypeError):
        PoseGraph.params(struct_size=8)


def test_refusals_come_before_the_device(lib):
    assert call(lib, None) == -1                                        # AKZ_E_INVALID
    p = PoseGraph.params()
    p.struct_size -= 4
    assert call(lib, p) == -1
    for rate in (float("nan"), float("inf"), float("-inf")):
        assert call(lib, PoseGraph.params(graph_optimization_rate=rate)) == -1
    # valid parameters get as far as the context, and there is none here: iterations beyond RS_PG_MAX_ITERATIONS count as
    # that, a rate of zero or below is the caller's business
    for kw in (dict(), dict(optimization_iterations=0xFFFFFFFF), dict(optimization_iterations=0), dict(graph_optimization_rate=0.0),
               dict(graph_optimization_rate=-1e-3)):
        assert call(lib, PoseGraph.params(**kw)) == -1
    assert lib.rs_pose_graph_edges_device(None, None, None, None, 1, None, None) == -1
    assert lib.rs_pose_graph_debug_resident_views(None, 0) == -1
    assert lib.rs_pose_graph_debug_resident_views(None, _lib.RS_PG_RESIDENT_VIEWS + 1) == -1


def test_no_device_behaviour_matches_the_other_entry_points(lib):
    import torch
    h = C.c_void_p()
    if not torch.cuda.is_available():
        assert lib.rs_create(0, 64, 64, C.byref(h)) == -2
        assert not h.value
    assert call(lib, PoseGraph.params(), None) == -1


def test_flatten_is_constraint_ascending_then_slot_order():
    assert SLOT_TARGET == (0, 0, 1, 1, 2, 2) and SLOT_OTHER == (2, 1, 0, 2, 1, 0)
    views = [[0, 1, 2], [2, 3, 0], [1, 0, 3]]
    row_start, row_edges = flatten(views, 5)
    assert row_start.dtype == np.uint32 and row_edges.dtype == np.uint32
    assert row_start.tolist() == [0, 6, 10, 14, 18, 18]                 # view 4 has no edge
    assert row_edges.tolist() == [0, 1, 10, 11, 14, 15,                 # view 0: constraint 0 slots 0 1, 1 slots 4 5, 2 slots 2 3
                                  2, 3, 12, 13,                         # view 1: constraint 0 slots 2 3, constraint 2 slots 0 1
                                  4, 5, 6, 7,                           # view 2
                                  8, 9, 16, 17]                         # view 3
    for v in range(5):
        for e in row_edges[row_start[v]:row_start[v + 1]]:
            assert views[e // 6][SLOT_TARGET[e % 6]] == v
    # another walk of the constraints: the rows hold the same edges in that order
    rs2, re2 = flatten(views, 5, order=[2, 0, 1])
    assert rs2.tolist() == row_start.tolist() and re2[:6].tolist() == [14, 15, 0, 1, 10, 11]
    assert sorted(re2.tolist()) == sorted(row_edges.tolist()) == list(range(18))
    assert flatten(np.zeros((0, 3)), 2)[0].tolist() == [0, 0, 0] and flatten([], 0)[1].tolist() == []
    with pytest.raises(ValueError):
        flatten(views, 3)
    with pytest.raises(ValueError):
        flatten(views, 5, order=[0, 0, 1])
    # the checker the GPU tests use builds the same rows
    import pose_graph_checker as P
    assert [e for row in P.flatten(views, 5) for e in row] == row_edges.tolist()
