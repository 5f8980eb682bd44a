"""The C ABI of the three-view constraints (include/akz.h): defaults, struct size, early refusals; the ABI number stays 11,
since the two entry points are pure additions.  No GPU needed: the parameters are checked before anything else, so the
refusals are visible without a context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cv_amd import _lib
from cv_amd.three_view import ThreeViewConstraints, order_landmarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from cv_amd.build import build
    build()
    return _lib.lib()


def call(lib, prm, ctx=None):
    """rs_three_view_constraint_batch_device with no context and null buffers: only the parameter checks can answer"""
    cam = _lib.Camera(1000.0, 1000.0, 640.0, 360.0, 0.0, 0.0, 0, 0)
    return lib.rs_three_view_constraint_batch_device(ctx, None, 64, 3, None, C.byref(cam), None, None, None, 0, 1,
                                                     C.byref(prm) if prm is not None else None, None, None, None, None)


def test_abi_number_stays_11(lib):
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    assert int(re.search(r"#define\s+AKZ_ABI_VERSION\s+(\d+)u", hdr).group(1)) == 11
    assert lib.akz_abi_version() == 11 == _lib.ABI_VERSION
    for name in ("rs_three_view_constraint_params_default", "rs_three_view_constraint_batch_device"):
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, hdr)


def test_header_constants_are_the_bindings():
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    for name in ("RS_TVC_OK", "RS_TVC_FEW_LANDMARKS", "RS_TVC_FEW_BEARING_PAIRS", "RS_TVC_BAD_INDEX", "RS_TVC_MAX_LANDMARKS",
                 "RS_TVC_S_LANDMARKS", "RS_TVC_S_USED", "RS_TVC_S_PAIRS", "RS_TVC_S_ORIGINAL_SCALE", "RS_TVC_S_FINAL_SCALE",
                 "RS_TVC_S_STAGE", "RS_TVC_STATS"):
        assert int(re.search(r"\b%s = (\d+)" % name, hdr).group(1)) == getattr(_lib, name), name
    assert re.search(r"RS_TVC_MAX_ITERATIONS = 1 << 20", hdr) and _lib.RS_TVC_MAX_ITERATIONS == 1 << 20


def test_defaults_are_the_references(lib):
    p = _lib.ThreeViewConstraintParams()
    assert lib.rs_three_view_constraint_params_default(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(_lib.ThreeViewConstraintParams) == 32
    assert p.optimization_minimum_landmarks == 24                       # settings.rs:465-467
    assert p.optimization_maximum_landmarks == 64                       # settings.rs:469-471
    assert p.constraint_patience == 1 << 12                             # settings.rs:481-483
    assert p.robust_view_num_robust_bearing_pair == 3                   # settings.rs:336-338
    assert p.robust_view_bearing_pair_minimum_cosine_distance == 1e-2   # settings.rs:332-334
    assert p.optimization_maximum_landmarks <= _lib.RS_TVC_MAX_LANDMARKS == 256
    assert lib.rs_three_view_constraint_params_default(None) == -1
    q = ThreeViewConstraints.params(constraint_patience=7)
    assert q.constraint_patience == 7 and q.optimization_maximum_landmarks == 64
    with pytest.raises(TypeError):
        ThreeViewConstraints.params(patience=7)
    with pytest.raises(TypeError):
        ThreeViewConstraints.params(struct_size=8)


def test_refusals_come_before_the_device(lib):
    assert call(lib, None) == -1                                        # AKZ_E_INVALID
    p = ThreeViewConstraints.params()
    p.struct_size -= 4
    assert call(lib, p) == -1
    assert call(lib, ThreeViewConstraints.params(optimization_maximum_landmarks=257)) == -6    # AKZ_E_TOO_LARGE
    assert call(lib, ThreeViewConstraints.params(robust_view_bearing_pair_minimum_cosine_distance=float("nan"))) == -1
    # the cap itself, an infinite threshold and a patience beyond RS_TVC_MAX_ITERATIONS are valid parameters: they get as far
    # as the context, and there is none here
    for kw in (dict(), dict(optimization_maximum_landmarks=256), dict(robust_view_bearing_pair_minimum_cosine_distance=float("inf")),
               dict(constraint_patience=0xFFFFFFFF), dict(optimization_minimum_landmarks=0)):
        assert call(lib, ThreeViewConstraints.params(**kw)) == -1
    # TOO_LARGE is answered although the context is missing as well: the parameters come first
    assert call(lib, ThreeViewConstraints.params(optimization_maximum_landmarks=1 << 20), None) == -6


def test_no_device_behaviour_matches_the_other_entry_points(lib):
    import torch
    h = C.c_void_p()
    if not torch.cuda.is_available():
        assert lib.rs_create(0, 64, 64, C.byref(h)) == -2
        assert not h.value
    assert call(lib, ThreeViewConstraints.params(), None) == -1


def test_order_landmarks_is_the_permutation_then_a_stable_descending_sort():
    counts = [3, 5, 3, 7, 5, 3]
    assert order_landmarks(counts).tolist() == [3, 1, 4, 0, 2, 5]
    assert order_landmarks(counts, permutation=[5, 4, 3, 2, 1, 0]).tolist() == [3, 4, 1, 5, 2, 0]
    assert order_landmarks([]).tolist() == []
    got = order_landmarks(counts, permutation=[2, 0, 1, 5, 3, 4])
    assert sorted(got.tolist()) == list(range(6)) and np.all(np.diff(np.asarray(counts)[got]) <= 0)
    with pytest.raises(ValueError):
        order_landmarks(counts, permutation=[0, 0, 1, 2, 3, 4])
