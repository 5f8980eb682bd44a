"""The C ABI of the three-view bootstrap (include/akz.h, ABI 11): defaults, struct size, early refusals.  No GPU needed: the
parameters are checked before anything else, so the refusals are visible without a context."""
import ctypes as C

import pytest

from cv_amd import _lib
from cv_amd.three_view import ThreeViewInit, join_pairs


@pytest.fixture(scope="module")
def lib():
    from cv_amd.build import build
    build()
    return _lib.lib()


def call(lib, prm, ctx=None):
    """rs_three_view_init_batch_device with no context and null buffers: only the parameter checks can answer"""
    one = (C.c_uint32 * 1)(0)
    cam = _lib.Camera(1000.0, 1000.0, 640.0, 360.0, 0.0, 0.0, 0, 0)
    return lib.rs_three_view_init_batch_device(ctx, None, 64, 3, one, one, one, C.byref(cam), None, None, None, None, None, None, None,
                                               None, 1, C.byref(prm) if prm is not None else None, None, None, None, None, None, None, None)


def test_abi_version_is_11(lib):
    assert lib.akz_abi_version() == 11 == _lib.ABI_VERSION


def test_defaults_are_the_references(lib):
    p = _lib.ThreeViewParams()
    assert lib.rs_three_view_params_default(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(_lib.ThreeViewParams) == 104
    assert (p.maximum_cosine_distance, p.maximum_sine_distance) == (1e-5, 1e-1)
    assert p.robust_observation_incidence_minimum_cosine_distance == 1e-3
    assert p.robust_view_bearing_pair_minimum_cosine_distance == 1e-2
    assert p.robust_view_num_robust_bearing_pair == 3
    assert p.three_view_minimum_relative_scales == 16
    assert p.three_view_filter_loop_iterations == 8
    assert p.three_view_optimization_landmarks == 1024 == _lib.RS_TV_MAX_LANDMARKS
    assert p.three_view_patience == 65536
    assert p.three_view_minimum_robust_matches == 32
    assert p.optimization_rate == 0.001
    assert p.hard_minimum_matches == 32
    t = _lib.TriangulateParams()
    assert lib.rs_triangulate_params_default(C.byref(t)) == 0
    assert bytes(p.triangulate) == bytes(t)
    assert lib.rs_three_view_params_default(None) == -1
    q = ThreeViewInit.params(three_view_patience=7)
    assert q.three_view_patience == 7 and q.three_view_filter_loop_iterations == 8
    with pytest.raises(TypeError):
        ThreeViewInit.params(patience=7)


def test_refusals_come_before_the_device(lib):
    p = ThreeViewInit.params()
    assert call(lib, None) == -1                                       # AKZ_E_INVALID
    p.struct_size -= 4
    assert call(lib, p) == -1
    p = ThreeViewInit.params(three_view_optimization_landmarks=1025)
    assert call(lib, p) == -6                                          # AKZ_E_TOO_LARGE
    p = ThreeViewInit.params(three_view_filter_loop_iterations=9)
    assert call(lib, p) == -1
    p = ThreeViewInit.params()
    p.triangulate.struct_size = 0
    assert call(lib, p) == -1
    p = ThreeViewInit.params(maximum_cosine_distance=float("nan"))
    assert call(lib, p) == -1
    # valid parameters get as far as the context: none here
    assert call(lib, ThreeViewInit.params()) == -1


def test_no_device_behaviour_matches_the_other_entry_points(lib):
    """Without a usable device no rs_ctx can be made (AKZ_E_NO_DEVICE, no fallback), and the entry point refuses a null one."""
    import torch
    h = C.c_void_p()
    if not torch.cuda.is_available():
        assert lib.rs_create(0, 64, 64, C.byref(h)) == -2
        assert not h.value
    assert call(lib, ThreeViewInit.params(), None) == -1


def test_join_pairs_follows_the_reference_order():
    first = [(5, 50), (1, 10), (9, 90), (3, 30), (7, 70)]
    second = [(3, 300), (8, 800), (5, 500), (1, 100)]
    t, fo, so = join_pairs(first, second)
    assert t.tolist() == [[5, 50, 500], [1, 10, 100], [3, 30, 300]]
    assert fo.tolist() == [[9, 90], [7, 70]] and so.tolist() == [[8, 800]]
    t2, _, _ = join_pairs(first, second, permutation=[2, 0, 1])
    assert t2.tolist() == [[3, 30, 300], [5, 50, 500], [1, 10, 100]]
    # a centre feature named twice: the HashMap keeps the last
    assert join_pairs([(1, 10)], [(1, 100), (1, 101)])[0].tolist() == [[1, 10, 101]]
    with pytest.raises(ValueError):
        join_pairs(first, second, permutation=[0, 0, 1])
    e = join_pairs([], [])
    assert [x.shape for x in e] == [(0, 3), (0, 2), (0, 2)]
