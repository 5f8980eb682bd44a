"""The one rule of the Python layer (cv_amd/_device.py) at every enqueuing wrapper, without a GPU: a recording stand-in
takes the library's place, every symbol of it records its arguments and returns 0.  What a wrapper hands to ctypes must be
as many arguments as the real symbol's argtypes and pass each one's from_param; a wrapper driven with device addresses
(ints) and with tensors (objects whose data_ptr() gives the same ints) must record the same call; a stream object given as
stream_to_wait must arrive as the handle _lib.wait_handle names."""
import ctypes as C
import inspect
from types import SimpleNamespace

import pytest

from cv_amd import _device, _lib
from cv_amd.covisibility import Covisibility
from cv_amd.landmark_table import LandmarkUpdate
from cv_amd.pose_graph import PoseGraph
from cv_amd.ransac import EssentialConsensus
from cv_amd.reconstruction import ObservationFilter, ReconstructionOptimizer
from cv_amd.single_view import SingleViewRefiner
from cv_amd.three_view import ThreeViewConstraints, ThreeViewInit
from cv_amd import triangulation

HANDLE = 0x7700
CONSENSUS = SimpleNamespace(_h=C.c_void_p(HANDLE))        # a stand-in consensus carries only _h
BLOCKS = [3, 1, 2]
NULLABLE = ("d_best", "d_skip", "d_split", "d_split_count", "d_lm")    # required by position, None by their wrappers' docstrings


class Tensor:
    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


class Stream:
    def __init__(self, handle):
        self.cuda_stream = handle


def consensus_method(name):
    return lambda: getattr(EssentialConsensus, name).__get__(CONSENSUS)


def stage(cls, name, *args):
    return lambda: getattr(cls(*(args or (CONSENSUS,))), name)


# (the wrapper, the symbol it calls, the struct type of its `params` argument)
WRAPPERS = [
    (consensus_method("model_inliers_batch_device"), "rs_essential_arrsac_batch_device", _lib.ArrsacParams),
    (consensus_method("p3p_model_inliers_batch_device"), "rs_p3p_arrsac_batch_device", _lib.ArrsacParams),
    (consensus_method("triangulate_inliers"), "rs_triangulate_pairs_batch_device", _lib.TriangulateParams),
    (lambda: triangulation.triangulate_landmarks_device, "rs_triangulate_landmarks_device", _lib.TriangulateParams),
    (lambda: triangulation.triangulate_merged_device, "rs_triangulate_merged_device", _lib.TriangulateParams),
    (stage(ThreeViewInit, "init_batch_device"), "rs_three_view_init_batch_device", _lib.ThreeViewParams),
    (stage(ThreeViewConstraints, "batch_device"), "rs_three_view_constraint_batch_device", _lib.ThreeViewConstraintParams),
    (stage(PoseGraph, "edges_device"), "rs_pose_graph_edges_device", None),
    (stage(PoseGraph, "relax_batch_device"), "rs_pose_graph_relax_batch_device", _lib.PoseGraphParams),
    (stage(PoseGraph, "rows_device"), "rs_pose_graph_rows_device", None),
    (stage(ObservationFilter, "filter_device"), "rs_filter_observations_device", _lib.ObservationFilterParams),
    (stage(ReconstructionOptimizer, "optimize_device", PoseGraph(CONSENSUS)), "rs_optimize_reconstruction_batch_device",
     _lib.ObservationFilterParams),
    (stage(Covisibility, "candidates_device"), "rs_covisibility_candidates_device", _lib.CovisibilityParams),
    (stage(Covisibility, "record_device"), "rs_covisibility_record_device", _lib.CovisibilityParams),
    (stage(SingleViewRefiner, "refine_batch_device"), "rs_refine_poses_batch_device", _lib.SingleViewParams),
    (stage(LandmarkUpdate, "sharing_view_device"), "rs_landmarks_sharing_view_device", None),
    (stage(LandmarkUpdate, "add_views_device"), "rs_add_views_device", None),
]
IDS = [w[1] for w in WRAPPERS]


@pytest.fixture(scope="module")
def real():
    from cv_amd.build import build
    build()
    return _lib.lib()


class Recorder:
    """stands where _lib.lib() looks: every symbol the real library has records its arguments and returns 0"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, symbol):
        getattr(self.real, symbol)                       # a symbol the library does not export stays an AttributeError

        def record(*args):
            self.calls.append((symbol, args))
            return 0
        return record


@pytest.fixture
def recorder(real, monkeypatch):
    rec = Recorder(real)
    monkeypatch.setattr(_lib, "_lib", rec)
    assert _lib.lib() is rec
    return rec


def arguments(wrapper, params_type, structs, device, optional, stream):
    """One argument per parameter of `wrapper` by its name: d_* a device address (through `device`: the int itself or a
    Tensor of it), optional and NULLABLE d_* None unless `optional`, cam* / *params the structs of `structs`, host lists
    BLOCKS, the table of the triangulation calls a stand-in of the same kind, counts small ints."""
    out = {}
    for k, (name, p) in enumerate(inspect.signature(wrapper).parameters.items()):
        address = 0x10000 + 0x100 * k
        if name.startswith("d_"):
            out[name] = None if not optional and (p.default is None or name in NULLABLE) else device(address)
        elif name.startswith("cam"):
            out[name] = structs.setdefault(name, _lib.Camera())
        elif name == "pg_params":
            out[name] = structs.setdefault(name, _lib.PoseGraphParams())
        elif name == "params":
            out[name] = structs.setdefault(name, params_type())
        elif name in ("ia", "ib", "ik", "ic", "i_first", "i_second"):
            out[name] = BLOCKS
        elif name == "table":
            out[name] = SimpleNamespace(d_start=device(address), d_obs=device(address + 8), n_obs=40, n_landmarks=7)
        elif name == "handle":
            out[name] = CONSENSUS._h
        elif name == "stream_to_wait":
            out[name] = stream
        elif name == "shuffle":
            out[name] = True
        else:
            out[name] = 5 + k
    return out


def plain(a):
    """an argument as ctypes received it, in a form that compares"""
    if isinstance(a, C.Array):
        return ("array",) + tuple(a)
    if isinstance(a, C.c_void_p):
        return ("handle", a.value)
    if hasattr(a, "_obj"):                              # byref(struct)
        return ("byref", type(a._obj).__name__, C.addressof(a._obj))
    return a


def drive(recorder, real, make, symbol, params_type, structs, device, optional, stream=0x1234):
    wrapper = make()
    del recorder.calls[:]
    wrapper(**arguments(wrapper, params_type, structs, device, optional, stream))
    assert [c[0] for c in recorder.calls] == [symbol]
    args = recorder.calls[0][1]
    argtypes = getattr(real, symbol).argtypes
    assert len(args) == len(argtypes), (symbol, len(args), len(argtypes))
    for i, (a, t) in enumerate(zip(args, argtypes)):
        try:
            t.from_param(a)
        except (TypeError, C.ArgumentError) as e:
            raise AssertionError(f"{symbol}: argument {i} ({a!r}) is not what {t.__name__} takes: {e}")
    return tuple(plain(a) for a in args)


@pytest.mark.parametrize("optional", [True, False], ids=["optional-given", "optional-none"])
@pytest.mark.parametrize("make,symbol,params_type", WRAPPERS, ids=IDS)
def test_ints_and_tensors_record_the_same_call(recorder, real, make, symbol, params_type, optional):
    structs = {}
    ints = drive(recorder, real, make, symbol, params_type, structs, int, optional)
    tensors = drive(recorder, real, make, symbol, params_type, structs, Tensor, optional)
    assert ints == tensors
    assert ints[0] == ("handle", HANDLE) and ints[-1] == 0x1234
    names = inspect.signature(make()).parameters
    if not optional and any(n.startswith("d_") and (p.default is None or n in NULLABLE) for n, p in names.items()):
        assert None in ints
    if any(n in names for n in ("ia", "ik", "ic")):
        assert ("array",) + tuple(BLOCKS) in ints and len(BLOCKS) in ints


@pytest.mark.parametrize("make,symbol,params_type", WRAPPERS, ids=IDS)
def test_a_stream_object_arrives_as_its_handle(recorder, real, make, symbol, params_type):
    """every wrapper of every module: the legacy default stream (handle 0) arrives as AKZ_STREAM_LEGACY, another stream as
    its handle, None as None"""
    assert drive(recorder, real, make, symbol, params_type, {}, Tensor, True, Stream(0))[-1] == _lib.STREAM_LEGACY
    assert drive(recorder, real, make, symbol, params_type, {}, Tensor, True, Stream(0x4321))[-1] == 0x4321
    assert drive(recorder, real, make, symbol, params_type, {}, int, True, None)[-1] is None


def test_the_stream_function():
    assert _device.wait(None) is None
    assert _device.wait(Stream(0)) == _lib.STREAM_LEGACY == 1
    assert _device.wait(Stream(0x1234)) == 0x1234
    assert _device.wait(0x1234) == 0x1234


def test_the_index_list(real):
    vp = real.rs_add_views_device.argtypes[11]
    assert vp is C.c_void_p
    empty, n = _device.index_list([])
    assert n == 0 and C.addressof(empty) != 0 and C.sizeof(empty) >= 4
    vp.from_param(empty)
    words, n = _device.index_list([3, 1, 2])
    assert n == 3 and list(words) == [3, 1, 2] and C.sizeof(words) == 12 and isinstance(words, C.Array)
    vp.from_param(words)


def test_from_param_is_a_check(real):
    """what the assertions above rest on: from_param takes ints, None, byref and arrays and refuses other objects"""
    vp, u32 = C.c_void_p, C.c_uint32
    for ok in (0x1000, None, C.byref(_lib.Camera()), (C.c_uint32 * 2)(1, 2), C.c_void_p(5)):
        vp.from_param(ok)
    C.POINTER(_lib.Camera).from_param(C.byref(_lib.Camera()))
    u32.from_param(7)
    for t, bad in ((vp, Tensor(0x1000)), (vp, Stream(0)), (vp, 1.5), (u32, None), (u32, Tensor(1)),
                   (C.POINTER(_lib.Camera), _lib.PoseGraphParams()), (C.POINTER(_lib.Camera), C.byref(_lib.PoseGraphParams()))):
        with pytest.raises((TypeError, C.ArgumentError)):
            t.from_param(bad)
