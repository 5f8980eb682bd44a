"""The C ABI of the two steps that start a reconstruction (include/akz.h): rs_join_pairs_batch_device and
rs_add_reconstruction_batch_device — symbols, argument counts and kinds, constants, the refusals that come before the device; the
ABI number stays 11, since the entry points are pure additions.  No GPU needed: every refusal here is decided from the arguments
alone, before the context is looked at."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cv_amd import _lib
from cv_amd import bootstrap
from cv_amd.bootstrap import PairJoin, ReconstructionStart

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_join_pairs_batch_device", "rs_add_reconstruction_batch_device")
INVALID, TOO_LARGE = -1, -6


@pytest.fixture(scope="module")
def lib():
    from cv_amd.build import build
    build()
    return _lib.lib()


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_abi_number_stays_11(lib):
    hdr, rust, hpp = read("include", "akz.h"), read("rust", "akaze-mi355x", "src", "lib.rs"), read("include", "akaze.hpp")
    assert int(re.search(r"#define\s+AKZ_ABI_VERSION\s+(\d+)u", hdr).group(1)) == 11
    assert lib.akz_abi_version() == 11 == _lib.ABI_VERSION
    assert re.search(r"ABI_VERSION: u32 = 11\b", rust)
    for name in NAMES:
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"fn %s\(" % name, rust), name
        assert re.search(r"\b%s\(" % name, hpp.split("class ReconstructionStart")[1]), name
    assert "pub struct ReconstructionStart" in rust and "class ReconstructionStart" in hpp
    for method in ("join_pairs_device", "add_reconstruction_device"):
        assert re.search(r"pub unsafe fn %s\(" % method, rust.split("pub struct ReconstructionStart")[1]), method
        assert "void %s(" % method in hpp.split("class ReconstructionStart")[1], method
    assert "not compiled here" in rust.split("pub struct ReconstructionStart")[0].rsplit("///", 1)[1]
    for method in ("join_device", "join_tensors", "run"):
        assert callable(getattr(PairJoin, method)), method
    for method in ("add_device", "add_tensors", "run"):
        assert callable(getattr(ReconstructionStart, method)), method
    assert len(bootstrap.JOIN_VERDICTS) == 4 and len(bootstrap.VERDICTS) == 5
    assert "rs_bootstrap_table.hip" in read("cv_amd", "build.py") and "akz_bootstrap_table_math.h" in read("cv_amd", "build.py")


def _header_args(hdr, name):
    return [a.strip() for a in re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S).group(1).split(",")]


def test_the_declarations_have_the_headers_argument_counts_and_kinds(lib):
    hdr, rust = read("include", "akz.h"), read("rust", "akaze-mi355x", "src", "lib.rs")
    for name in NAMES:
        args = _header_args(hdr, name)
        kinds = [C.c_uint32 if re.match(r"uint32_t\s+\w+$", a) else C.c_uint64 if re.match(r"uint64_t\s+\w+$", a) else None for a in args]
        declared = getattr(lib, name).argtypes
        assert len(declared) == len(kinds), name
        for k, (want, got) in enumerate(zip(kinds, declared)):
            assert (got is C.c_uint32) == (want is C.c_uint32) and (got is C.c_uint64) == (want is C.c_uint64), (name, k)
        r_args = re.search(r"fn %s\(([^;]*?)\)\s*->\s*i32;" % name, rust, re.S).group(1).split(",")
        assert len(r_args) == len(args), name
        for k, (a, r) in enumerate(zip(args, r_args)):
            assert (r.strip().endswith(": u32")) == (kinds[k] is C.c_uint32) and (r.strip().endswith(": u64")) == (kinds[k] is C.c_uint64), (name, k)
            assert r.strip().split(":")[0] == re.search(r"(\w+)$", a).group(1), (name, k)
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [25, 49]


def test_header_constants_are_the_bindings_and_the_math_headers():
    hdr, math, rust = read("include", "akz.h"), read("include", "akz_bootstrap_table_math.h"), read("rust", "akaze-mi355x", "src", "lib.rs")
    names = ("RS_JP_OK", "RS_JP_NO_MODEL", "RS_JP_FEW_INLIERS", "RS_JP_BAD_INDEX", "RS_AR_OK", "RS_AR_NOT_ACCEPTED", "RS_AR_BAD_INDEX", "RS_AR_TAKEN",
             "RS_AR_BAD_TABLE", "RS_AR_S_TRIPLES", "RS_AR_S_FIRST", "RS_AR_S_SECOND", "RS_AR_S_LANDMARKS", "RS_AR_STATS", "RS_AR_COUNTS")
    for name in names:
        value = int(re.search(r"\b%s = (\d+)" % name, hdr).group(1))
        assert value == getattr(_lib, name), name
        assert int(re.search(r"\bAKZ_%s = (\d+)" % name[3:], math).group(1)) == value, name
        m = re.search(r"pub const %s: \w+ = (\d+);" % name, rust)
        if m:
            assert int(m.group(1)) == value, name
    for name in ("RS_JP_DEFAULT_MINIMUM_ROBUST_MATCHES", "RS_JP_MAX_FEATURES"):
        value = int(re.search(r"\b%s = (\d+)" % name, hdr).group(1))
        assert value == getattr(_lib, name) == int(re.search(r"pub const %s: u32 = (\d+);" % name, rust).group(1)), name
    assert _lib.RS_JP_DEFAULT_MINIMUM_ROBUST_MATCHES == 1 << 8 and _lib.RS_JP_MAX_FEATURES == _lib.RS_TV_MAX_COMMON
    for k, name in enumerate(("Ok", "NoModel", "FewInliers", "BadIndex")):
        assert re.search(r"%s = %d," % (name, k), rust.split("pub enum JoinVerdict")[1].split("}")[0])
    for k, name in enumerate(("Ok", "NotAccepted", "BadIndex", "Taken", "BadTable")):
        assert re.search(r"%s = %d," % (name, k), rust.split("pub enum AddReconstructionVerdict")[1].split("}")[0])
    # the stages' own verdicts the math header restates, and the tile the kernels scan
    assert int(re.search(r"AKZ_BT_NOT_RECORDED = (\d+)", math).group(1)) == _lib.RS_CV_NOT_RECORDED
    assert int(re.search(r"AKZ_BT_TV_OK = (\d+)", math).group(1)) == _lib.RS_TV_OK == _lib.RS_TVC_OK
    hip = read("cv_amd", "csrc", "rs_bootstrap_table.hip")
    # the tile the kernels scan is the exported one: stated once, in the header of the table stages' shared pieces
    tbl = open(os.path.join(ROOT, "cv_amd", "csrc", "rs_table.h")).read()
    assert "static_assert(kTblTile == (uint32_t)RS_LT_TILE" in tbl and '#include "rs_table.h"' in hip and "kTblTile" in hip
    assert not re.search(r"constexpr \w+ k\w+Tile\b", hip)
    # the helpers are akz_common.h's: used, not copied
    assert "lds_radix_sort_ids(" in hip and "akz_block_scan<" in hip and "uint32_t* lds_radix_sort_ids" not in hip
    import bootstrap_table_checker as K
    assert (K.JP_OK, K.JP_NO_MODEL, K.JP_FEW_INLIERS, K.JP_BAD_INDEX) == (_lib.RS_JP_OK, _lib.RS_JP_NO_MODEL, _lib.RS_JP_FEW_INLIERS, _lib.RS_JP_BAD_INDEX)
    assert (K.AR_OK, K.AR_NOT_ACCEPTED, K.AR_BAD_INDEX, K.AR_TAKEN, K.AR_BAD_TABLE, K.STATS, K.COUNTS, K.TILE) == (
        _lib.RS_AR_OK, _lib.RS_AR_NOT_ACCEPTED, _lib.RS_AR_BAD_INDEX, _lib.RS_AR_TAKEN, _lib.RS_AR_BAD_TABLE, _lib.RS_AR_STATS, _lib.RS_AR_COUNTS,
        _lib.RS_LT_TILE)
    assert K.KP_BYTES == _lib.KP_DTYPE.itemsize


class Join:
    """rs_join_pairs_batch_device on host memory that no kernel will ever see: every refusal below is returned before the
    context (NULL here) is looked at"""
    ORDER = ("pairs", "npairs", "inliers", "n_inliers", "best_id", "pose", "n_slots", "cap", "slot_first", "slot_second", "n_scenes", "minimum",
             "flags", "seed", "triples", "ntriples", "first_only", "nfirst", "second_only", "nsecond", "pose_first", "pose_second", "verdict")

    def __init__(self, n_slots=3, cap=4, scenes=((0, 1), (2, 1))):
        w = lambda n: np.zeros(max(n, 1), np.uint32)
        S = len(scenes)
        self.keep = dict(pairs=w(2 * n_slots * cap), npairs=w(n_slots), inliers=w(n_slots * cap), n_inliers=w(n_slots), best_id=w(n_slots),
                         pose=np.zeros(12 * n_slots), slot_first=np.array([a for a, _ in scenes], np.uint32),
                         slot_second=np.array([b for _, b in scenes], np.uint32), triples=w(3 * S * cap), ntriples=w(S), first_only=w(2 * S * cap),
                         nfirst=w(S), second_only=w(2 * S * cap), nsecond=w(S), pose_first=np.zeros(12 * S), pose_second=np.zeros(12 * S), verdict=w(S))
        self.v = dict(n_slots=n_slots, cap=cap, n_scenes=S, minimum=0, flags=0, seed=0)

    def run(self, lib, ctx=None, **over):
        p = {k: a.ctypes.data for k, a in self.keep.items()}
        p.update(self.v)
        p.update(over)
        return lib.rs_join_pairs_batch_device(ctx, *(p[k] for k in self.ORDER), None)


class Add:
    """rs_add_reconstruction_batch_device the same way"""
    ORDER = ("triples", "ntriples", "first_only", "nfirst", "second_only", "nsecond", "combined", "first_ok", "second_ok", "pose_out", "tv_verdict",
             "ic", "i_first", "i_second", "n_scenes", "kps", "counts", "n_src_blocks", "cap", "skip", "obs_start", "obs", "n_obs", "n_landmarks",
             "recon_start", "view_start", "n_recons", "kps_dst", "counts_dst", "poses", "n_blocks", "view_base", "obs_room", "lm_room",
             "obs_start_out", "obs_out", "obs_counts_out", "counts_out", "landmarks_out", "recon_start_out", "view_start_out", "views_out",
             "constraint_poses_out", "constraint_verdict_out", "frame_verdict", "stats", "call_verdict")

    def __init__(self, cap=4, n_src_blocks=6, n_blocks=9, view_base=3, frames=((0, 1, 2), (3, 4, 5)), n_landmarks=4, n_obs=6, n_recons=1):
        w = lambda n: np.zeros(max(n, 1), np.uint32)
        b = lambda n: np.zeros(max(n, 1), np.uint8)
        S = len(frames)
        self.obs_room, self.lm_room = n_obs + 3 * S * cap, n_landmarks + 3 * S * cap
        self.keep = dict(triples=w(3 * S * cap), ntriples=w(S), first_only=w(2 * S * cap), nfirst=w(S), second_only=w(2 * S * cap), nsecond=w(S),
                         combined=b(S * cap), first_ok=b(S * cap), second_ok=b(S * cap), pose_out=np.zeros(24 * S), tv_verdict=w(S),
                         ic=np.array([f[0] for f in frames], np.uint32), i_first=np.array([f[1] for f in frames], np.uint32),
                         i_second=np.array([f[2] for f in frames], np.uint32), kps=b(28 * n_src_blocks * cap), counts=w(n_src_blocks), skip=w(S),
                         obs_start=w(n_landmarks + 1), obs=w(2 * n_obs), recon_start=w(n_recons + 1), view_start=w(n_recons + 1),
                         kps_dst=b(28 * n_blocks * cap), counts_dst=w(n_blocks), poses=np.zeros(12 * n_blocks), obs_start_out=w(self.lm_room + 1),
                         obs_out=w(2 * self.obs_room), obs_counts_out=w(self.lm_room), counts_out=w(4), landmarks_out=w(n_blocks * cap),
                         recon_start_out=w(n_recons + S + 1), view_start_out=w(n_recons + S + 1), views_out=w(3 * S), constraint_poses_out=np.zeros(24 * S),
                         constraint_verdict_out=w(S), frame_verdict=w(S), stats=w(4 * S), call_verdict=w(1))
        self.v = dict(n_scenes=S, n_src_blocks=n_src_blocks, cap=cap, n_obs=n_obs, n_landmarks=n_landmarks, n_recons=n_recons, n_blocks=n_blocks,
                      view_base=view_base, obs_room=self.obs_room, lm_room=self.lm_room)

    def ptr(self, name):
        return self.keep[name].ctypes.data

    def run(self, lib, ctx=None, **over):
        p = {k: a.ctypes.data for k, a in self.keep.items()}
        p.update(self.v)
        p.update(over)
        return lib.rs_add_reconstruction_batch_device(ctx, *(p[k] for k in self.ORDER), None)


BOGUS = C.c_void_p(8)     # a context that is not NULL but that no accepted call may reach: a refusal must return before touching it


def test_the_joins_refusals_come_before_the_device(lib):
    j = Join()
    assert j.run(lib) == INVALID                                           # a complete call gets as far as the context: there is none
    for name in j.keep:
        assert j.run(lib, ctx=BOGUS, **{name: None}) == INVALID, name
    assert j.run(lib, ctx=BOGUS, cap=0) == INVALID and j.run(lib, ctx=BOGUS, n_scenes=65536) == INVALID
    assert j.run(lib, ctx=BOGUS, flags=2) == INVALID and j.run(lib, ctx=BOGUS, flags=3) == INVALID
    assert j.run(lib, ctx=BOGUS, cap=_lib.RS_JP_MAX_FEATURES + 1) == TOO_LARGE
    assert j.run(lib, ctx=BOGUS, cap=8193, flags=_lib.RS_BATCH_SHUFFLE) == TOO_LARGE    # the flag needs cap_per_img <= 8192
    assert j.run(lib, cap=8193) == INVALID and j.run(lib, cap=8192, flags=_lib.RS_BATCH_SHUFFLE) == INVALID   # as far as the context
    assert Join(scenes=((0, 3),)).run(lib, ctx=BOGUS) == INVALID and Join(scenes=((3, 0),)).run(lib, ctx=BOGUS) == INVALID


def test_the_refusals_of_add_reconstruction_come_before_the_device(lib):
    a = Add()
    assert a.run(lib) == INVALID                                           # as far as the context
    optional = ("skip",)
    for name in a.keep:
        if name not in optional:
            assert a.run(lib, ctx=BOGUS, **{name: None}) == INVALID, name
    assert a.run(lib, skip=None) == INVALID
    assert a.run(lib, ctx=BOGUS, cap=0) == INVALID and a.run(lib, ctx=BOGUS, n_blocks=0) == INVALID and a.run(lib, ctx=BOGUS, n_scenes=65536) == INVALID
    # the ranges come with a table of reconstructions or not at all
    assert a.run(lib, ctx=BOGUS, n_recons=0) == INVALID and a.run(lib, n_recons=0, recon_start=None, view_start=None) == INVALID
    assert a.run(lib, ctx=BOGUS, n_recons=0, recon_start=None) == INVALID
    # the destination range
    assert a.run(lib, ctx=BOGUS, view_base=4) == INVALID and a.run(lib, ctx=BOGUS, n_blocks=8) == INVALID
    # the rooms
    assert a.run(lib, ctx=BOGUS, obs_room=a.obs_room - 1) == INVALID and a.run(lib, ctx=BOGUS, lm_room=a.lm_room - 1) == INVALID
    assert a.run(lib, ctx=BOGUS, lm_room=0xFFFFFFFF) == INVALID
    assert a.run(lib, ctx=BOGUS, n_landmarks=0xFFFFFFFF - 2048 + 1, lm_room=0xFFFFFFFE) == TOO_LARGE
    # a source block outside the pool
    assert Add(frames=((0, 1, 6),)).run(lib, ctx=BOGUS) == INVALID and Add(frames=((6, 1, 2),)).run(lib, ctx=BOGUS) == INVALID
    # the pools: a partial overlap; one pool whose destination range holds a named source block
    assert a.run(lib, ctx=BOGUS, kps_dst=a.ptr("kps") + 28 * 4) == INVALID and a.run(lib, ctx=BOGUS, kps_dst=a.ptr("kps") - 28 * 4) == INVALID
    assert a.run(lib, ctx=BOGUS, kps_dst=a.ptr("kps"), n_src_blocks=9) == INVALID           # blocks 3, 4, 5 are sources and views
    same_pool = Add(frames=((0, 1, 2),), view_base=3)
    assert same_pool.run(lib, ctx=None, kps_dst=same_pool.ptr("kps"), n_src_blocks=9) == INVALID   # apart: as far as the context ...
    one = Add(frames=((0, 1, 5),), view_base=3)
    assert one.run(lib, ctx=BOGUS, kps_dst=one.ptr("kps"), n_src_blocks=9) == INVALID        # ... and view 5 is a source: refused
    # outputs that lie over the input table or its ranges
    for out in ("obs_start_out", "obs_out", "obs_counts_out", "landmarks_out", "counts_out", "recon_start_out", "view_start_out"):
        for inp in ("obs_start", "obs", "recon_start", "view_start"):
            assert a.run(lib, ctx=BOGUS, **{out: a.ptr(inp)}) == INVALID, (out, inp)
        assert a.run(lib, ctx=BOGUS, **{out: a.ptr("obs") + 4}) == INVALID, out
    assert a.run(lib, ctx=BOGUS, obs_start_out=a.ptr("obs_start") - 4 * a.lm_room) == INVALID    # its last word only


def test_the_cpp_mirror_compiles(lib, tmp_path):
    import host_build
    exe = host_build.native(tmp_path, "bootstrap.cpp", hip=True)
    assert os.path.exists(exe)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
        assert r.returncode == 2
