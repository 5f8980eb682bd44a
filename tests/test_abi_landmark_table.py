"""The C ABI of the landmark bookkeeping (include/akz.h): rs_landmarks_sharing_view_device and rs_add_views_device — symbols,
argument counts, constants, the refusals that come before the device; the ABI number stays 11, since the entry points are pure
additions.  No GPU needed: every refusal here is decided from the arguments alone, before the context is looked at."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cv_amd import _lib
from cv_amd import landmark_table
from cv_amd.landmark_table import LandmarkUpdate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_landmarks_sharing_view_device", "rs_add_views_device")


@pytest.fixture(scope="module")
def lib():
    from cv_amd.build import build
    build()
    return _lib.lib()


def test_abi_number_stays_11(lib):
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    assert int(re.search(r"#define\s+AKZ_ABI_VERSION\s+(\d+)u", hdr).group(1)) == 11
    assert lib.akz_abi_version() == 11 == _lib.ABI_VERSION
    rust = open(os.path.join(ROOT, "rust", "akaze-mi355x", "src", "lib.rs")).read()
    assert re.search(r"ABI_VERSION: u32 = 11\b", rust)
    for name in NAMES:
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"fn %s\(" % name, rust), name
    assert "pub struct LandmarkBook" in rust and "pub unsafe fn add_views(" in rust and "pub unsafe fn sharing_view(" in rust
    hpp = open(os.path.join(ROOT, "include", "akaze.hpp")).read()
    assert "class LandmarkBook" in hpp and "void sharing_view(" in hpp and "void add_views(" in hpp
    assert callable(LandmarkUpdate.sharing_view_tensors) and callable(LandmarkUpdate.add_views_tensors)
    assert len(landmark_table.VERDICTS) == 4


def _header_args(hdr, name):
    return [a.strip() for a in re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S).group(1).split(",")]


def test_the_declarations_have_the_headers_argument_counts(lib):
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    rust = open(os.path.join(ROOT, "rust", "akaze-mi355x", "src", "lib.rs")).read()
    for name in NAMES:
        args = _header_args(hdr, name)
        kinds = [C.c_uint32 if re.match(r"uint32_t\s+\w+$", a) else None for a in args]
        declared = getattr(lib, name).argtypes
        assert len(declared) == len(kinds), name
        for k, (want, got) in enumerate(zip(kinds, declared)):
            assert (got is C.c_uint32) == (want is C.c_uint32), (name, k)
        r_args = re.search(r"fn %s\(([^;]*?)\)\s*->\s*i32;" % name, rust, re.S).group(1).split(",")
        assert len(r_args) == len(args), name
        for k, (a, r) in enumerate(zip(args, r_args)):
            assert (r.strip().endswith(": u32")) == (kinds[k] is C.c_uint32), (name, k)
            assert r.strip().split(":")[0] == re.search(r"(\w+)$", a).group(1), (name, k)


def test_header_constants_are_the_bindings():
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    math = open(os.path.join(ROOT, "include", "akz_landmark_table_math.h")).read()
    rust = open(os.path.join(ROOT, "rust", "akaze-mi355x", "src", "lib.rs")).read()
    names = ("RS_AV_OK", "RS_AV_NOT_ACCEPTED", "RS_AV_BAD_INDEX", "RS_AV_BAD_TABLE", "RS_AV_S_OBSERVATIONS", "RS_AV_S_MERGED", "RS_AV_S_DEMOTED",
             "RS_AV_S_NEW_LANDMARKS", "RS_AV_STATS", "RS_AV_COUNTS", "RS_LT_TILE")
    for name in names:
        value = int(re.search(r"\b%s = (\d+)" % name, hdr).group(1))
        assert value == getattr(_lib, name), name
        if name != "RS_LT_TILE":
            assert int(re.search(r"\bAKZ_AV_%s = (\d+)" % name[6:], math).group(1)) == value, name
        m = re.search(r"pub const %s: \w+ = (\d+);" % name, rust)
        if m:
            assert int(m.group(1)) == value, name
    for k, name in enumerate(("Ok", "NotAccepted", "BadIndex", "BadTable")):
        assert re.search(r"%s = %d," % (name, k), rust.split("pub enum AddViewVerdict")[1].split("}")[0])
    assert re.search(r"pub const RS_LT_TILE: u32 = 1024;", rust) and re.search(r"pub const RS_AV_STATS: usize = 4;", rust)
    # the verdict the math header takes for "registered" is the refinement's RS_SV_OK
    assert int(re.search(r"AKZ_LT_SV_OK = (\d+)", math).group(1)) == _lib.RS_SV_OK
    hip = open(os.path.join(ROOT, "cv_amd", "csrc", "rs_landmark_table.hip")).read()
    # the tile the kernels scan is the exported one: stated once, in the header of the table stages' shared pieces
    tbl = open(os.path.join(ROOT, "cv_amd", "csrc", "rs_table.h")).read()
    assert "static_assert(kTblTile == (uint32_t)RS_LT_TILE" in tbl and '#include "rs_table.h"' in hip and "kTblTile" in hip
    assert not re.search(r"constexpr \w+ k\w+Tile\b", hip)


class Call:
    """rs_add_views_device on host memory that no kernel will ever see: every refusal below is returned before the context (NULL
    here) is looked at, so a status other than AKZ_E_INVALID from the base call would mean the checks came in another order"""

    def __init__(self, n_landmarks=4, n_obs=6, cap=4, n_blocks=5, ik=(3, 4), split_room=2):
        self.n_landmarks, self.n_obs, self.cap, self.n_blocks, self.split_room = n_landmarks, n_obs, cap, n_blocks, split_room
        self.ik = np.array(ik, np.uint32)
        F = len(ik)
        grow = split_room + F * cap
        self.obs_room, self.lm_room = n_obs + grow, n_landmarks + grow
        w = lambda n: np.zeros(max(n, 1), np.uint32)
        self.a = dict(start=w(n_landmarks + 1), obs=w(2 * n_obs), split=w(2 * split_room), split_count=w(1), counts=w(n_blocks),
                      matches=w(2 * F * cap), nmatches=w(F), final=np.zeros(max(F * cap, 1), np.uint8), verdict=w(F), pose_out=np.zeros(12 * max(F, 1)),
                      best=w(6 * F * cap), skip=w(F), poses=np.zeros(12 * n_blocks), start_out=w(self.lm_room + 1), obs_out=w(2 * self.obs_room),
                      counts_out=w(4), landmarks_out=w(n_blocks * cap), obs_counts_out=w(self.lm_room), frame_verdict=w(F), stats=w(4 * F),
                      call_verdict=w(1))

    def run(self, lib, ctx=None, **over):
        p = {k: v.ctypes.data for k, v in self.a.items()}
        v = dict(n_obs=self.n_obs, n_landmarks=self.n_landmarks, n_world=self.n_landmarks, split_room=self.split_room, cap=self.cap,
                 n_blocks=self.n_blocks, ik=self.ik.ctypes.data, n_frames=len(self.ik), obs_room=self.obs_room, lm_room=self.lm_room)
        p.update(v)
        p.update(over)
        return lib.rs_add_views_device(ctx, p["start"], p["obs"], p["n_obs"], p["n_landmarks"], p["n_world"], p["split"], p["split_count"],
                                       p["split_room"], p["cap"], p["n_blocks"], p["ik"], p["n_frames"], p["counts"], p["matches"], p["nmatches"],
                                       p["final"], p["verdict"], p["pose_out"], p["best"], p["skip"], p["obs_room"], p["lm_room"], p["poses"],
                                       p["start_out"], p["obs_out"], p["counts_out"], p["landmarks_out"], p["obs_counts_out"],
                                       p["frame_verdict"], p["stats"], p["call_verdict"], None)


def test_refusals_come_before_the_device(lib):
    c = Call()
    assert c.run(lib) == -1                                               # a complete call gets as far as the context: there is none
    for name in ("start", "obs", "ik", "counts", "matches", "nmatches", "final", "verdict", "pose_out", "poses", "start_out", "obs_out", "counts_out",
                 "landmarks_out", "obs_counts_out", "frame_verdict", "stats", "call_verdict"):
        assert c.run(lib, **{name: None}) == -1, name
    assert c.run(lib, cap=0) == -1 and c.run(lib, n_blocks=0) == -1 and c.run(lib, n_frames=65536) == -1
    assert c.run(lib, split=None) == -1 and c.run(lib, split_count=None) == -1            # one without the other
    assert c.run(lib, split=None, split_count=None) == -1                                 # no list, but a room for one
    assert c.run(lib, n_landmarks=0xFFFFFFFF) == -6 and c.run(lib, n_landmarks=0xFFFFFFFF - 2048 + 1) == -6       # AKZ_E_TOO_LARGE
    assert c.run(lib, obs_room=c.obs_room - 1) == -1 and c.run(lib, lm_room=c.lm_room - 1) == -1
    assert c.run(lib, lm_room=0xFFFFFFFF) == -1


def test_refusals_are_told_apart_from_the_missing_context(lib):
    """With a context that is not NULL but that no accepted call may reach: a refusal must return before touching it.  The
    pointer is never dereferenced, because every call below is refused."""
    bogus = C.c_void_p(8)
    c = Call()
    assert c.run(lib, ctx=bogus, obs_room=c.obs_room - 1) == -1                           # rooms too small
    assert c.run(lib, ctx=bogus, lm_room=c.lm_room - 1) == -1
    assert Call(ik=(3, 3)).run(lib, ctx=bogus) == -1                                      # a repeated block
    assert Call(ik=(3, 5)).run(lib, ctx=bogus) == -1                                      # a block outside the blocks
    # outputs that lie over the input table
    start, obs = c.a["start"].ctypes.data, c.a["obs"].ctypes.data
    for out in ("start_out", "obs_out", "obs_counts_out", "landmarks_out", "counts_out"):
        assert c.run(lib, ctx=bogus, **{out: start}) == -1, out
        assert c.run(lib, ctx=bogus, **{out: obs + 4}) == -1, out
    assert c.run(lib, ctx=bogus, start_out=start - 4 * c.lm_room) == -1                   # its last word only
    # the mask
    assert lib.rs_landmarks_sharing_view_device(None, start, obs, 6, 4, obs, obs, 4, 2, obs, None) == -1
    for k in (1, 5, 6, 9):
        args = [bogus, start, obs, 6, 4, obs, obs, 4, 2, obs, None]
        args[k] = None
        assert lib.rs_landmarks_sharing_view_device(*args) == -1, k
    assert lib.rs_landmarks_sharing_view_device(bogus, start, obs, 6, 4, obs, obs, 0, 2, obs, None) == -1
    assert lib.rs_landmarks_sharing_view_device(bogus, start, obs, 6, 4, obs, obs, 4, 65536, obs, None) == -1


def test_the_cpp_mirror_compiles(lib, tmp_path):
    import host_build
    exe = host_build.native(tmp_path, "landmark_table.cpp", hip=True)
    assert os.path.exists(exe)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
        assert r.returncode == 2
