"""The C ABI of the merge of two reconstructions (include/akz.h): rs_merge_map_device, rs_incorporate_reconstruction_device
and rs_normalize_reconstruction_device — symbols, argument counts and kinds, constants, the refusals that come before the
device; the ABI number stays 11, since the entry points are pure additions.  No GPU needed: every refusal here is decided from
the arguments alone, before the context is looked at."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cv_amd import _lib
from cv_amd import reconstruction_merge
from cv_amd.reconstruction_merge import ReconstructionMerge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_merge_map_device", "rs_incorporate_reconstruction_device", "rs_normalize_reconstruction_device")
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
        assert re.search(r"fn %s\(" % name, rust) and re.search(r"\b%s\(ctx_" % name, hpp), name
    assert "pub struct ReconstructionMerge" in rust
    assert "class ReconstructionMerge" in hpp
    for method in ("merge_map", "incorporate", "normalize"):
        assert "pub unsafe fn %s(" % method in rust.split("pub struct ReconstructionMerge")[1], method
        assert "void %s(" % method in hpp.split("class ReconstructionMerge")[1], method
        for form in ("%s_device", "%s_tensors", "run_%s"):
            assert callable(getattr(ReconstructionMerge, form % method)), (form, method)
    assert len(reconstruction_merge.VERDICTS) == 4 and len(reconstruction_merge.NORMALIZE_VERDICTS) == 3
    from cv_amd.reconstruction import merge_reconstructions
    assert callable(merge_reconstructions)
    assert "rs_reconstruction_merge.hip" in read("cv_amd", "build.py")


def _header_args(hdr, name):
    return [a.strip() for a in re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S).group(1).split(",")]


def test_the_declarations_have_the_headers_argument_counts_and_kinds(lib):
    hdr, rust = read("include", "akz.h"), read("rust", "akaze-mi355x", "src", "lib.rs")
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
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [16, 30, 15]


def test_header_constants_are_the_bindings_and_the_math_headers():
    hdr, math = read("include", "akz.h"), read("include", "akz_reconstruction_merge_math.h")
    rust = read("rust", "akaze-mi355x", "src", "lib.rs")
    names = ("RS_IR_OK", "RS_IR_BAD_TABLE", "RS_IR_BAD_INDEX", "RS_IR_SHARED_BLOCK", "RS_IR_C_ROWS", "RS_IR_C_OBSERVATIONS", "RS_IR_C_APPLIED",
             "RS_IR_C_DEMOTED", "RS_IR_C_NEW_ROWS", "RS_IR_C_DROPPED", "RS_IR_COUNTS", "RS_NR_OK", "RS_NR_NOT_NORMAL", "RS_NR_BAD_INDEX")
    for name in names:
        value = int(re.search(r"\b%s = (\d+)" % name, hdr).group(1))
        assert value == getattr(_lib, name), name
        assert int(re.search(r"\bAKZ_%s = (\d+)" % name[3:], math).group(1)) == value, name
        m = re.search(r"pub const %s: \w+ = (\d+);" % name, rust)
        if m:
            assert int(m.group(1)) == value, name
    assert re.search(r"pub const RS_IR_COUNTS: usize = 6;", rust)
    for k, name in enumerate(("Ok", "BadTable", "BadIndex", "SharedBlock")):
        assert re.search(r"%s = %d," % (name, k), rust.split("pub enum IncorporateVerdict")[1].split("}")[0])
    for k, name in enumerate(("Ok", "NotNormal", "BadIndex")):
        assert re.search(r"%s = %d," % (name, k), rust.split("pub enum NormalizeVerdict")[1].split("}")[0])
    hip = read("cv_amd", "csrc", "rs_reconstruction_merge.hip")
    # the tile the kernels scan is the exported one: stated once, in the header of the table stages' shared pieces
    tbl = open(os.path.join(ROOT, "cv_amd", "csrc", "rs_table.h")).read()
    assert "static_assert(kTblTile == (uint32_t)RS_LT_TILE" in tbl and '#include "rs_table.h"' in hip and "kTblTile" in hip
    assert not re.search(r"constexpr \w+ k\w+Tile\b", hip) and "static_assert(kTblBlock == AKZ_SUM_THREADS" in hip
    # the source is "not compiled here" where the others say so
    assert "not compiled here" in rust.split("pub struct ReconstructionMerge")[0].rsplit("///", 1)[1]


class Incorporate:
    """rs_incorporate_reconstruction_device on host memory that no kernel will ever see: every refusal below is returned before
    the context (NULL here) is looked at, so a status other than AKZ_E_INVALID from the base call would mean the checks came in
    another order"""

    def __init__(self, n_dst=4, n_dst_obs=6, n_src=3, n_src_obs=5, cap=4, n_blocks=6, src_blocks=(3, 4), bridge_block=2, map_room=2):
        self.v = dict(n_dst_obs=n_dst_obs, n_dst=n_dst, n_src_obs=n_src_obs, n_src=n_src, map_room=map_room, cap=cap, n_blocks=n_blocks,
                      n_src_views=len(src_blocks), bridge_block=bridge_block, obs_room=n_dst_obs + n_src_obs, lm_room=n_dst + n_src)
        self.obs_room, self.lm_room = self.v["obs_room"], self.v["lm_room"]
        w = lambda n: np.zeros(max(n, 1), np.uint32)
        self.a = dict(dst_start=w(n_dst + 1), dst_obs=w(2 * n_dst_obs), src_start=w(n_src + 1), src_obs=w(2 * n_src_obs), map=w(2 * map_room),
                      map_count=w(1), src_blocks=np.array(src_blocks, np.uint32), src_pose=np.zeros(12), skip=w(len(src_blocks)),
                      poses=np.zeros(12 * n_blocks), start_out=w(self.lm_room + 1), obs_out=w(2 * self.obs_room), counts_out=w(6),
                      landmarks_out=w(n_blocks * cap), obs_counts_out=w(self.lm_room), src_key_out=w(n_src), call_verdict=w(1))

    def run(self, lib, ctx=None, **over):
        p = {k: v.ctypes.data for k, v in self.a.items()}
        p.update(self.v)
        p.update(over)
        return lib.rs_incorporate_reconstruction_device(
            ctx, p["dst_start"], p["dst_obs"], p["n_dst_obs"], p["n_dst"], p["src_start"], p["src_obs"], p["n_src_obs"], p["n_src"], p["map"],
            p["map_count"], p["map_room"], p["cap"], p["n_blocks"], p["src_blocks"], p["n_src_views"], p["bridge_block"], p["src_pose"], p["skip"],
            p["obs_room"], p["lm_room"], p["poses"], p["start_out"], p["obs_out"], p["counts_out"], p["landmarks_out"], p["obs_counts_out"],
            p["src_key_out"], p["call_verdict"], None)


def test_incorporate_refusals_come_before_the_device(lib):
    c = Incorporate()
    assert c.run(lib) == INVALID                                          # a complete call gets as far as the context: there is none
    for name in ("dst_start", "dst_obs", "src_start", "src_obs", "map", "map_count", "src_blocks", "src_pose", "poses", "start_out", "obs_out",
                 "counts_out", "landmarks_out", "obs_counts_out", "src_key_out", "call_verdict"):
        assert c.run(lib, **{name: None}) == INVALID, name
    assert c.run(lib, cap=0) == INVALID and c.run(lib, n_blocks=0) == INVALID and c.run(lib, bridge_block=6) == INVALID
    assert c.run(lib, n_dst=0xFFFFFFFF) == TOO_LARGE and c.run(lib, n_src=0xFFFFFFFF - 2048 + 1) == TOO_LARGE
    assert c.run(lib, n_src_obs=0xFFFFFFFF) == TOO_LARGE
    assert c.run(lib, lm_room=0xFFFFFFFF) == INVALID


def test_incorporate_refusals_are_told_apart_from_the_missing_context(lib):
    """With a context that is not NULL but that no accepted call may reach: a refusal must return before touching it.  The
    pointer is never dereferenced, because every call below is refused."""
    bogus = C.c_void_p(8)
    c = Incorporate()
    assert c.run(lib, ctx=bogus, obs_room=c.obs_room - 1) == INVALID      # rooms one too small
    assert c.run(lib, ctx=bogus, lm_room=c.lm_room - 1) == INVALID
    assert Incorporate(src_blocks=(3, 3)).run(lib, ctx=bogus) == INVALID   # a repeated block
    assert Incorporate(src_blocks=(3, 6)).run(lib, ctx=bogus) == INVALID   # a block outside the blocks
    assert Incorporate(src_blocks=(3, 2)).run(lib, ctx=bogus) == INVALID   # the bridging frame's block among the source's views
    # outputs that lie over an input table or the map
    for table in ("dst_start", "dst_obs", "src_start", "src_obs", "map"):
        at = c.a[table].ctypes.data
        for out in ("start_out", "obs_out", "obs_counts_out", "landmarks_out", "counts_out", "src_key_out"):
            assert c.run(lib, ctx=bogus, **{out: at}) == INVALID, (table, out)
            assert c.run(lib, ctx=bogus, **{out: at + 4}) == INVALID, (table, out)
    assert c.run(lib, ctx=bogus, start_out=c.a["dst_start"].ctypes.data - 4 * c.lm_room) == INVALID     # its last word only


def test_merge_map_and_normalize_refusals_come_before_the_device(lib):
    bogus = C.c_void_p(8)
    w = np.zeros(64, np.uint32).ctypes.data
    # ctx, matches, nmatches, final, best, n_world, n_dst, cap, slot, counts, src_landmarks, n_blocks, bridge, map, map_count, stream
    base = [bogus, w, w, w, None, 6, 6, 4, 0, w, w, 4, 2, w, w, None]
    assert lib.rs_merge_map_device(*([None] + base[1:])) == INVALID        # complete, but for the context
    for k in (1, 2, 3, 9, 10, 13, 14):
        args = list(base)
        args[k] = None
        assert lib.rs_merge_map_device(*args) == INVALID, k
    for k, v in ((7, 0), (11, 0), (12, 4), (8, 65535)):
        args = list(base)
        args[k] = v
        assert lib.rs_merge_map_device(*args) == INVALID, k
    views = np.array([1, 0, 3], np.uint32)
    d = np.zeros(64).ctypes.data
    # ctx, view_blocks, n_views, counts, landmarks, cap, n_blocks, world, n_world, poses, constraint_poses, n_constraints, stats, verdict, stream
    base = [bogus, views.ctypes.data, 3, w, w, 4, 4, d, 5, d, d, 2, d, w, None]
    assert lib.rs_normalize_reconstruction_device(*([None] + base[1:])) == INVALID
    for k in (1, 3, 4, 7, 9, 10, 12, 13):
        args = list(base)
        args[k] = None
        assert lib.rs_normalize_reconstruction_device(*args) == INVALID, k
    for k, v in ((2, 0), (5, 0), (6, 0)):
        args = list(base)
        args[k] = v
        assert lib.rs_normalize_reconstruction_device(*args) == INVALID, k
    twice = np.array([1, 0, 1], np.uint32)
    assert lib.rs_normalize_reconstruction_device(*([bogus, twice.ctypes.data] + base[2:])) == INVALID     # a repeated block
    no_constraints = list(base)
    no_constraints[0], no_constraints[10], no_constraints[11] = None, None, 0                              # complete without constraints
    assert lib.rs_normalize_reconstruction_device(*no_constraints) == INVALID


def test_merge_reconstructions_wants_adjacent_ranges():
    from cv_amd.reconstruction import merge_reconstructions
    for dst, src, bridge in (((0, 4), (5, 9), 5), ((0, 4), (3, 9), 3), ((0, 4), (4, 9), 9)):
        with pytest.raises(ValueError):
            merge_reconstructions(None, None, None, None, None, 8, None, None, dst, src, bridge, None, 0, None, None, None, None, None)


def test_the_cpp_mirror_compiles(lib, tmp_path):
    import host_build
    exe = host_build.native(tmp_path, "reconstruction_merge.cpp", hip=True)
    assert os.path.exists(exe)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
        assert r.returncode == 2
