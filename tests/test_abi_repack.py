"""The C ABI of the repacking (include/akz.h): rs_repack_table_device, rs_gather_blocks_device, rs_repack_constraints_device and
hm_place_remap_views_device — symbols, argument counts and kinds, constants, the refusals that come before the device; the ABI
number stays 11, since the entry points are pure additions.  No GPU needed: every refusal here is decided from the arguments
alone, before the context is looked at."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cv_amd import _lib, repack
from cv_amd.place_recognition import FrameIndex
from cv_amd.repack import TableRepack

import repack_catalogue as cat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_repack_table_device", "rs_gather_blocks_device", "rs_repack_constraints_device", "hm_place_remap_views_device")
INVALID = -1


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
    hpp = open(os.path.join(ROOT, "include", "akaze.hpp")).read()
    assert "class TableRepack" in hpp and "void table(" in hpp and "void gather(" in hpp and "void constraints(" in hpp
    for f in ("table_device", "table_tensors", "run_table", "gather_device", "gather_tensors", "run_gather", "constraints_device",
              "constraints_tensors", "run_constraints"):
        assert callable(getattr(TableRepack, f)), f
    assert callable(FrameIndex.remap_views)
    assert len(repack.VERDICTS) == 5
    from cv_amd import reconstruction
    assert callable(reconstruction.repack)
    assert "rs_repack.hip" in open(os.path.join(ROOT, "cv_amd", "build.py")).read()


def _header_args(hdr, name):
    return [a.strip() for a in re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S).group(1).split(",")]


def test_the_declarations_have_the_headers_argument_counts_and_kinds(lib):
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


def test_header_constants_are_the_bindings_and_the_math_headers():
    hdr = open(os.path.join(ROOT, "include", "akz.h")).read()
    math = open(os.path.join(ROOT, "include", "akz_repack_math.h")).read()
    names = ("RS_RP_OK", "RS_RP_BAD_TABLE", "RS_RP_BAD_INDEX", "RS_RP_BAD_MAP", "RS_RP_NO_ROOM", "RS_RP_C_ROWS", "RS_RP_C_OBSERVATIONS",
             "RS_RP_C_EMPTY_DROPPED", "RS_RP_C_ROWS_DROPPED", "RS_RP_C_OBS_DROPPED", "RS_RP_COUNTS")
    for name in names:
        value = int(re.search(r"\b%s = (\d+)" % name, hdr).group(1))
        assert value == getattr(_lib, name), name
        assert int(re.search(r"\bAKZ_RP_%s = (\d+)" % name[6:], math).group(1)) == value, name
    # the compiled header says the same, and its tail values are the stages' own
    L = cat._lib()
    assert [L.rp_constant(k) for k in range(7)] == [_lib.RS_RP_OK, _lib.RS_RP_BAD_TABLE, _lib.RS_RP_BAD_INDEX, _lib.RS_RP_BAD_MAP,
                                                    _lib.RS_RP_NO_ROOM, _lib.RS_RP_COUNTS, _lib.RS_TVC_BAD_INDEX]
    assert (cat.OK, cat.BAD_TABLE, cat.BAD_INDEX, cat.BAD_MAP, cat.NO_ROOM) == tuple(range(5)) and cat.TILE == _lib.RS_LT_TILE
    assert "#define AKZ_RP_NONE 0xFFFFFFFFu" in math and _lib.HM_PL_NONE == 0xFFFFFFFF == repack.NONE
    hip = open(os.path.join(ROOT, "cv_amd", "csrc", "rs_repack.hip")).read()
    # the tile the kernels scan is the exported one: stated once, in the header of the table stages' shared pieces
    tbl = open(os.path.join(ROOT, "cv_amd", "csrc", "rs_table.h")).read()
    assert "static_assert(kTblTile == (uint32_t)RS_LT_TILE" in tbl and '#include "rs_table.h"' in hip and "kTblTile" in hip
    assert not re.search(r"constexpr \w+ k\w+Tile\b", hip)
    # the helpers are akz_common.h's and rs_table.h's: used, not copied
    assert "akz_block_sum<" in hip and "akz_block_scan<" in hip and "tbl_scan_step(" in hip and "tbl_scan_in_place(" in hip
    assert "akz_block_exclusive<" in tbl and "uint32_t tbl_scan" not in hip and "uint32_t akz_block_" not in hip


class Table:
    """rs_repack_table_device on host memory that no kernel will ever see: every refusal below is returned before the context is
    looked at"""

    def __init__(self):
        w = lambda n: np.zeros(max(n, 1), np.uint32)
        self.v = dict(n_obs=6, n_landmarks=4, cap=4, n_blocks=5, n_blocks_out=5, n_recons=2, obs_room=20, lm_room=20)
        self.a = dict(start=w(5), obs=w(12), map=w(5), recon_start=w(3), start_out=w(21), obs_out=w(40), obs_counts_out=w(20), landmarks_out=w(20),
                      key_out=w(4), recon_start_out=w(3), counts_out=w(5), call_verdict=w(1))

    def run(self, lib, ctx=None, **over):
        p = {k: v.ctypes.data for k, v in self.a.items()}
        p.update(self.v)
        p.update(over)
        return lib.rs_repack_table_device(ctx, p["start"], p["obs"], p["n_obs"], p["n_landmarks"], p["cap"], p["n_blocks"], p["map"],
                                          p["n_blocks_out"], p["recon_start"], p["n_recons"], p["obs_room"], p["lm_room"], p["start_out"],
                                          p["obs_out"], p["obs_counts_out"], p["landmarks_out"], p["key_out"], p["recon_start_out"],
                                          p["counts_out"], p["call_verdict"], None)


def test_table_refusals_come_before_the_device(lib):
    bogus = C.c_void_p(8)                      # never dereferenced: every call below with it is refused
    t = Table()
    assert t.run(lib) == INVALID                                                        # a complete call gets as far as the context: none
    for name in ("start", "obs", "start_out", "obs_out", "obs_counts_out", "landmarks_out", "key_out", "counts_out", "call_verdict"):
        assert t.run(lib, ctx=bogus, **{name: None}) == INVALID, name
    assert t.run(lib, ctx=bogus, recon_start=None) == INVALID and t.run(lib, ctx=bogus, recon_start_out=None) == INVALID
    assert t.run(lib, ctx=bogus, recon_start=None, recon_start_out=None) == INVALID     # no ranges, but a count of them
    assert t.run(lib, ctx=bogus, cap=0) == INVALID and t.run(lib, ctx=bogus, n_blocks=0) == INVALID
    assert t.run(lib, ctx=bogus, lm_room=0xFFFFFFFF) == INVALID
    assert t.run(lib, ctx=bogus, map=None, n_blocks_out=4) == INVALID                   # the identity keeps the block count
    assert t.run(lib, ctx=bogus, n_landmarks=0xFFFFFFFF - 2048 + 1) == -6               # AKZ_E_TOO_LARGE
    ins = {k: t.a[k].ctypes.data for k in ("start", "obs", "map", "recon_start")}
    for out in ("start_out", "obs_out", "obs_counts_out", "landmarks_out", "key_out", "recon_start_out", "counts_out", "call_verdict"):
        for name, at in ins.items():
            assert t.run(lib, ctx=bogus, **{out: at}) == INVALID, (out, name)
    assert t.run(lib, ctx=bogus, start_out=ins["start"] - 4 * 20) == INVALID            # its last word only
    assert t.run(lib, ctx=bogus, obs_out=ins["obs"] + 4) == INVALID


def test_gather_refusals_come_before_the_device(lib):
    bogus = C.c_void_p(8)
    src, dst, m, v = (np.zeros(64, np.uint32) for _ in range(4))
    call = lambda ctx=bogus, s=src.ctypes.data, d=dst.ctypes.data, rb=16, nb=4, mp=m.ctypes.data, out=4, vd=v.ctypes.data: \
        lib.rs_gather_blocks_device(ctx, s, d, rb, nb, mp, out, vd, None)
    assert call(ctx=None) == INVALID
    assert call(s=None) == INVALID and call(d=None) == INVALID and call(vd=None) == INVALID
    assert call(rb=0) == INVALID and call(rb=6) == INVALID and call(nb=0) == INVALID
    assert call(mp=None, out=3) == INVALID
    assert call(s=src.ctypes.data + 2) == INVALID and call(d=dst.ctypes.data + 1) == INVALID              # 4-byte words at the least
    assert call(d=src.ctypes.data) == INVALID and call(d=src.ctypes.data + 60) == INVALID and call(d=src.ctypes.data - 60) == INVALID
    assert call(d=m.ctypes.data) == INVALID and call(vd=dst.ctypes.data + 8) == INVALID and call(vd=src.ctypes.data) == INVALID


def test_constraint_and_frame_refusals_come_before_the_device(lib):
    bogus = C.c_void_p(8)
    n = 4
    a = dict(views=np.zeros(3 * n, np.uint32), poses=np.zeros(24 * n), verdict=np.zeros(n, np.uint32), map=np.zeros(5, np.uint32),
             start=np.zeros(3, np.uint32), views_out=np.zeros(3 * n, np.uint32), poses_out=np.zeros(24 * n), verdict_out=np.zeros(n, np.uint32),
             count=np.zeros(1, np.uint32), start_out=np.zeros(3, np.uint32))

    def call(ctx=bogus, n=n, n_blocks=5, out=5, n_ranges=2, **over):
        p = {k: v.ctypes.data for k, v in a.items()}
        p.update(over)
        return lib.rs_repack_constraints_device(ctx, p["views"], p["poses"], p["verdict"], n, p["map"], n_blocks, out, p["start"], n_ranges,
                                                p["views_out"], p["poses_out"], p["verdict_out"], p["count"], p["start_out"], None)
    assert call(ctx=None) == INVALID
    for name in ("views", "poses", "verdict", "views_out", "poses_out", "verdict_out", "count"):
        assert call(**{name: None}) == INVALID, name
    assert call(start=None) == INVALID and call(start_out=None) == INVALID and call(start=None, start_out=None) == INVALID
    assert call(n_blocks=0) == INVALID and call(map=None, out=4) == INVALID
    assert call(views_out=a["views"].ctypes.data) == INVALID and call(poses_out=a["poses"].ctypes.data + 8) == INVALID      # out of place only
    assert call(verdict_out=a["verdict"].ctypes.data) == INVALID and call(count=a["map"].ctypes.data) == INVALID

    recon, view, m, flags = (np.zeros(8, np.uint32) for _ in range(4))
    frames = lambda ctx=bogus, r=recon.ctypes.data, v=view.ctypes.data, n=8, which=0, mp=m.ctypes.data, nb=8, f=flags.ctypes.data: \
        lib.hm_place_remap_views_device(ctx, r, v, n, which, mp, nb, f, None)
    assert frames(ctx=None) == INVALID
    assert frames(r=None) == INVALID and frames(v=None) == INVALID and frames(f=None) == INVALID and frames(nb=0) == INVALID
    assert frames(which=0xFFFFFFFF) == INVALID                                           # HM_PL_NONE is no reconstruction
    assert frames(v=recon.ctypes.data) == INVALID and frames(mp=view.ctypes.data) == INVALID and frames(f=recon.ctypes.data + 4) == INVALID


def test_the_cpp_mirror_compiles(lib, tmp_path):
    import host_build
    exe = host_build.native(tmp_path, "repack.cpp", hip=True)
    assert os.path.exists(exe)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
        assert r.returncode == 2
