"""The C ABI of the export of a reconstruction (include/akz.h): rs_export_reconstruction_device, rs_write_ply and
akz_sample_colors_batch_device — symbols, argument counts and kinds, constants, the refusals that come before the device; the
ABI number stays 11, since the entry points are pure additions.  No GPU needed: every refusal here is decided from the
arguments alone, before the context is looked at."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cv_amd import _lib
from cv_amd import export
from cv_amd.export import ReconstructionExport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_export_reconstruction_device", "rs_write_ply", "akz_sample_colors_batch_device")
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
    for name in NAMES[:2]:
        assert re.search(r"\b%s\(" % name, hpp.split("class ReconstructionExport")[1]), name
    assert "pub struct ReconstructionExport" in rust and "class ReconstructionExport" in hpp
    for method in ("export_device", "write_ply"):
        assert re.search(r"pub (unsafe )?fn %s\(" % method, rust.split("pub struct ReconstructionExport")[1]), method
        assert "void %s(" % method in hpp.split("class ReconstructionExport")[1], method
    for method in ("export_device", "export_tensors", "run_export"):
        assert callable(getattr(ReconstructionExport, method)), method
    assert callable(export.write_ply) and callable(export.read_ply) and len(export.VERDICTS) == 3
    from cv_amd.akaze import Akaze, Context
    from cv_amd.reconstruction import export_reconstruction
    assert callable(export_reconstruction) and callable(Akaze.sample_colors_device) and callable(Context.sample_colors_device)
    assert "rs_export.hip" in read("cv_amd", "build.py") and "akz_export_math.h" in read("cv_amd", "build.py")


def _header_args(hdr, name):
    return [a.strip() for a in re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S).group(1).split(",")]


def test_the_declarations_have_the_headers_argument_counts_and_kinds(lib):
    hdr, rust = read("include", "akz.h"), read("rust", "akaze-mi355x", "src", "lib.rs")
    for name in NAMES:
        args = _header_args(hdr, name)
        kinds = [C.c_uint32 if re.match(r"uint32_t\s+\w+$", a) else C.c_int32 if re.match(r"int32_t\s+\w+$", a) else None for a in args]
        declared = getattr(lib, name).argtypes
        assert len(declared) == len(kinds), name
        for k, (want, got) in enumerate(zip(kinds, declared)):
            assert (got is C.c_uint32) == (want is C.c_uint32) and (got is C.c_int32) == (want is C.c_int32), (name, k)
        r_args = re.search(r"fn %s\(([^;]*?)\)\s*->\s*i32;" % name, rust, re.S).group(1).split(",")
        assert len(r_args) == len(args), name
        for k, (a, r) in enumerate(zip(args, r_args)):
            assert (r.strip().endswith(": u32")) == (kinds[k] is C.c_uint32) and (r.strip().endswith(": i32")) == (kinds[k] is C.c_int32), (name, k)
            assert r.strip().split(":")[0] == re.search(r"(\w+)$", a).group(1), (name, k)
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [23, 6, 11]


def test_header_constants_are_the_bindings_and_the_math_headers():
    hdr, math, rust = read("include", "akz.h"), read("include", "akz_export_math.h"), read("rust", "akaze-mi355x", "src", "lib.rs")
    names = ("RS_EX_OK", "RS_EX_OVERFLOW", "RS_EX_BAD_TABLE", "RS_EX_C_POINTS", "RS_EX_C_NO_POINT", "RS_EX_C_INFINITE", "RS_EX_C_BAD_ROWS",
             "RS_EX_COUNTS", "RS_EX_CAMERA_WORDS", "RS_EX_CAMERA_VERTICES")
    for name in names:
        value = int(re.search(r"\b%s = (\d+)" % name, hdr).group(1))
        assert value == getattr(_lib, name), name
        assert int(re.search(r"\bAKZ_%s = (\d+)" % name[3:], math).group(1)) == value, name
        m = re.search(r"pub const %s: \w+ = (\d+);" % name, rust)
        if m:
            assert int(m.group(1)) == value, name
    assert re.search(r"pub const RS_EX_COUNTS: usize = 4;", rust)
    for k, name in enumerate(("Ok", "Overflow", "BadTable")):
        assert re.search(r"%s = %d," % (name, k), rust.split("pub enum ExportVerdict")[1].split("}")[0])
    hip = read("cv_amd", "csrc", "rs_export.hip")
    # the tile the kernels scan is the exported one: stated once, in the header of the table stages' shared pieces
    tbl = open(os.path.join(ROOT, "cv_amd", "csrc", "rs_table.h")).read()
    assert "static_assert(kTblTile == (uint32_t)RS_LT_TILE" in tbl and '#include "rs_table.h"' in hip and "kTblTile" in hip
    assert not re.search(r"constexpr \w+ k\w+Tile\b", hip) and "static_assert(kTblBlock == AKZ_SUM_THREADS" in hip
    assert "akz_nr_distance(" in math and "akz_nr_mean(" in math and math.count("sqrt") == 0        # reused, not restated
    assert "not compiled here" in rust.split("pub struct ReconstructionExport")[0].rsplit("///", 1)[1]
    import export_checker as K
    assert (K.OK, K.OVERFLOW, K.BAD_TABLE, K.COUNTS, K.CAMERA_WORDS, K.CAMERA_VERTICES) == (
        _lib.RS_EX_OK, _lib.RS_EX_OVERFLOW, _lib.RS_EX_BAD_TABLE, _lib.RS_EX_COUNTS, _lib.RS_EX_CAMERA_WORDS, _lib.RS_EX_CAMERA_VERTICES)


class Export:
    """rs_export_reconstruction_device on host memory that no kernel will ever see: every refusal below is returned before the
    context (NULL here) is looked at, so a status other than AKZ_E_INVALID from the base call would mean the checks came in
    another order"""

    def __init__(self, n_world=5, n_landmarks=4, n_obs=6, cap=4, n_blocks=3, view_blocks=(2, 0), room=5):
        self.v = dict(n_world=n_world, n_obs=n_obs, n_landmarks=n_landmarks, n_views=len(view_blocks), cap=cap, n_blocks=n_blocks, room=room)
        n = 5 * len(view_blocks) + room
        w = lambda k: np.zeros(max(k, 1), np.uint32)
        self.a = dict(world=np.zeros(4 * n_world), start=w(n_landmarks + 1), obs=w(2 * n_obs), colors=np.zeros(3 * n_blocks * cap, np.uint8),
                      view_blocks=np.array(view_blocks, np.uint32), counts=w(n_blocks), landmarks=w(n_blocks * cap), poses=np.zeros(12 * n_blocks),
                      xyz=np.zeros(3 * n), rgb=np.zeros(3 * n, np.uint8), key=w(room), cameras=np.zeros(10 * len(view_blocks)), counts_out=w(4),
                      verdict=w(1))

    def run(self, lib, ctx=None, **over):
        p = {k: v.ctypes.data for k, v in self.a.items()}
        p.update(self.v)
        p.update(over)
        return lib.rs_export_reconstruction_device(ctx, p["world"], p["n_world"], p["start"], p["obs"], p["n_obs"], p["n_landmarks"], p["colors"],
                                                   p["view_blocks"], p["n_views"], p["counts"], p["landmarks"], p["cap"], p["n_blocks"], p["poses"],
                                                   p["room"], p["xyz"], p["rgb"], p["key"], p["cameras"], p["counts_out"], p["verdict"], None)


def test_export_refusals_come_before_the_device(lib):
    c = Export()
    assert c.run(lib) == INVALID                                          # a complete call gets as far as the context: there is none
    for name in c.a:
        assert c.run(lib, **{name: None}) == INVALID, name
    assert c.run(lib, cap=0) == INVALID and c.run(lib, n_blocks=0) == INVALID and c.run(lib, n_views=0) == INVALID
    assert c.run(lib, n_world=0xFFFFFFFF) == TOO_LARGE and c.run(lib, n_world=0xFFFFFFFF - 2048 + 1) == TOO_LARGE
    assert c.run(lib, n_landmarks=0xFFFFFFFF) == TOO_LARGE
    assert c.run(lib, room=0xFFFFFFFF - 9) == TOO_LARGE                   # 5 * n_views + room leaves 32 bits


def test_export_refusals_are_told_apart_from_the_missing_context(lib):
    """With a context that is not NULL but that no accepted call may reach: a refusal must return before touching it.  The
    pointer is never dereferenced, because every call below is refused."""
    bogus = C.c_void_p(8)
    assert Export(view_blocks=(2, 2)).run(lib, ctx=bogus) == INVALID      # a repeated block
    assert Export(view_blocks=(2, 3)).run(lib, ctx=bogus) == INVALID      # a block outside the blocks
    c = Export()
    for table in ("world", "start", "obs", "colors", "counts", "landmarks", "poses"):
        at = c.a[table].ctypes.data
        for out in ("xyz", "rgb", "key", "cameras", "counts_out", "verdict"):
            assert c.run(lib, ctx=bogus, **{out: at}) == INVALID, (table, out)
            assert c.run(lib, ctx=bogus, **{out: at + c.a[table].nbytes - 1}) == INVALID, (table, out)
    assert c.run(lib, ctx=bogus, verdict=c.a["world"].ctypes.data - 3) == INVALID          # its last byte only
    # what may be absent: a world table of no rows, a table of no observations, a key array of no room
    assert c.run(lib, world=None, n_world=0) == INVALID and c.run(lib, obs=None, n_obs=0) == INVALID
    assert c.run(lib, key=None, room=0) == INVALID                        # accepted as far as the context: there is none


def test_colour_batch_refusals_come_before_the_device(lib):
    bogus = C.c_void_p(8)
    w = np.zeros(64, np.uint32).ctypes.data
    # ctx, rgb, n, w, h, stride, kps, counts, cap, colors, stream
    base = [bogus, w, 3, 64, 48, 192, w, w, 8, w, None]
    assert lib.akz_sample_colors_batch_device(*([None] + base[1:])) == INVALID           # complete, but for the context
    for k in (1, 6, 7, 9):
        args = list(base)
        args[k] = None
        assert lib.akz_sample_colors_batch_device(*args) == INVALID, k
    for k, v in ((2, 0), (2, 65536), (3, 0), (4, 0), (5, 191), (8, 0)):
        args = list(base)
        args[k] = v
        assert lib.akz_sample_colors_batch_device(*args) == INVALID, k
    args = list(base)
    args[8] = 0xFFFFFFFF
    assert lib.akz_sample_colors_batch_device(*args) == TOO_LARGE


def test_the_cpp_mirror_compiles(lib, tmp_path):
    import host_build
    exe = host_build.native(tmp_path, "export.cpp", hip=True)
    assert os.path.exists(exe)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "/nonexistent", str(tmp_path / "out.ply")], capture_output=True, text=True)
        assert r.returncode == 2
