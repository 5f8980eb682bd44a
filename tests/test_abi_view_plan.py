"""The C ABI of the view plan on the device (include/akz.h): hm_view_plan_device, hm_knn_planned_batch_device and
hm_best_of_views_planned_batch_device — symbols, argument counts and kinds, constants, the refusals that come before the device; the
ABI number stays 11, since the entry points are pure additions.  No GPU needed: every refusal here is decided from the arguments
alone, before the context is looked at."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cv_amd import _lib
from cv_amd import place_recognition, registration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hm_view_plan_device", "hm_knn_planned_batch_device", "hm_best_of_views_planned_batch_device")
INVALID = -1


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
        assert re.search(r"\b%s\(" % name, hpp.split("class FrameIndex")[1]), name
    for method in ("plan_views", "knn_planned", "best_of_views_planned"):
        assert re.search(r"pub unsafe fn %s\(" % method, rust.split("pub struct FrameIndex")[1]), method
        assert re.search(r"\b%s\(" % method, hpp.split("class FrameIndex")[1]), method
    assert callable(place_recognition.plan_views) and callable(registration.Registration.match_found)
    assert len(place_recognition.PLAN_VERDICTS) == 6
    build = read("cv_amd", "build.py")
    assert "hm_view_plan.hip" in build and "akz_view_plan_math.h" in build and "hm_tables.h" in build


def _header_args(hdr, name):
    return [a.strip() for a in re.search(r"^u?int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S | re.M).group(1).split(",")]


def test_the_declarations_have_the_headers_argument_counts_and_kinds(lib):
    hdr, rust = read("include", "akz.h"), read("rust", "akaze-mi355x", "src", "lib.rs")
    for name in NAMES:
        args = _header_args(hdr, name)
        kinds = [C.c_uint32 if re.match(r"uint32_t\s+\w+$", a) else None for a in args]
        declared = getattr(lib, name).argtypes
        assert len(declared) == len(kinds), name
        for k, (want, got) in enumerate(zip(kinds, declared)):
            assert (got is C.c_uint32) == (want is C.c_uint32), (name, k)
        r_args = re.search(r"fn %s\(([^;]*?)\)\s*->\s*[iu]32;" % name, rust, re.S).group(1).split(",")
        assert len(r_args) == len(args), name
        for k, (a, r) in enumerate(zip(args, r_args)):
            assert (r.strip().endswith(": u32")) == (kinds[k] is C.c_uint32), (name, k)
            assert r.strip().split(":")[0] == re.search(r"(\w+)$", a).group(1), (name, k)
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [18, 16, 17]


def test_header_constants_are_the_bindings_and_the_math_header():
    hdr, math, rust = read("include", "akz.h"), read("include", "akz_view_plan_math.h"), read("rust", "akaze-mi355x", "src", "lib.rs")
    names = ("HM_VP_OK", "HM_VP_CUT", "HM_VP_NO_GROUP", "HM_VP_FIND_REFUSED", "HM_VP_BAD_VIEW", "HM_VP_NO_ROOM", "HM_VP_C_BLOCKS", "HM_VP_C_LIVE",
             "HM_VP_C_VERDICT", "HM_VP_C_FRAMES", "HM_VP_COUNTS", "HM_VP_PICK_RECON", "HM_VP_MAX_VIEWS")
    for name in names:
        value = int(re.search(r"\b%s = (\d+)" % name, hdr).group(1))
        assert value == getattr(_lib, name), name
        assert int(re.search(r"\bAKZ_%s = (\d+)" % name[3:], math).group(1)) == value, name
        assert int(re.search(r"pub const %s: \w+ = (\d+);" % name, rust).group(1)) == value, name
    for k, name in enumerate(("Ok", "Cut", "NoGroup", "FindRefused", "BadView", "NoRoom")):
        assert re.search(r"%s = %d," % (name, k), rust.split("pub enum PlanVerdict")[1].split("}")[0])
    import view_plan_statement as S
    assert (S.OK, S.CUT, S.NO_GROUP, S.FIND_REFUSED, S.BAD_VIEW, S.NO_ROOM) == (_lib.HM_VP_OK, _lib.HM_VP_CUT, _lib.HM_VP_NO_GROUP,
                                                                                 _lib.HM_VP_FIND_REFUSED, _lib.HM_VP_BAD_VIEW, _lib.HM_VP_NO_ROOM)
    assert (S.C_BLOCKS, S.C_LIVE, S.C_VERDICT, S.C_FRAMES, S.COUNTS) == (_lib.HM_VP_C_BLOCKS, _lib.HM_VP_C_LIVE, _lib.HM_VP_C_VERDICT,
                                                                         _lib.HM_VP_C_FRAMES, _lib.HM_VP_COUNTS)
    assert (S.PICK_RECON, S.MAX_VIEWS, S.NONE) == (_lib.HM_VP_PICK_RECON, _lib.HM_VP_MAX_VIEWS, _lib.HM_PL_NONE)
    # the kernels are a file of their own; the matcher's kernels stay where they were, launched there; the tables are stated once
    hip, match = read("cv_amd", "csrc", "hm_view_plan.hip"), read("cv_amd", "csrc", "hm_match.hip")
    for kernel in ("k_vp_pick", "k_vp_mark", "k_vp_scan", "k_vp_tables"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, hip) and kernel not in match, kernel
    for kernel in ("k_knn_mfma4w", "k_knn_mfma4", "k_knn_mfma", "k_knn2", "k_expand", "k_expand4", "k_best_of_views"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, match) and not re.search(r"\b%s\b" % kernel, hip), kernel
    assert "akz_view_plan_math.h" in hip and "hm_internal_planned(" in hip and "hm_internal_planned(" in match
    # the scan behind a running carry is the table stages' (rs_table.h, over akz_common.h's block scan): used, not copied
    assert "tbl_scan<kVpScanWaves>(" in hip and "akz_block_exclusive<" in read("cv_amd", "csrc", "rs_table.h") and "uint32_t tbl_scan" not in hip
    for struct in ("HmProb", "HmProbX", "HmExpandJob"):
        assert len(re.findall(r"^struct %s \{" % struct, read("cv_amd", "csrc", "hm_tables.h"), re.M)) == 1
        assert not re.search(r"^struct %s \{" % struct, hip + match, re.M)


class Plan:
    """hm_view_plan_device on host memory that no kernel will ever see"""
    ORDER = ("views_out", "group_recon", "group_start", "counts", "verdict", "room", "pick", "flags", "n_frames", "n_views", "n_blocks", "exp_blocks",
             "view_idx", "n_views_of", "plan_verdict", "plan_counts")

    def __init__(self):
        w = lambda n: np.zeros(max(n, 1), np.uint32)
        self.keep = dict(views_out=w(8), group_recon=w(8), group_start=w(10), counts=w(10), verdict=w(2), pick=w(2), view_idx=w(6), n_views_of=w(2),
                         plan_verdict=w(2), plan_counts=w(4))
        self.v = dict(room=4, flags=0, n_frames=2, n_views=3, n_blocks=9, exp_blocks=6)

    def run(self, lib, ctx=None, **over):
        p = {k: a.ctypes.data for k, a in self.keep.items()}
        p.update(self.v)
        p.update(over)
        return lib.hm_view_plan_device(ctx, *(p[k] for k in self.ORDER), None)


class Knn:
    ORDER = ("q", "nq", "t", "nt", "cap", "iq", "view_idx", "n_views_of", "n_frames", "n_views", "n_blocks", "exp_blocks", "k", "out")

    def __init__(self):
        w = lambda n: np.zeros(max(n, 1), np.uint32)
        self.keep = dict(q=w(16), nq=w(4), t=w(16), nt=w(4), iq=w(2), view_idx=w(6), n_views_of=w(2), out=w(64))
        self.v = dict(cap=4, n_frames=2, n_views=3, n_blocks=9, exp_blocks=6, k=3)

    def run(self, lib, ctx=None, **over):
        p = {k: a.ctypes.data for k, a in self.keep.items()}
        p.update(self.v)
        p.update(over)
        return lib.hm_knn_planned_batch_device(ctx, *(p[k] for k in self.ORDER), None)


class Best:
    ORDER = ("knn", "nq", "iq", "cap", "view_idx", "n_views_of", "n_frames", "n_views", "n_blocks", "k", "landmarks", "nviews", "better_by", "best", "decision")

    def __init__(self):
        w = lambda n: np.zeros(max(n, 1), np.uint32)
        self.keep = dict(knn=w(64), nq=w(4), iq=w(2), view_idx=w(6), n_views_of=w(2), landmarks=w(16), nviews=w(4), best=w(48), decision=w(8))
        self.v = dict(cap=4, n_frames=2, n_views=3, n_blocks=9, k=3, better_by=24)

    def run(self, lib, ctx=None, **over):
        p = {k: a.ctypes.data for k, a in self.keep.items()}
        p.update(self.v)
        p.update(over)
        return lib.hm_best_of_views_planned_batch_device(ctx, *(p[k] for k in self.ORDER), None)


BOGUS = C.c_void_p(8)     # a context that is not NULL but that no accepted call may reach: a refusal must return before touching it


@pytest.mark.parametrize("Call", [Plan, Knn, Best])
def test_the_refusals_come_before_the_device(lib, Call):
    f = Call()
    assert f.run(lib) == INVALID                                           # a complete call gets as far as the context: there is none
    for name in f.keep:
        if name == "pick":
            assert f.run(lib, pick=None) == INVALID                        # optional: as far as the context
        else:
            assert f.run(lib, ctx=BOGUS, **{name: None}) == INVALID, name
    assert f.run(lib, ctx=BOGUS, n_views=0) == INVALID and f.run(lib, ctx=BOGUS, n_views=65) == INVALID and f.run(lib, n_views=64) == INVALID
    assert f.run(lib, ctx=BOGUS, n_frames=0) == 0                          # nothing to do: the context is not looked at either
    if Call is not Plan:
        assert f.run(lib, ctx=BOGUS, k=0) == INVALID and f.run(lib, ctx=BOGUS, k=4) == INVALID and f.run(lib, k=1) == INVALID
        assert f.run(lib, ctx=BOGUS, cap=0) == INVALID and f.run(lib, ctx=BOGUS, cap=1 << 21) == INVALID and f.run(lib, cap=(1 << 21) - 1) == INVALID
    if Call is Best:
        assert f.run(lib, ctx=BOGUS, n_frames=65536) == INVALID and f.run(lib, n_frames=65535) == INVALID
        return
    assert f.run(lib, ctx=BOGUS, n_frames=21846, exp_blocks=1) == INVALID and f.run(lib, n_frames=21845, exp_blocks=1) == INVALID   # x 3 views
    assert f.run(lib, ctx=BOGUS, n_frames=2, exp_blocks=65534) == INVALID and f.run(lib, n_frames=2, exp_blocks=65533) == INVALID
    assert f.run(lib, ctx=BOGUS, exp_blocks=0) == INVALID
    if Call is Plan:
        assert f.run(lib, ctx=BOGUS, flags=2) == INVALID and f.run(lib, flags=_lib.HM_VP_PICK_RECON) == INVALID
        assert f.run(lib, room=1) == INVALID and f.run(lib, room=0) == INVALID          # room < n_views is fine: as far as the context


def test_the_cpp_mirror_compiles(lib, tmp_path):
    import host_build
    exe = host_build.native(tmp_path, "view_plan.cpp", hip=True)
    assert os.path.exists(exe)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
        assert r.returncode == 2
