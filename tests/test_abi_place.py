"""The C ABI of the place recognition on the device (include/akz.h): hm_find_frames_batch_device, hm_place_params_default and
hm_place_room — symbols, argument counts and kinds, constants, the refusals that come before the device; the ABI number stays 11,
since the entry points are pure additions.  No GPU needed: every refusal here is decided from the arguments alone, before the
context is looked at."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cv_amd import _lib
from cv_amd import place_recognition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hm_place_params_default", "hm_place_room", "hm_find_frames_batch_device")
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
        assert re.search(r"\b%s\(" % name, hpp.split("class FrameIndex")[1]), name
    assert "pub struct FrameIndex" in rust and "class FrameIndex" in hpp
    for method in ("append_rows", "set_views", "find"):
        assert re.search(r"pub (unsafe )?fn %s\(" % method, rust.split("pub struct FrameIndex")[1]), method
        assert re.search(r"\b%s\(" % method, hpp.split("class FrameIndex")[1]), method
        assert callable(getattr(place_recognition.FrameIndex, method)), method
    assert "not compiled here" in rust.split("pub struct FrameIndex")[0].rsplit("///", 1)[1]
    assert callable(place_recognition.view_blocks) and len(place_recognition.VERDICTS) == 3
    assert "hm_place.hip" in read("cv_amd", "build.py") and "akz_place_math.h" in read("cv_amd", "build.py")


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
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [1, 1, 22]
    assert lib.hm_place_room.restype is C.c_uint32 and re.search(r"uint32_t\s+hm_place_room\(", hdr)
    # the parameter struct: four words, in the header's order, in every binding
    fields = re.findall(r"uint32_t\s+(\w+);", hdr.split("typedef struct hm_place_params {")[1].split("}")[0])
    assert fields == [f for f, _ in _lib.PlaceParams._fields_] == ["num_similar", "num_recent", "recent_threshold", "search_num"]
    assert re.findall(r"pub (\w+): u32,", rust.split("pub struct HmPlaceParams {")[1].split("}")[0]) == fields
    assert C.sizeof(_lib.PlaceParams) == 16


def test_header_constants_are_the_bindings_and_the_math_header():
    hdr, math, rust = read("include", "akz.h"), read("include", "akz_place_math.h"), read("rust", "akaze-mi355x", "src", "lib.rs")
    names = ("HM_PL_OK", "HM_PL_BAD_INDEX", "HM_PL_BAD_TABLE", "HM_PL_C_RECENT", "HM_PL_C_SIMILAR", "HM_PL_C_SEARCHED", "HM_PL_C_GROUPS", "HM_PL_C_FREE",
             "HM_PL_COUNTS", "HM_PL_MAX_HASH_BYTES", "HM_PL_MAX_SEARCH", "HM_PL_MAX_RECENT")
    for name in names:
        value = int(re.search(r"\b%s = (\d+)" % name, hdr).group(1))
        assert value == getattr(_lib, name), name
        assert int(re.search(r"\bAKZ_%s = (\d+)" % name[3:], math).group(1)) == value, name
        assert int(re.search(r"pub const %s: \w+ = (\d+);" % name, rust).group(1)) == value, name
    assert (_lib.HM_PL_MAX_HASH_BYTES, _lib.HM_PL_MAX_SEARCH, _lib.HM_PL_MAX_RECENT, _lib.HM_PL_COUNTS) == (4096, 2048, 256, 5)
    for text in (hdr, math):
        assert re.search(r"#define (HM|AKZ)_PL_NONE 0xFFFFFFFFu", text)
    assert _lib.HM_PL_NONE == 0xFFFFFFFF == place_recognition.NONE and "pub const HM_PL_NONE: u32 = 0xFFFF_FFFF;" in rust
    for k, name in enumerate(("Ok", "BadIndex", "BadTable")):
        assert re.search(r"%s = %d," % (name, k), rust.split("pub enum PlaceVerdict")[1].split("}")[0])
    hip = read("cv_amd", "csrc", "hm_place.hip")
    # the helpers are akz_common.h's: used, not copied; the matcher's file is not where the kernels went
    assert "akz_block_scan<" in hip and "bitonic_sort_lds_u64<" in hip and "akz_block_exclusive<" in hip
    assert "void bitonic_sort_lds_u64" not in hip and "uint32_t akz_block_scan" not in hip
    assert "k_place_" not in read("cv_amd", "csrc", "hm_match.hip") and "akz_place_math.h" in hip
    import place_statement as S
    assert (S.OK, S.BAD_INDEX, S.BAD_TABLE, S.COUNTS, S.NONE) == (_lib.HM_PL_OK, _lib.HM_PL_BAD_INDEX, _lib.HM_PL_BAD_TABLE, _lib.HM_PL_COUNTS, _lib.HM_PL_NONE)
    assert (S.C_RECENT, S.C_SIMILAR, S.C_SEARCHED, S.C_GROUPS, S.C_FREE) == (_lib.HM_PL_C_RECENT, _lib.HM_PL_C_SIMILAR, _lib.HM_PL_C_SEARCHED,
                                                                             _lib.HM_PL_C_GROUPS, _lib.HM_PL_C_FREE)


def test_the_defaults_and_the_room(lib):
    p = place_recognition.params()
    assert (p.num_similar, p.num_recent, p.recent_threshold, p.search_num) == (0, 32, 0, 512)          # settings.rs:437-451
    assert lib.hm_place_params_default(None) == INVALID and lib.hm_place_room(None) == 0
    import place_statement as S
    assert S.DEFAULTS == dict(num_similar=0, num_recent=32, recent_threshold=0, search_num=512)
    for ns, nr in ((0, 32), (8, 32), (0, 0), (5, 0), (3, 1), (2048, 256), (7, 2)):
        q = place_recognition.params(num_similar=ns, num_recent=nr)
        assert place_recognition.room(q) == max(2 * nr - 2, 0) + ns == S.room(dict(num_similar=ns, num_recent=nr))
    with pytest.raises(TypeError):
        place_recognition.params(similar=3)


class Find:
    """hm_find_frames_batch_device on host memory that no kernel will ever see: every refusal below is returned before the
    context (NULL here) is looked at"""
    ORDER = ("hashes", "feed", "pos", "recon", "view", "n_stored", "hash_bytes", "query", "visible", "nq", "params", "room", "found", "views_out",
             "group_recon", "group_start", "free", "search", "counts", "verdict")

    def __init__(self, n_stored=6, hash_bytes=8, nq=2, **prm):
        w = lambda n: np.zeros(max(n, 1), np.uint32)
        self.prm = place_recognition.params(**{**dict(num_similar=2, num_recent=3, search_num=4), **prm})
        room = place_recognition.room(self.prm)
        self.keep = dict(hashes=np.zeros(n_stored * hash_bytes, np.uint8), feed=w(n_stored), pos=w(n_stored), recon=w(n_stored), view=w(n_stored),
                         query=w(nq), visible=w(nq), found=w(nq * room), views_out=w(nq * room), group_recon=w(nq * room),
                         group_start=w(nq * (room + 1)), free=w(nq * room), search=w(2 * nq * self.prm.search_num), counts=w(nq * _lib.HM_PL_COUNTS),
                         verdict=w(nq))
        self.v = dict(n_stored=n_stored, hash_bytes=hash_bytes, nq=nq, room=room)

    def run(self, lib, ctx=None, **over):
        p = {k: a.ctypes.data for k, a in self.keep.items()}
        p.update(self.v)
        p["params"] = C.byref(self.prm)
        p.update(over)
        return lib.hm_find_frames_batch_device(ctx, *(p[k] for k in self.ORDER), None)


BOGUS = C.c_void_p(8)     # a context that is not NULL but that no accepted call may reach: a refusal must return before touching it


def test_the_refusals_come_before_the_device(lib):
    f = Find()
    assert f.run(lib) == INVALID                                           # a complete call gets as far as the context: there is none
    optional = ("visible", "search")
    for name in f.keep:
        if name not in optional:
            assert f.run(lib, ctx=BOGUS, **{name: None}) == INVALID, name
        else:
            assert f.run(lib, **{name: None}) == INVALID, name              # as far as the context
    assert f.run(lib, ctx=BOGUS, params=None) == INVALID
    assert f.run(lib, ctx=BOGUS, hash_bytes=0) == INVALID and f.run(lib, ctx=BOGUS, hash_bytes=6) == INVALID
    assert f.run(lib, ctx=BOGUS, hash_bytes=_lib.HM_PL_MAX_HASH_BYTES + 4) == TOO_LARGE and f.run(lib, hash_bytes=_lib.HM_PL_MAX_HASH_BYTES) == INVALID
    assert f.run(lib, ctx=BOGUS, nq=65536) == INVALID and f.run(lib, nq=65535) == INVALID
    assert f.run(lib, ctx=BOGUS, room=f.v["room"] - 1) == INVALID and f.run(lib, room=f.v["room"] + 9) == INVALID
    assert Find(search_num=_lib.HM_PL_MAX_SEARCH + 1).run(lib, ctx=BOGUS) == TOO_LARGE and Find(search_num=_lib.HM_PL_MAX_SEARCH).run(lib) == INVALID
    assert Find(num_recent=_lib.HM_PL_MAX_RECENT + 1).run(lib, ctx=BOGUS) == TOO_LARGE and Find(num_recent=_lib.HM_PL_MAX_RECENT).run(lib) == INVALID
    assert Find(num_similar=5, search_num=4).run(lib, ctx=BOGUS) == INVALID and Find(num_similar=4, search_num=4).run(lib) == INVALID
    assert f.run(lib, ctx=BOGUS, nq=0) == 0                                # nothing to do: the context is not looked at either


def test_the_cpp_mirror_compiles(lib, tmp_path):
    import host_build
    exe = host_build.native(tmp_path, "place.cpp", hip=True)
    assert os.path.exists(exe)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "/nonexistent"], capture_output=True, text=True)
        assert r.returncode == 2
