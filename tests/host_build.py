"""The two builds the tests make with the host compilers.

`load` gives the CPU checkers their host build: a tests/cpp/*_host.c (thin wrappers around one of the include/*_math.h
headers that the HIP kernels compile too) as a shared object, with -ffp-contract=off because the kernels are built without
contraction to FMA — that flag is what makes "host build == device, bit for bit" a fair demand.
`native` links a tests/cpp/*.cpp host mirror of include/akaze.hpp against cv_amd/lib/libakz.so, for the tests that drive the
library from a native process."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dir = None      # the shared objects' directory, kept for the life of the process
_loaded = {}


def load(source):
    """tests/cpp/<source> compiled with the host C compiler (-O2 -ffp-contract=off -std=gnu11) into a shared object in a
    temporary directory -> its ctypes.CDLL, one per source."""
    global _dir
    if source not in _loaded:
        cc = shutil.which("gcc") or shutil.which("cc")
        assert cc, "the CPU checker needs a host C compiler"
        if _dir is None:
            _dir = tempfile.TemporaryDirectory(prefix="akz_host_")
        so = os.path.join(_dir.name, "lib" + os.path.splitext(source)[0] + ".so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-std=gnu11", "-shared", "-fPIC", "-Wall",
                               os.path.join(ROOT, "tests", "cpp", source), "-o", so, "-lm"])
        _loaded[source] = C.CDLL(so)
    return _loaded[source]


def native(tmp_path, source, hip):
    """tests/cpp/<source> built against cv_amd/lib/libakz.so -> the executable's path (in tmp_path).  `hip`: the source calls
    the HIP runtime itself and is linked to it as well."""
    exe = str(tmp_path / os.path.splitext(source)[0])
    lib_dir = os.path.join(ROOT, "cv_amd", "lib")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hip_compile = ["-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include")] if hip else []
    hip_link = ["-L", os.path.join(rocm, "lib"), "-lamdhip64"] if hip else []
    hip_rpath = [f"-Wl,-rpath,{os.path.join(rocm, 'lib')}"] if hip else []
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + hip_compile +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", source), "-o", exe,
                           "-L", lib_dir, "-lakz"] + hip_link + [f"-Wl,-rpath,{lib_dir}"] + hip_rpath)
    return exe
