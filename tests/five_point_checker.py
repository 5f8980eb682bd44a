"""The CPU checker of the five-point kernels for the tests: tests/cpp/five_point_host.c (thin wrappers around
include/akz_five_point_math.h) as host_build.load compiles it — the host compiler, no contraction to FMA, as the kernels —
loaded with ctypes."""
import ctypes as C

import numpy as np

import host_build

EPS, MAX_SWEEPS = 1e-16, 1000        # AKZ_FP_JACOBI_EPS, AKZ_FP_JACOBI_SWEEPS of include/akz_five_point_math.h

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = host_build.load("five_point_host.c")
    vp, u32 = C.c_void_p, C.c_uint32
    L.fp_essentials.argtypes = [vp, vp, vp, u32, C.c_double, C.c_int, vp, vp]
    L.fp_essentials.restype = None
    L.fp_nullspace.argtypes = [vp, vp, C.c_double, C.c_int, vp]
    L.fp_o1.argtypes = [vp, vp, vp]
    L.fp_o1.restype = None
    L.fp_o2.argtypes = [vp, vp, vp]
    L.fp_o2.restype = None
    _lib = L
    return L


def essentials(a, b, samples, fill=0.0):
    """(E [n_samples, 10, 3, 3], n_solutions [n_samples]) of the host build for samples [n_samples, 5] of the matches
    a / b [n, 3]; unused slots hold `fill`."""
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    s = np.ascontiguousarray(samples, np.uint32).reshape(-1, 5)
    E = np.full((len(s), 10, 3, 3), fill, np.float64); n = np.zeros(len(s), np.uint32)
    lib().fp_essentials(a.ctypes.data, b.ctypes.data, s.ctypes.data, len(s), EPS, MAX_SWEEPS, E.ctypes.data, n.ctypes.data)
    return E, n


def solve(a5, b5):
    """The solutions [n, 3, 3] for five matches."""
    E, n = essentials(a5, b5, np.arange(5, dtype=np.uint32)[None])
    return E[0, :n[0]]


def o1(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64); out = np.zeros(20)
    lib().fp_o1(a.ctypes.data, b.ctypes.data, out.ctypes.data)
    return out


def o2(a20, b):
    a = np.ascontiguousarray(a20, np.float64); b = np.ascontiguousarray(b, np.float64); out = np.zeros(20)
    lib().fp_o2(a.ctypes.data, b.ctypes.data, out.ctypes.data)
    return out
