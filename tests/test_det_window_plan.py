"""The determinant pass's window and launch arithmetic (cv_amd/csrc/akz_det_window.h over the plan of cv_amd/csrc/akz_plan.cpp)
is host code that enqueues nothing: tests/cpp/det_window.cpp, a stand-alone program built with -fsanitize=address,undefined,
holds it to its properties on every level of the 1080p plan and of the sizes tests/test_gpu_det_window.py runs, empty windows
included.  What it prints is compared here with the same figures worked out in Python (tests/det_window_plan.py), which is
what the GPU tests assert their cases by."""
import os
import re
import subprocess

import det_window_plan as dw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_and_launch_arithmetic_under_sanitizers(tmp_path):
    from cv_amd import build
    exe = str(tmp_path / "det_window")
    # host code only, but akz_common.h includes the HIP runtime's header: the project's compiler, sanitizers on the host side
    subprocess.check_call([build.hipcc(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "--offload-arch=gfx950",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "det_window.cpp"), os.path.join(ROOT, "cv_amd", "csrc", "akz_plan.cpp"),
                           "-o", exe])
    # (the program links the HIP runtime, which it never calls: what that library allocates while it loads is not the program's)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "all windows hold" and not any(l.startswith("FAILED") for l in lines)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    plans, cur = {}, None
    for l in lines[:-1]:
        m = re.fullmatch(r"plan (\d+)x(\d+): (\d+) levels", l)
        if m:
            cur = plans.setdefault((int(m[1]), int(m[2])), [])
            continue
        m = re.fullmatch(r"level (\d+) (\d+)x(\d+) sigma (\d+) window (empty|(\d+) (\d+) (\d+) (\d+) bands (\d+) of (\d+) segments (\d+) rows (\d+))", l)
        assert m, l
        assert int(m[1]) == len(cur)
        cur.append((int(m[2]), int(m[3]), int(m[4]), None if m[5] == "empty" else tuple(int(v) for v in m.groups()[5:])))
    for size in ((1920, 1080), (640, 400), (333, 251), (700, 300), (240, 160)):
        assert size in plans and plans[size], size
    assert len(plans[(1920, 1080)]) == 16 and all(lv[3] is not None for lv in plans[(1920, 1080)])
    for (w, h), levels in plans.items():
        for i, (lw, lh, sigma, got) in enumerate(levels):
            win = dw.window(lw, lh, sigma)
            if win is None:
                assert got is None, (w, h, i)
                continue
            x_lo, x_hi, y_lo, y_hi = win
            nb, nseg, rows = dw.stream_grid(x_hi + 1 - x_lo, y_hi + 1 - y_lo, sigma, 64, 2)       # (what the program prints)
            assert got == (x_lo, x_hi + 1, y_lo, y_hi + 1, nb, -(-lw // dw.stream_band(sigma)), nseg, rows), (w, h, i, got)
    # the frame of the benchmark: a ring of 28 / 42 / 57 pixels is left out at every octave, and the sigma-4 levels of octaves
    # 0 and 1 lose a band of waves
    assert [lv[3][:4] for lv in plans[(1920, 1080)][:4]] == [(29, 1891, 29, 1051), (43, 1877, 43, 1037), (43, 1877, 43, 1037), (58, 1862, 58, 1022)]
    # 240x160: octave 0 holds candidates at every level, octave 1 at its first level only, octave 2 nowhere
    assert [lv[3] is None for lv in plans[(240, 160)]] == [False] * 5 + [True] * 4
