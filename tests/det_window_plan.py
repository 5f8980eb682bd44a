"""The pixels of an evolution level that may hold a detector candidate, and how the streaming determinant kernel cuts them
into launches, worked out in Python from the reference's own expressions (scale_space_extrema.rs:50, :69-70, :96-104) — the
CPU side of tests/test_gpu_det_window.py and tests/test_det_window_plan.py.  Nothing here reads the library."""
import math

import numpy as np

F = np.float32
SMAX = F(10.0) * np.sqrt(F(2.0))           # scale_space_extrema.rs:16, f32


def _roundf(v):
    """f32::round — half away from zero — of an f32 value (exact in Python's float)."""
    v = float(v)
    return math.copysign(math.floor(abs(v) + 0.5), v)


def admissible_range(extent, sigma_size):
    """(lo, hi), inclusive, of the coordinates p in 1 .. extent - 2 with round(p - b) - 1 >= 0 and round(p + b) + 1 < extent,
    b = smax * sigma_size in f32; None when there is none.  The test is monotone, so the set is a range."""
    b = F(SMAX * F(sigma_size))
    ok = [p for p in range(1, extent - 1)
          if not (_roundf(F(p) - b) - 1.0 < 0.0) and not (_roundf(F(p) + b) + 1.0 >= float(extent))]
    if not ok:
        return None
    assert ok == list(range(ok[0], ok[-1] + 1))
    return ok[0], ok[-1]


def window(width, height, sigma_size):
    """(x_lo, x_hi, y_lo, y_hi), inclusive, of a level's candidate positions, or None (no pixel passes the border test)."""
    xr, yr = admissible_range(width, sigma_size), admissible_range(height, sigma_size)
    if xr is None or yr is None:
        return None
    return xr[0], xr[1], yr[0], yr[1]


def stream_band(sigma):
    """useful columns of a wave of the streaming kernel: 128 minus an even halo of at least sigma + 1 on each side"""
    return 128 - 2 * ((sigma + 2) & ~1)


def stream_grid(win_w, win_h, sigma, target_waves, nframes):
    """(bands, segments, rows per segment) of a streaming launch over a window of win_w x win_h candidate positions"""
    nb = -(-win_w // stream_band(sigma))
    nseg = max(1, min(-(-target_waves // (nb * nframes)), -(-win_h // 32)))
    rows = -(-win_h // nseg)
    return nb, -(-win_h // rows), rows


def levels_of(orc):
    """[(level, width, height, octave, deriv_sigma)] of an oracle.Akaze"""
    out = []
    for i in range(orc.num_levels):
        L = orc.level(i)
        out.append((i, L.width, L.height, L.octave, L.deriv_sigma))
    return out
