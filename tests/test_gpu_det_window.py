"""The determinant / candidate pass visits only the window of a level that the border test of scale_space_extrema.rs:96-104
admits (cv_amd/csrc/akz_det_window.h), with the streaming kernel k_det_stream and with the tile kernels alike.  Every case
here is held to the CPU oracle bit for bit: the stage-0 list (find_scale_space_extrema), the refined and the sorted lists,
final keypoints and descriptor bytes, and the Ldet planes where that tap is on.

The inputs are dense seeded noise at a low detector threshold, so that candidates sit on every admissible row and column:
for each derivative sigma (2, 3, 4) the ORACLE's stage-0 list holds at least one keypoint on each of the four extreme lines
of the window (rows y_lo and y_hi, columns x_lo and x_hi) — asserted below, on the CPU — so a window cut one pixel short on
any side loses a keypoint and fails the comparison."""
import numpy as np
import pytest

import det_window_plan as dw
from test_gpu_parity import _eq, _kp_eq, _opts, gpu  # noqa: F401  (the same fixture, helpers and comparisons)

pytestmark = pytest.mark.gpu

THR = 0.0001
STREAM = dict(stream_min_waves=1, stream_waves=64)      # the streaming kernel at every level, several segments per band


def _noise(w, h, seed, nfr):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(nfr)]


_want = {}


def _oracle(O, w, h, seed, nfr):
    """The oracle's lists of every frame of a case, computed once per (size, seed) and shared: per frame
    (stage 0, stage 1, stage 2, final keypoints, descriptors, [Ldet of every level])."""
    key = (w, h, seed, nfr)
    if key not in _want:
        orc = O.Akaze(w, h, O.default_config(threshold=THR))
        out = []
        for f in _noise(w, h, seed, nfr):
            kp, desc = orc.extract(f)
            out.append(([orc.keypoints(s) for s in (0, 1, 2)], kp, desc, [orc.buffer(l, "Ldet") for l in range(orc.num_levels)]))
        _want[key] = (dw.levels_of(orc), out)
        orc.close()
    return _want[key]


def _lines_hit(levels, frames_want):
    """{sigma: set of 'y_lo' / 'y_hi' / 'x_lo' / 'x_hi'} — the extreme lines of the window on which the oracle's stage-0 list
    of some frame holds a keypoint of a level of that sigma.  A stage-0 keypoint of level i, octave o lies at
    x * 2^o + (2^o - 1) / 2 (scale_space_extrema.rs:106-109): exact in f32, inverted here."""
    hit = {2: set(), 3: set(), 4: set()}
    for (lvl, lw, lh, octave, sigma) in levels:
        win = dw.window(lw, lh, sigma)
        if win is None:
            continue
        ratio = float(2 ** octave)
        for stages, _, _, _ in frames_want:
            s0 = stages[0][stages[0]["class_id"] == lvl]
            xs = (s0["x"].astype(np.float64) - 0.5 * (ratio - 1.0)) / ratio
            ys = (s0["y"].astype(np.float64) - 0.5 * (ratio - 1.0)) / ratio
            assert np.all(xs == np.round(xs)) and np.all(ys == np.round(ys))
            assert np.all((xs >= win[0]) & (xs <= win[1]) & (ys >= win[2]) & (ys <= win[3]))     # the window is the oracle's too
            for name, vals, line in (("x_lo", xs, win[0]), ("x_hi", xs, win[1]), ("y_lo", ys, win[2]), ("y_hi", ys, win[3])):
                if np.any(vals == line):
                    hit[sigma].add(name)
    return hit


def _assert_can_fail(levels, frames_want):
    hit = _lines_hit(levels, frames_want)
    for sigma in (2, 3, 4):
        assert hit[sigma] == {"x_lo", "x_hi", "y_lo", "y_hi"}, (sigma, sorted(hit[sigma]))


def _run(akaze, O, w, h, seed, nfr, opts, what, ldet=False):
    levels, want = _oracle(O, w, h, seed, nfr)
    frames = _noise(w, h, seed, nfr)
    ctx = akaze.Context(akaze.Akaze.new(THR), w, h, nfr, _opts(**opts))
    got = ctx.extract_batch(frames)
    for i in range(nfr):
        stages, okp, od, oldet = want[i]
        for s in (0, 1, 2):
            g = ctx.keypoints(i, s)
            if s > 0 and not opts.get("keep_all"):
                # (without the taps the orientation is found by the descriptor kernel: the refined and the sorted lists
                # carry no angle yet — every other field is compared here, the angle with the final keypoints below)
                assert len(g) == len(stages[s]), (what, i, s, len(g), len(stages[s]))
                for f in g.dtype.names:
                    if f != "angle":
                        _eq(g[f], stages[s][f], f"{what} frame {i} stage {s}.{f}")
            else:
                _kp_eq(g, stages[s], f"{what} frame {i} stage {s}")
        _kp_eq(got[i][0], okp, f"{what} frame {i} keypoints")
        _eq(got[i][1], od, f"{what} frame {i} descriptors")
        if ldet:
            for (lvl, *_rest) in levels:
                _eq(ctx.level_buffer(i, lvl, "Ldet", w, h), oldet[lvl], f"{what} frame {i} Ldet[{lvl}]")
    ctx.close()
    return levels, want


def _grids(levels, nfr, target=64):
    """{level: (bands of the window, bands of the plane, segments, rows per segment, window height)} of the streaming launches"""
    out = {}
    for (lvl, lw, lh, _o, sigma) in levels:
        win = dw.window(lw, lh, sigma)
        if win is not None:
            ww, wh = win[1] + 1 - win[0], win[3] + 1 - win[2]
            nb, nseg, rows = dw.stream_grid(ww, wh, sigma, target, nfr)
            out[lvl] = (nb, -(-lw // dw.stream_band(sigma)), nseg, rows, wh)
    return out


# seeds: chosen on the CPU so that the oracle's stage-0 lists meet _assert_can_fail (change the seed if a line stays empty)
@pytest.mark.parametrize("w,h,nfr,seed", [(640, 400, 2, 11), (333, 251, 3, 14), (700, 300, 2, 13)],
                         ids=["640x400", "ragged 333x251", "700x300: a band fewer at sigma 4, as many at sigma 2"])
def test_streaming_kernel_walks_the_window(gpu, oracle, w, h, nfr, seed):
    """k_det_stream<sigma, false> forced onto small frames.  640x400 and 700x300 cut every octave-0 window into several
    segments whose length does not divide the window's height (the last segment is short); at 700x300 the sigma-4 level of
    octave 0 launches one band fewer than the plane would need and the sigma-2 level as many: both branches of the count."""
    akaze, _ = gpu
    levels, want = _oracle(oracle, w, h, seed, nfr)
    _assert_can_fail(levels, want)
    g = _grids(levels, nfr)
    if (w, h) == (700, 300):
        assert g[0][0] == g[0][1] and levels[0][4] == 2            # sigma 2: ceil(window / band) == ceil(w / band)
        assert g[3][0] < g[3][1] and levels[3][4] == 4             # sigma 4: smaller
    if (w, h) != (333, 251):
        for lvl in range(4):
            nb, _, nseg, rows, wh = g[lvl]
            assert nseg > 1 and wh % rows != 0 and (nseg - 1) * rows < wh < nseg * rows
    _run(akaze, oracle, w, h, seed, nfr, STREAM, f"stream {w}x{h}")


def test_levels_with_an_empty_window_launch_nothing(gpu, oracle):
    """240x160: every level of octave 0 and the first of octave 1 (120x80, sigma 2) hold candidates; the other levels of
    octave 1 (sigma 3, 3, 4) and octave 2 (60x40) are too small for the border test and launch no determinant kernel — their
    counters stay zero and the lists equal the oracle's, with the streaming kernel and with the tile kernels."""
    akaze, _ = gpu
    w, h, nfr, seed = 240, 160, 3, 14
    levels, want = _oracle(oracle, w, h, seed, nfr)
    assert [dw.window(lw, lh, sigma) is None for (_l, lw, lh, _o, sigma) in levels] == [False] * 5 + [True] * 4
    s0 = np.concatenate([stages[0] for stages, _, _, _ in want])
    assert all(np.any(s0["class_id"] == lvl) for lvl in range(5)) and not np.any(s0["class_id"] >= 5)
    for opts in (STREAM, dict(stream_kernels=False), dict(stream_kernels=False, frame_pairs=False)):
        _run(akaze, oracle, w, h, seed, nfr, opts, f"empty windows {opts}")


def test_ldet_tap_keeps_the_whole_plane(gpu, oracle):
    """k_det_stream<sigma, true>: with the Ldet tap on (keep_all) the window is the whole plane — Ldet of every level of
    every frame equals the oracle's on every pixel, the ring that a default context leaves out included."""
    akaze, _ = gpu
    for (w, h, nfr, seed) in ((640, 400, 2, 11), (333, 251, 3, 14)):
        _run(akaze, oracle, w, h, seed, nfr, dict(keep_all=True, **STREAM), f"Ldet tap {w}x{h}", ldet=True)


@pytest.mark.parametrize("nfr,opts", [(1, {}), (2, dict(stream_kernels=False)), (2, dict(stream_kernels=False, frame_pairs=False)),
                                      (2, dict(stream_kernels=False, keep_all=True))],
                         ids=["single-frame call", "tile kernels, frame pairs", "tile kernels, one frame per block",
                              "tile kernels with the Ldet tap: the whole plane"])
def test_tile_kernels_skip_the_tiles_outside_the_window(gpu, oracle, nfr, opts):
    """k_deriv_second_cand2 / k_deriv_second_cand on a grid that starts at the first tile of the window (grown by one pixel)
    at 640x400: the same lists as the oracle; with the Ldet tap the grid is the whole plane and every pixel is compared."""
    akaze, _ = gpu
    w, h, seed = 640, 400, 11
    levels, want = _oracle(oracle, w, h, seed, 2)
    _assert_can_fail(levels, want[:nfr])
    # the case removes tiles: the window of octave 0's sigma-4 level starts in the second row of 32-row tiles
    assert dw.window(640, 400, 4)[2] - 1 >= 32
    _run(akaze, oracle, w, h, seed, nfr, opts, f"tiles {opts}", ldet=bool(opts.get("keep_all")))
