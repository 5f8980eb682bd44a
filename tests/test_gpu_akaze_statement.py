"""The HIP extractor held to the independent float64 statement of the reference (tests/akaze_statement.py), with the
comparison functions and the tolerance table of test_akaze_statement.py: nothing is measured anew on the device, which
is meant to equal the oracle bit for bit, so the oracle's margins are the device's."""
import numpy as np
import pytest

import akaze_statement as S
import test_akaze_statement as T
from conftest import synth_frame
from test_gpu_parity import _opts, gpu  # noqa: F401  (gpu: the module fixture that builds the library)

pytestmark = pytest.mark.gpu

FIELDS = ("width", "height", "octave", "sublevel", "esigma", "etime", "n_fed_steps", "deriv_sigma")


def device_view(ctx, idx, w, h, kp, desc, names=T.PLANES, stages=True):
    """What the context exposes for frame `idx` of its last call, as the comparison functions read it."""
    n = ctx.num_levels(w, h)
    levels = [dict({f: getattr(ctx.level(w, h, i), f) for f in FIELDS}, taus=ctx.fed_tau(w, h, i)) for i in range(n)]
    planes = [{name: ctx.level_buffer(idx, i, name, w, h) for name in names if not (i == 0 and name == "Lflow")}
              for i in range(n)]
    return dict(levels=levels, contrast=ctx.contrast(idx), planes=planes,
                stages=[ctx.keypoints(idx, s) for s in (0, 1, 2)] if stages else None, final_kp=kp, desc=desc)


def _statement(cfg, img):
    h, w = img.shape
    levels = S.schedule(cfg, w, h)
    contrast, margin = S.contrast_factor(S.to_unit_float(img), cfg.contrast_percentile, cfg.contrast_factor_num_bins)
    assert margin >= T.CONTRAST_MARGIN, margin
    _, planes, _ = S.scale_space(cfg, img, levels, contrast)
    return levels, contrast, planes


def _check_taps(akaze, img, kw, what):
    """A keep_all context against the statement: schedule, contrast factor and every exposed plane as in section c,
    stages 0 to 2 and the final keypoints and descriptors as in section d of test_akaze_statement.py."""
    h, w = img.shape
    cfg = T.statement_config(kw)
    levels, contrast, planes = _statement(cfg, img)
    ctx = akaze.Context(akaze.Akaze(**kw), w, h, 1, _opts(keep_all=True))
    try:
        (kp, desc), = ctx.extract_batch([img])
        view = device_view(ctx, 0, w, h, kp, desc)
    finally:
        ctx.close()
    T.check_schedule(levels, view["levels"])
    T.check_contrast(contrast, view["contrast"])
    T.check_planes(planes, view["planes"], what=what)
    return T.check_discrete_stages(cfg, levels, view, what)


@pytest.mark.parametrize("frame,thr", [(0, 0.01), (0, 0.001), (1, 0.01), (1, 0.001)])
def test_kitti_taps_against_the_statement(gpu, kitti, frame, thr):
    akaze, _ = gpu
    st = _check_taps(akaze, kitti[frame], dict(detector_threshold=thr), f"kitti[{frame}] {thr}")
    if thr == 0.01:
        assert st["keypoints"] == (399, 343)[frame]


def test_ragged_frame_taps_against_the_statement(gpu):
    akaze, _ = gpu
    st = _check_taps(akaze, synth_frame(333, 251, seed=6, n_rect=40, n_disc=40), dict(), "synth 333x251")
    assert st["keypoints"] > 100


@pytest.mark.parametrize("kw", [dict(derivative_factor=2.0), dict(base_scale_offset=2.4), dict(descriptor_pattern_size=12),
                                dict(num_sublevels=5, max_octave_evolution=5)],
                         ids=["derivative_factor=2.0", "base_scale_offset=2.4", "descriptor_pattern_size=12",
                              "sublevels=5,octaves=5"])
def test_non_default_taps_against_the_statement(gpu, kw):
    """Four configurations that select other kernels: the generic derivative kernels, the 11-tap level-0 blur, another
    descriptor grid, another level schedule; on the width divisible by 4 and on the ragged one."""
    akaze, _ = gpu
    for (w, h, seed) in T.SYNTH:
        st = _check_taps(akaze, synth_frame(w, h, seed=seed, n_rect=40, n_disc=40), kw, f"{kw} {w}x{h}")
        assert st["keypoints"] > 20


@pytest.mark.parametrize("make", [T._u16_frame, T._f32_frame], ids=["u16", "f32"])
def test_input_types_against_the_statement(gpu, make):
    akaze, _ = gpu
    st = _check_taps(akaze, make(), dict(), make.__name__)
    assert st["keypoints"] > 50


@pytest.mark.parametrize("resident", [False, True], ids=["call-size defaults", "resident_min_frames=1"])
def test_benchmarked_mode_against_the_statement(gpu, resident):
    """Default options (transient Lsmooth / Lflow, no Ldet planes), one 1920x1080 frame of a 5-frame call: the planes
    that survive the call — Lt, Lx, Ly at every level — against the statement chained in float64 from the u8 frame, and
    the final descriptors against the statement's M-LDB on the device's own planes at the device's own keypoints."""
    akaze, _ = gpu
    W, H, B, IDX = 1920, 1080, 5, 3
    frames = [synth_frame(W, H, 7300 + i, n_rect=150, n_disc=150) for i in range(B)]
    cfg = S.Config()
    levels, _, planes = _statement(cfg, frames[IDX])
    ctx = akaze.Context(akaze.Akaze.default(), W, H, B, _opts(resident_min_frames=1) if resident else None)
    try:
        out = ctx.extract_batch(frames)
        kp, desc = out[IDX]
        view = device_view(ctx, IDX, W, H, kp, desc, names=("Lt", "Lx", "Ly"), stages=False)
    finally:
        ctx.close()
    T.check_schedule(levels, view["levels"])
    T.check_planes(planes, view["planes"], names=("Lt", "Lx", "Ly"), what="1080p")
    assert len(kp) > 1000 and np.all(np.diff(kp["response"]) <= 0)
    kps = {f: np.asarray(kp[f], np.int64 if f in ("octave", "class_id") else np.float64) for f in S.KP_FIELDS}
    st = T.check_descriptors(cfg, levels, T.as_f64_planes(view["planes"]), kps, np.ones(len(kp), bool), desc,
                             np.zeros(len(kp), bool), "1080p")
    assert st["keypoints"] == len(kp)
