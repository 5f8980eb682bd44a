"""The contrast factor of the streaming contrast passes (k_contrast_pair, cv_amd/csrc/akz_scale_space.hip) held to the
oracle bit for bit.  A wave walks one column band (kCBand = 120 output columns, the last band aligned to the right
edge) of one row segment of a frame pair, so the cases put the frame's edges, the band seams and the segment ends in
every position the kernel treats apart:
  - widths that are not a multiple of the band (1920, 1916, 644, 260 and the smallest the pair path runs on, 40) and
    heights that do not divide into segments (1080, 1079, 41, 40);  (a frame below 40 pixels has no level: the scale
    space, and with it the contrast factor, does not run)
  - n = 1 .. 5 (few-frame segments, odd counts: a last pair of one frame), 64 and 257 (batch segments);
  - the largest gradient on row 1, row h - 2, column 1, column w - 2 and on either side of a band seam;
  - a constant frame (no non-zero magnitude: the threshold is 0) paired with a textured one;
  - u16 and f32 pixels, 510 bins, the exact and the mixed (odd frames exact) histogram paths, and the arithmetic orders.
The scale space alone runs (akz_scale_space_device); the last test checks a 1080p frame's keypoints, which every
conductivity, and so the contrast factor, feeds."""
import numpy as np
import pytest

from conftest import synth_frame
from test_gpu_parity import _kp_eq, gpu  # noqa: F401  (gpu: the module fixture that builds the library)

pytestmark = pytest.mark.gpu

BAND = 120


def _u8(w, h, seed):
    return synth_frame(w, h, seed)


def _as(fmt, img8, seed):
    """The u8 frame in another pixel format, with values the u8 arm never produces."""
    rng = np.random.default_rng(seed)
    if fmt == "u8":
        return img8
    if fmt == "u16":
        return (img8.astype(np.float64) * 257.0 + rng.uniform(0, 256, img8.shape)).clip(0, 65535).astype(np.uint16)
    return (img8.astype(np.float32) / np.float32(255.0) + rng.uniform(0, 1e-3, img8.shape).astype(np.float32)).astype(np.float32)


def _to_f32(img):
    """image.rs:47-66: f32::from(v) / 255 (u8) or / 65535 (u16), one IEEE division per pixel."""
    if img.dtype == np.uint8:
        return img.astype(np.float32) / np.float32(255.0)
    if img.dtype == np.uint16:
        return img.astype(np.float32) / np.float32(65535.0)
    return np.ascontiguousarray(img, np.float32)


def _oracle(imgs, nbins=300, arith=0):
    from oracle import oracle as O
    O.set_option(O.OPT_REDUCE, arith & 1)
    O.set_option(O.OPT_FMA, (arith >> 1) & 1)
    O.set_option(O.OPT_HALFSUM, (arith >> 2) & 1)
    try:
        cfg = O.default_config()
        return [O.contrast_factor(_to_f32(im), cfg.contrast_percentile, 1.0, nbins) for im in imgs]
    finally:
        for o in (O.OPT_REDUCE, O.OPT_FMA, O.OPT_HALFSUM):
            O.set_option(o, 0)


def _contrast(akaze_mod, imgs, kw=None, **okw):
    """The contrast factor of every frame after one akz_scale_space_device call on a context of the frames' size."""
    import torch
    from cv_amd import _lib
    h, w = imgs[0].shape
    n = len(imgs)
    ak = akaze_mod.Akaze(**(kw or {}))
    ctx = akaze_mod.Context(ak, w, h, n, _lib.make_options(**okw))
    d_in = None
    try:
        arr = np.stack(imgs)
        if arr.dtype == np.uint16:
            arr = arr.view(np.int16)            # torch has no uint16: the same bytes as int16
        d_in = torch.from_numpy(arr).to(torch.device("cuda", 0))
        fcode = {np.dtype(np.uint8): _lib.FMT_U8, np.dtype(np.int16): _lib.FMT_U16, np.dtype(np.float32): _lib.FMT_F32}[arr.dtype]
        _lib.check(_lib.lib().akz_scale_space_device(ctx.handle, d_in.data_ptr(), fcode, n, w, h,
                                                     _lib.wait_handle(torch.cuda.current_stream())),
                   "akz_scale_space_device")
        _lib.check(_lib.lib().akz_sync(ctx.handle), "akz_sync")
        return [ctx.contrast(i) for i in range(n)]
    finally:
        ctx.close()
        del d_in
        torch.cuda.empty_cache()


def _check(got, want, what):
    bad = [(i, g, wt) for i, (g, wt) in enumerate(zip(got, want)) if np.float64(g).view(np.uint64) != np.float64(wt).view(np.uint64)]
    assert not bad, f"{what}: {len(bad)} of {len(want)} frames differ; first: frame {bad[0][0]} {bad[0][1]!r} vs {bad[0][2]!r}"


SHAPES = [
    (1920, 1080, 1), (1920, 1080, 2), (1916, 1079, 3), (644, 1080, 4), (260, 1079, 5), (40, 1080, 2),
    (1916, 41, 3), (644, 40, 2), (40, 40, 1), (260, 41, 64), (644, 43, 257), (1920, 1080, 5),
]


@pytest.mark.parametrize("w,h,n", SHAPES, ids=[f"{w}x{h}x{n}" for w, h, n in SHAPES])
def test_shapes_and_counts(gpu, w, h, n):
    akaze_mod, _ = gpu
    imgs = [_u8(w, h, 7001 + 31 * i + w + h) for i in range(n)]
    _check(_contrast(akaze_mod, imgs), _oracle(imgs), f"{w}x{h} n={n}")


def _spike_positions(w, h):
    pos = [("row 1", 1, w // 3), ("row h-2", h - 2, w // 2), ("col 1", h // 2, 1), ("col w-2", h // 3, w - 2)]
    last = max(w - BAND, 0)
    for x in (BAND - 1, BAND, 2 * BAND - 1, 2 * BAND, last - 1, last, last + 1):
        if 1 <= x <= w - 2:
            pos.append((f"seam x={x}", h // 2 + x % 7, x))
    return pos


@pytest.mark.parametrize("w,h", [(1916, 1079), (644, 41), (260, 40)])
def test_maximum_on_edges_and_seams(gpu, w, h):
    """A faint textured frame with one bright pixel: the largest magnitude sits next to it, so the frame's maximum (and
    with it every bin) comes from the position under test."""
    akaze_mod, _ = gpu
    base = (_u8(w, h, 99 + w).astype(np.int32) // 16 + 100).astype(np.uint8)
    imgs = []
    for _, y, x in _spike_positions(w, h):
        img = base.copy()
        img[y, x] = 255
        imgs.append(img)
    imgs.append(base)
    got, want = _contrast(akaze_mod, imgs), _oracle(imgs)
    names = [p[0] for p in _spike_positions(w, h)] + ["no spike"]
    for i, name in enumerate(names):
        _check(got[i:i + 1], want[i:i + 1], f"{w}x{h} spike at {name}")


@pytest.mark.parametrize("order", ["flat-first", "flat-second"])
def test_constant_frame_beside_a_textured_one(gpu, order):
    akaze_mod, _ = gpu
    w, h = 644, 401
    flat = np.full((h, w), 77, np.uint8)
    tex = _u8(w, h, 4711)
    imgs = [flat, tex, tex, flat, flat] if order == "flat-first" else [tex, flat, flat, tex, tex]
    want = _oracle(imgs)
    _check(_contrast(akaze_mod, imgs), want, order)


@pytest.mark.parametrize("fmt", ["u16", "f32"])
@pytest.mark.parametrize("w,h,n", [(1916, 1079, 3), (260, 41, 5), (40, 40, 2)])
def test_u16_and_f32(gpu, fmt, w, h, n):
    akaze_mod, _ = gpu
    imgs = [_as(fmt, _u8(w, h, 300 + i + w), 17 * i + h) for i in range(n)]
    _check(_contrast(akaze_mod, imgs), _oracle(imgs), f"{fmt} {w}x{h} n={n}")


def test_510_bins(gpu):
    akaze_mod, _ = gpu
    imgs = [_u8(1916, 1079, 510 + i) for i in range(3)]
    _check(_contrast(akaze_mod, imgs, {"contrast_factor_num_bins": 510}), _oracle(imgs, nbins=510), "510 bins")


@pytest.mark.parametrize("mode", ["exact", "force_odd"])
@pytest.mark.parametrize("w,h,n", [(1916, 1079, 3), (644, 41, 5), (260, 40, 64)])
def test_histogram_pass(gpu, mode, w, h, n):
    """The exact histogram pass for every frame, and for odd frames only (pairs of one settled and one flagged frame)."""
    akaze_mod, _ = gpu
    imgs = [_u8(w, h, 808 + 3 * i) for i in range(n)]
    _check(_contrast(akaze_mod, imgs, contrast=mode), _oracle(imgs), f"{mode} {w}x{h} n={n}")


@pytest.mark.parametrize("arith", [1, 2, 3, 4, 5, 6, 7])
def test_arithmetic_orders(gpu, arith):
    akaze_mod, _ = gpu
    imgs = [_u8(1916, 1079, 4000 + arith + i) for i in range(3)]
    _check(_contrast(akaze_mod, imgs, arith=arith), _oracle(imgs, arith=arith), f"arith {arith}")


def test_keypoints_of_a_1080p_frame(gpu):
    akaze_mod, _ = gpu
    from oracle import oracle as O
    img = _u8(1920, 1080, 1080)
    o = O.Akaze(1920, 1080, O.default_config())
    okp, od = o.extract(img)
    ak = akaze_mod.Akaze()
    kp, d = ak.extract_arrays(img)
    assert len(kp) == len(okp) and len(okp) > 100, (len(kp), len(okp))
    _kp_eq(kp, okp, "1080p keypoints")
    assert np.array_equal(d, od)
