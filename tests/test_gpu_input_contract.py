"""What include/akz.h promises beyond tightly packed u8 frames at the context's own size, held to the oracle bit for bit
(float32 as bits, every keypoint field, every descriptor byte; the level taps through keep_all where they matter):
  - u16 and f32 pixels in batches, two different frames in every pair, through every launch site that reads the input;
  - host rows with stride > w, staged through the pinned block and through hipMemcpy2DAsync, and colour rows with
    stride > w * channels;
  - frames below the context's creation size, and size changes between calls (host calls, pipelined device calls);
  - f32 values the u8 arm never produces: exact 0 / 1 plateaus, a power-of-two scale (tests/test_oracle_scaling.py),
    and a frame whose squared gradients and determinant planes are subnormal.

Launch sites that read the input (scale_space_impl<InT>, cv_amd/csrc/akz_scale_space.hip), the condition that selects
each, and the case of test_input_typed_kernel_matrix that reaches it (every case runs for u8, u16 and f32):
  level 0 front end (fused0 = base_scale_offset gives radius 4 and level 0's derivative sigma is 2):
    k_level_front2<4,2,..,InT,..>   fused0, w % 4 == 0, frame pairs on        pairs-5 (odd last pair), pairs-2, exact-5,
                                                                              1080p-2, bins510-2
    k_level_front<4,2,InT,false>    fused0, w % 4 != 0 or frame pairs off     ragged-3, no-pairs-2
    launch_blur<4,0,InT,EPI_BLUR>   radius 4, derivative sigma != 2           deriv2-2 (derivative_factor 2.0: sigma 3)
    k_to_f32<InT> (+ k_filter1d)    radius != 4                               bso1.2-2 (base_scale_offset 1.2: radius 3)
  contrast factor (pairc = w % 4 == 0, frame pairs on, contrast_factor_num_bins <= 510):
    k_contrast_pair<InT,EPI_CMAX>,  pairc; grid of kCTilesFew tiles for n <= kLatencyFrames (4), kCTiles above;
    k_contrast_pair<InT,EPI_CHIST>  fine histogram unless contrast "exact"     pairs-2, deriv2-2, bso1.2-2, 1080p-2 (few);
                                                                              pairs-5 (many); exact-5 (many, exact pass)
    launch_blur<2,1,InT,EPI_CMAX>,  not pairc                                 ragged-3 (w % 4), no-pairs-2
    launch_blur<2,1,InT,EPI_CHIST>
  (akz_create refuses more than 510 bins, so the bin count never takes the last two; bins510-2 runs the pair kernels at
  the largest count they accept.)
Each case runs through akz_extract_batch on a keep_all context (level 0's Lt / Lx / Ly, the last level's Lt and the
contrast factor of every frame are compared too) and through akz_extract_batch_device on a default-options context."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import synth_frame
from test_gpu_parity import _eq, _kp_eq, gpu  # noqa: F401  (gpu: the module fixture that builds the library)

pytestmark = pytest.mark.gpu

FMTS = ("u8", "u16", "f32")
ESZ = {"u8": 1, "u16": 2, "f32": 4}
STAGE_MAX = 96 << 20        # kAkzHostStageMax (cv_amd/csrc/akz_api.hip): larger host inputs take hipMemcpy2DAsync
AKZ_E_TOO_LARGE = -6
PAD = 37                    # extra elements per row of a strided buffer

# (name, w, h, frames, Akaze fields, akz_options) — the docstring's table says which launch site each one reaches
CASES = [
    ("pairs-5", 640, 400, 5, {}, {}),
    ("pairs-2", 640, 400, 2, {}, {}),
    ("ragged-3", 333, 251, 3, {}, {}),
    ("no-pairs-2", 640, 400, 2, {}, {"frame_pairs": False}),
    ("deriv2-2", 640, 400, 2, {"derivative_factor": 2.0}, {}),
    ("bso1.2-2", 640, 400, 2, {"base_scale_offset": 1.2}, {}),
    ("bins510-2", 640, 400, 2, {"contrast_factor_num_bins": 510}, {}),
    ("exact-5", 640, 400, 5, {}, {"contrast": "exact"}),
    ("1080p-2", 1920, 1080, 2, {}, {}),
]
SEQ_MAX = (960, 544, 5)
SEQ = [(960, 544, 5), (333, 251, 2), (640, 360, 3), (960, 544, 5), (48, 64, 1)]


def _frame(fmt, w, h, seed):
    """synth_frame in the given pixel format: u16 carries low-byte noise (not u8 * 257), f32 values off the k / 255 grid."""
    u8 = synth_frame(w, h, seed, n_rect=max(4, w * h // 5000), n_disc=max(4, w * h // 5000))
    rng = np.random.default_rng(seed + 7919)
    if fmt == "u8":
        return u8
    if fmt == "u16":
        return (u8.astype(np.int32) * 257 + rng.integers(-120, 121, u8.shape)).clip(0, 65535).astype(np.uint16)
    return np.clip(u8.astype(np.float32) / np.float32(255) + rng.uniform(-1 / 600, 1 / 600, u8.shape).astype(np.float32),
                   0, 1).astype(np.float32)


def _seed(fmt, w, h, i):
    return 40000 + 1000 * FMTS.index(fmt) + (w * 7 + h) % 997 + 13 * i


# ---- the oracle, in a spawn pool whose workers never import torch -------------------------------------------------------
def _pool_size():
    return min(16, len(os.sched_getaffinity(0)))      # (os.cpu_count() reports the whole host)


def _oracle_job(args):
    """(image, Akaze fields, taps) -> (keypoints, descriptors, contrast factor, {(level, name): plane}, stage lists).
    taps: None, "front" (level 0's Lt / Lx / Ly and the last level's Lt) or "all" (every plane of every level and the
    keypoint lists of stages 0-2)."""
    img, kw, taps = args
    from oracle import oracle as O
    cfg = O.default_config()
    for k, v in kw.items():
        setattr(cfg, k, v)
    o = O.Akaze(img.shape[1], img.shape[0], cfg)
    kp, d = o.extract(img)
    planes, stages = {}, []
    if taps == "front":
        for name in ("Lt", "Lx", "Ly"):
            planes[(0, name)] = o.buffer(0, name)
        planes[(o.num_levels - 1, "Lt")] = o.buffer(o.num_levels - 1, "Lt")
    elif taps == "all":
        for lvl in range(o.num_levels):
            for name in ("Lt", "Lsmooth", "Lflow", "Lx", "Ly", "Ldet"):
                if not (lvl == 0 and name == "Lflow"):
                    planes[(lvl, name)] = o.buffer(lvl, name)
        stages = [o.keypoints(s) for s in (0, 1, 2)]
    return kp, d, o.contrast, planes, stages


def _scaled(img, k):
    return (img * np.float32(2.0 ** -k)).astype(np.float32)


def _plateau_frame(w, h):
    """An f32 frame with large exact-0.0 and exact-1.0 plateaus next to textured regions (and a disc of each)."""
    img = _frame("f32", w, h, 4242).copy()
    img[40:200, 30:300] = 0.0
    img[210:380, 330:620] = 1.0
    yy, xx = np.mgrid[0:h, 0:w]
    img[(yy - 300) ** 2 + (xx - 150) ** 2 <= 60 ** 2] = 1.0
    img[(yy - 100) ** 2 + (xx - 480) ** 2 <= 50 ** 2] = 0.0
    return img


@pytest.fixture(scope="module")
def want(gpu):
    """Every input of the module and the oracle's answer for it, computed in one pool."""
    import multiprocessing as mp
    from oracle import oracle as O
    frames, jobs = {}, {}

    def add(key, img, kw=None, taps=None):
        frames[key] = img
        jobs[key] = (img, kw or {}, taps)

    for fmt in FMTS:
        for w, h, n in ((640, 400, 5), (333, 251, 3), (1920, 1080, 3)):
            for i in range(n):
                add((fmt, w, h, i), _frame(fmt, w, h, _seed(fmt, w, h, i)), taps="front" if w < 1920 else None)
        for name, w, h, n, kw, _ in CASES:
            if kw:
                for i in range(n):
                    add((fmt, w, h, i, name), frames[(fmt, w, h, i)], kw, "front")
        for ch in (3, 4):
            rng = np.random.default_rng(0xC0 + ch + 8 * FMTS.index(fmt))
            base = synth_frame(336, 200, 91 + ch).astype(np.float64)
            planes = [np.clip(base * f + rng.uniform(-12, 12, base.shape), 0, 255) for f in (1.0, 0.8, 1.15, 0.5)[:ch]]
            rgb = np.stack(planes, 2)
            rgb = {"u8": rgb.astype(np.uint8), "u16": (rgb * 257.0 + rng.uniform(0, 200, rgb.shape)).clip(0, 65535).astype(np.uint16),
                   "f32": (rgb / 255.0 + rng.uniform(0, 1e-3, rgb.shape)).clip(0, 1).astype(np.float32)}[fmt]
            frames[("colour", fmt, ch)] = rgb
            add(("colour-luma", fmt, ch), O.luma(rgb))
    for w, h, n in SEQ:
        for i in range(n):
            if (w, h) != (333, 251):
                add(("u8", w, h, i), _frame("u8", w, h, _seed("u8", w, h, i)))
    add(("u8", 640, 480, 0), _frame("u8", 640, 480, 515))
    for i in range(2):
        add(("plateau", i), _plateau_frame(640, 400) if i == 0 else frames[("f32", 640, 400, 3)], taps="all")
        add(("2^-60", i), _scaled(frames[("f32", 640, 400, i)], 60), {"detector_threshold": 0.001 * 2.0 ** -120}, "all")
    keys = list(jobs)
    O.build()
    with mp.get_context("spawn").Pool(_pool_size()) as pool:
        res = pool.map(_oracle_job, [jobs[k] for k in keys], chunksize=1)
    out = dict(zip(keys, res))
    # a mix-up between frames must not pass as agreement: neighbours differ
    for fmt in FMTS:
        for w, h, n in ((640, 400, 5), (333, 251, 3), (1920, 1080, 3)):
            for i in range(1, n):
                a, b = out[(fmt, w, h, i - 1)][0], out[(fmt, w, h, i)][0]
                assert len(a) > 50 and a.tobytes() != b.tobytes(), f"{fmt} {w}x{h} frames {i - 1} and {i}"
    return frames, out


def _check_frame(kp, desc, n, wanted, what):
    """Frame `what` of the library (KP_DTYPE rows or raw 28-byte rows, descriptor rows, count) equals the oracle's."""
    from cv_amd import _lib
    okp, od = wanted[0], wanted[1]
    assert n == len(okp), f"{what}: {n} keypoints, the oracle has {len(okp)}"
    kp = np.ascontiguousarray(kp[:n])
    if kp.dtype != _lib.KP_DTYPE:
        kp = kp.view(_lib.KP_DTYPE).reshape(-1)
    _kp_eq(kp, okp, what)
    _eq(desc[:n], od, f"{what}.descriptors")


def _check_taps(ctx, i, w, h, wanted, what):
    """The contrast factor and the oracle's planes (wanted[3]) of frame i of the context's last call."""
    assert ctx.contrast(i) == wanted[2], f"{what}: contrast factor {ctx.contrast(i)!r}, the oracle has {wanted[2]!r}"
    for (lvl, name), plane in wanted[3].items():
        _eq(ctx.level_buffer(i, lvl, name, w, h), plane, f"{what} {name}[{lvl}]")


def _device_call(ctx, frames, fmt, dev):
    """Enqueue one akz_extract_batch_device call on `frames`; returns the buffers (inputs kept alive until a sync)."""
    import torch
    from cv_amd import _lib
    arr = np.stack(frames)
    if fmt == "u16":
        arr = arr.view(np.int16)                # torch has no uint16: the same bytes as int16
    d_in = torch.from_numpy(arr).to(dev)
    n, cap = len(frames), ctx.max_kp
    kps = torch.zeros((n, cap, 28), dtype=torch.uint8, device=dev)
    descs = torch.zeros((n, cap, 64), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    h, w = frames[0].shape
    fcode = {"u8": _lib.FMT_U8, "u16": _lib.FMT_U16, "f32": _lib.FMT_F32}[fmt]
    _lib.check(_lib.lib().akz_extract_batch_device(ctx.handle, d_in.data_ptr(), fcode, n, w, h, kps.data_ptr(),
                                                   descs.data_ptr(), cap, cnt.data_ptr(),
                                                   _lib.wait_handle(torch.cuda.current_stream())),
               "akz_extract_batch_device")
    return d_in, kps, descs, cnt


def _check_device(bufs, wanted, what):
    _, kps, descs, cnt = bufs
    h_kps, h_descs, h_cnt = kps.cpu().numpy(), descs.cpu().numpy(), cnt.cpu().numpy()
    for i, wt in enumerate(wanted):
        _check_frame(h_kps[i], h_descs[i], int(h_cnt[i]), wt, f"{what} frame {i}")


# ---- 1. the input-typed kernel matrix -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_input_typed_kernel_matrix(gpu, want, case, fmt):
    """One case of the docstring's table in one pixel format: a host call on a keep_all context (keypoints, descriptors,
    contrast factor, level 0's Lt / Lx / Ly and the last level's Lt of every frame) and a device call on a default-options
    context (keypoints, descriptors) equal the oracle's answers for the same frames."""
    import torch
    akaze, _ = gpu
    from cv_amd import _lib
    frames, out = want
    name, w, h, n, kw, okw = case
    key = (lambda i: (fmt, w, h, i, name)) if kw else (lambda i: (fmt, w, h, i))
    imgs = [frames[(fmt, w, h, i)] for i in range(n)]
    wanted = [out[key(i)] for i in range(n)]
    ak = akaze.Akaze(**kw)
    what = f"{name} {fmt}"
    ctx = akaze.Context(ak, w, h, n, _lib.make_options(keep_all=True, **okw))
    try:
        got = ctx.extract_batch(imgs)
        for i in range(n):
            _check_frame(got[i][0], got[i][1], len(got[i][0]), wanted[i], f"{what} host frame {i}")
            if wanted[i][3]:
                _check_taps(ctx, i, w, h, wanted[i], f"{what} host frame {i}")
    finally:
        ctx.close()
    dev = torch.device("cuda", 0)
    ctx = akaze.Context(ak, w, h, n, _lib.make_options(**okw))
    bufs = None
    try:
        bufs = _device_call(ctx, imgs, fmt, dev)
        _lib.check(_lib.lib().akz_sync(ctx.handle), "akz_sync")
        _check_device(bufs, wanted, f"{what} device")
    finally:
        ctx.close()
        del bufs
        torch.cuda.empty_cache()


# ---- 2. strided host rows ------------------------------------------------------------------------------------------------
def _padded(img, pad, rng):
    """img inside a buffer `pad` elements wider per row (a view of it); the padding holds values that would change the
    result if read."""
    h, w = img.shape[:2]
    shape = (h, w + pad) + img.shape[2:]
    if img.dtype == np.float32:
        buf = rng.uniform(0, 1, shape).astype(np.float32)
    else:
        buf = rng.integers(0, np.iinfo(img.dtype).max + 1, shape).astype(img.dtype)
    buf[:, :w] = img
    v = buf[:, :w]
    assert v.strides[0] == (w + pad) * int(np.prod(img.shape[2:])) * img.itemsize
    return v


@pytest.mark.parametrize("fmt", FMTS)
def test_strided_host_rows(gpu, want, fmt):
    """akz_extract_batch with stride = w + 37, the padding full of other values: staged through the pinned block (a 1080p
    pair: several ~512 KB row blocks per frame; a ragged 333 x 251 triple) and, above 96 MB of input, through
    hipMemcpy2DAsync (the fewest 1080p frames that exceed it: 13 f32, 25 u16 or 49 u8 ones, three distinct contents in
    turn).  Then akz_extract_gray_{u8,u16,f32} directly with a padded stride.  Everything equals the oracle on the unpadded
    frames."""
    akaze, _ = gpu
    from cv_amd import _lib
    frames, out = want
    rng = np.random.default_rng(17 + FMTS.index(fmt))
    ak = akaze.Akaze.default()
    for w, h, n in ((1920, 1080, 2), (333, 251, 3)):
        assert n * w * h * ESZ[fmt] <= STAGE_MAX
        ctx = akaze.Context(ak, w, h, n)
        try:
            got = ctx.extract_batch([_padded(frames[(fmt, w, h, i)], PAD, rng) for i in range(n)], keep_stride=True)
        finally:
            ctx.close()
        for i in range(n):
            _check_frame(got[i][0], got[i][1], len(got[i][0]), out[(fmt, w, h, i)], f"staged stride {w + PAD} {fmt} {w}x{h} frame {i}")
    w, h = 1920, 1080
    n = STAGE_MAX // (w * h * ESZ[fmt]) + 1
    assert n * w * h * ESZ[fmt] > STAGE_MAX
    views = [_padded(frames[(fmt, w, h, i)], PAD, rng) for i in range(3)]
    ctx = akaze.Context(ak, w, h, n)
    try:
        got = ctx.extract_batch([views[i % 3] for i in range(n)], keep_stride=True)
    finally:
        ctx.close()
    for i in range(n):
        _check_frame(got[i][0], got[i][1], len(got[i][0]), out[(fmt, w, h, i % 3)],
                     f"hipMemcpy2DAsync stride {w + PAD} {fmt} frame {i} (content {i % 3})")
    # the one-frame entry points, straight through ctypes
    w, h = 333, 251
    img = _padded(frames[(fmt, w, h, 1)], PAD, rng)
    fn = {"u8": _lib.lib().akz_extract_gray_u8, "u16": _lib.lib().akz_extract_gray_u16, "f32": _lib.lib().akz_extract_gray_f32}[fmt]
    ctx = akaze.Context(ak, 640, 400, 1)            # (and a frame below the context's size)
    try:
        cap = ctx.max_kp
        kps = np.zeros(cap, _lib.KP_DTYPE); descs = np.zeros((cap, 64), np.uint8); cnt = C.c_uint32()
        _lib.check(fn(ctx.handle, img.ctypes.data, w, h, w + PAD, kps.ctypes.data, descs.ctypes.data, cap, C.byref(cnt)),
                   f"akz_extract_gray_{fmt}")
    finally:
        ctx.close()
    _check_frame(kps, descs, cnt.value, out[(fmt, w, h, 1)], f"akz_extract_gray_{fmt} stride {w + PAD}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("ch", [3, 4])
def test_strided_colour_rows(gpu, want, fmt, ch):
    """akz_extract_color with stride = w * channels + 37 elements, the padding full of other values: the oracle's answer
    on the luma plane of the unpadded pixels."""
    akaze, _ = gpu
    frames, out = want
    rgb = frames[("colour", fmt, ch)]
    h, w = rgb.shape[:2]
    rng = np.random.default_rng(23 + ch)
    rows = _padded(rgb.reshape(h, w * ch), PAD, rng)
    view = np.lib.stride_tricks.as_strided(rows, shape=(h, w, ch), strides=(rows.strides[0], ch * rgb.itemsize, rgb.itemsize))
    assert np.array_equal(view, rgb) and view.strides[0] == (w * ch + PAD) * rgb.itemsize
    ctx = akaze.Context(akaze.Akaze.default(), w, h, 1)
    try:
        kp, d = ctx.extract_color(view, keep_stride=True)
    finally:
        ctx.close()
    wt = out[("colour-luma", fmt, ch)]
    assert len(wt[0]) > 50
    _check_frame(kp, d, len(kp), wt, f"colour {fmt} x{ch} stride {w * ch + PAD}")


# ---- 3. frames below the context's size, size changes ---------------------------------------------------------------------
def _seq_frames(frames, step):
    """The frames of step `step` of SEQ: the second 960 x 544 call takes the first one's frames in reverse order."""
    w, h, n = SEQ[step]
    order = range(n - 1, -1, -1) if step == 3 else range(n)
    return [("u8", w, h, i) for i in order]


@pytest.mark.parametrize("mode", ["host", "host resident", "device pipelined"])
def test_frames_below_the_context_size(gpu, want, mode):
    """One context created for 5 frames of 960 x 544, called in sequence with 5 frames at 960 x 544, 2 at 333 x 251 (ragged:
    the one-frame kernels), 3 at 640 x 360 (fewer octaves, other resident levels), 5 at 960 x 544 again (reversed) and 1 at
    48 x 64: every frame equals the oracle of its own size.  Host calls with default options and with
    resident_min_frames = 1; device calls issued back to back without a sync in between (each size change synchronises
    and re-carves while the other buffer set may hold work), outputs in distinct device buffers.  A frame above the
    creation size is refused with AKZ_E_TOO_LARGE."""
    import torch
    akaze, _ = gpu
    from cv_amd import _lib
    frames, out = want
    W, H, N = SEQ_MAX
    opts = _lib.make_options(resident_min_frames=1) if mode == "host resident" else None
    ctx = akaze.Context(akaze.Akaze.default(), W, H, N, opts)
    pending = []
    try:
        for step, (w, h, n) in enumerate(SEQ):
            keys = _seq_frames(frames, step)
            imgs = [frames[k] for k in keys]
            what = f"{mode} call {step} ({n} x {w}x{h})"
            if mode == "device pipelined":
                pending.append((_device_call(ctx, imgs, "u8", torch.device("cuda", 0)), keys, what))
                continue
            got = ctx.extract_batch(imgs)
            for i, k in enumerate(keys):
                _check_frame(got[i][0], got[i][1], len(got[i][0]), out[k], f"{what} frame {i}")
        if pending:
            _lib.check(_lib.lib().akz_sync(ctx.handle), "akz_sync")
            for bufs, keys, what in pending:
                _check_device(bufs, [out[k] for k in keys], what)
        for w, h in ((W + 1, H), (W, H + 1)):
            with pytest.raises(_lib.AkzError) as e:
                ctx.extract_batch([np.zeros((h, w), np.uint8)])
            assert e.value.status == AKZ_E_TOO_LARGE, (w, h, e.value.status)
        # the context still works after the refusals
        got = ctx.extract_batch([frames[("u8", 48, 64, 0)]])
        _check_frame(got[0][0], got[0][1], len(got[0][0]), out[("u8", 48, 64, 0)], f"{mode} after the refusals")
    finally:
        ctx.close()
        del pending
        torch.cuda.empty_cache()


def test_high_level_api_reuses_its_context_for_a_smaller_frame(gpu, want):
    """Akaze.default().extract_arrays on a 1080p frame, then on a 640 x 480 one: the instance keeps its 1080p context (the
    smaller frame re-carves it) and both answers equal the oracle's."""
    akaze, _ = gpu
    frames, out = want
    ak = akaze.Akaze.default()
    first = None
    try:
        for k in (("u8", 1920, 1080, 0), ("u8", 640, 480, 0), ("u8", 1920, 1080, 1)):
            kp, d = ak.extract_arrays(frames[k])
            _check_frame(kp, d, len(kp), out[k], f"extract_arrays {k[1]}x{k[2]} frame {k[3]}")
            first = first or ak.__dict__["_ctx"]
            assert ak.__dict__["_ctx"] is first and (first.max_w, first.max_h) == (1920, 1080), "the cached context was not reused"
    finally:
        ak.close()


# ---- 4. f32 values the u8 arm never produces --------------------------------------------------------------------------------
def _full_compare(akaze, ctx, imgs, wanted, what):
    """Every plane of every level, the contrast factor, the keypoint lists of stages 0-2 and the outputs of every frame of
    one keep_all host call."""
    h, w = imgs[0].shape
    got = ctx.extract_batch(imgs)
    for i, wt in enumerate(wanted):
        for (lvl, name), plane in wt[3].items():
            assert not np.isnan(plane).any(), f"{what} frame {i}: the oracle's {name}[{lvl}] holds NaN"
        _check_taps(ctx, i, w, h, wt, f"{what} frame {i}")
        for s in (0, 1, 2):
            _kp_eq(ctx.keypoints(i, s), wt[4][s], f"{what} frame {i} stage {s}")
        _check_frame(got[i][0], got[i][1], len(got[i][0]), wt, f"{what} frame {i}")


def test_f32_plateaus_of_exact_zero_and_one(gpu, want):
    """A pair whose first frame holds large exact-0.0 and exact-1.0 plateaus (rectangles and discs) next to texture:
    every plane, the contrast factor, every keypoint stage and the outputs equal the oracle's, on a keep_all context and,
    for the outputs, on a default-options one."""
    akaze, _ = gpu
    from cv_amd import _lib
    frames, out = want
    imgs = [frames[("plateau", i)] for i in range(2)]
    assert (imgs[0] == 0.0).mean() > 0.1 and (imgs[0] == 1.0).mean() > 0.1
    wanted = [out[("plateau", i)] for i in range(2)]
    ctx = akaze.Context(akaze.Akaze.default(), 640, 400, 2, _lib.make_options(keep_all=True))
    try:
        _full_compare(akaze, ctx, imgs, wanted, "plateaus")
    finally:
        ctx.close()
    ctx = akaze.Context(akaze.Akaze.default(), 640, 400, 2)
    try:
        got = ctx.extract_batch(imgs)
    finally:
        ctx.close()
    for i in range(2):
        _check_frame(got[i][0], got[i][1], len(got[i][0]), wanted[i], f"plateaus (default options) frame {i}")


@pytest.mark.parametrize("k", [4, 12])
def test_f32_power_of_two_scaling(gpu, want, k):
    """tests/test_oracle_scaling.py's property on the device: a 640 x 400 f32 pair times 2^-k with detector_threshold times
    2^-2k gives the oracle's keypoints of the unscaled pair in x, y, size, angle, octave and class_id, bit for bit, the
    response times 2^-2k exactly, the same descriptor bytes and a contrast factor of exactly 2^-k times the oracle's."""
    akaze, _ = gpu
    from cv_amd import _lib
    frames, out = want
    s = np.float32(2.0 ** -k)
    imgs = [_scaled(frames[("f32", 640, 400, i)], k) for i in range(2)]
    ctx = akaze.Context(akaze.Akaze.new(0.001 * 2.0 ** (-2 * k)), 640, 400, 2)
    try:
        got = ctx.extract_batch(imgs)
        contrast = [ctx.contrast(i) for i in range(2)]
    finally:
        ctx.close()
    for i in range(2):
        okp, od, oc = out[("f32", 640, 400, i)][:3]
        what = f"2^-{k} frame {i}"
        kp, d = got[i]
        assert len(kp) == len(okp), f"{what}: {len(kp)} keypoints, the unscaled oracle has {len(okp)}"
        for f in ("x", "y", "size", "angle", "octave", "class_id"):
            _eq(kp[f], okp[f], f"{what}.{f}")
        _eq(kp["response"], (okp["response"] * s * s).astype(np.float32), f"{what}.response (times 2^-{2 * k})")
        _eq(d, od, f"{what}.descriptors")
        assert contrast[i] == oc * 2.0 ** -k, f"{what}: contrast factor {contrast[i]!r}, want {oc * 2.0 ** -k!r}"


def test_f32_subnormal_planes(gpu, want):
    """A 640 x 400 f32 pair times 2^-60, detector_threshold times 2^-120: squared gradients and most Ldet entries are
    subnormal f32 (the refinement's reciprocal overflows, so no keypoint survives, but the extrema of stage 0 exist).
    Every plane of every level — Ldet included —, the contrast factor and every keypoint stage equal the oracle's bit for
    bit: no kernel flushes subnormals."""
    akaze, _ = gpu
    from cv_amd import _lib
    frames, out = want
    imgs = [frames[("2^-60", i)] for i in range(2)]
    wanted = [out[("2^-60", i)] for i in range(2)]
    tiny = np.finfo(np.float32).tiny
    for i, wt in enumerate(wanted):
        ldet = wt[3][(0, "Ldet")]
        assert ((ldet != 0) & (np.abs(ldet) < tiny)).mean() > 0.5, f"frame {i}: Ldet[0] is not mostly subnormal"
        assert len(wt[4][0]) > 50, f"frame {i}: {len(wt[4][0])} extrema in stage 0"
    ctx = akaze.Context(akaze.Akaze.new(0.001 * 2.0 ** -120), 640, 400, 2, _lib.make_options(keep_all=True))
    try:
        _full_compare(akaze, ctx, imgs, wanted, "2^-60")
    finally:
        ctx.close()
