"""The configuration bench.py times, held to the oracle: 256 frames of 1920x1080 per step (tools/bench_common.make_frames,
the exact frames of the timed step), Akaze::default(), default akz_options, the symmetric better-by-24 match of frame j
against frame (j - 1) mod 256 — frame 0 against frame 255.  A plain bench run only times the step; this module checks
what it computes:
  - bench.py itself, in its default configuration (one 256-frame call per step) and with four 64-frame calls, every
    keypoint count and pair list of the dumped step (the one that reuses output set 0) against the oracle;
  - one 256-frame call in process, every byte of every frame, in order and in reverse order (other content past the
    2^31-byte mark of a level's {Lx, Ly} plane), with the library's default choice of k_level_resident proven by its timer;
  - the default threshold of that choice, (3 n_cu + 7) / 8 frames per call: one frame below it and at it."""
import json
import os

import numpy as np
import pytest

from conftest import synth_frame
from test_gpu_parity import _eq, _kp_eq, _oracle_one, gpu  # noqa: F401  (gpu: the module fixture that builds the library)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = 256                    # frames per step (tools/bench_common.FRAMES_PER_STEP)
W, H, CAP = 1920, 1080, 8192
AKZ_T_LEVEL_RESIDENT = 29   # include/akz.h


def _pool_size():
    return min(16, len(os.sched_getaffinity(0)))      # (os.cpu_count() reports the whole host)


def _oracle_pair(args):
    d_a, d_b = args
    from oracle import oracle as O
    return O.match(d_a, d_b, rule=O.RULE_STRICT, param_u=24, symmetric=True)


def _oracle_extract(frames):
    """oracle.extract of every frame in a spawn pool whose workers never import torch."""
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(min(_pool_size(), len(frames))) as pool:
        return pool.map(_oracle_one, [(f, {}) for f in frames], chunksize=1)


def _same_frame(kps, descs, n, want, what):
    """Frame `what` of the library (raw 28-byte keypoint rows, descriptor rows, count) equals the oracle's (okp, od)."""
    from cv_amd import _lib
    okp, od = want
    assert n == len(okp), f"{what}: {n} keypoints, the oracle has {len(okp)}"
    _kp_eq(np.ascontiguousarray(kps[:n]).view(_lib.KP_DTYPE).reshape(-1), okp, what)
    _eq(descs[:n], od, f"{what}.descriptors")


@pytest.fixture(scope="module")
def bench_step(gpu):
    """The bench's 256 frames (generated on the device, as bench.py does) and the oracle's answers for them: keypoints and
    descriptors of every frame, and the pair list of every (j, (j - 1) mod 256)."""
    import multiprocessing as mp
    import torch
    from tools.bench_common import make_frames
    d_frames = make_frames(torch, torch.device("cuda", 0), rank=0, n_frames=NF, world_size=1)
    frames = d_frames.cpu().numpy()
    del d_frames
    torch.cuda.empty_cache()
    assert frames.shape == (NF, H, W) and frames.dtype == np.uint8
    with mp.get_context("spawn").Pool(_pool_size()) as pool:
        ext = pool.map(_oracle_one, [(f, {}) for f in frames], chunksize=1)
        pairs = pool.map(_oracle_pair, [(ext[j][1], ext[(j - 1) % NF][1]) for j in range(NF)], chunksize=1)
    # a mix-up between frames must not pass as agreement
    for j in range(NF):
        assert len(ext[j][0]) > 1000, f"frame {j}: {len(ext[j][0])} keypoints"
        assert ext[j][0].tobytes() != ext[(j - 1) % NF][0].tobytes(), f"frames {j} and {(j - 1) % NF} give the same keypoints"
    return {"frames": frames, "ext": ext, "pairs": pairs}


def test_a_256_frame_call_in_order_and_reversed_equals_the_oracle(gpu, bench_step):
    """The bench's context (Akaze::default(), 8 192 keypoint slots, 256 frames, default options, kernel timers on) and two
    akz_extract_batch_device calls of all 256 frames back to back with no synchronisation in between, into two output
    sets: the frames in order, then in reverse order, so other content lies past the 2^31-byte mark of every level's
    {Lx, Ly} plane (frames 130 and up).  All 512 results equal the oracle's keypoint and descriptor bytes, and
    k_level_resident ran: the library chose it by itself, as it does for the benchmark's call."""
    import torch
    akaze, _ = gpu
    from cv_amd import _lib
    L = _lib.lib()
    ext = bench_step["ext"]
    dev = torch.device("cuda", 0)
    ak = akaze.Akaze.default()
    ak.max_keypoints = CAP
    ctx = akaze.Context(ak, W, H, NF)
    d_frames = torch.from_numpy(bench_step["frames"]).to(dev)
    d_sets = [d_frames, torch.flip(d_frames, [0]).contiguous()]
    kps = torch.zeros((2, NF, CAP, 28), dtype=torch.uint8, device=dev)
    descs = torch.zeros((2, NF, CAP, 64), dtype=torch.uint8, device=dev)
    cnt = torch.zeros((2, NF), dtype=torch.int32, device=dev)
    cur = torch.cuda.current_stream()
    try:
        ctx.timing_enable(2)
        ctx.timing_reset()
        for s in range(2):
            _lib.check(L.akz_extract_batch_device(ctx.handle, d_sets[s].data_ptr(), 0, NF, W, H, kps[s].data_ptr(),
                                                  descs[s].data_ptr(), CAP, cnt[s].data_ptr(), _lib.wait_handle(cur)),
                       f"extract call {s}")
        _lib.check(L.akz_sync(ctx.handle), "sync")
        _, res_launches, _ = ctx.timing_get(AKZ_T_LEVEL_RESIDENT)
        ctx.timing_enable(0)
        h_kps, h_descs, h_cnt = kps.cpu().numpy(), descs.cpu().numpy(), cnt.cpu().numpy()
    finally:
        ctx.close()
        del d_frames, d_sets, kps, descs, cnt
        torch.cuda.empty_cache()
    for s, order in enumerate(("in order", "reversed")):
        for j in range(NF):
            src = j if s == 0 else NF - 1 - j
            _same_frame(h_kps[s, j], h_descs[s, j], int(h_cnt[s, j]), ext[src],
                        f"call {s} ({order}) frame {j} (bench frame {src})")
    assert res_launches > 0, "the 256-frame call did not take k_level_resident"


def test_the_default_resident_threshold(gpu):
    """By default a call of at least (3 n_cu + 7) / 8 frames hands the levels that fit one compute unit to k_level_resident
    (96 frames on a 256-CU MI355X, so the benchmark's 256-frame call takes it).  480x270: octave 1 is 240 x 135, the plane
    octave 3 has at 1080p.  One call a frame below the threshold runs no k_level_resident launch, one call at it runs
    some, and every frame of both equals the oracle byte for byte."""
    import torch
    akaze, _ = gpu
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    res_min = (3 * n_cu + 7) // 8
    assert 2 <= res_min <= NF, (n_cu, res_min)
    w, h = 480, 270
    frames = [synth_frame(w, h, seed=9300 + i) for i in range(res_min)]
    want = _oracle_extract(frames)
    ctx = akaze.Context(akaze.Akaze.default(), w, h, res_min)
    launches = {}
    try:
        ctx.timing_enable(2)
        for n in (res_min - 1, res_min):
            ctx.timing_reset()
            got = ctx.extract_batch(frames[:n])
            launches[n] = ctx.timing_get(AKZ_T_LEVEL_RESIDENT)[1]
            for i in range(n):
                okp, od = want[i]
                _kp_eq(got[i][0], okp, f"call of {n} frames, frame {i}")
                _eq(got[i][1], od, f"call of {n} frames, frame {i}.descriptors")
    finally:
        ctx.close()
    assert launches[res_min - 1] == 0, f"a call of {res_min - 1} frames (n_cu {n_cu}) ran k_level_resident {launches[res_min - 1]} times"
    assert launches[res_min] > 0, f"a call of {res_min} frames (n_cu {n_cu}) did not take k_level_resident"


@pytest.mark.parametrize("mb", [256, 64], ids=["one 256-frame call", "four 64-frame calls"])
def test_bench_step_equals_the_oracle(bench_step, tmp_path, mb):
    """`bench.py --steps 2 --warmup 1` in its default configuration (micro-batch 256: one call per step, k_level_resident
    by default) and with four 64-frame calls (below the resident threshold; pairs that span calls).  The dumped step is
    the third, the one that reuses output set 0.  The keypoint counts of all 256 frames, the pair list of every
    (j, (j - 1) mod 256) — (0, 255) included — and the match counts equal the oracle's; so do the keypoints,
    descriptors and pair lists of the frames the dump samples."""
    import subprocess
    import sys
    out, mfile = tmp_path / "out", tmp_path / "m.npy"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--micro-batch", str(mb),
                        "--dump-outputs", str(out), "--dump-matches", str(mfile)],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    h = json.loads(r.stdout.strip().splitlines()[-1])
    assert h["steps"] == 2 and h["config"]["frames_per_gpu_per_step"] == NF and h["config"]["micro_batch"] == mb
    _check_dump(out, mfile, bench_step["ext"], bench_step["pairs"])


def _check_dump(out, mfile, ext, opairs):
    """What bench.py --dump-outputs OUT --dump-matches MFILE wrote against the oracle's answers for the same frames."""
    nf = len(ext)
    a = {n[:-4]: np.load(out / n) for n in os.listdir(out)}
    okc = np.array([len(e[0]) for e in ext])
    kc = a["keypoint_counts"].astype(np.int64)
    assert kc.shape == (nf,)
    bad = np.flatnonzero(kc != okc)
    assert not bad.size, f"frame {bad[0]}: {kc[bad[0]]} keypoints, the oracle has {okc[bad[0]]} ({bad.size} frames differ)"
    pl = np.load(str(mfile) + ".r0.npz")
    mc = a["match_counts"].astype(np.int64)
    for j in range(nf):
        what = f"pairs of frame {j} against frame {(j - 1) % nf}"
        got = pl[f"g{j}"]
        assert got.shape == (len(opairs[j]), 2), f"{what}: {len(got)} pairs, the oracle has {len(opairs[j])}"
        _eq(got.astype(np.int64), opairs[j].astype(np.int64), what)
        assert mc[j] == len(got), f"frame {j}: match count {mc[j]}, pair list {len(got)}"
    # the sampled frames: keypoints as the dump writes them (7 float32 columns), descriptor bytes, pair lists
    sample = a["sample_frames"].astype(int)
    assert len(sample) == min(16, nf)
    k0 = m0 = 0
    for j in sample:
        okp, od = ext[j]
        n, m = len(okp), len(opairs[j])
        for c, f in enumerate(okp.dtype.names):
            _eq(a["keypoints"][k0:k0 + n, c], okp[f].astype(np.float32), f"sampled frame {j} keypoints.{f}")
        _eq(a["descriptors"][k0:k0 + n], od.astype(np.float32), f"sampled frame {j} descriptors")
        _eq(a["matches"][m0:m0 + m], opairs[j].astype(np.float32), f"sampled frame {j} matches")
        k0, m0 = k0 + n, m0 + m
    assert a["keypoints"].shape == (k0, 7) and len(a["descriptors"]) == k0 and len(a["matches"]) == m0
