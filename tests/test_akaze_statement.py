"""The CPU oracle of the AKAZE extractor held to an independent float64 statement of the reference
(tests/akaze_statement.py).  CPU only.

Every GPU test of the extractor asks the kernels to equal oracle/akaze_oracle.c bit for bit; this file asks whether the
oracle reads the reference as a second reader does.  The statement was written from the akaze crate alone and shares
no code or arithmetic order with the oracle, so the two can only agree to rounding in the planes (section c) and
exactly in the discrete stages, which are fed the oracle's own planes (section d).  The comparison functions are
shared with test_gpu_akaze_statement.py, which asks the same of the device.
"""
import numpy as np
import pytest

import akaze_statement as S
from conftest import synth_frame
from test_gpu_parity import NON_DEFAULT

EPS = 2.0 ** -24

# Per-plane tolerance: C[name] * 2^-24 * max|plane| (Lt and Lflow have scale 1: absolute).  C is four times (Lflow: 2.7 times, below) the worst
# ratio |oracle - statement| / (2^-24 * scale) measured over every case of CASES (all eight arithmetic orders on the
# `arith` case included); the measured worst stands beside each entry, the full table is in docs/EXPERIMENTS.md.
# No entry may let a tolerance pass 1e-4 of the plane's maximum (C <= 1677): test_tolerances_stay_sharp.
PLANE_C = {
    #           C       measured worst ratio, case
    "Lt":      210,   # 52.6   num_sublevels=3 640x400
    "Lsmooth": 23,    # 5.7    base_scale_offset=1.2 640x400
    "Lflow":   1600,  # 597.4  contrast_percentile=0.5 333x251 (KITTI: 89); 4 x 597 = 2390 would pass 1e-4, see below
    "Lx":      24,    # 6.0    base_scale_offset=1.2 640x400
    "Ly":      28,    # 7.0    synth 97x83
    "Ldet":    55,    # 13.6   derivative_factor=1.0 333x251
}
# Lflow = 1 / (1 + |grad|^2 / k^2) magnifies the float32 rounding of the sigma-1 gradient where |grad| ~ k << max|grad|:
# the synthetic frames (hard edges, low contrast factor) reach 2^-24 * 600, the KITTI frames 2^-24 * 90.  Four times the
# worst would break the 1e-4 condition, so Lflow's C is held at that condition instead (2.7 times the worst).
ABSOLUTE = ("Lt", "Lflow")
PLANES = ("Lt", "Lsmooth", "Lflow", "Lx", "Ly", "Ldet")

CONTRAST_RTOL = 1e-6          # contrast factor, relative
CONTRAST_MARGIN = 8           # points between the percentile crossing and a bin edge, at least
POS_TOL = 1e-3                # refined positions, pixels
OFFSET_EDGE = 1e-4            # a sub-pixel offset this near +-1 may be kept or dropped by either side
ANGLE_TOL = 1e-4              # radians, modulo 2 pi
EXCUSED_FRAC = 0.005          # of a case's keypoints, for the offset edge and for window flips each
GAP_C = 64                    # a bit may differ if its two cell means are closer than GAP_C * 2^-24 * max|plane|
TIE_EDGE = 1e-4               # ... or if a sample coordinate is this near a rounding tie
ADMISSIBLE_KP_FRAC = 0.03     # keypoints touched by admissible bits
ADMISSIBLE_BIT_FRAC = 1e-4    # admissible bits of all bits


# ---------------------------------------------------------------------------------------------------------------
# views: what an implementation under test hands to the comparison functions
def oracle_view(orc, img):
    """Everything the oracle exposes after extract(img): a dict the comparison functions read."""
    final_kp, desc = orc.extract(img)
    n = orc.num_levels
    info = [orc.level(i) for i in range(n)]
    fields = ("width", "height", "octave", "sublevel", "esigma", "etime", "n_fed_steps", "deriv_sigma")
    levels = [dict({f: getattr(li, f) for f in fields}, taus=orc.fed_tau(i)) for i, li in enumerate(info)]
    planes = [{name: orc.buffer(i, name) for name in PLANES if not (i == 0 and name == "Lflow")} for i in range(n)]
    return dict(levels=levels, contrast=orc.contrast, planes=planes, stages=[orc.keypoints(s) for s in (0, 1, 2)],
                final_kp=final_kp, desc=desc)


def statement_config(kw):
    return S.Config(**kw)


# ---------------------------------------------------------------------------------------------------------------
# b. schedule and contrast factor
def check_schedule(levels, got):
    assert len(levels) == len(got), (len(levels), len(got))
    for i, (a, b) in enumerate(zip(levels, got)):
        for f in ("width", "height", "octave", "sublevel", "deriv_sigma"):
            assert a[f] == b[f], (i, f, a[f], b[f])
        assert len(a["taus"]) == b["n_fed_steps"] == len(b["taus"]), (i, len(a["taus"]), b["n_fed_steps"])
        for f in ("esigma", "etime"):
            assert abs(a[f] - b[f]) <= 1e-12 * abs(a[f]), (i, f, a[f], b[f])
        for k, (ta, tb) in enumerate(zip(a["taus"], b["taus"])):
            assert abs(ta - tb) <= 1e-12 * abs(ta), (i, "tau", k, ta, tb)


def check_contrast(want, got):
    rel = abs(got - want) / abs(want)
    assert rel <= CONTRAST_RTOL, (want, got, rel)
    return rel


# ---------------------------------------------------------------------------------------------------------------
# c. planes
def plane_ratios(want_planes, got_planes, names=PLANES, check_scale=False):
    """Worst |got - want| / (2^-24 * scale) per plane name over all levels: name -> (ratio, level, max|plane| there)."""
    worst = {}
    for lvl, (wp, gp) in enumerate(zip(want_planes, got_planes)):
        for name in names:
            if name not in gp or gp[name] is None:
                continue
            w, g = wp[name], np.asarray(gp[name], np.float64)
            assert w.shape == g.shape, (lvl, name, w.shape, g.shape)
            top = np.abs(w).max()
            scale = 1.0 if name in ABSOLUTE else top
            r = np.abs(g - w).max() / (EPS * scale)
            if r >= worst.get(name, (-1.0,))[0]:
                worst[name] = (r, lvl, top)
            if name in ABSOLUTE and check_scale:   # an absolute tolerance stays below 1e-4 of this plane's maximum too
                assert PLANE_C[name] * EPS <= 1e-4 * top, (lvl, name, top)
    return worst


def check_planes(want_planes, got_planes, names=PLANES, what=""):
    worst = plane_ratios(want_planes, got_planes, names, check_scale=True)
    print(f"planes {what}: " + ", ".join(f"{k} {v[0]:.1f}@{v[1]}" for k, v in worst.items()))
    for name, (r, lvl, _) in worst.items():
        assert r <= PLANE_C[name], (what, name, lvl, r, PLANE_C[name])
    return worst


# ---------------------------------------------------------------------------------------------------------------
# d. discrete stages
def check_extrema(cfg, levels, ldet, got_stage0):
    """The statement's search and both suppression passes on the given Ldet planes == the given stage-0 list, exactly."""
    want = S.find_extrema(cfg, levels, ldet)
    assert len(want["x"]) == len(got_stage0), (len(want["x"]), len(got_stage0))
    for f in S.KP_FIELDS:
        a, b = np.asarray(want[f]), got_stage0[f]
        if b.dtype == np.float32:
            same = a.astype(np.float32).view(np.uint32) == b.view(np.uint32)
        else:
            same = a == b
        assert same.all(), (f, int(np.argmin(same)), a[np.argmin(same)], b[np.argmin(same)])
    return want


def _subsequence(parent, child, fields):
    """Indices into `parent` of the rows of `child`, which keeps the parent's order and its values of `fields`."""
    idx, p = [], 0
    for row in child:
        while p < len(parent) and any(parent[f][p] != row[f] for f in fields):
            p += 1
        assert p < len(parent), "a keypoint that its parent list does not hold"
        idx.append(p)
        p += 1
    return np.array(idx, np.int64)


def check_refinement(levels, planes, stage0, got_stage1, what=""):
    """Sub-pixel refinement and main orientation of the statement, on the given planes and stage-0 list, against the
    given stage-1 list.  Returns (statement keypoints aligned with got_stage1, excused mask over got_stage1)."""
    ldet = [p["Ldet"] for p in planes]
    ref, kept, off = S.refine(stage0, levels, ldet)
    ref["angle"] = S.main_orientation(ref, levels, [p["Lx"] for p in planes], [p["Ly"] for p in planes])
    got_kept = _subsequence(stage0, got_stage1, ("response", "class_id", "octave"))
    edge = np.abs(np.abs(off) - 1.0).min(axis=1) < OFFSET_EDGE
    only_one = np.setxor1d(kept, got_kept)
    assert edge[only_one].all(), (what, "kept by one side only, away from the +-1 edge", only_one[~edge[only_one]][:5],
                                  off[only_one[~edge[only_one]][:5]])
    assert len(only_one) <= EXCUSED_FRAC * max(len(stage0), 1), (what, len(only_one), len(stage0))
    # align the statement's keypoints with got_stage1; a row the statement dropped borrows the given values, excused
    pos = {int(k): i for i, k in enumerate(kept)}
    n = len(got_stage1)
    excused = np.zeros(n, bool)
    mine = {f: np.zeros(n, np.int64 if f in ("octave", "class_id") else np.float64) for f in S.KP_FIELDS}
    for r, k in enumerate(got_kept):
        if int(k) in pos:
            for f in S.KP_FIELDS:
                mine[f][r] = ref[f][pos[int(k)]]
        else:
            excused[r] = True
            for f in S.KP_FIELDS:
                mine[f][r] = got_stage1[f][r]
    ok = ~excused
    dpos = np.maximum(np.abs(mine["x"] - got_stage1["x"]), np.abs(mine["y"] - got_stage1["y"]))
    dang = np.abs(np.mod(mine["angle"] - got_stage1["angle"] + np.pi, 2.0 * np.pi) - np.pi)
    flips = ok & (dang > ANGLE_TOL)
    print(f"refinement {what}: {n} keypoints, offset-edge {len(only_one)}, worst position {dpos[ok].max(initial=0.0):.2e} px, "
          f"median angle {np.median(dang[ok]) if ok.any() else 0.0:.2e} rad, window flips {int(flips.sum())}")
    assert (dpos[ok] <= POS_TOL).all(), (what, "position", int(np.argmax(dpos * ok)), dpos.max())
    for f in ("size", "response"):
        assert (mine[f].astype(np.float32) == got_stage1[f])[ok].all(), (what, f)
    for f in ("octave", "class_id"):
        assert (mine[f] == got_stage1[f]).all(), (what, f)
    assert flips.sum() <= EXCUSED_FRAC * max(n, 1), (what, "angles off by more than the tolerance", int(flips.sum()), n)
    return mine, excused | flips


def check_sort(got_stage1, got_stage2, maximum_features):
    """Descending response (equal responses in list order) and truncation of the given stage-1 list == stage 2."""
    _, order = S.sort_and_truncate({f: got_stage1[f] for f in S.KP_FIELDS}, maximum_features)
    assert got_stage1[order].tobytes() == got_stage2.tobytes()
    return order


def plane_scales(planes):
    """max|plane| per level for the three descriptor channels: intensity, and the two gradient channels."""
    out = np.zeros((len(planes), 3))
    for i, p in enumerate(planes):
        g = max(np.abs(p["Lx"]).max(), np.abs(p["Ly"]).max())
        out[i] = (np.abs(p["Lt"]).max(), g, g)
    return out


def check_descriptors(cfg, levels, planes, kps, got_keep, got_desc, excused, what="", got_kps=None):
    """M-LDB of the statement at `kps` on the given Lt / Lx / Ly against the given descriptors.
    got_keep [n] says which of `kps` the implementation kept; got_desc holds one row per kept keypoint.
    got_kps: the implementation's own float32 keypoints, row for row, where `kps` are the statement's.  The two differ
    within POS_TOL / ANGLE_TOL, which moves a sample coordinate by about as much as TIE_EDGE: the distance of a sample
    from a rounding tie is taken at whichever of the two keypoints puts it nearer (both evaluated in float64)."""
    n = len(kps["x"])
    lt_lx_ly = [[p[name] for p in planes] for name in ("Lt", "Lx", "Ly")]
    d = S.mldb(cfg, kps, levels, *lt_lx_ly)
    if got_kps is not None:
        at_got = {f: np.asarray(got_kps[f], np.int64 if f in ("octave", "class_id") else np.float64) for f in S.KP_FIELDS}
        d["tie"] = np.minimum(d["tie"], S.mldb(cfg, at_got, levels, *lt_lx_ly)["tie"])
    nbits = d["bits"].shape[1]
    got_bits = np.zeros((n, nbits), bool)
    full = S.unpack_bits(got_desc, 512)
    assert not full[:, nbits:].any(), (what, "bits past the descriptor's length are set")
    got_bits[got_keep] = full[:, :nbits]
    ok = ~excused
    near_tie = d["tie"].min(axis=1) < TIE_EDGE
    wrong_keep = ok & (d["keep"] != got_keep)
    assert not (wrong_keep & ~near_tie).any(), (what, "dropped by one side only", np.nonzero(wrong_keep & ~near_tie)[0][:5])
    both = ok & d["keep"] & got_keep
    scale = plane_scales(planes)[np.asarray(kps["class_id"], np.int64)][:, d["chan"]]        # [n, nbits]
    differ = (d["bits"] != got_bits) & both[:, None]
    admissible = differ & ((d["gap"] < GAP_C * EPS * scale) | (d["tie"] < TIE_EDGE))
    bad = differ & ~admissible
    touched = int((admissible.any(axis=1) | wrong_keep).sum())
    total = max(int(both.sum()) * nbits, 1)
    print(f"descriptors {what}: {int(both.sum())} keypoints, differing bits {int(differ.sum())} (admissible "
          f"{int(admissible.sum())}), keypoints touched {touched}, most in one {int(differ.sum(axis=1).max(initial=0))}")
    assert not bad.any(), (what, "bits that differ with a clear margin", int(bad.sum()), np.argwhere(bad)[:5],
                           d["gap"][bad][:5])
    assert touched <= ADMISSIBLE_KP_FRAC * max(int(ok.sum()), 1), (what, touched, int(ok.sum()))
    assert admissible.sum() <= ADMISSIBLE_BIT_FRAC * total, (what, int(admissible.sum()), total)
    return dict(differ=int(differ.sum()), touched=touched, keypoints=int(both.sum()))


def as_f64_planes(planes):
    return [{k: np.asarray(v, np.float64) for k, v in p.items() if v is not None} for p in planes]


def check_discrete_stages(cfg, levels, view, what=""):
    """Section d on one view: its own planes in, its stage lists and descriptors against the statement."""
    planes = as_f64_planes(view["planes"])
    s0, s1, s2 = view["stages"]
    check_extrema(cfg, levels, [p["Ldet"] for p in view["planes"]], s0)
    mine, excused = check_refinement(levels, planes, s0, s1, what)
    order = check_sort(s1, s2, cfg.maximum_features)
    kps = {f: mine[f][order] for f in S.KP_FIELDS}
    got_keep = np.zeros(len(s2), bool)
    got_keep[_subsequence(s2, view["final_kp"], S.KP_FIELDS)] = True
    assert view["final_kp"].tobytes() == s2[got_keep].tobytes()
    return check_descriptors(cfg, levels, planes, kps, got_keep, view["desc"], excused[order], what, got_kps=s2)


# ---------------------------------------------------------------------------------------------------------------
# cases
def _u16_frame():
    img8 = synth_frame(320, 240, seed=320, n_rect=30, n_disc=30)
    rng = np.random.default_rng(16)
    return (img8.astype(np.uint16) * 257 + rng.integers(-120, 121, img8.shape)).clip(0, 65535).astype(np.uint16)


def _f32_frame():
    img8 = synth_frame(333, 219, seed=77, n_rect=30, n_disc=30)
    return ((img8.astype(np.float32) / np.float32(255.0)) ** np.float32(1.1) * np.float32(0.9)).astype(np.float32)


def _synth(w, h, seed):
    return lambda: synth_frame(w, h, seed=seed, n_rect=40, n_disc=40)


def _kitti(i):
    return ("kitti", i)


SYNTH = ((640, 400, 5), (333, 251, 6))

CASES = [
    ("kitti0 0.01", _kitti(0), dict(detector_threshold=0.01), 0),
    ("kitti0 0.001", _kitti(0), dict(), 0),
    ("kitti14 0.01", _kitti(1), dict(detector_threshold=0.01), 0),
    ("kitti14 0.001", _kitti(1), dict(), 0),
    ("synth 640x400", _synth(640, 400, 5), dict(), 0),
    ("synth 333x251", _synth(333, 251, 6), dict(), 0),
    ("synth 97x83", _synth(97, 83, 97083), dict(), 0),
    ("synth 1920x1080", lambda: synth_frame(1920, 1080, 7303, n_rect=150, n_disc=150), dict(), 0),
] + [
    (f"{name} {w}x{h}", _synth(w, h, seed), kw, 0) for name, kw in NON_DEFAULT for (w, h, seed) in SYNTH
] + [
    ("channels=1 333x251", _synth(333, 251, 6), dict(descriptor_channels=1), 0),
    ("channels=2 333x251", _synth(333, 251, 6), dict(descriptor_channels=2), 0),
    ("channels=3 640x400", _synth(640, 400, 5), dict(descriptor_channels=3), 0),
    ("u16 320x240", _u16_frame, dict(), 0),
    ("f32 333x219", _f32_frame, dict(), 0),
    ("arith=7 333x251", _synth(333, 251, 6), dict(), 7),
]


def case_image(src, kitti):
    return kitti[src[1]] if isinstance(src, tuple) else src()


class Run:
    pass


def run_case(O, kitti, name, src, kw, arith):
    """The oracle and the chained statement on one case."""
    r = Run()
    r.name, r.img = name, case_image(src, kitti)
    r.cfg = statement_config(kw)
    ocfg = O.default_config()
    for k, v in kw.items():
        setattr(ocfg, k, v)
    h, w = r.img.shape
    opts = (O.OPT_REDUCE, O.OPT_FMA, O.OPT_HALFSUM)
    try:
        for bit, o in enumerate(opts):
            O.set_option(o, (arith >> bit) & 1)
        r.view = oracle_view(O.Akaze(w, h, ocfg), r.img)
    finally:
        for o in opts:
            O.set_option(o, 0)
    f = S.to_unit_float(r.img)
    r.levels = S.schedule(r.cfg, w, h)
    r.contrast, r.margin = S.contrast_factor(f, r.cfg.contrast_percentile, r.cfg.contrast_factor_num_bins)
    _, r.planes, _ = S.scale_space(r.cfg, r.img, r.levels, r.contrast)
    return r


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def run(request, oracle, kitti):
    return run_case(oracle, kitti, *request.param)


# ---------------------------------------------------------------------------------------------------------------
# a. the statement stands on the reference's pins by itself
def test_statement_alone_reproduces_the_reference_pins(kitti):
    """akaze/tests/estimate_pose.rs: Akaze::sparse() gives exactly 399 and 343 descriptors on the two KITTI frames and
    2-NN with Lowe's ratio 0.5 gives exactly 11 matches — from the statement alone, chained in float64 from the u8
    image with its own schedule and contrast factor, nothing of the oracle in it."""
    cfg = S.Config(detector_threshold=0.01)
    k0, d0 = S.extract(cfg, kitti[0])
    k1, d1 = S.extract(cfg, kitti[1])
    assert (len(d0), len(d1)) == (399, 343)
    assert len(k0["x"]) == 399 and len(k1["x"]) == 343
    assert len(S.match_lowe(d0, d1, 0.5)) == 11
    assert np.all(np.diff(k0["response"]) <= 0)


def test_statement_gaussian_known_answer():
    """akaze/src/image.rs, gaussian_kernel_correct."""
    known = [0.10628852, 0.14032133, 0.16577007, 0.17524014, 0.16577007, 0.14032133, 0.10628852]
    assert np.all(np.abs(S.gaussian_kernel(3.0, 7) - np.array(known)) < 1e-4)


def test_orientation_weights_are_the_tabulated_gaussian():
    """Corners and centre of the reference's 7x7 table (scale_space_extrema.rs), from the formula, within 2e-8."""
    w = S.orientation_weights()
    for (i, j, v) in ((0, 0, 0.02546481), (0, 6, 0.00142946), (6, 6, 0.00008024), (3, 3, 0.00603332), (2, 5, 0.00250252)):
        assert abs(w[i, j] - v) < 2e-8 and abs(w[j, i] - v) < 2e-8


def test_tolerances_stay_sharp():
    """No plane tolerance may pass 1e-4 of the plane's maximum: every plausible misreading (a wrong tap weight, a missed
    0.75, sigma^4 for sigma^2, a wrong border) moves a plane by 1e-3 of it or more."""
    for name, c in PLANE_C.items():
        assert c * EPS <= 1e-4, (name, c)
    assert GAP_C * EPS < 1e-5 and POS_TOL <= 1e-3 and ANGLE_TOL <= 1e-4


# ---------------------------------------------------------------------------------------------------------------
# b - d on every case
@pytest.mark.parametrize("w,h", [(1392, 512), (1920, 1080), (333, 251)])
def test_default_schedule(oracle, w, h):
    orc = oracle.Akaze(w, h, oracle.default_config())
    fields = ("width", "height", "octave", "sublevel", "esigma", "etime", "n_fed_steps", "deriv_sigma")
    got = [dict({f: getattr(orc.level(i), f) for f in fields}, taus=orc.fed_tau(i)) for i in range(orc.num_levels)]
    check_schedule(S.schedule(S.Config(), w, h), got)
    assert len(got) == {1392: 13, 1920: 16, 333: 9}[w]


def test_schedule_and_contrast_factor(run):
    check_schedule(run.levels, run.view["levels"])
    assert run.margin >= CONTRAST_MARGIN, (run.name, "percentile crossing too near a bin edge: use another seed", run.margin)
    rel = check_contrast(run.contrast, run.view["contrast"])
    print(f"contrast {run.name}: {run.contrast:.9g} vs {run.view['contrast']:.9g}, relative {rel:.1e}, margin {run.margin}")


def test_planes_chained(run):
    """From the raw input to every plane of every level, statement (float64 throughout) against the oracle."""
    check_planes(run.planes, run.view["planes"], what=run.name)


def test_discrete_stages(run):
    """Extrema, suppression, refinement, orientation, sort, truncation and M-LDB on the oracle's own planes."""
    check_discrete_stages(run.cfg, run.levels, run.view, run.name)


def _tie_setup(oracle):
    w, h = 640, 480
    cfg = statement_config(dict(base_scale_offset=2.0))
    ocfg = oracle.default_config()
    ocfg.base_scale_offset = 2.0
    return cfg, S.schedule(cfg, w, h), oracle.Akaze(w, h, ocfg)


def test_extrema_search_with_exact_ties(oracle):
    """Natural frames never put an equality in front of the search's `<=` comparisons, so `<` for `<=` passes every case
    above.  Here the oracle's search runs on made-up Ldet planes (orc_extrema_of_planes): sparse spikes of four heights
    (k / 8), so equal responses meet inside one level and across adjacent levels, and base_scale_offset = 2.0, which
    makes the keypoint size 3.0, 6.0 and 12.0 at the first sublevel of each octave, so squared distances of 9, 36 and
    144 meet size * size exactly.  The list must equal the statement's, keypoint for keypoint."""
    cfg, levels, orc = _tie_setup(oracle)
    rng = np.random.default_rng(11)
    planes = []
    for lv in levels:
        shape = (lv["height"], lv["width"])
        planes.append(np.where(rng.random(shape) < 0.05, rng.integers(1, 5, shape) / 8.0, 0.0).astype(np.float32))
    got = orc.extrema_of_planes(planes)
    want = check_extrema(cfg, levels, planes, got)
    assert len(got) > 1000 and want["n_candidates"] == orc.num_candidates
    assert len(np.unique(got["class_id"])) >= 8
    assert np.float32(3.0) == got["size"][got["class_id"] == 0][0]


@pytest.mark.parametrize("resp_a,resp_b,survivors", [(0.5, 0.5, 1), (0.5, 0.625, 1), (0.625, 0.5, 2)],
                         ids=["equal responses", "upper level stronger", "lower level stronger"])
def test_upper_level_pass_on_a_planted_pair(oracle, resp_a, resp_b, survivors):
    """The upper-level pass only ever meets a pair across an octave boundary: inside an octave the first pass has already
    settled every pair it could see (same coordinates, larger radius).  Across one, the first pass measures from the
    upper keypoint's unshifted position and the second from the shifted one (+ 0.5 (ratio - 1)), so a pair can be out of
    range first and in range later.  Planted here: A at (124, 124) of level 7 (octave 1, size 10.09), B at (60, 60) of
    level 8 (octave 2, size 12): first pass 8.5^2 + 8.5^2 = 144.5 > 144, second pass 7^2 + 7^2 = 98 <= 101.8.  A goes
    if and only if its response is at most B's — equality included."""
    cfg, levels, orc = _tie_setup(oracle)
    assert (levels[7]["octave"], levels[8]["octave"], levels[8]["sublevel"]) == (1, 2, 0)
    planes = [np.zeros((lv["height"], lv["width"]), np.float32) for lv in levels]
    planes[7][124, 124] = resp_a
    planes[8][60, 60] = resp_b
    got = orc.extrema_of_planes(planes)
    want = check_extrema(cfg, levels, planes, got)
    assert want["n_candidates"] == 2 and len(got) == survivors
    assert got["class_id"][-1] == 8 and (got["x"][-1], got["y"][-1]) == (241.5, 241.5)


# ---------------------------------------------------------------------------------------------------------------
# e. the checker can say no
@pytest.fixture(scope="module")
def small(oracle, kitti):
    return run_case(oracle, kitti, "synth 640x400", _synth(640, 400, 5), dict(), 0)


def _altered(view, **kw):
    out = dict(view)
    out.update(kw)
    return out


def test_checker_accepts_the_unaltered_case(small):
    check_planes(small.planes, small.view["planes"])
    check_discrete_stages(small.cfg, small.levels, small.view)


@pytest.mark.parametrize("name", PLANES)
def test_checker_refuses_a_shifted_row(small, name):
    """1e-4 of the plane's maximum added to one row of one plane."""
    lvl = 5
    planes = [dict(p) for p in small.view["planes"]]
    p = planes[lvl][name].copy()
    p[p.shape[0] // 3] += np.float32(1e-4) * np.abs(p).max()
    planes[lvl][name] = p
    with pytest.raises(AssertionError):
        check_planes(small.planes, planes)


def test_checker_refuses_swapped_neighbours(small):
    s0 = small.view["stages"][0].copy()
    s0[[10, 11]] = s0[[11, 10]]
    with pytest.raises(AssertionError):
        check_extrema(small.cfg, small.levels, [p["Ldet"] for p in small.view["planes"]], s0)


def test_checker_refuses_a_moved_keypoint(small):
    planes = as_f64_planes(small.view["planes"])
    s0, s1, _ = small.view["stages"]
    check_refinement(small.levels, planes, s0, s1)
    for f in ("x", "y"):
        moved = s1.copy()
        moved[f][len(moved) // 2] += np.float32(0.01)
        with pytest.raises(AssertionError):
            check_refinement(small.levels, planes, s0, moved)


def test_checker_refuses_turned_angles(small):
    planes = as_f64_planes(small.view["planes"])
    s0, s1, _ = small.view["stages"]
    turned = s1.copy()
    assert len(turned) >= 200
    turned["angle"][::100] += np.float32(0.01)                # 1 % of the keypoints
    with pytest.raises(AssertionError):
        check_refinement(small.levels, planes, s0, turned)


@pytest.mark.parametrize("how", ["one random bit in 5 % of the descriptors", "the same bit in every descriptor"])
def test_checker_refuses_flipped_bits(small, how):
    rng = np.random.default_rng(3)
    desc = small.view["desc"].copy()
    if how.startswith("the same"):
        rows, bits = np.arange(len(desc)), np.full(len(desc), 200)
    else:
        rows = rng.choice(len(desc), len(desc) // 20, replace=False)
        bits = rng.integers(0, 486, len(rows))
    desc[rows, bits >> 3] ^= (1 << (bits & 7)).astype(np.uint8)
    with pytest.raises(AssertionError):
        check_discrete_stages(small.cfg, small.levels, _altered(small.view, desc=desc))
