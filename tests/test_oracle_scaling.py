"""A power-of-two scaling property of the oracle's extract, the yardstick tests/test_gpu_input_contract.py holds the device to.

Multiplying an f32 frame by s = 2^-k is exact in IEEE arithmetic, and so is every sum, product and quotient of scaled
values as long as each result stays a normal number: rounding commutes with a power-of-two factor.  Through the pipeline:
  - the blurs, the half-size means, the Scharr derivatives and the FED steps are linear in the image: Lt, Lsmooth, Lx, Ly
    scale by s;
  - the contrast factor is a percentile of gradient magnitudes over their maximum (bins are magnitude / max): it scales by
    s, and the conductance g(|grad L|^2 / k^2) sees s^2 / s^2 — unchanged, so the diffusion stays linear;
  - Ldet = Lxx Lyy - Lxy^2 (times a power of the scale) scales by s^2, and so does a threshold of detector_threshold * s^2:
    the same extrema, the same suppression (it compares responses and positions only);
  - the subpixel refinement solves a 2 x 2 system of Ldet differences: the offset is a quotient of an s^2 * s^2 numerator
    and an s^4 determinant, so x, y are unchanged; the response is |Ldet| and scales by s^2;
  - the orientation is atan2 of Gaussian-weighted sums of Lx, Ly (a ratio), the descriptor compares sample means of Lt, Lx,
    Ly with each other: size, angle, octave, class_id and every descriptor bit are unchanged.
The property breaks first in the refinement: its determinant d_xx d_yy - d_xy^2 scales by s^4, and its reciprocal
overflows f32 once s^4 times the determinant leaves the normal range (around k = 26 for these frames; at k = 32 no keypoint
survives while the extrema are still the same).  At k = 4 and k = 12 every intermediate is normal and the property holds
for every field, bit for bit."""
import numpy as np
import pytest

from conftest import synth_frame

W, H = 320, 240


def _f32_frame(seed):
    """synth_frame as f32 with values that are not k / 255 (low-order noise, clipped to the documented [0, 1])."""
    rng = np.random.default_rng(seed)
    img = synth_frame(W, H, seed, n_rect=30, n_disc=30).astype(np.float32) / np.float32(255)
    return np.clip(img + rng.uniform(-1 / 600, 1 / 600, img.shape).astype(np.float32), 0, 1).astype(np.float32)


def _extract(O, img, thr):
    o = O.Akaze(W, H, O.default_config(threshold=thr))
    kp, d = o.extract(img)
    return o, kp, d


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("k", [4, 12])
@pytest.mark.parametrize("seed", [71, 72])
def test_power_of_two_scaling_is_exact(oracle, seed, k):
    """Frame * 2^-k with detector_threshold * 2^-2k: every keypoint field but the response bit-identical, the response
    exactly 2^-2k times the unscaled one, every descriptor byte identical, the contrast factor exactly 2^-k times."""
    O = oracle
    img = _f32_frame(seed)
    s = np.float32(2.0 ** -k)
    base, kp0, d0 = _extract(O, img, 0.001)
    o, kp, d = _extract(O, img * s, 0.001 * 2.0 ** (-2 * k))
    assert len(kp0) > 100
    assert len(kp) == len(kp0), f"seed {seed}, 2^-{k}: {len(kp)} keypoints, unscaled {len(kp0)}"
    for f in ("x", "y", "size", "angle", "octave", "class_id"):
        assert np.array_equal(kp[f].view(np.uint32), kp0[f].view(np.uint32)), f"seed {seed}, 2^-{k}: keypoints.{f} changed"
    want = (kp0["response"] * s * s).astype(np.float32)
    assert np.array_equal(_bits(kp["response"]), _bits(want)), f"seed {seed}, 2^-{k}: response is not 2^-{2 * k} times"
    assert np.array_equal(d, d0), f"seed {seed}, 2^-{k}: descriptors changed"
    assert o.contrast == base.contrast * 2.0 ** -k, (o.contrast, base.contrast)
    # and the planes in between: Lt / Lx / Ly by s, Ldet by s^2, at every level
    for lvl in range(base.num_levels):
        for name, f in (("Lt", s), ("Lx", s), ("Ly", s), ("Ldet", s * s)):
            a, b = o.buffer(lvl, name), base.buffer(lvl, name)
            assert np.array_equal(_bits(a), _bits((b * f).astype(np.float32))), f"seed {seed}, 2^-{k}: {name}[{lvl}]"


def test_the_property_ends_in_the_refinement(oracle):
    """Where it stops holding, and why: at 2^-32 the extrema (stage 0: positions, level, response * s^2) are still those
    of the unscaled frame, but the refinement's s^4 determinant has left the normal range and its reciprocal overflows —
    no keypoint survives.  (So the GPU test uses 2^-4 and 2^-12, well inside the range, and holds 2^-60 to the oracle
    bit for bit instead.)"""
    O = oracle
    k = 32
    img = _f32_frame(71)
    s = np.float32(2.0 ** -k)
    base, kp0, _ = _extract(O, img, 0.001)
    o, kp, _ = _extract(O, img * s, 0.001 * 2.0 ** (-2 * k))
    e0, e = base.keypoints(0), o.keypoints(0)
    assert len(e0) > 100 and len(e) == len(e0)
    for f in ("x", "y", "size", "octave", "class_id"):
        assert np.array_equal(e[f].view(np.uint32), e0[f].view(np.uint32)), f"stage 0 keypoints.{f}"
    assert np.array_equal(_bits(e["response"]), _bits((e0["response"] * s * s).astype(np.float32)))
    assert len(kp0) > 100 and len(kp) == 0
