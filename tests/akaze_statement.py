"""An independent float64 statement of akaze::Akaze::extract_from_gray_float_image.

Test helper (the same kind of thing as triangulate_checker.py).  Written from reading the akaze crate
(akaze/src/{image,evolution,fed_tau,contrast_factor,derivatives,nonlinear_diffusion,detector_response,
scale_space_extrema,descriptors,lib}.rs); numpy and the standard library only.  It shares no code, no header and no
arithmetic order with oracle/ or cv_amd/: every expression is evaluated once, plainly, in float64.  Two places are
deliberately float32, because there the single-precision value is part of what the reference means rather than how
accurately it computes: the discrete extrema / suppression decisions (so that equal planes give exactly one list)
and a few constants (the window starts of the orientation search, the descriptor grid step, sigma for the kernel
radius).
"""
import math
from dataclasses import dataclass

import numpy as np

F32 = np.float32
PI32 = float(np.float32(math.pi))          # std::f32::consts::PI, as the orientation code uses it


@dataclass
class Config:
    """akaze::Akaze and its Default (lib.rs)."""
    maximum_features: int = None           # None: usize::MAX
    num_sublevels: int = 4
    max_octave_evolution: int = 4
    base_scale_offset: float = 1.6
    initial_contrast: float = 0.001
    contrast_percentile: float = 0.7
    contrast_factor_num_bins: int = 300
    derivative_factor: float = 1.5
    detector_threshold: float = 0.001
    descriptor_channels: int = 3
    descriptor_pattern_size: int = 10


KP_FIELDS = ("x", "y", "response", "size", "angle", "octave", "class_id")


def round_away(x):
    """f32::round / f64::round: halves away from zero (numpy's round goes to even)."""
    x = np.asarray(x)
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0).astype(x.dtype)


# ---------------------------------------------------------------------------------------------------------------
# level schedule
def _is_prime(n):
    return n >= 2 and all(n % d for d in range(2, int(math.isqrt(n)) + 1))


def fed_tau(T, tau_max=0.25, reordering=True):
    """fed_tau_by_process_time(T, 1, tau_max, reordering)."""
    n = int(math.ceil(math.sqrt(3.0 * T / tau_max + 0.25) - 0.5 - 1.0e-8) + 0.5)
    scale = 3.0 * T / (tau_max * (n * (n + 1)))
    tau = [scale * tau_max / 2.0 / math.cos(math.pi * (2.0 * k + 1.0) / (4.0 * n + 2.0)) ** 2 for k in range(n)]
    if not reordering:
        return tau
    if n < 2:
        raise ValueError("a one-step cycle: the reference's reordering loop does not end (kappa = 0)")
    kappa, prime = n // 2, n + 1
    while not _is_prime(prime):
        prime += 1
    out, k = [], 0
    for _ in range(n):
        # the index is unsigned in the reference: 0 - 1 wraps to a huge value, which is "not below n"
        while not 0 <= ((k + 1) * kappa) % prime - 1 < n:
            k += 1
        out.append(tau[((k + 1) * kappa) % prime - 1])
        k += 1
    return out


def schedule(cfg, width, height):
    """allocate_evolutions + the derivative sigma of detector_response: a list of dicts, one per level."""
    levels = []
    for octave in range(cfg.max_octave_evolution):
        lw, lh = int(width * 2.0 ** -octave), int(height * 2.0 ** -octave)
        smallest = min(lw, lh)
        if smallest < 40:
            continue
        for sub in range(1 if smallest < 80 else cfg.num_sublevels):
            esigma = cfg.base_scale_offset * 2.0 ** (sub / cfg.num_sublevels + octave)
            levels.append(dict(octave=octave, sublevel=sub, esigma=esigma, etime=0.5 * esigma * esigma,
                               sigma_size=int(round_away(np.float64(esigma))), taus=[],
                               deriv_sigma=int(round_away(np.float64(esigma * cfg.derivative_factor / 2.0 ** octave)))))
    w, h = width, height
    for i, lv in enumerate(levels):
        if i and lv["octave"] > levels[i - 1]["octave"]:
            w, h = w // 2, h // 2                         # what half_size leaves
        lv["width"], lv["height"] = w, h
        if i:
            lv["taus"] = fed_tau(lv["etime"] - levels[i - 1]["etime"])
    return levels


# ---------------------------------------------------------------------------------------------------------------
# images and filters
def to_unit_float(img):
    """GrayFloatImage::from_dynamic: u8 / 255, u16 / 65535, f32 as it is."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.astype(np.float64) / 255.0
    if img.dtype == np.uint16:
        return img.astype(np.float64) / 65535.0
    assert img.dtype == np.float32, img.dtype
    return img.astype(np.float64)


def filter_axis(img, kernel, axis):
    """horizontal_filter (axis 1) / vertical_filter (axis 0): correlation, border pixels repeated."""
    r = len(kernel) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(np.asarray(img, np.float64), pad, mode="edge")
    n = img.shape[axis]
    out = np.zeros(img.shape, np.float64)
    for i, kv in enumerate(kernel):
        if kv != 0.0:
            out += float(kv) * (p[:, i:i + n] if axis == 1 else p[i:i + n, :])
    return out


def separable_filter(img, h_kernel, v_kernel):
    return filter_axis(filter_axis(img, h_kernel, 1), v_kernel, 0)


def gaussian_kernel(sigma, size):
    assert size % 2 == 1
    x = np.arange(size, dtype=np.float64) - size // 2
    k = np.exp(-x * x / (2.0 * sigma * sigma)) / (math.sqrt(2.0 * math.pi) * sigma)
    return k / k.sum()


def gaussian_blur(img, sigma):
    sigma = float(F32(sigma))                             # the reference takes sigma as f32
    radius = int(math.ceil(2.0 * sigma))
    k = gaussian_kernel(sigma, 2 * radius + 1)
    return separable_filter(img, k, k)


def half_size(img):
    img = np.asarray(img, np.float64)
    h, w = img.shape[0] // 2, img.shape[1] // 2
    a = img[:2 * h, :2 * w]
    out = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) * 0.25
    if 2 * h != img.shape[0]:                             # odd height: the last row comes from the last input row alone
        out[-1, :] = (img[-1, 0:2 * w:2] + img[-1, 1:2 * w:2]) * 0.5
    if 2 * w != img.shape[1]:
        out[:, -1] = (img[0:2 * h:2, -1] + img[1:2 * h:2, -1]) * 0.5
    if 2 * h != img.shape[0] and 2 * w != img.shape[1]:
        out[-1, -1] = img[-1, -1]
    return out


def scharr_kernels(sigma):
    """(main, off): the difference taps and the smoothing taps of the Scharr filter at an integer scale."""
    if sigma == 1:
        return np.array([-1.0, 0.0, 1.0]), np.array([3.0, 10.0, 3.0])
    size = 2 * sigma + 1
    w = 10.0 / 3.0
    norm = 1.0 / (2.0 * sigma * (w + 2.0))
    main = np.zeros(size)
    main[0], main[-1] = -1.0, 1.0
    off = np.zeros(size)
    off[0] = off[-1] = norm
    off[size // 2] = norm * w
    return main, off


def scharr(img, sigma, vertical):
    main, off = scharr_kernels(int(sigma))
    return separable_filter(img, off, main) if vertical else separable_filter(img, main, off)


# ---------------------------------------------------------------------------------------------------------------
# contrast factor and diffusion
def contrast_factor(img, percentile, num_bins, scale=1.0):
    """compute_contrast_factor.  Returns (k, margin): margin is how many points the cumulative histogram is away,
    on the nearer side, from crossing the percentile one bin earlier or later."""
    g = gaussian_blur(img, scale)
    lx, ly = scharr(g, 1, False)[1:-1, 1:-1], scharr(g, 1, True)[1:-1, 1:-1]
    mod = np.sqrt(lx * lx + ly * ly)
    hmax = mod.max()
    mod = mod[mod != 0.0]
    bins = np.minimum(np.floor(num_bins * (mod / hmax)).astype(np.int64), num_bins - 1)
    cum = np.cumsum(np.bincount(bins, minlength=num_bins))
    threshold = int(mod.size * percentile)
    k, count = 0, 0
    while count < threshold and k < num_bins:
        count = int(cum[k])
        k += 1
    if count < threshold:
        return 0.03, 0
    below = int(cum[k - 2]) if k >= 2 else 0
    return hmax * k / num_bins, min(count - threshold, threshold - below)


def pm_g2(lx, ly, k):
    return 1.0 / (1.0 + (1.0 / (k * k)) * (lx * lx + ly * ly))


def fed_step(L, c, tau):
    """calculate_step: one explicit step; no flow crosses the image border."""
    hf = 0.5 * tau * (c[:, :-1] + c[:, 1:]) * (L[:, 1:] - L[:, :-1])
    vf = 0.5 * tau * (c[:-1, :] + c[1:, :]) * (L[1:, :] - L[:-1, :])
    out = L.copy()
    out[:, :-1] += hf
    out[:, 1:] -= hf
    out[:-1, :] += vf
    out[1:, :] -= vf
    return out


def detector_planes(lsmooth, sigma):
    lx, ly = scharr(lsmooth, sigma, False), scharr(lsmooth, sigma, True)
    lxx, lyy, lxy = scharr(lx, sigma, False), scharr(ly, sigma, True), scharr(lx, sigma, True)
    return dict(Lx=lx, Ly=ly, Lxx=lxx, Lyy=lyy, Lxy=lxy, Ldet=(lxx * lyy - lxy * lxy) * float(sigma) ** 4)


def scale_space(cfg, img, levels=None, contrast=None):
    """create_nonlinear_scale_space + detector_response from the raw image.  Returns (levels, planes, contrast):
    planes[i] maps Lt, Lsmooth, Lflow (absent at level 0), Lx, Ly, Lxx, Lyy, Lxy, Ldet to float64 arrays."""
    f = to_unit_float(img)
    levels = levels if levels is not None else schedule(cfg, f.shape[1], f.shape[0])
    if contrast is None:
        contrast, _ = contrast_factor(f, cfg.contrast_percentile, cfg.contrast_factor_num_bins)
    k = contrast
    planes = []
    for i, lv in enumerate(levels):
        if i == 0:
            lt = gaussian_blur(f, cfg.base_scale_offset)
            p = dict(Lt=lt, Lsmooth=lt)
        else:
            lt = planes[-1]["Lt"]
            if lv["octave"] > levels[i - 1]["octave"]:
                lt = half_size(lt)
                k *= 0.75
            sm = gaussian_blur(lt, 1.0)
            flow = pm_g2(scharr(sm, 1, False), scharr(sm, 1, True), k)
            for tau in lv["taus"]:
                lt = fed_step(lt, flow, float(F32(tau)))   # the step is handed over as f32
            p = dict(Lt=lt, Lsmooth=sm, Lflow=flow)
        p.update(detector_planes(p["Lsmooth"], lv["deriv_sigma"]))
        planes.append(p)
    return levels, planes, contrast


# ---------------------------------------------------------------------------------------------------------------
# scale-space extrema: float32 scalars, decisions only
def find_extrema(cfg, levels, ldet):
    """find_scale_space_extrema on given Ldet planes (float32).  Returns a dict of arrays, one entry per keypoint."""
    thr = F32(cfg.detector_threshold)
    smax = F32(10.0) * np.sqrt(F32(2.0))
    cap = 1024
    cx, cy, cr, cs = (np.zeros(cap, F32) for _ in range(4))
    cc, co = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
    n = 0
    n_candidates = 0
    for e_id, lv in enumerate(levels):
        d = np.asarray(ldet[e_id], F32)
        h, w = d.shape
        c = d[1:-1, 1:-1]
        m = c > thr
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if (dy, dx) != (1, 1):
                    m &= c > d[dy:dy + h - 2, dx:dx + w - 2]
        ys, xs = np.nonzero(m)                             # row-major, as the reference walks the plane
        n_candidates += len(ys)
        size = F32(lv["esigma"] * cfg.derivative_factor)
        ratio = F32(2.0) ** F32(lv["octave"])
        sigma_size = round_away(size / ratio)
        reach = smax * sigma_size
        for y, x in zip(ys + 1, xs + 1):
            resp = np.abs(d[y, x])
            px, py = F32(x), F32(y)
            near = (cc[:n] == e_id) | (cc[:n] == e_id - 1)
            ddx, ddy = px * ratio - cx[:n], py * ratio - cy[:n]
            near &= ddx * ddx + ddy * ddy <= size * size
            slot = n
            if near.any():
                first = int(np.argmax(near))               # the first cached keypoint in range decides
                if not resp > cr[first]:
                    continue
                slot = first
            if (round_away(px - reach) - F32(1) < 0 or round_away(px + reach) + F32(1) >= F32(w)
                    or round_away(py - reach) - F32(1) < 0 or round_away(py + reach) + F32(1) >= F32(h)):
                continue
            if slot == cap:
                cap *= 2
                cx, cy, cr, cs = (np.resize(a, cap) for a in (cx, cy, cr, cs))
                cc, co = np.resize(cc, cap), np.resize(co, cap)
            cx[slot] = px * ratio + F32(0.5) * (ratio - F32(1))
            cy[slot] = py * ratio + F32(0.5) * (ratio - F32(1))
            cr[slot], cs[slot], cc[slot], co[slot] = resp, size, e_id, lv["octave"]
            n += slot == n
    cx, cy, cr, cs, cc, co = (a[:n] for a in (cx, cy, cr, cs, cc, co))
    keep = np.ones(n, bool)
    for i in range(n):                                     # the upper-level pass
        j = np.nonzero(cc[i + 1:] == cc[i] + 1)[0] + i + 1
        ddx, ddy = cx[i] - cx[j], cy[i] - cy[j]
        keep[i] = not np.any((ddx * ddx + ddy * ddy <= cs[i] * cs[i]) & (cr[i] <= cr[j]))
    return dict(x=cx[keep], y=cy[keep], response=cr[keep], size=cs[keep], angle=np.zeros(int(keep.sum()), F32),
                octave=co[keep], class_id=cc[keep], n_candidates=n_candidates)


# ---------------------------------------------------------------------------------------------------------------
# sub-pixel refinement and main orientation
def refine(kps, levels, ldet):
    """do_subpixel_refinement without the orientation.  Returns (keypoints, kept, offsets): `kept` indexes the input
    list, `offsets` [n_in, 2] are the solved offsets of every input keypoint (the test looks at those near +-1)."""
    n = len(kps["x"])
    off = np.zeros((n, 2))
    px, py = np.zeros(n), np.zeros(n)
    for lvl in np.unique(kps["class_id"]):
        sel = np.nonzero(kps["class_id"] == lvl)[0]
        d = np.asarray(ldet[lvl], np.float64)
        ratio = 2.0 ** levels[lvl]["octave"]
        x = round_away(kps["x"][sel].astype(np.float64) / ratio).astype(np.int64)
        y = round_away(kps["y"][sel].astype(np.float64) / ratio).astype(np.int64)
        dx = 0.5 * (d[y, x + 1] - d[y, x - 1])
        dy = 0.5 * (d[y + 1, x] - d[y - 1, x])
        dxx = d[y, x + 1] + d[y, x - 1] - 2.0 * d[y, x]
        dyy = d[y + 1, x] + d[y - 1, x] - 2.0 * d[y, x]
        dxy = 0.25 * (d[y + 1, x + 1] + d[y - 1, x - 1]) - 0.25 * (d[y - 1, x + 1] + d[y + 1, x - 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            det = dxx * dyy - dxy * dxy
            off[sel, 0] = (-dx * dyy + dy * dxy) / det
            off[sel, 1] = (dx * dxy - dy * dxx) / det
        px[sel] = (x + off[sel, 0]) * ratio + 0.5 * (ratio - 1.0)
        py[sel] = (y + off[sel, 1]) * ratio + 0.5 * (ratio - 1.0)
    kept = np.nonzero((np.abs(off[:, 0]) <= 1.0) & (np.abs(off[:, 1]) <= 1.0))[0]
    out = {f: np.asarray(kps[f])[kept] for f in KP_FIELDS}
    out["x"], out["y"] = px[kept], py[kept]
    out["size"] = out["size"].astype(np.float64) * 2.0
    out["response"] = out["response"].astype(np.float64)
    out["angle"] = np.zeros(len(kept))
    return out, kept, off


def orientation_weights():
    """The 7x7 quadrant table the reference tabulates: a Gaussian of sigma 2.5, normalised by 1 / (2 pi sigma^2)."""
    i = np.arange(7, dtype=np.float64)
    s2 = 2.5 * 2.5
    return np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2.0 * s2)) / (2.0 * math.pi * s2)


def window_starts():
    """ang1 of every window: the reference adds 0.15f32 to an f32 until it passes 2 pi."""
    out, a = [], F32(0.0)
    while a < F32(2.0) * F32(math.pi):
        out.append(float(a))
        a = F32(a + F32(0.15))
    return np.array(out)


def _angle_0_2pi(y, x):
    return np.mod(np.arctan2(y, x) + 2.0 * math.pi, 2.0 * math.pi)


def main_orientation(kps, levels, lx, ly):
    """compute_main_orientation for every keypoint.  Returns angles in [0, 2 pi)."""
    n = len(kps["x"])
    angle = np.zeros(n)
    kps = {f: np.asarray(kps[f], np.int64 if f in ("octave", "class_id") else np.float64) for f in KP_FIELDS}
    jj, ii = np.mgrid[-6:7, -6:7]
    inside = (ii * ii + jj * jj) < 36
    jj, ii = jj[inside], ii[inside]                        # 109 samples, rows (j) outside, columns (i) inside
    assert len(ii) == 109
    gw = orientation_weights()[np.abs(jj), np.abs(ii)]
    a1 = window_starts()
    assert len(a1) == 42
    a2 = np.where(a1 + PI32 / 3.0 > 2.0 * PI32, a1 - 5.0 * PI32 / 3.0, a1 + PI32 / 3.0)
    for lvl in np.unique(kps["class_id"]):
        sel = np.nonzero(kps["class_id"] == lvl)[0]
        ratio = float(1 << levels[lvl]["octave"])
        s = round_away(0.5 * kps["size"][sel] / ratio)
        xf, yf = kps["x"][sel] / ratio, kps["y"][sel] / ratio
        iy = round_away(yf[:, None] + jj[None, :] * s[:, None]).astype(np.int64)
        ix = round_away(xf[:, None] + ii[None, :] * s[:, None]).astype(np.int64)
        rx = gw[None, :] * np.asarray(lx[lvl], np.float64)[iy, ix]
        ry = gw[None, :] * np.asarray(ly[lvl], np.float64)[iy, ix]
        ang = _angle_0_2pi(ry, rx)[:, None, :]             # [n, 1, 109] against [42, 1]
        b1, b2 = a1[None, :, None], a2[None, :, None]
        member = ((b1 < b2) & (b1 < ang) & (ang < b2)) | \
                 ((b2 < b1) & (((ang > 0.0) & (ang < b2)) | ((ang > b1) & (ang < 2.0 * PI32))))
        sx, sy = (member * rx[:, None, :]).sum(axis=2), (member * ry[:, None, :]).sum(axis=2)
        val = sx * sx + sy * sy
        best = np.argmax(val, axis=1)                      # the first of equal maxima, as `val > max` keeps it
        r = np.arange(len(sel))
        angle[sel] = np.where(val[r, best] > 0.0, _angle_0_2pi(sy[r, best], sx[r, best]), 0.0)
    return angle


def sort_and_truncate(kps, maximum_features=None):
    """Descending response, then truncation.  The reference's sort is unstable; equal responses keep their order here."""
    order = np.argsort(-np.asarray(kps["response"], np.float64), kind="stable")
    if maximum_features is not None:
        order = order[:maximum_features]
    return {f: np.asarray(kps[f])[order] for f in KP_FIELDS}, order


# ---------------------------------------------------------------------------------------------------------------
# M-LDB
def descriptor_bit_count(channels):
    return channels * (6 + 36 + 120)


def mldb(cfg, kps, levels, lt, lx, ly):
    """get_mldb_descriptor for every keypoint on given planes.  Returns a dict:
       keep   [n] bool         False: a sample left the plane, the reference drops the keypoint
       bits   [n, nbits] bool  in descriptor order
       gap    [n, nbits]       |a - b| of the two cell means a bit compares
       tie    [n, nbits]       the least distance of a sample coordinate of either cell from a rounding tie
       chan   [nbits]          the channel of each bit."""
    n, nch, P = len(kps["x"]), cfg.descriptor_channels, cfg.descriptor_pattern_size
    assert 1 <= nch <= 3
    nbits = descriptor_bit_count(nch)
    keep = np.ones(n, bool)
    bits, gap = np.zeros((n, nbits), bool), np.zeros((n, nbits))
    tie = np.full((n, nbits), 0.5)
    chan = np.zeros(nbits, np.int64)
    values = np.zeros((n, 16 * 3))                         # filled grid after grid, never cleared in between
    vtie = np.full((n, 16 * 3), 0.5)
    x, y = np.asarray(kps["x"], np.float64), np.asarray(kps["y"], np.float64)
    size, ang = np.asarray(kps["size"], np.float64), np.asarray(kps["angle"], np.float64)
    cls = np.asarray(kps["class_id"])
    ratio = np.array([float(1 << int(levels[c]["octave"])) for c in cls]).reshape(n)
    scale = round_away(0.5 * size / ratio)
    xf, yf, co, si = x / ratio, y / ratio, np.cos(ang), np.sin(ang)
    dpos = 0
    for g, mult in enumerate((F32(1.0), F32(2.0) / F32(3.0), F32(1.0) / F32(2.0))):
        step = int(np.ceil(F32(P) * mult))
        starts = list(range(-P, P, step))
        assert len(starts) ** 2 * nch <= 48, "more cells than the reference has room for"
        inner = np.arange(step, dtype=np.float64)
        # cell order: the outer loop (i) steps k, the inner loop (j) steps l
        k = np.array([[i + a for a in inner for _ in inner] for i in starts for _ in starts])   # [cells, step^2]
        l = np.array([[j + b for _ in inner for b in inner] for _ in starts for j in starts])
        for lvl in np.unique(cls):
            sel = np.nonzero(cls == lvl)[0]
            c_, s_, sc = co[sel, None, None], si[sel, None, None], scale[sel, None, None]
            sy = yf[sel, None, None] + (l * c_ * sc + k * s_ * sc)
            sx = xf[sel, None, None] + (-l * s_ * sc + k * c_ * sc)
            iy, ix = round_away(sy).astype(np.int64), round_away(sx).astype(np.int64)
            t = np.minimum(np.abs(np.abs(sy - np.trunc(sy)) - 0.5), np.abs(np.abs(sx - np.trunc(sx)) - 0.5)).min(axis=2)
            h, w = lt[lvl].shape
            inb = ((ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)).all(axis=(1, 2))
            keep[sel[~inb]] = False
            iy, ix = np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)
            v = [np.asarray(lt[lvl], np.float64)[iy, ix].mean(axis=2)]
            if nch > 1:
                rx, ry = np.asarray(lx[lvl], np.float64)[iy, ix], np.asarray(ly[lvl], np.float64)[iy, ix]
                if nch == 2:
                    v.append(np.sqrt(rx * rx + ry * ry).mean(axis=2))
                else:
                    v.append((-rx * s_ + ry * c_).mean(axis=2))
                    v.append((rx * c_ + ry * s_).mean(axis=2))
            ncell = len(starts) ** 2
            for ch in range(nch):
                values[sel[:, None], nch * np.arange(ncell)[None, :] + ch] = v[ch]
                vtie[sel[:, None], nch * np.arange(ncell)[None, :] + ch] = t
        count = (g + 2) * (g + 2)
        a, b = np.triu_indices(count, 1)                   # i ascending, j > i ascending: the reference's order
        for ch in range(nch):
            va, vb = values[:, nch * a + ch], values[:, nch * b + ch]
            sl = slice(dpos, dpos + len(a))
            bits[:, sl], gap[:, sl] = va > vb, np.abs(va - vb)
            tie[:, sl] = np.minimum(vtie[:, nch * a + ch], vtie[:, nch * b + ch])
            chan[sl] = ch
            dpos += len(a)
    assert dpos == nbits
    return dict(keep=keep, bits=bits, gap=gap, tie=tie, chan=chan)


def pack_bits(bits):
    """[n, nbits] bool -> [n, 64] uint8, bit p in byte p >> 3 at position p & 7."""
    full = np.zeros((bits.shape[0], 512), np.uint8)
    full[:, :bits.shape[1]] = bits
    return np.packbits(full, axis=1, bitorder="little")


def unpack_bits(desc, nbits):
    return np.unpackbits(np.asarray(desc, np.uint8), axis=1, bitorder="little")[:, :nbits].astype(bool)


# ---------------------------------------------------------------------------------------------------------------
# the whole extractor, and the matcher of akaze/tests/estimate_pose.rs
def extract(cfg, img):
    """extract_from_gray_float_image, chained in float64 (the planes are rounded to float32 once, where the discrete
    extrema search reads them).  Returns (keypoints dict, descriptors [n, 64] uint8)."""
    levels, planes, _ = scale_space(cfg, img)
    ldet = [p["Ldet"].astype(F32) for p in planes]
    ext = find_extrema(cfg, levels, ldet)
    kps, _, _ = refine(ext, levels, [p["Ldet"] for p in planes])
    lt, lx, ly = ([p[name] for p in planes] for name in ("Lt", "Lx", "Ly"))
    kps["angle"] = main_orientation(kps, levels, lx, ly)
    kps, _ = sort_and_truncate(kps, cfg.maximum_features)
    d = mldb(cfg, kps, levels, lt, lx, ly)
    return {f: kps[f][d["keep"]] for f in KP_FIELDS}, pack_bits(d["bits"][d["keep"]])


def match_lowe(d1, d2, ratio=0.5):
    """Brute-force 2-NN (Hamming, lowest index first among equals) and Lowe's ratio in f32."""
    b1, b2 = unpack_bits(d1, 512), unpack_bits(d2, 512)
    dist = (b1[:, None, :] != b2[None, :, :]).sum(axis=2)
    order = np.argsort(dist, axis=1, kind="stable")[:, :2]
    r = np.arange(len(d1))
    d_0, d_1 = dist[r, order[:, 0]], dist[r, order[:, 1]]
    ok = d_0.astype(F32) < d_1.astype(F32) * F32(ratio)
    return [(int(i), int(order[i, 0])) for i in np.nonzero(ok)[0]]
