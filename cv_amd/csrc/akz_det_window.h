// akz_det_window.h — which pixels the determinant / candidate pass of a level visits, and how its launches are cut.
// Host integer arithmetic only (no HIP, no libm): akz_scale_space.hip launches by it, tests/cpp/det_window.cpp holds it to
// its properties under a sanitizer.
//
// A pixel can become a candidate only where it is interior (scale_space_extrema.rs:50) and passes the border test
// (:96-104); akz_plan.cpp reduces both to the inclusive ranges cand_x_lo..cand_x_hi, cand_y_lo..cand_y_hi of a level.  A
// candidate record carries its own 3x3 determinant neighbourhood and the Ldet plane is not written unless the parity taps
// are on, so the determinant is needed one pixel around that window and nowhere else: the frame-shaped ring outside it
// (10 sqrt(2) deriv_sigma pixels on each side, 28 / 42 / 57 for sigma 2 / 3 / 4 at every octave) is not visited.
#pragma once

// candidate positions [x0, x1) x [y0, y1) a launch answers for
struct AkzDetWindow {
    int x0, x1, y0, y1;
    bool empty() const { return x1 <= x0 || y1 <= y0; }
    int width() const { return x1 - x0; }
    int height() const { return y1 - y0; }
};

// whole_plane: the Ldet tap is on (every pixel of the plane is written and compared)
inline AkzDetWindow akz_det_window(int w, int h, int x_lo, int x_hi, int y_lo, int y_hi, bool whole_plane)
{
    if (whole_plane) return AkzDetWindow{0, w, 0, h};
    if (x_hi < x_lo || y_hi < y_lo) return AkzDetWindow{0, 0, 0, 0};      // no pixel passes the border test
    return AkzDetWindow{x_lo, x_hi + 1, y_lo, y_hi + 1};
}

// Streaming kernel (k_det_stream<SG>): a wave holds 128 columns, two per lane, of which the outer `halo` on each side only
// feed the stencil of the `band` useful ones in between.
constexpr int det_stream_halo(int SG) { return (SG + 2) & ~1; }                    // columns each side: even, >= SG + 1
constexpr int det_stream_band(int SG) { return 128 - 2 * det_stream_halo(SG); }     // useful columns per wave

// Band b answers for columns x0 + b * band .. and segment s for rows y0 + s * seg_rows ..; segments are
// sized so that the launch holds about target_waves waves over its n frames, never shorter than 32 rows (each segment
// re-reads 2 sigma + 2 rows of warm-up).  The window must not be empty.
struct AkzDetStreamGrid {
    int nb, nseg, seg_rows;
};
inline AkzDetStreamGrid akz_det_stream_grid(const AkzDetWindow& W, int band, int target_waves, int n)
{
    AkzDetStreamGrid G;
    G.nb = (W.width() + band - 1) / band;
    long long per = (long long)G.nb * n;
    int nseg = (int)((target_waves + per - 1) / per);
    const int max_seg = (W.height() + 31) / 32;
    nseg = nseg < 1 ? 1 : (nseg > max_seg ? max_seg : nseg);
    G.seg_rows = (W.height() + nseg - 1) / nseg;
    G.nseg = (W.height() + G.seg_rows - 1) / G.seg_rows;
    return G;
}

// Tile kernels: tiles of tw x th pixels on the plane's own tile lattice (tile origins stay multiples of tw, th: the 16-byte
// staging loads keep their alignment); the grid covers the tiles that hold a pixel of the window grown by one pixel.
// The window must not be empty.
struct AkzDetTileGrid {
    int tx0, ty0, ntx, nty;      // first tile and number of tiles, in tile units
};
inline AkzDetTileGrid akz_det_tile_grid(const AkzDetWindow& W, int w, int h, int tw, int th)
{
    const int xa = W.x0 > 0 ? W.x0 - 1 : 0, xb = W.x1 < w ? W.x1 : w - 1;    // inclusive pixel range, grown by one, on the plane
    const int ya = W.y0 > 0 ? W.y0 - 1 : 0, yb = W.y1 < h ? W.y1 : h - 1;
    AkzDetTileGrid G;
    G.tx0 = xa / tw;
    G.ty0 = ya / th;
    G.ntx = xb / tw - G.tx0 + 1;
    G.nty = yb / th - G.ty0 + 1;
    return G;
}
