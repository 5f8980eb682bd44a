// The determinant pass's window and launch arithmetic (cv_amd/csrc/akz_det_window.h) on the host alone, over every level of
// the plans (cv_amd/csrc/akz_plan.cpp) of the benchmarked 1080p frame and of the sizes tests/test_gpu_det_window.py runs.
// Prints one line per level and exits 1 on the first failed check (tests/test_det_window_plan.py builds it with
// -fsanitize=address,undefined).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../cv_amd/csrc/akz_common.h"
#include "../../cv_amd/csrc/akz_det_window.h"

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            printf("FAILED %s: %s (line %d)\n", what, #cond, __LINE__);                 \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

// scale_space_extrema.rs:50 and :96-104 for one pixel, written out once more (not through the plan's ranges)
static bool may_hold_a_candidate(const AkzLevel& L, int x, int y)
{
    if (x < 1 || x > L.w - 2 || y < 1 || y > L.h - 2) return false;
    const float ratio = ldexpf(1.0f, (int)L.octave);
    const float sigma_size = roundf(L.kp_size / ratio);
    const float smax = 10.0f * sqrtf(2.0f);
    volatile float b = smax * sigma_size;
    volatile float lx = (float)x - b, rx = (float)x + b, uy = (float)y - b, dy = (float)y + b;
    const float left_x = roundf(lx) - 1.0f, right_x = roundf(rx) + 1.0f, up_y = roundf(uy) - 1.0f, down_y = roundf(dy) + 1.0f;
    return !(left_x < 0.0f || right_x >= (float)L.w || up_y < 0.0f || down_y >= (float)L.h);
}

static int band_of(uint32_t sigma)
{
    return sigma == 2 ? det_stream_band(2) : sigma == 3 ? det_stream_band(3) : det_stream_band(4);
}

static void check_level(const char* what, const AkzLevel& L, int level)
{
    // ---- the window
    const AkzDetWindow whole = akz_det_window(L.w, L.h, L.cand_x_lo, L.cand_x_hi, L.cand_y_lo, L.cand_y_hi, true);
    CHECK(whole.x0 == 0 && whole.y0 == 0 && whole.x1 == L.w && whole.y1 == L.h && !whole.empty());
    const AkzDetWindow W = akz_det_window(L.w, L.h, L.cand_x_lo, L.cand_x_hi, L.cand_y_lo, L.cand_y_hi, false);
    long inside = 0;
    for (int y = 0; y < L.h; ++y)
        for (int x = 0; x < L.w; ++x) {
            const bool in_w = !W.empty() && x >= W.x0 && x < W.x1 && y >= W.y0 && y < W.y1;
            CHECK(may_hold_a_candidate(L, x, y) == in_w);          // the window is exactly the admissible pixels
            inside += in_w;
        }
    if (W.empty()) {
        CHECK(inside == 0);
        printf("level %d %dx%d sigma %u window empty\n", level, L.w, L.h, L.deriv_sigma);
        return;
    }
    CHECK(W.x0 >= 1 && W.y0 >= 1 && W.x1 <= L.w - 1 && W.y1 <= L.h - 1);
    CHECK(inside == (long)W.width() * W.height());
    // ---- streaming launches: bands x segments tile the window, once each
    const int band = band_of(L.deriv_sigma);
    const AkzDetWindow wins[2] = {W, whole};
    int shown_nb = 0, shown_nseg = 0, shown_rows = 0;
    for (const AkzDetWindow& V : wins)
        for (int n : {1, 2, 3, 5, 256})
            for (int target : {1, 64, 8192, 1 << 30}) {
                const AkzDetStreamGrid G = akz_det_stream_grid(V, band, target, n);
                CHECK(G.nb >= 1 && G.nseg >= 1 && G.seg_rows >= 1);
                CHECK((long)(G.nb - 1) * band < V.width() && (long)G.nb * band >= V.width());
                CHECK((long)(G.nseg - 1) * G.seg_rows < V.height() && (long)G.nseg * G.seg_rows >= V.height());
                CHECK(G.nseg <= (V.height() + 31) / 32);                                   // the 32-row floor
                CHECK(G.nseg == 1 || (long)G.nb * n * (G.nseg - 1) < target);               // no more waves than asked for
                std::vector<int> col(V.width(), 0), row(V.height(), 0);
                for (int b = 0; b < G.nb; ++b) {
                    const int bx = V.x0 + b * band, ux = bx + band < V.x1 ? bx + band : V.x1;
                    CHECK(bx < ux);
                    for (int x = bx; x < ux; ++x) col[x - V.x0]++;
                }
                for (int s = 0; s < G.nseg; ++s) {
                    const int ys = V.y0 + s * G.seg_rows, ye = ys + G.seg_rows < V.y1 ? ys + G.seg_rows : V.y1;
                    CHECK(ys < ye);
                    for (int y = ys; y < ye; ++y) row[y - V.y0]++;
                }
                for (int v : col) CHECK(v == 1);
                for (int v : row) CHECK(v == 1);
                if (&V == &wins[0] && n == 2 && target == 64) {
                    shown_nb = G.nb;
                    shown_nseg = G.nseg;
                    shown_rows = G.seg_rows;
                }
            }
    // ---- tile launches: whole tiles of the plane's own lattice that cover the window grown by one pixel
    for (const AkzDetWindow& V : wins)
        for (int th : {12, 32}) {
            const int tw = 64;
            const AkzDetTileGrid T = akz_det_tile_grid(V, L.w, L.h, tw, th);
            CHECK(T.tx0 >= 0 && T.ty0 >= 0 && T.ntx >= 1 && T.nty >= 1);
            CHECK((T.tx0 + T.ntx - 1) * tw < L.w && (T.ty0 + T.nty - 1) * th < L.h);        // every tile holds pixels of the plane
            for (int y = V.y0 - 1; y <= V.y1; ++y)
                for (int x = V.x0 - 1; x <= V.x1; ++x) {
                    if (x < 0 || x >= L.w || y < 0 || y >= L.h) continue;
                    CHECK(x / tw >= T.tx0 && x / tw < T.tx0 + T.ntx && y / th >= T.ty0 && y / th < T.ty0 + T.nty);
                }
            // and no row or column of tiles that holds none of those pixels
            CHECK((T.tx0 + 1) * tw > V.x0 - 1 && (T.tx0 + T.ntx - 1) * tw <= V.x1);
            CHECK((T.ty0 + 1) * th > V.y0 - 1 && (T.ty0 + T.nty - 1) * th <= V.y1);
            if (&V == &wins[1]) CHECK(T.tx0 == 0 && T.ty0 == 0 && T.ntx == (L.w + tw - 1) / tw && T.nty == (L.h + th - 1) / th);
        }
    printf("level %d %dx%d sigma %u window %d %d %d %d bands %d of %d segments %d rows %d\n", level, L.w, L.h, L.deriv_sigma, W.x0,
           W.x1, W.y0, W.y1, shown_nb, (L.w + band - 1) / band, shown_nseg, shown_rows);
}

int main()
{
    akz_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    // Akaze::default() (akaze/src/lib.rs:169-185): the fields the plan reads
    cfg.num_sublevels = 4;
    cfg.max_octave_evolution = 4;
    cfg.base_scale_offset = 1.6;
    cfg.derivative_factor = 1.5;
    const int sizes[][2] = {{1920, 1080}, {640, 400}, {333, 251}, {700, 300}, {240, 160}, {160, 120}, {64, 32}, {97, 83}, {4096, 41}};
    for (const auto& wh : sizes) {
        AkzPlan P;
        akz_build_plan(cfg, wh[0], wh[1], &P);
        char what[64];
        snprintf(what, sizeof(what), "%dx%d", wh[0], wh[1]);
        printf("plan %s: %d levels\n", what, (int)P.levels.size());
        for (size_t i = 0; i < P.levels.size(); ++i) check_level(what, P.levels[i], (int)i);
    }
    printf("all windows hold\n");
    return 0;
}
