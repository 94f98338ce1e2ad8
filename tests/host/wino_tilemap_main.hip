// Host check of the Winograd tile map (quber_amd/csrc/winograd_xf.h: Axis) - no GPU: every property is checked on the host instance of
// the functions the transform kernels call.  Built and run by tests/test_winograd_tilemap.py; exit status 0 = every check passed.
#include <cstdio>
#include <vector>

#include "../../quber_amd/csrc/winograd_xf.h"

using namespace quber::wxf;

static int g_bad = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (g_bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                     \
    } while (0)

static int ceil_div(int a, int b) { return (a + b - 1) / b; }

// the tile counts of an axis, written out from the definition (not from the header)
static int t_phase(int n, int d, int m) { return d * ceil_div(ceil_div(n, d), m); }
static int t_packed(int n, int d, int m) {
    int phases = 0;
    for (int p = 0; p < d; ++p)
        if (p < n) ++phases;                 // phase p has ceil((n - p) / d) > 0 pixels iff p < n
    return ceil_div(n + phases - 1, m);
}

static void check_axis(int n, int d, int m, bool pack) {
    const Axis a = make_axis(n, d, m, pack);
    const int tph = t_phase(n, d, m), tpk = t_packed(n, d, m);
    const int want = pack ? (tpk < tph ? tpk : tph) : tph;
    CHECK(a.T == want, "n %d d %d m %d pack %d: T %d, expected %d", n, d, m, (int)pack, a.T, want);
    CHECK(a.packed == (pack && tpk < tph), "n %d d %d m %d pack %d: packed %d", n, d, m, (int)pack, a.packed);
    std::vector<int> owners(n, 0), c(m + 2);
    for (int t = 0; t < a.T; ++t) {
        AxisPos s = axis_begin(a, t);
        for (int i = 0; i < m + 2; ++i) {
            c[i] = axis_coord(a, s);
            CHECK(c[i] >= -1 && c[i] < n, "n %d d %d m %d pack %d tile %d slot %d: coordinate %d", n, d, m, (int)pack, t, i, c[i]);
            s = axis_next(a, s);
        }
        for (int i = 1; i <= m; ++i) {
            if (c[i] < 0 || c[i] >= n) continue;
            ++owners[c[i]];
            const int p = c[i] % d, r = c[i] / d;
            const int prev = r > 0 ? d * (r - 1) + p : -1, next = d * (r + 1) + p < n ? d * (r + 1) + p : -1;
            CHECK(c[i - 1] == prev, "n %d d %d m %d pack %d tile %d: slot before pixel %d is %d, expected %d", n, d, m, (int)pack, t, c[i], c[i - 1], prev);
            CHECK(c[i + 1] == next, "n %d d %d m %d pack %d tile %d: slot after pixel %d is %d, expected %d", n, d, m, (int)pack, t, c[i], c[i + 1], next);
        }
    }
    for (int x = 0; x < n; ++x) CHECK(owners[x] == 1, "n %d d %d m %d pack %d: pixel %d is owned by %d tiles", n, d, m, (int)pack, x, owners[x]);
}

int main() {
    const int ms[3] = {2, 4, 6};
    for (int mi = 0; mi < 3; ++mi)
        for (int d = 1; d <= 20; ++d) {
            const int m = ms[mi];
            for (int n = 1; n <= 48; ++n) {
                check_axis(n, d, m, true);
                check_axis(n, d, m, false);
            }
            for (int H = 1; H <= 48; ++H)
                for (int W = 1; W <= 48; ++W) {
                    const int ty = t_packed(H, d, m) < t_phase(H, d, m) ? t_packed(H, d, m) : t_phase(H, d, m);
                    const int tx = t_packed(W, d, m) < t_phase(W, d, m) ? t_packed(W, d, m) : t_phase(W, d, m);
                    CHECK(wino_tiles_run(H, W, d, m, true) == (long)ty * tx, "H %d W %d d %d m %d: %ld tiles", H, W, d, m, wino_tiles_run(H, W, d, m, true));
                    CHECK(wino_tiles_run(H, W, d, m, false) == wino_tiles(H, W, d, m), "H %d W %d d %d m %d: per-phase count", H, W, d, m);
                    if (d == 1) CHECK(wino_tiles_run(H, W, d, m, true) == wino_tiles(H, W, d, m), "H %d W %d m %d: an undilated layer changed", H, W, m);
                }
        }
    // the counts the layers of the 640x480 and 1280x720 frames come out at, F(4x4): {H, W, d, rows per phase, rows packed, cols per phase, cols packed, now, best}
    const int table[8][9] = {{30, 40, 2, 8, 8, 10, 11, 80, 80},     {30, 40, 4, 8, 9, 12, 11, 96, 88},     {30, 40, 8, 8, 10, 16, 12, 128, 96},
                             {30, 40, 6, 12, 9, 12, 12, 144, 108},  {30, 40, 12, 12, 11, 12, 13, 144, 132}, {45, 80, 8, 16, 13, 24, 22, 384, 286},
                             {45, 80, 6, 12, 13, 24, 22, 288, 264}, {45, 80, 12, 12, 14, 24, 23, 288, 276}};
    for (const auto& r : table) {
        CHECK(axis_tiles_phase(r[0], r[2], 4) == r[3] && axis_tiles_packed(r[0], r[2], 4) == r[4], "rows of %dx%d d %d: %d -> %d", r[0], r[1], r[2],
              axis_tiles_phase(r[0], r[2], 4), axis_tiles_packed(r[0], r[2], 4));
        CHECK(axis_tiles_phase(r[1], r[2], 4) == r[5] && axis_tiles_packed(r[1], r[2], 4) == r[6], "columns of %dx%d d %d: %d -> %d", r[0], r[1], r[2],
              axis_tiles_phase(r[1], r[2], 4), axis_tiles_packed(r[1], r[2], 4));
        CHECK(wino_tiles(r[0], r[1], r[2], 4) == r[7], "%dx%d d %d: %ld tiles per phase", r[0], r[1], r[2], wino_tiles(r[0], r[1], r[2], 4));
        CHECK(wino_tiles_run(r[0], r[1], r[2], 4, true) == r[8], "%dx%d d %d: %ld tiles", r[0], r[1], r[2], wino_tiles_run(r[0], r[1], r[2], 4, true));
    }
    if (g_bad) {
        std::printf("%d checks failed\n", g_bad);
        return 1;
    }
    std::printf("tile map ok\n");
    return 0;
}
