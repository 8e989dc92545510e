// Host-only check of the mutual feature path's route (csrc/featnn_route.h): which
// screens a call of pcr_feature_correspondences runs under each PCR_FEAT_* hook,
// the column slices of the 3-term list screens and the tile padding of the
// packed images.  Compiled with -fsanitize=address,undefined and run as a plain
// executable (tests/test_feat_route_cpu.py).
#include <cstdio>
#include <cstdlib>

#include "featnn_route.h"

static int fails = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                    \
        }                                                               \
    } while (0)

static const char *kHooks[] = {"PCR_FEAT_ONE", "PCR_FEAT_ROW9", "PCR_FEAT_THRESH", "PCR_FEAT_IMAGE"};

// the four hooks as given (null: unset)
static void hooks(const char *one, const char *row9, const char *thresh, const char *image) {
    const char *v[] = {one, row9, thresh, image};
    for (int i = 0; i < 4; ++i) {
        if (v[i]) setenv(kHooks[i], v[i], 1);
        else unsetenv(kHooks[i]);
    }
}

static bool is(const pcr::FeatRoute &r, bool one, bool use9, bool thresh, bool compact) {
    return r.one == one && r.use9 == use9 && r.thresh == thresh && r.compact == compact;
}

int main() {
    using pcr::feat_route;
    using pcr::feat_tiles;
    // the tile padding: F's 32-row tiles to whole 16s, G's to whole LDS groups of both row screens
    const int g = pcr::kRow8G > pcr::kRow9G ? pcr::kRow8G : pcr::kRow9G;
    CHECK(g % pcr::kRow8G == 0 && g % pcr::kRow9G == 0 && pcr::kRow9G1 <= pcr::kRow9G);
    const int counts[] = {1, 32, 33, 512, 513}, tiles[] = {1, 1, 2, 16, 17};
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) {
            const pcr::FeatTiles t = feat_tiles(counts[i], counts[j]);
            CHECK(t.ntn == (tiles[i] + 15) / 16 * 16);
            CHECK(t.ntm == (tiles[j] + g - 1) / g * g);
            CHECK(t.ntn * 32 >= counts[i] && t.ntm * 32 >= counts[j]);
            const pcr::FeatRoute r = feat_route(3, counts[i], counts[j], 32);  // the route carries the same padding
            CHECK(r.ntn == t.ntn && r.ntm == t.ntm);
        }
    CHECK(feat_tiles(512, 513).ntn == 16 && feat_tiles(513, 512).ntn == 32);
    if (g == 16) CHECK(feat_tiles(513, 512).ntm == 16 && feat_tiles(512, 513).ntm == 32);

    // column slices of the 3-term list screens: 256 / P, 1 to 8
    CHECK(pcr::list_slices(1) == 8 && pcr::list_slices(32) == 8 && pcr::list_slices(64) == 4);
    CHECK(pcr::list_slices(256) == 1 && pcr::list_slices(257) == 1 && pcr::list_slices(0) == 8);
    hooks(nullptr, nullptr, nullptr, nullptr);
    CHECK(feat_route(1, 600, 500, 32).fsl == 8 && feat_route(32, 600, 500, 32).fsl == 8);
    CHECK(feat_route(256, 600, 500, 32).fsl == 1 && feat_route(257, 600, 500, 32).fsl == 1);

    // the route table: S = ceil(D / 16) = 1 .. 4 under each hook setting
    const int dims[] = {1, 16, 17, 32, 33, 48, 49, 64};
    for (int D : dims) {
        const int S = (D + 15) / 16;
        const bool lo = S <= 2;  // the 1-term screens exist at S <= 2 only
        hooks(nullptr, nullptr, nullptr, nullptr);
        CHECK(feat_route(3, 513, 257, D).S == S);
        CHECK(is(feat_route(3, 513, 257, D), lo, lo, lo, lo));
        hooks("1", "1", "1", "compact");  // only a leading '0' / "full" switch anything
        CHECK(is(feat_route(3, 513, 257, D), lo, lo, lo, lo));
        hooks(nullptr, nullptr, nullptr, "full");
        CHECK(is(feat_route(3, 513, 257, D), lo, lo, lo, false));
        hooks(nullptr, nullptr, "0", nullptr);
        CHECK(is(feat_route(3, 513, 257, D), lo, lo, false, false));
        hooks(nullptr, nullptr, "0", "full");
        CHECK(is(feat_route(3, 513, 257, D), lo, lo, false, false));
        hooks(nullptr, "0", nullptr, nullptr);
        CHECK(is(feat_route(3, 513, 257, D), lo, false, false, false));
        hooks(nullptr, "0", "1", nullptr);  // no threshold route without featnn_row9
        CHECK(is(feat_route(3, 513, 257, D), lo, false, false, false));
        hooks("0", nullptr, nullptr, nullptr);
        CHECK(is(feat_route(3, 513, 257, D), false, false, false, false));
        hooks("0", "1", "1", nullptr);
        CHECK(is(feat_route(3, 513, 257, D), false, false, false, false));
    }
    // the hooks are read on every call
    hooks(nullptr, nullptr, nullptr, nullptr);
    CHECK(feat_route(3, 513, 257, 32).compact);
    hooks(nullptr, nullptr, nullptr, "full");
    CHECK(!feat_route(3, 513, 257, 32).compact && feat_route(3, 513, 257, 32).thresh);
    hooks(nullptr, nullptr, nullptr, nullptr);
    CHECK(feat_route(3, 513, 257, 32).compact);

    // featnn_row9 falls off when either pass has more column steps (two tiles
    // each) than the regroup's LDS prefix holds: the featnn_row8 1-term passes
    const int fit = pcr::kRegroupMaxSteps * 2 * 32;  // rows of the most tiles that fit
    CHECK(is(feat_route(1, fit, 100, 32), true, true, true, true));
    CHECK(is(feat_route(1, 100, fit, 32), true, true, true, true));
    CHECK(is(feat_route(1, fit + 1, 100, 32), true, false, false, false));
    CHECK(is(feat_route(1, 100, fit + 1, 32), true, false, false, false));
    CHECK(is(feat_route(1, fit + 1, 100, 48), false, false, false, false));
    if (fails) return 1;
    std::printf("ok: feature route\n");
    return 0;
}
