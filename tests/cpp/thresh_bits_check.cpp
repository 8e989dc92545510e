// Host check of thresh_bits_up (csrc/featnn_thresh.h), the threshold pattern
// of featnn_thresh9: never below the f64 threshold, monotone in the pattern
// order, +inf and the largest finite value.  Plain C++, no HIP.
#include "featnn_thresh.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

static float as_float(uint32_t b) {
    float f;
    memcpy(&f, &b, sizeof(f));
    return f;
}

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL line %d: %s\n", __LINE__, #c);            \
            ++fails;                                               \
        }                                                          \
    } while (0)

// one threshold: the pattern is a non-negative f32's (or +inf's), its value is
// not below t, and the pattern below it is
static void check_one(double t) {
    const uint32_t b = pcr::thresh_bits_up(t);
    CHECK(b <= 0x7f800000u);
    if (std::isnan(t)) {
        CHECK(b == 0x7f800000u);
        return;
    }
    if (t <= 0.0) {
        CHECK(b == 0u);
        return;
    }
    CHECK((double)as_float(b) >= t);
    CHECK(b > 0u ? (double)as_float(b - 1u) < t : true);
}

int main() {
    const float fmax = std::numeric_limits<float>::max();
    const double inf = std::numeric_limits<double>::infinity();
    // the ends
    CHECK(pcr::thresh_bits_up(inf) == 0x7f800000u);
    CHECK(pcr::thresh_bits_up(std::nan("")) == 0x7f800000u);
    CHECK(pcr::thresh_bits_up((double)fmax) == 0x7f7fffffu);
    CHECK(pcr::thresh_bits_up(std::nextafter((double)fmax, inf)) == 0x7f800000u);
    CHECK(pcr::thresh_bits_up(std::nextafter((double)fmax, 0.0)) == 0x7f7fffffu);
    CHECK(pcr::thresh_bits_up(1e300) == 0x7f800000u);
    CHECK(pcr::thresh_bits_up(0.0) == 0u);
    CHECK(pcr::thresh_bits_up(-1.0) == 0u);
    CHECK(pcr::thresh_bits_up(-inf) == 0u);
    CHECK(pcr::thresh_bits_up(1e-300) == 1u);  // below the smallest subnormal: its pattern
    CHECK(pcr::thresh_bits_up(1.0) == 0x3f800000u);
    CHECK(pcr::thresh_bits_up(std::nextafter(1.0, 2.0)) == 0x3f800001u);
    CHECK(pcr::thresh_bits_up(std::nextafter(1.0, 0.0)) == 0x3f800000u);
    // every f32 neighbourhood of a pattern sample: the value itself, just above, just below
    std::mt19937_64 rng(9);
    for (int i = 0; i < 200000; ++i) {
        const uint32_t b = (uint32_t)(rng() % 0x7f800000u);
        const double v = (double)as_float(b);
        check_one(v);
        check_one(std::nextafter(v, inf));
        check_one(std::nextafter(v, -inf));
        const double w = (double)as_float(b + 1u);  // b + 1 may be +inf
        if (std::isfinite(w)) check_one(v + (w - v) * ((rng() >> 11) * 0x1p-53));
    }
    // monotone: t1 <= t2 gives pattern(t1) <= pattern(t2), over magnitudes from
    // subnormals to past the largest finite value
    double prev_t = 0.0;
    uint32_t prev_b = 0u;
    for (int e = -160; e <= 130; ++e)
        for (int k = 0; k < 64; ++k) {
            const double t = std::ldexp(1.0 + k / 64.0 + 1e-9 * k, e);
            const uint32_t b = pcr::thresh_bits_up(t);
            CHECK(t >= prev_t && b >= prev_b);
            check_one(t);
            prev_t = t;
            prev_b = b;
        }
    // the screen's use: an f32 value v <= t (as reals) has pattern(v) <= thresh_bits_up(t)
    for (int i = 0; i < 200000; ++i) {
        const uint32_t bv = (uint32_t)(rng() % 0x7f800000u);
        const double v = (double)as_float(bv);
        const double bnd = std::ldexp((double)(rng() >> 11) * 0x1p-53, (int)(rng() % 60) - 30);
        const uint32_t bt = pcr::thresh_bits_up(v + bnd);
        CHECK(bv <= bt);
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok: thresh_bits_up\n");
    return 0;
}
