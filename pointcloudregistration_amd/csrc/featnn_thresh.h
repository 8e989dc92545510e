// The threshold of featnn_thresh9 as an f32 bit pattern.  Host and device, no
// HIP needed: a plain host compiler builds it (tests/cpp/thresh_bits_check.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PCR_THRESH_HD __host__ __device__
#else
#define PCR_THRESH_HD
#endif

namespace pcr {

// The smallest non-negative f32 bit pattern whose value is >= t: the screen
// compares value patterns as unsigned integers (the float order of
// non-negative values), so `pattern <= thresh_bits_up(t)` holds for every f32
// value v >= 0 with v <= t.  t above the largest finite f32, +inf or NaN gives
// the pattern of +inf (0x7f800000); t <= 0 gives 0.
PCR_THRESH_HD inline uint32_t thresh_bits_up(double t) {
    if (!(t == t)) return 0x7f800000u;
    if (!(t > 0.0)) return 0u;
    const float f = (float)t;  // round to nearest: at most one ulp below t
    uint32_t b;
    memcpy(&b, &f, sizeof(b));
    // f < t: the next pattern up (from the largest finite value: +inf's)
    return (double)f < t ? b + 1u : b;
}

}  // namespace pcr
