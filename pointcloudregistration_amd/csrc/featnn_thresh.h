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

// featnn_thresh9's flush of one row's block-local hits: the block counted
// `local` hits of the row (the first min(local, K) of them in its K local
// slots) and `base` is what its one atomicAdd(rec.x, local) returned, the hits
// other blocks had added before.  Returns how many local slots i = 0 .. n - 1
// to copy to the row's global slots base + i: those that land below K, none
// once base >= K.  The row's total is the sum of every block's `local`
// whatever was copied, so it exceeds K exactly when the row has more than K
// counted hits (featnn_exact_cand reads min(total, K + 1): overflow).
PCR_THRESH_HD inline int thresh_flush_count(uint32_t base, uint32_t local, int K) {
    if (base >= (uint32_t)K) return 0;
    const uint32_t room = (uint32_t)K - base;
    return (int)(local < room ? local : room);
}

}  // namespace pcr
