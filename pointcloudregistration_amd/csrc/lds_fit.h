// The fit rule of a hashed grid's LDS copy: one float4 per point (x, y, z, index
// bits) and u16 slot starts, the layout RANSAC, ICP and the batch Chamfer query
// stage.  Host-only arithmetic (no HIP header), so tests/cpp can check it.
#pragma once
#include <cstddef>

namespace pcr {

// bytes of the copy of one cloud's grid -- `stride` float4 points, then S + 1
// u16 slot starts, rounded up to 16 -- or 0 if it does not fit: a u16 start
// holds an offset <= 65535, and the copy must lie within `budget` bytes
inline size_t lds4_fit_bytes(int stride, int S, size_t budget) {
    if (stride < 0 || S < 0 || stride > 65535 || S + 1 > 65536) return 0;
    const size_t b = (size_t)stride * 16 + (size_t)(S + 1) * 2;
    const size_t a = (b + 15) & ~size_t(15);
    return a <= budget ? a : 0;
}

}  // namespace pcr
