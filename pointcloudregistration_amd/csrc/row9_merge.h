// featnn_row9's per-(row, lane half) state and how two of them combine.  Host
// and device, no HIP headers: tests/cpp/row9_merge_check.cpp includes nothing
// else.
//
// The sweep keeps per row and lane half, over the steps (column-tile pairs) it
// has seen, the triple
//   b1 -- the smallest group minimum (a group: the lane's 32 values of a step),
//   b2 -- the second smallest group minimum,
//   i  -- the first step, in ascending order, whose minimum is b1
// as unsigned f32 patterns (the screen's values are >= 0 or +inf: the unsigned
// order is the float order, NaN patterns sort above +inf and never enter).
// The empty state is (+inf, +inf, 0): a step at +inf or above changes nothing.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCR_ROW9_HD __host__ __device__ __forceinline__
#else
#define PCR_ROW9_HD inline
#endif

namespace pcr {

constexpr unsigned kRow9Inf = 0x7f800000u;

PCR_ROW9_HD unsigned row9_min(unsigned a, unsigned b) { return a < b ? a : b; }
PCR_ROW9_HD unsigned row9_max(unsigned a, unsigned b) { return a > b ? a : b; }

// one more step, taken in ascending order: st's group minimum mn
PCR_ROW9_HD void row9_close(unsigned &b1, unsigned &b2, unsigned &i, unsigned mn, unsigned st) {
    // 2nd smallest of {b1, b2, mn}: their median (one v_med3_u32)
    const unsigned n2 = row9_max(row9_min(b1, b2), row9_min(row9_max(b1, b2), mn));
    i = mn < b1 ? st : i;
    b1 = row9_min(b1, mn);
    b2 = n2;
}

// the triple of the union of two disjoint sets of steps: (b1, b2) the two
// smallest of {b1, b2} u {o1, o2} (a multiset's two smallest do not depend on
// the order it was seen in), i the step of the smaller b1 and, on equal b1, the
// lower step -- what row9_close's strict < gives over all the steps ascending
PCR_ROW9_HD void row9_merge(unsigned &b1, unsigned &b2, unsigned &i, unsigned o1, unsigned o2, unsigned oi) {
    const unsigned n2 = row9_min(row9_max(b1, o1), row9_min(b2, o2));
    const bool take = o1 < b1 || (o1 == b1 && oi < i);
    i = take ? oi : i;
    b1 = row9_min(b1, o1);
    b2 = n2;
}

}  // namespace pcr
