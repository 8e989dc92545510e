// Index arithmetic of the dense r-cell grid ("GridDense", see grid.h): linear
// cell ids, the occupancy bitmap's word / bit split, rank + popcount lookups,
// the per-axis box gaps and the trimming of a row's x-cells.  Plain inline
// functions, __host__ __device__ under hipcc, so that the same code compiles
// for the CPU (tests/cpp/grid_dense_check.cpp runs it under sanitizers).
//
// Layout of one cloud: cells 1.005 r wide, coordinates relative to the cloud's
// minimum cell (ox, oy, oz), dimensions DX x DY x DZ, linear id
// (z DY + y) DX + x.  Points are sorted by id.  bits: one bit per cell (u32
// words, bit id & 31 of word id >> 5); rank[w]: occupied cells before word w;
// start[k], k = 0..occ: point offset of the k-th occupied cell in id order.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PCR_HD __host__ __device__ inline
#else
#define PCR_HD inline
#endif

namespace pcr {

// the build's counting sort keeps one u16 counter per cell in LDS
constexpr int kDenseCellCap = 72 * 1024;
constexpr int kDenseWordCap = kDenseCellCap / 32;
constexpr int kDenseMaxPoints = 32767;      // offsets and packed scan sums stay below 2^15
constexpr int kDenseMaxCoord = 1 << 30;     // |cell coordinate| of a dense cloud
constexpr double kDenseCellFactor = 1.005;  // cell width / r

// per-pair header (HBM): mode 1 = dense tables valid, 0 = hashed grid
struct GridHdr {
    int mode;
    int ox, oy, oz;
    int DX, DY, DZ;
    int occ;    // occupied cells
    int words;  // bitmap words (>= 1 even for an empty cloud)
    int pad[3];
};

PCR_HD size_t dense_table_bytes(int words, int occ) {
    return (size_t)words * 6 + (size_t)(occ + 1) * 2;
}

// cells of a DX x DY x DZ box, or -1 when they exceed the cap (no overflow)
PCR_HD int dense_cells(long long dx, long long dy, long long dz) {
    if (dx < 1 || dy < 1 || dz < 1 || dx > kDenseCellCap || dy > kDenseCellCap || dz > kDenseCellCap) return -1;
    const long long xy = dx * dy;
    if (xy > kDenseCellCap) return -1;
    const long long c = xy * dz;
    return c > kDenseCellCap ? -1 : (int)c;
}

PCR_HD int dense_id(int x, int y, int z, int DX, int DY) { return (z * DY + y) * DX + x; }

// One axis of the query box [u - w, u + w] (u = p / cell, w < 1: at most 3
// cells): first cell c0 relative to the origin o, cell count n, and per cell
// the squared gap from p to the cell's box, in f32 and never above the true
// squared distance along the axis to any point the build put in that cell.
//
// a0, a1 = floor(u -+ w) as the caller computed them (saturated casts are
// fine).  They are clamped to [o - 3, o + D + 2]: a clamp only ever moves a box
// that lies wholly outside [o, o + D), and it stays outside.  t = u - a0 is
// the query's position in cells from the box's first cell; cell i's box is
// [i, i + 1].  Errors: u against the true p / cell < 2^-21 cells and the
// build's floor(v / cell) < 2^-23 cells (|coordinates| < 2^30), t's f32
// rounding 2^-23: the gap is shrunk by 1e-5 cells, which covers them ten
// times over.  The caller drops cells whose summed gaps exceed thr (1 + 1e-6).
struct DenseAxis {
    int c0, n;
    float g[3];
};
PCR_HD DenseAxis dense_axis(double u, int a0, int a1, int o, int D, float cellf) {
    const int lo = o - 3, hi = o + D + 2;
    a0 = a0 < lo ? lo : (a0 > hi ? hi : a0);
    a1 = a1 < lo ? lo : (a1 > hi ? hi : a1);
    DenseAxis ax;
    ax.c0 = a0 - o;
    ax.n = a1 - a0 + 1;
    const float t = (float)(u - (double)a0);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i) {
        const float below = (float)i - t, above = t - (float)(i + 1);
        float gap = (below > above ? below : above) - 1e-5f;
        gap = gap > 0.f ? gap * cellf : 0.f;
        ax.g[i] = gap * gap;
    }
    return ax;
}

// The x-cells of a row that the gap test keeps: box cells [i0, i1] (i0 > i1:
// none).  The kept cells of a convex test are one interval; taking first and
// last kept makes that no assumption (anything between only adds candidates).
PCR_HD void dense_trim(const float gx[3], int nx, float gyz, float lim, int &i0, int &i1) {
    const bool k0 = nx > 0 && gx[0] + gyz <= lim;
    const bool k1 = nx > 1 && gx[1] + gyz <= lim;
    const bool k2 = nx > 2 && gx[2] + gyz <= lim;
    i0 = k0 ? 0 : (k1 ? 1 : (k2 ? 2 : 3));
    i1 = k2 ? 2 : (k1 ? 1 : (k0 ? 0 : -1));
}

// Occupied cells among ids [ida, idb] of one row (idb - ida <= 2, so at most
// two bitmap words): lo = occupied cells before ida, n = occupied cells in the
// interval.  ba / bb: bitmap words of ida / idb, rk: rank of ida's word.
PCR_HD void dense_range(uint32_t ba, uint32_t bb, int rk, int ida, int idb, int &lo, int &n) {
    const uint32_t from = ~0u << (ida & 31);           // bits >= ida's
    const uint32_t upto = (2u << (idb & 31)) - 1u;     // bits <= idb's (bit 31: all)
    lo = rk + __builtin_popcount(ba & ~from);
    n = (ida >> 5) == (idb >> 5) ? __builtin_popcount(ba & from & upto)
                                 : __builtin_popcount(ba & from) + __builtin_popcount(bb & upto);
}

// floor(v) as an int, saturated (the device's conversion saturates by itself)
PCR_HD int dense_floor_int(double v) {
    v = __builtin_floor(v);
#if !defined(__HIP_DEVICE_COMPILE__)
    v = v < -2147483000.0 ? -2147483000.0 : (v > 2147483000.0 ? 2147483000.0 : v);
    if (v != v) v = 0.0;
#endif
    return (int)v;
}

// one cloud's tables (in HBM, in LDS or on the host)
struct DenseTab {
    const uint32_t *bits;
    const uint16_t *rank;
    const uint16_t *start;
    int ox, oy, oz, DX, DY, DZ;
    double inv_cell;
    float cellf;
};

// The candidate ranges of the query p: emit(s, e) for each of the <= 3 x 3
// (y, z) rows of the box [p - 1.001 r, p + 1.001 r], with [s, e) the sorted
// points of the row's kept x-cells (s == e: nothing to examine; the caller
// skips those).  Together the ranges hold every point with d2 < thr.  A row
// outside the grid, beyond reach or without kept cells reads word 0 and
// start[0] -- always valid -- so all loads are unconditional and issue together.
template <typename F>
PCR_HD void dense_ranges(const DenseTab &g, double r, double thr, double px, double py, double pz, F &&emit) {
    const double ic = g.inv_cell, w = 1.001 * r * ic;
    const double ux = px * ic, uy = py * ic, uz = pz * ic;
    const DenseAxis ax = dense_axis(ux, dense_floor_int(ux - w), dense_floor_int(ux + w), g.ox, g.DX, g.cellf);
    const DenseAxis ay = dense_axis(uy, dense_floor_int(uy - w), dense_floor_int(uy + w), g.oy, g.DY, g.cellf);
    const DenseAxis az = dense_axis(uz, dense_floor_int(uz - w), dense_floor_int(uz + w), g.oz, g.DZ, g.cellf);
    const float lim32 = (float)(thr * (1.0 + 1e-6));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 9; ++c) {
        const int iz = c / 3, iy = c - 3 * iz;
        const int y = ay.c0 + iy, z = az.c0 + iz;
        const float gyz = ay.g[iy] + az.g[iz];
        int i0, i1;
        dense_trim(ax.g, ax.n, gyz, lim32, i0, i1);
        int xl = ax.c0 + i0, xh = ax.c0 + i1;
        xl = xl < 0 ? 0 : xl;
        xh = xh > g.DX - 1 ? g.DX - 1 : xh;
        const bool in = iy < ay.n && iz < az.n && (unsigned)y < (unsigned)g.DY && (unsigned)z < (unsigned)g.DZ &&
                        gyz <= lim32 && xl <= xh;
        const int base = in ? (z * g.DY + y) * g.DX : 0;
        const int ida = in ? base + xl : 0, idb = in ? base + xh : 0;
        const uint32_t ba = g.bits[ida >> 5], bb = g.bits[idb >> 5];
        const int rk = (int)g.rank[ida >> 5];
        int lo, n;
        dense_range(ba, bb, rk, ida, idb, lo, n);
        if (!in) { lo = 0; n = 0; }
        emit((int)g.start[lo], (int)g.start[lo + n]);
    }
}

}  // namespace pcr
