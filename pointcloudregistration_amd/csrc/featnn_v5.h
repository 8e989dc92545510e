// The f16 x3 split feature screen (D <= 64), shared by its units: the operand
// layout, the certification bounds, the kernels' argument structs (their layout
// is the kernels' ABI), the per-cloud view of the packed workspace (V5Side,
// V5Buf) and the host entry points that cross units (featnn.hip has the map of
// the units; featnn_route.h the route's constants and the tile padding).
#pragma once
#include "featnn_common.h"
#include "featnn_route.h"

namespace pcr {

struct Split5 {
    int T;   // target exponent of max|x|
    int cs;  // norm slot scale c = 2^cs
};
inline Split5 split5_params(int D) {
    int L = 0;
    while ((1 << L) < D) ++L;
    Split5 s;
    s.T = (30 - L) / 2 < 12 ? (30 - L) / 2 : 12;
    s.cs = 2 * s.T + L - 15;
    return s;
}

namespace {

// ---------------------------------------------------------------------------
// v5: f16 x3 split screen on v_mfma_f32_32x32x16_f16 (32 cycles per 16-deep
// k-step vs 64 per 2-deep step of the f32 MFMA: 7 instead of 17 x 4 cycles
// per 32x32 tile at D = 32).
//   scale: per pair x = f * 2^e (exact), e chosen so max|x| in [2^(T-1), 2^T)
//          (T = 12 at D <= 64) -> every x fits f16 with room for the products.
//   split: x = hi + lo + e_x, hi = f16(x), lo = f16(x - hi): |e_x| <= 2^-22|x|
//          + 2^-14 (the 2^-14 covers f16 subnormals even if flushed).
//   operands (k order, each D-segment padded to S = ceil(D/16) chunks of 16):
//          A_i = [-2hi | -2hi | -2lo | nx_hi nx_mid nx_lo | c c c | 0 | 2^15]
//          B_j = [  hi |   lo |   hi | c c c | ny_hi ny_mid ny_lo | 2^15 | 0]
//          (norm chunk k = 6 / k = 7: the bias slots.  The G image (role 1)
//          stores 2^15 at k = 6, the F image (role 0) at k = 7; featnn_row8
//          patches the row operand's opposite slot in registers -- 1.0 at k = 6
//          for pass 1 (F rows), k = 7 for pass 2 (G rows), 64 for the 1-term
//          screens -- see kRowBias / kRowBias1)
//          nx = |x|^2 / c split into three f16 parts, c = 2^cs fits f16.
//          Executed: NX = 3S + 1 k-chunks (one MFMA each).  Stored: NM = 2S + 1
//          -- A as [-2hi | -2lo | norms], B as [hi | lo | norms]; the MFMA of
//          chunk c reads A chunk amap(c) and B chunk bmap(c) (the repeated
//          segment is the same registers), so the packed operands, the
//          L2 -> LDS stream and the B-fragment LDS reads are 5/7 of the
//          executed k at D = 32.
//   C = 0 -> d'_ij = |x_i|^2 + |y_j|^2 - 2 x_i.y_j (scaled by 2^2e) with
//   |d' - d'_exact| <= err(q, G) (bound5 below).  Products are exact in f32;
//   the accumulation is charged 2 (Kt + 2) u (|x| + |y|)^2 whatever the
//   MFMA's internal summation order.  Rows/columns whose top-2 gap is not
//   above 2 err are rescanned exactly in f64 (featnn_rescan2).
// Packed layout: [pair][tile][stored chunk][lane] of 8 halves (lane l: row/col l&31,
// k = 16 chunk + 8 (l>>5) + j); padded tiles are valid encodings of +inf
// rows, so no loop has a tail.  Grid: 1-D, XCD-aware: all row blocks of a
// pair run on one XCD, whose L2 then holds that pair's B image (1.8 MB).
// Compact image (round 11): featnn_row9 with the threshold route reads the hi
// segment only, so for it the packs store S chunks per tile, [-2hi] / [hi] (the
// same bits as the full image's first S chunks), and the tile stride is S
// chunks.  V5Buf::ich / RowArgs5::ich carry the stored chunks per tile; every
// reader of the lo or norm chunks (the dual screen, featnn_row8, featnn_row7)
// requires ich = NM.
// ---------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// executed k-chunk c -> stored A / B chunk (see the operand layout above)
__host__ __device__ constexpr int amap(int c, int S) { return c < S ? c : (c < 3 * S ? c - S : 2 * S); }
__host__ __device__ constexpr int bmap(int c, int S) { return c < 2 * S ? c : (c < 3 * S ? c - 2 * S : 2 * S); }

__device__ __forceinline__ float pair_scale5(unsigned mbits, int T) {
    const int E = (int)((mbits >> 23) & 0xff);
    if (E == 0 || E == 255) return 1.0f;
    const int e = min(max(T + 126 - E, -126), 127);
    return __int_as_float((e + 127) << 23);
}

// Where a pack launch takes its pairs and their scale (see feat_sample):
// normal: grid.y = P, the pair's sample max with kSpecMargin binades of
// headroom, rows outside the split's range flag the pair; repair: grid.y =
// kRepairR, the flagged pairs by rank, the full max from feat_maxabs.
struct PackCtl {
    const unsigned *smax;  // [P] sample max bits (normal)
    const unsigned *mxp;   // [P][2][Z] full partial maxima (repair)
    int Z, P, repair;
    int *bad;              // [P] flags
    unsigned *sc;          // [P] the scale used (f32 bits), for the rescans
};

// both clouds in one launch: blockIdx.z = role (0: F as rows, 1: G as columns)
struct PackIO {
    const float *X[2];
    const int32_t *n[2];
    int Nmax[2], ntiles[2];
    f16x8 *Xp[2];
    float *nrm[2];
    unsigned *nmax[2];
    unsigned *emax[2];  // per pair: max over the cloud's rows of |x s - f16(x s)| (the 1-term screen's bound)
    float *rex[2];      // per row: its |x s - f16(x s)| (rounded up; featnn_regroup9's bound)
    float *ct[2];       // per row: f32(|x s|^2), -1 on padding rows (feat_colterms adds the bias)
};

// |x - f16(x)| of one row (x already scaled), rounded up: e^2 summed exactly
// enough in f64 (each term exact), the sqrt's rounding covered by the factor
__device__ __forceinline__ float split_err_norm(double e2) {
    return (float)(__builtin_sqrt(e2) * (1.0 + 1e-6));
}

// certification threshold for a top-2 gap in scaled units (see header)
__device__ __forceinline__ double bound5(double q, double G, int Kt, int D) {
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double qg = q + G;
    const double err = 2.0 * (Kt + 2) * u * qg * qg + 6.0 * 2.384185791015625e-07 * q * G +
                       1.220703125e-04 * __builtin_sqrt((double)D) * qg +
                       1.1641532182693481e-10 * (q * q + G * G) + 4.0;
    return 2.0 * err;
}

struct DualArgs5 {
    const f16x8 *Ap, *Bp;
    const float *fnr, *gnr;  // scaled norms
    const unsigned *fmax, *gmax;
    const int32_t *n_src, *n_tgt;
    int P, Nmax, Mmax, ntn, ntm, nrb, D, ctbits;
    int32_t *nn12;
    int *list12, *count12;
    float *cp1, *cp2;
    int *cpi;
};

// B: pass 1 1.0 (row k = 6) x 2^15 (G's column image, k = 6); pass 2 (featnn_row8
// <.., false>, the J rows of G against F's image) 1.0 (row k = 7) x 2^15 (F's
// image, k = 7).  dual7 pairs F's image with G's: 0 x 2^15 at both slots.
constexpr double kRowBias = 32768.0;
constexpr double kRowBias1 = 2097152.0;  // 2^21: the 1-term screens' (featnn_row8<.., kOne>, see there)

// certification threshold of the 1-term screen (scaled units), 2 x the error
// bound; ex, E: the row's and the columns' max |x - f16(x)|, subnormal term added
__device__ __forceinline__ double bound1(double q, double ex, double G, double E, int Kt) {
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double qg = q + G;
    const double err = 2.0 * (Kt + 2) * u * qg * qg + 2.0 * (ex * G + (q + ex) * E) +
                       1.1641532182693481e-10 * (q * q + G * G) + 4.0;
    return 2.0 * err;
}
__device__ __forceinline__ double sub_term(int D) { return 6.103515625e-05 * __builtin_sqrt((double)D); }  // 2^-14 sqrt(D)

// featnn_row9's certificate bound, 2 x the error of one screened value in its
// row's frame (row_tail's kCT branch has the terms): q, ex the row's norm and
// |x - f16(x)|, G, E the columns' maxima (ex, E with sub_term), B the pair's
// bias, Kt the executed k
__device__ __forceinline__ double bound_ct(double q, double ex, double G, double E, double B, int Kt) {
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double err = 2.0 * (Kt + 2) * u * ((B + G * G) + 2.0 * (q + ex) * (G + E)) +
                       2.0 * (ex * G + (q + ex) * E) + u * (2.0 * B + G * G) * (1.0 + 0x1p-20) + 4.0;
    return 2.0 * err;
}

__device__ __forceinline__ unsigned umin2(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned umax2(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned fbits(float v) { return __float_as_uint(v); }

// a lane's 16 column terms of column tile ct (register r: column
// 8 (r / 4) + 4 h + (r % 4)), from 32 floats per tile
__device__ __forceinline__ f32x16 colterms(const float *tile32, int h) {
    f32x16 c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 v = *reinterpret_cast<const float4 *>(tile32 + 8 * j + 4 * h);
        c[4 * j] = v.x; c[4 * j + 1] = v.y; c[4 * j + 2] = v.z; c[4 * j + 3] = v.w;
    }
    return c;
}

// featnn_thresh9 / featnn_exact_cand: candidate slots per listed row.  On the
// C4 benchmark a failing row has 2 columns within its threshold on average and
// 4 at most; a row with more goes to the exact rescan
constexpr int kThreshK = 8;

struct MutArgs {
    const int32_t *nn12, *n_src, *n_tgt;
    int Nmax, Mmax, mutual, ransac_n, Kt, D, ntm;
    int *used;        // [P][Mmax + 1]: 1 = j in J (2: listed for the rescan), 3: listed, not in J
    int *pos;         // [P][Mmax + 1] scan scratch
    int *jlist, *nj;  // [P][Mmax], [P]: the rows of pass 2, ascending
    const double *v12;
    const float *e12;
    const float4 *wq;   // (w1, w2, e2, the bias in w1 / w2)
    const unsigned *fmax;
    const int32_t *nns; // the screened argmins J is built from (never overwritten by the rescans)
    const float *F, *G; // the f32 clouds and the scale the packs used: the exact distance of a
    const unsigned *mx; // candidate whose screened value is too coarse for its column's gap
    int *flag;        // [P][Nmax + 1]: mutual 0 / 1, 2 = decided by the exact column
    int *list21, *cnt21;
    const int32_t *nn21x;
    int32_t *corres, *n_corres;
};

}  // namespace

struct RescanArgs5 {
    const float *F, *G;
    const int32_t *n_src, *n_tgt;
    int Nmax, Mmax, D;
    const int *list12, *list21, *cnt12, *cnt21;
    int32_t *nn12, *nn21;
    // candidate slices (gridDim.z = S): the first `cap` listed rows of a pair and
    // direction are scanned by S blocks over disjoint candidate ranges, each
    // writing its lexicographic (d, j) minimum to slot (p, dir, e, s), merged by
    // featnn_rescan_merge; rows past `cap` are scanned whole by slice 0
    int cap;
    double *sd;
    int *sj;
    // mutual path (feature_corres_v5): the exact distance of a rescanned F row,
    // in the screen's scaled units (x s^2, s = pair_scale5(mx[p], T): a power of
    // two, exact), and its error 0; null elsewhere
    double *v12;
    float *e12;
    const unsigned *mx;
    int T;
};

// The row screens' arguments (the mutual path, featnn.hip).  Every field has a
// default, and the screen of a pass is filled in one place (screen_args there);
// the other kernels take views of it that re-point three (list, count) pairs:
//                      rlist / rcount         list / count            llist / lcount
//   featnn_row7/8/9    pass 2: the rows J     rows left uncertified   -
//   featnn_regroup9    -                      -                       -
//   featnn_finish9     -                      -                       its failing rows
//   featnn_row8 list,  the screen's list      rows left uncertified   -
//    featnn_slicemerge                        (to the exact rescan)
//   featnn_thresh9,    the screen's list      -                       rows left unsettled
//    featnn_exact_cand                                                (to the exact rescan)
// A null list drops the rows (pass 2: featmut_resolve sends an undecided column to
// the exact column rescan).  With thresh = 1 the finish's llist is the screen's
// own list: it appends to what the sweep listed.
struct RowArgs5 {
    const f16x8 *Ap = nullptr;  // row operand (register-resident): [P][ntr][ich][64]
    const f16x8 *Bp = nullptr;  // column operand (LDS-streamed): [P][ntc][ich][64]
    int ich = 0;                // stored chunks per tile of both images: NM, or S (compact: the hi segment only)
    const float *rnr = nullptr;      // scaled row norms, [P][ntr * 32] by original row index
    const unsigned *cmax = nullptr;  // per pair max scaled column norm (f32 bits)
    const int32_t *n_rows = nullptr, *n_cols = nullptr;
    const int *rlist = nullptr, *rcount = nullptr;  // pass 2: rows rlist[p][0 .. rcount[p]) (original indices)
    int P = 0, Rmax = 0, Cmax = 0, ntr = 0, ntc = 0, nrb = 0, D = 0, ctbits = 0;
    int32_t *nn = nullptr;      // pass 1: argmin (screened), value, its error, uncertified rows
    double *v = nullptr;
    float *e = nullptr;
    int *list = nullptr, *count = nullptr;
    float4 *wq = nullptr;       // pass 2: (top-2 values, the screen's error bound, -) by original row index
    // pass 2: the gathered rows built in registers from the f32 cloud (one
    // 128-byte row per lane instead of ten 16-byte pieces in ten lines of the
    // packed image), with the scale the packs used and the image's role
    const float *Xr = nullptr;
    const unsigned *sc = nullptr;
    int role = 0, cs = 0;
    const unsigned *cemax = nullptr;  // featnn_row8<.., kOne>: per pair max |y - f16(y)| of the column image
    int32_t *nns = nullptr;     // pass 1: a copy of the screened argmin for featmut_jbuild (nullable)
    int fbdiag = 0;             // 1 / 2: count the listed rows in g_featnn_fallback_rows[0 / 1]
    int rbmajor = 0;            // featnn_row8: blocks ordered row block first (short lists, below)
    const float *rre = nullptr; // the rows' |x - f16(x)| from the pack, [P][ntr * 32]
    // featnn_row9's buckets (rows by winning step): [P][steps] counts and
    // [P][steps][bcap] entries (row, B1, B2, lane half of the winning group)
    int *bcnt = nullptr, bcap = 0;
    uint4 *blist = nullptr;
    uint4 *rec = nullptr;       // featnn_regroup9 -> featnn_finish9, by row: (column, B1, B2, skip)
    int *llist = nullptr, *lcount = nullptr;  // featnn_finish9: where its failing rows go (nullable)
    // featnn_row8 list mode over column slices (csl > 1: short lists at small
    // batches): slice sl's partial (B1, B2, column) per listed row position k,
    // [P][csl][Rmax], merged by featnn_slicemerge
    int csl = 0;
    uint4 *part = nullptr;
    // featnn_row9: the column cloud's and the row cloud's per-row terms
    // f32(|.|^2 + B) ([P][ntc * 32], [P][ntr * 32]) and B
    const float *cct = nullptr, *rct = nullptr;
    const float *cbias = nullptr;  // [P] B
    // the threshold route (featnn_thresh.hip): thresh = 1 makes featnn_finish9
    // re-mark the rows it lists as the sweep marks its own, rec = (0, B1,
    // 0xffffffff, 1) -- featnn_thresh9's candidate counter, the row's smallest
    // value, its first column (pass 1) and the skip flag; cand: [P][Rmax]
    // [kThreshK] candidate columns; used: featmut's column flags (pass 2);
    // Xc: the column cloud (f32); fbctr: g_featnn_fallback_rows; dbg:
    // featnn_exact_cand keeps statistics
    int thresh = 0;
    int *cand = nullptr, *used = nullptr;
    const float *Xc = nullptr;
    unsigned long long *fbctr = nullptr;
    int dbg = 0;
};

namespace {

// The 1-term row operand of one row (lane half h) built from its f32 values:
// its -2 f16(x) chunks exactly as the packs store them (row_frags) -- one
// 128-byte line per row where the packed image spreads it over S lines: the
// regroup gathers rows.  The sweep, the regroup and the threshold sweep all
// take it from here or from the image (row_operand below: the same bits), so
// their MFMA chains agree bit for bit.  (No norm chunk:
// featnn_row9 takes the columns' |y|^2 + B as the MFMA's accumulator input and
// leaves |x|^2 out.)
template <int S>
__device__ __forceinline__ void row_operand1(const RowArgs5 &a, int p, int row, bool valid, int h,
                                             f16x8 (&A)[S]) {
    const float sc = __uint_as_float(a.sc[p]);
    float x[16 * S];
    const float *xr = a.Xr + ((size_t)p * a.Rmax + row) * a.D;
    if (valid && a.D == 16 * S && ((uintptr_t)xr & 15) == 0) {
#pragma unroll
        for (int q = 0; q < 4 * S; ++q) {
            const float4 v = reinterpret_cast<const float4 *>(xr)[q];
            x[4 * q] = v.x * sc; x[4 * q + 1] = v.y * sc; x[4 * q + 2] = v.z * sc; x[4 * q + 3] = v.w * sc;
        }
    } else if (valid) {
#pragma unroll
        for (int q = 0; q < 16 * S; ++q) x[q] = q < a.D ? xr[q] * sc : 0.0f;
    } else {
#pragma unroll
        for (int q = 0; q < 16 * S; ++q) x[q] = 0.0f;
    }
    // both lane halves' elements at compile-time indices, then the half's pick
    // (an index by h is a select chain over the row)
    auto seg = [&](int k) {
        const _Float16 hi = (_Float16)x[k];
        return k < a.D ? (a.role == 0 ? (_Float16)(-2.0f * (float)hi) : hi) : (_Float16)0.0f;
    };
#pragma unroll
    for (int c = 0; c < S; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const _Float16 v0 = seg(16 * c + j), v1 = seg(16 * c + 8 + j);
            A[c][j] = h ? v1 : v0;
        }
}

// The same operand from the row cloud's own packed image (a.Ap: its first S
// chunks per tile are these bits by the packs' definition, whichever layout):
// S 16-byte fragments per lane, no conversion.  PCR_ROW_IMG selects it per
// kernel at compile time -- bit 0 featnn_row9 pass 1, bit 1 featnn_row9 pass 2,
// bit 2 featnn_regroup9, bit 3 featnn_thresh9.  Measured per slot (DESIGN.md
// Round 11): pass 1's sweep gains 0.02 ms per 256-pair step and keeps it; pass
// 2's gain is inside three run-to-run ranges at 256 pairs; the regroups and the
// threshold sweeps, which gather their rows, lose at 256 pairs.
#ifndef PCR_ROW_IMG
#define PCR_ROW_IMG 1
#endif
template <int S>
__device__ __forceinline__ void row_operand_img(const RowArgs5 &a, int p, int row, int h, f16x8 (&A)[S]) {
    const f16x8 *q = a.Ap + ((size_t)p * a.ntr + (row >> 5)) * a.ich * 64 + (row & 31) + 32 * h;  // row < 32 ntr
#pragma unroll
    for (int c = 0; c < S; ++c) A[c] = q[(size_t)c * 64];
}
template <int S, int kBit>
__device__ __forceinline__ void row_operand(const RowArgs5 &a, int p, int row, bool valid, int h, f16x8 (&A)[S]) {
    if constexpr ((PCR_ROW_IMG >> kBit) & 1) row_operand_img<S>(a, p, row, h, A);
    else row_operand1<S>(a, p, row, valid, h, A);
}

// the row's certificate bound (bound_ct) from a screen's arguments
__device__ __forceinline__ double row_bound_ct(const RowArgs5 &a, int p, int row, float rexv, int Kt) {
    const double sub = sub_term(a.D);
    return bound_ct((double)a.rnr[(size_t)p * a.ntr * 32 + row], (double)rexv + sub,
                    (double)__uint_as_float(a.cmax[p]), (double)__uint_as_float(a.cemax[p]) + sub,
                    (double)a.cbias[p], Kt);
}

}  // namespace

// what the pack produces for one cloud, and what addresses it
struct V5Side {
    const float *X;    // the f32 cloud, [P][Nmax][D]
    const int32_t *n;  // [P] counts (null: Nmax each)
    int Nmax, nt;      // rows per pair; 32-row tiles per pair as padded (feat_tiles)
    f16x8 *Xp;         // packed image, [P][nt][ich][64]
    float *nr;         // per row scaled norm, [P][nt * 32]
    unsigned *nmax;    // [P] max scaled norm (f32 bits)
    unsigned *emax;    // [P] max |x - f16(x)| (the 1-term screens' bound)
    float *re;         // per row |x - f16(x)| (scaled, rounded up)
    float *ct;         // per row f32(|x|^2 + B) (featnn_row9's column terms)
};

// packed operands, norms and per-pair maxima of both clouds (shared by the
// dual screen and the mutual path): side 0 = F (the sources), 1 = G (the targets)
struct V5Buf {
    int P, D;
    int S, NM, NX, W, nrb, ctbits;  // S chunks per D-segment, NM stored, NX executed
    int ich;  // chunks per tile the images hold: NM, or S when compact (v5_prepare)
    Split5 sp;
    V5Side side[2];
    unsigned *mx;                        // [P] the scale the packs used (f32 bits)
    int *cnt12, *cnt21, *list12, *list21;
    int *fbc12, *fbc21, *fbl12, *fbl21;  // the rows a 1-term screen left for the 3-term one
    float *cbias;                        // [P] the column terms' B (feat_colterms)
};

// featnn_pack.hip; compact: the images hold the hi segment only (S chunks per
// tile) -- for featnn_row9 with the threshold route, which reads nothing else
int v5_prepare(const float *F, const float *G, int P, int Nmax, int Mmax, int D, const int32_t *n_src,
               const int32_t *n_tgt, hipStream_t s, V5Buf &v, bool compact = false);
// featnn_dual.hip
int feature_match_v5(const float *F, const float *G, int P, int Nmax, int Mmax, int D, const int32_t *n_src,
                     const int32_t *n_tgt, int32_t *nn12, int32_t *nn21, hipStream_t s);
// featnn_rescan.hip
RescanArgs5 rescan_args(const float *F, const float *G, const int32_t *n_src, const int32_t *n_tgt, int Nmax,
                        int Mmax, int D);
int run_rescan(RescanArgs5 &ra, int P, int D, hipStream_t s);
// featnn_row.hip (instantiated there for every kIdx / kOne); each sets its own r.nrb
template <bool kIdx> int launch_row7(const RowArgs5 &r, int S, hipStream_t s);  // S = 3, 4
template <bool kIdx, bool kOne> int launch_row8(const RowArgs5 &r, int S, hipStream_t s);
template <bool kIdx> int launch_row9(const RowArgs5 &r, int S, hipStream_t s);
template <bool kIdx> int launch_regroup9(const RowArgs5 &r, int S, hipStream_t s);
int fallback_counter(unsigned long long **ctr);  // g_featnn_fallback_rows's device address
// featnn_thresh.hip: featnn_thresh9 + featnn_exact_cand over the rows r.rlist lists
template <bool kIdx> int launch_thresh9(const RowArgs5 &r, int S, hipStream_t s);

}  // namespace pcr
