// Batched point-to-plane ICP with a robust kernel (Open3D 0.13 RegistrationICP
// with TransformationEstimationPointToPlane(kernel), restated).
// Contract: tests/icp_plane_ref.py (the loop is oracle_icp's icp_core with the
// Umeyama step replaced by the weighted point-to-plane update).
//
// MI355X design, as icp.hip: the whole loop of a pair runs inside one launch on
// one 1024-thread workgroup -- or on G workgroups meeting at a per-pair barrier
// (coop.h) when the batch has fewer pairs than the chip has CUs -- with the
// pair's target hash grid in LDS.  Per iteration ONE sweep over 64-position
// chunks of the spatial order: a point is transformed by the last update,
// queried in the grid (radius-limited 1-NN), and on a hit the winner's normal is
// gathered (12 B from L2) and the 27 terms of the normal equations
//     A_ab += q((w J_a) J_b), a <= b (21),   g_a += q((w J_a) r) (6)
// are formed: J = (s x n, n), r = (s - t) . n, w = weight(r).  q truncates to a
// multiple of a per-pair quantum 2^-k (below), so every f64 addition is exact
// and the sums do not depend on the split over lanes, waves and workgroups.
// That freedom is also what keeps the registers down: a lane does not carry 27
// accumulators across the grid walk; after each chunk the wave's 27 terms go
// through the reduce-scatter butterfly (exact_sums.h) and every lane adds the
// one value it ends up with to a single accumulator -- 31 shuffles per 64 grid
// walks.  The 6x6 LDL^T solve, the rotation and T <- U*T run redundantly on
// thread 0 of every workgroup from the same totals.
//
// The quantum.  u = 2^-53.  bt = max_j |t_j|_inf over the targets, N = max
// |n_j|_inf over the normals whose three components are finite (others
// contribute nothing), both by order-free max reductions in a pre-pass.
//  * An inlier lies within sqrt(thr) <= d (1 + 2^-23) of its target, so
//    |s|_inf <= bt + 2d =: Bs with room to spare.
//  * |c_a| = |s_b n_c - s_c n_b| <= 2 Bs N, |n_a| <= N, and by Cauchy-Schwarz
//    |r| <= |e|_2 |n|_2 < sqrt(3) d N (1 + 2^-23) < 2 d N <= Bs N: every |J_a|
//    and |r| is at most Jm = N max(2 Bs, 1), up to the roundings of the three
//    or four operations behind it (a factor below 1 + 8u, Jm's own included).
//  * w <= W, the kernel's supremum weight (1; 1/k for GM, whose computed
//    weight can exceed the computed 1/k by a few u at most).
//  * A term fl(fl(w J_a) X) is below W Jm^2 (1 + 32u) in magnitude; with
//    W < 2^eW and Jm < 2^eJ from frexp it is below 2^e_max, e_max = eW + 2 eJ + 1.
//  * n <= 2^e_n terms and k = 52 - e_n - e_max: scaling by 2^k is exact, trunc
//    gives an integer below 2^(e_max + k), and any partial sum of at most n of
//    them is an integer below 2^52.  Integers below 2^53 add exactly.
// The kernel scales w J_a by 2^k once and truncates (w J_a 2^k) X: the scaling is
// exact, so this rounds to the same value as ((w J_a) X) 2^k; the sums are kept
// in quanta and scaled by 2^-k once after the reduction.
#include "pcr_internal.h"
#include "coop.h"
#include "exact_sums.h"
#include "geom.h"
#include "grid.h"
#include "wave.h"
#include <cmath>

namespace pcr {
namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kQ = 27;  // exact sums: A_ab, a <= b (21), g_a (6)

struct PArgs {
    const float *src, *tgt, *nrm;
    const int32_t *n_src, *n_tgt;
    int Nmax, Mmax;
    const double *init;  // P x 16
    double d, thr, rel_fit, rel_rmse;
    int max_iter;
    int kernel;          // PCR_KERNEL_*
    double kk, W;        // the kernel's scale and supremum weight
    GridBatch grid;
    double *P3;          // P x Nmax x 3 working copy by position in the order
    const float *srcp;   // (P, Nmax, 3) the source points in that order
    const int32_t *order;  // (P, Nmax) spatial order of the source points
    double *T_out, *fit_out;
    int32_t *stats;
    int32_t *corr_tgt;   // optional (P, Nmax)
    int G;               // workgroups per pair
    XPart<kQ> *part;     // (P, 2, G) when G > 1
    unsigned *bar;       // when G > 1: per pair 4 words, the pair barrier
};

// thread 0's 6x6 solve (ldlt_solve)
struct LdlScratch {
    double A[6][6], L[6][6], D[6], y[6], x[6];
};

struct PShared {  // LDS header; the grid copy (if any) follows
    double ws[kWaves][kQ];
    unsigned long long wacc[kWaves];
    int wcnt[kWaves];
    double tot[kQ];
    double mx[2][kWaves];  // the pre-pass's maxima per wave: targets, normals
    double sk, isk;        // 2^k, 2^-k: the quantum of the exact sums
    unsigned long long acc;
    int cnt;
    double T[16];     // the running transformation (init, then U * T per iteration)
    double U[12];     // this iteration's update
    int nred;         // reductions done (parity of the HBM partial slots)
    int chunk[2];     // next 64-position chunk of this workgroup's range, by sweep parity
    LdlScratch ls;    // thread 0's solve
};

__device__ __forceinline__ bool finite_d(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }

// ---- deterministic sine / cosine: + - * / and trunc only (the twin of
// det_sincos in tests/icp_plane_ref.py; the polynomials are det_cos's of
// fpfh.hip: nested Taylor forms to x^20) ---------------------------------------
__device__ inline double cos_poly(double x) {
    const double x2 = x * x;
    double s = 1.0;
    for (int k = 10; k >= 1; --k) s = 1.0 - x2 / (double)((2 * k - 1) * (2 * k)) * s;
    return s;
}
__device__ inline double sin_poly(double x) {
    const double x2 = x * x;
    double s = 1.0;
    for (int k = 10; k >= 1; --k) s = 1.0 - x2 / (double)((2 * k) * (2 * k + 1)) * s;
    return x * s;
}
// a = |x|; j = trunc(a 2/pi + 0.5) quarter turns are taken off in two steps
// (PIO2_HI holds 33 bits of pi/2: j PIO2_HI is exact for j < 2^20), leaving
// |y| <= pi/4; the quadrant j mod 4 picks the polynomial and the signs
__device__ inline void det_sincos(double x, double &s, double &c) {
    if (!finite_d(x)) {
        s = __builtin_nan("");
        c = s;
        return;
    }
    const double a = __builtin_fabs(x);
    const double j = __builtin_trunc(a * 6.36619772367581382433e-01 + 0.5);
    const double y = (a - j * 1.57079632673412561417e+00) - j * 6.07710050650619224932e-11;
    const double q = j - 4.0 * __builtin_trunc(j / 4.0);
    const double sp = sin_poly(y), cp = cos_poly(y);
    if (q == 0.0) { s = sp; c = cp; }
    else if (q == 1.0) { s = cp; c = -sp; }
    else if (q == 2.0) { s = -sp; c = -cp; }
    else { s = -cp; c = sp; }
    if (x < 0.0) s = -s;
}

__device__ __forceinline__ double weight_of(int kern, double k, double r) {
    const double a = __builtin_fabs(r);
    switch (kern) {
    case PCR_KERNEL_HUBER: return a <= k ? 1.0 : k / a;
    case PCR_KERNEL_CAUCHY: { const double q = r / k; return 1.0 / (1.0 + q * q); }
    case PCR_KERNEL_GM: { const double q = k + r * r; return k / (q * q); }
    case PCR_KERNEL_TUKEY: { const double q = r / k, t = 1.0 - q * q; return a <= k ? t * t : 0.0; }
    default: return 1.0;
    }
}

// x of A x = -g by LDL^T without pivoting (tot: 21 sums of A's upper triangle
// row by row, then g, in quanta; isk scales them back, exactly), in the
// reference's loop order; false when a pivot is not > 0 or not finite, or x is
// not finite.  One thread; the matrices live in LDS (ls), indexed in rolled
// loops, so the solve takes no registers from the sweep.
__device__ __noinline__ bool ldlt_solve(const double *tot, double isk, LdlScratch &ls) {
    int q = 0;
#pragma unroll 1
    for (int a = 0; a < 6; ++a)
#pragma unroll 1
        for (int b = a; b < 6; ++b) {
            const double t = tot[q] * isk;
            ls.A[a][b] = t;
            ls.A[b][a] = t;
            ++q;
        }
#pragma unroll 1
    for (int j = 0; j < 6; ++j) {
        double dj = ls.A[j][j];
#pragma unroll 1
        for (int k = 0; k < j; ++k) dj = dj - (ls.L[j][k] * ls.D[k]) * ls.L[j][k];
        if (!(dj > 0.0) || !finite_d(dj)) return false;
        ls.D[j] = dj;
#pragma unroll 1
        for (int i = j + 1; i < 6; ++i) {
            double v = ls.A[i][j];
#pragma unroll 1
            for (int k = 0; k < j; ++k) v = v - (ls.L[i][k] * ls.D[k]) * ls.L[j][k];
            ls.L[i][j] = v / dj;
        }
    }
#pragma unroll 1
    for (int i = 0; i < 6; ++i) {
        double v = -(tot[21 + i] * isk);
#pragma unroll 1
        for (int k = 0; k < i; ++k) v = v - ls.L[i][k] * ls.y[k];
        ls.y[i] = v;
    }
#pragma unroll 1
    for (int i = 5; i >= 0; --i) {
        double v = ls.y[i] / ls.D[i];
#pragma unroll 1
        for (int k = i + 1; k < 6; ++k) v = v - ls.L[k][i] * ls.x[k];
        ls.x[i] = v;
    }
    bool ok = true;
#pragma unroll 1
    for (int i = 0; i < 6; ++i) ok = ok && finite_d(ls.x[i]);
    return ok;
}

// U = [Rz(gamma) Ry(beta) Rx(alpha) | (tx, ty, tz)], the entries as written in
// the reference's update_from_x
__device__ inline void update_from_x(const double x[6], double U[12]) {
    double sa, ca, sb, cb, sg, cg;
    det_sincos(x[0], sa, ca);
    det_sincos(x[1], sb, cb);
    det_sincos(x[2], sg, cg);
    U[0] = cg * cb;
    U[1] = (cg * sb) * sa - sg * ca;
    U[2] = (cg * sb) * ca + sg * sa;
    U[3] = x[3];
    U[4] = sg * cb;
    U[5] = (sg * sb) * sa + cg * ca;
    U[6] = (sg * sb) * ca - cg * sa;
    U[7] = x[4];
    U[8] = -sb;
    U[9] = cb * sa;
    U[10] = cb * ca;
    U[11] = x[5];
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void icp_plane_kernel(PArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    PShared &sh = *reinterpret_cast<PShared *>(dsm);
    const int G = a.G, p = blockIdx.x / G, g = blockIdx.x - p * G;
    const int n = count_of(a.n_src, p, a.Nmax);
    const int m = count_of(a.n_tgt, p, a.Mmax);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float *S = a.src + (size_t)p * a.Nmax * 3;
    const float *NR = a.nrm + (size_t)p * a.Mmax * 3;
    const int32_t *ord = a.order ? a.order + (size_t)p * a.Nmax : nullptr;
    double *P3 = a.P3 + (size_t)p * a.Nmax * 3;
    const bool wt = G > 1;  // working copy stores write-through (put3)
    int32_t *CT = a.corr_tgt ? a.corr_tgt + (size_t)p * a.Nmax : nullptr;
    if (tid < 16) sh.T[tid] = a.init[(size_t)p * 16 + tid];
    if (tid == 0) { sh.nred = 0; sh.chunk[0] = 0; sh.chunk[1] = 0; }
    __syncthreads();
    const bool valid = a.d > 0.0 && n > 0 && m > 0;
    bool ident = true;
    for (int k = 0; k < 16; ++k) ident = ident && (sh.T[k] == ((k % 5 == 0) ? 1.0 : 0.0));
    const int stride = G * kThreads, base = g * kThreads + tid;
    // the workgroup's share of the sweep order: 64-position chunks [c_lo, c_hi),
    // the same in every sweep, so a position's working copy is only ever touched
    // by one workgroup
    const int nch = (n + 63) >> 6;
    const int c_lo = (int)((long long)nch * g / G), c_hi = (int)((long long)nch * (g + 1) / G);
    if (valid) {  // the quantum (every workgroup computes the same values)
        const float *Tg = a.tgt + (size_t)p * a.Mmax * 3;
        double bt = 0.0, bn = 0.0;
        for (int j = tid; j < m; j += kThreads) {
            const double t0 = __builtin_fabs((double)Tg[3 * j]), t1 = __builtin_fabs((double)Tg[3 * j + 1]),
                         t2 = __builtin_fabs((double)Tg[3 * j + 2]);
            if (t0 > bt) bt = t0;
            if (t1 > bt) bt = t1;
            if (t2 > bt) bt = t2;
            const double n0 = __builtin_fabs((double)NR[3 * j]), n1 = __builtin_fabs((double)NR[3 * j + 1]),
                         n2 = __builtin_fabs((double)NR[3 * j + 2]);
            if (finite_d(n0) && finite_d(n1) && finite_d(n2)) {
                if (n0 > bn) bn = n0;
                if (n1 > bn) bn = n1;
                if (n2 > bn) bn = n2;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double ot = __shfl_xor(bt, o, 64), on = __shfl_xor(bn, o, 64);
            if (ot > bt) bt = ot;
            if (on > bn) bn = on;
        }
        if (lane == 0) { sh.mx[0][wid] = bt; sh.mx[1][wid] = bn; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kWaves; ++w) {
                if (sh.mx[0][w] > bt) bt = sh.mx[0][w];
                if (sh.mx[1][w] > bn) bn = sh.mx[1][w];
            }
            const double Bs = bt + 2.0 * a.d, two = 2.0 * Bs;
            const double Jm = bn * (two > 1.0 ? two : 1.0);
            int eJ = 0, eW = 0;
            (void)frexp(Jm, &eJ);
            (void)frexp(a.W, &eW);
            const int emax = eW + 2 * eJ + 1;
            int en = 0;
            while ((1LL << en) < (long long)(n > 1 ? n : 1)) ++en;
            const int k = min(200, max(-200, 52 - en - emax));
            sh.sk = ldexp(1.0, k);
            sh.isk = ldexp(1.0, -k);
        }
        // working copy = init applied to the f32 input (Open3D's Transform)
        double T0[12];
        for (int q = 0; q < 12; ++q) T0[q] = sh.T[q];
        const float *Sp = (a.srcp && ord) ? a.srcp + (size_t)p * a.Nmax * 3 : nullptr;
        for (int k = 64 * c_lo + tid; k < min(n, 64 * c_hi); k += kThreads) {
            const float *q = Sp ? Sp + 3 * k : S + 3 * (ord ? ord[k] : k);
            double x = (double)q[0], y = (double)q[1], z = (double)q[2];
            if (!ident) {
                double ox, oy, oz;
                xform12(T0, x, y, z, ox, oy, oz);
                x = ox; y = oy; z = oz;
            }
            put3(P3 + 3 * k, x, y, z, wt);
        }
    }
    GridP4 gl{};
    GridView gg{};
    if (valid) {
        if constexpr (kLds) gl = grid_to_lds4(a.grid, p, m, dsm + ((sizeof(PShared) + 15) & ~size_t(15)));
        else gg = a.grid.view(p);
    }
    __syncthreads();
    const double scale = fx_scale(a.thr);
    double fit = 0.0, rmse = 0.0;
    int count = 0;
    int nsweep = 0;  // sweeps done: parity of the chunk counters
    // One sweep: the correspondences of the current points (moved by sh.U first
    // when with_u), their count / error sum and the 27 sums of the next update.
    auto evaluate = [&](bool with_u) {
        unsigned long long acc = 0;
        int cnt = 0;
        double tacc = 0.0;  // this lane's value of the butterfly, summed over the wave's chunks
        int *ctr = &sh.chunk[nsweep & 1];
        for (;;) {
            int c = 0;
            if (lane == 0) c = atomicAdd(ctr, 1);
            c = __shfl(c, 0, 64) + c_lo;
            if (c >= c_hi) break;
            const int k = (c << 6) + lane;
            double v[kQ];
#pragma unroll
            for (int q = 0; q < kQ; ++q) v[q] = 0.0;
            bool contrib = false;
            if (k < n) {
                double x = P3[3 * k], y = P3[3 * k + 1], z = P3[3 * k + 2];
                if (with_u) {  // U from LDS per chunk (volatile: not held across the query)
                    const volatile double *Uv = sh.U;
                    double U[12];
#pragma unroll
                    for (int q = 0; q < 12; ++q) U[q] = Uv[q];
                    double ox, oy, oz;
                    xform12(U, x, y, z, ox, oy, oz);
                    put3(P3 + 3 * k, ox, oy, oz, wt);
                    x = ox; y = oy; z = oz;
                }
                double d2;
                int q, sl;
                float qx = 0.f, qy = 0.f, qz = 0.f, qw;
                if constexpr (kLds) {
                    q = grid_query_exact<GridP4, true, 2, false>(gl, a.d, a.thr, x, y, z, d2, &sl);
                    if (q >= 0) gl.load(sl, qx, qy, qz, qw);
                } else {
                    q = grid_query_exact<GridView, true, 2, false>(gg, a.d, a.thr, x, y, z, d2, &sl);
                    if (q >= 0) gg.load(sl, qx, qy, qz, qw);
                }
                if (CT) CT[ord ? ord[k] : k] = q;
                if (q >= 0) {  // 0 <= q < m: an index the grid build stored
                    ++cnt;
                    acc += (unsigned long long)(d2 * scale);
                    const double n0 = (double)NR[3 * q], n1 = (double)NR[3 * q + 1], n2 = (double)NR[3 * q + 2];
                    const double e0 = x - (double)qx, e1 = y - (double)qy, e2 = z - (double)qz;
                    const double r = (e0 * n0 + e1 * n1) + e2 * n2;
                    const double J[6] = {y * n2 - z * n1, z * n0 - x * n2, x * n1 - y * n0, n0, n1, n2};
                    const double w = weight_of(a.kernel, a.kk, r);
                    if (finite_d(n0) && finite_d(n1) && finite_d(n2) && finite_d(w)) {
                        contrib = true;
                        const volatile double *skv = &sh.sk;
                        const double sk = skv[0];
                        int i = 0;
#pragma unroll
                        for (int aa = 0; aa < 6; ++aa) {
                            const double wj = (w * J[aa]) * sk;
#pragma unroll
                            for (int bb = aa; bb < 6; ++bb) v[i++] = __builtin_trunc(wj * J[bb]);
                            v[21 + aa] = __builtin_trunc(wj * r);
                        }
                    }
                }
            }
            if (__ballot(contrib) != 0ull) tacc = tacc + wave_scatter_sum<kQ>(v);
        }
        wave_park_lane<kQ>(sh, tacc);
        pair_reduce<kQ>(a.part, a.bar, sh, p, g, G, cnt, acc, [](int) {});
        // every workgroup has left this sweep (pair_reduce's barrier): re-arm its
        // counter for the sweep after next
        if (tid == 0) sh.chunk[nsweep & 1] = 0;
        ++nsweep;
        count = sh.cnt;
        if (count > 0) {
            fit = (double)count / (double)n;
            rmse = __builtin_sqrt(((double)sh.acc / scale) / (double)count);
        } else {
            fit = 0.0;
            rmse = 0.0;
        }
    };
    int it = 0;
    if (valid) {
        evaluate(false);
        for (; it < a.max_iter;) {
            if (count == 0) break;
            if (tid == 0) {
                double U[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
                if (ldlt_solve(sh.tot, sh.isk, sh.ls)) update_from_x(sh.ls.x, U);
                double Tn[16];
                for (int r = 0; r < 4; ++r)
                    for (int c = 0; c < 4; ++c) {
                        const double u0 = r < 3 ? U[4 * r + 0] : 0.0, u1 = r < 3 ? U[4 * r + 1] : 0.0,
                                     u2 = r < 3 ? U[4 * r + 2] : 0.0, u3 = r < 3 ? U[4 * r + 3] : 1.0;
                        Tn[4 * r + c] =
                            ((u0 * sh.T[c] + u1 * sh.T[4 + c]) + u2 * sh.T[8 + c]) + u3 * sh.T[12 + c];
                    }
                for (int k = 0; k < 16; ++k) sh.T[k] = Tn[k];
                for (int k = 0; k < 12; ++k) sh.U[k] = U[k];
            }
            __syncthreads();
            const double pf = fit, pr = rmse;
            evaluate(true);
            ++it;
            if (__builtin_fabs(pf - fit) < a.rel_fit && __builtin_fabs(pr - rmse) < a.rel_rmse) break;
        }
    }
    if (CT) {  // the last sweep wrote CT[0, n) when valid
        for (int i = valid ? n + base : base; i < a.Nmax; i += stride) CT[i] = -1;
    }
    if (g == 0 && tid == 0) {
        for (int k = 0; k < 16; ++k) a.T_out[(size_t)p * 16 + k] = sh.T[k];
        a.fit_out[2 * p] = valid ? fit : 0.0;
        a.fit_out[2 * p + 1] = valid ? rmse : 0.0;
        a.stats[2 * p] = it;
        a.stats[2 * p + 1] = valid ? count : 0;
    }
}

const void *plane_fn(bool lds) {
    return lds ? (const void *)icp_plane_kernel<true> : (const void *)icp_plane_kernel<false>;
}

int icp_plane_impl(const float *src, const float *tgt, const float *nrm, int P, int Nmax, int Mmax,
                   const int32_t *n_src, const int32_t *n_tgt, const double *init, const pcr_icp_params *prm,
                   const pcr_icp_plane_params *pl, double *T_out, double *fit_out, int32_t *stats,
                   int32_t *corr_tgt, hipStream_t s) {
    PArgs a;
    a.src = src; a.tgt = tgt; a.nrm = nrm; a.n_src = n_src; a.n_tgt = n_tgt; a.Nmax = Nmax; a.Mmax = Mmax;
    a.init = init;
    a.d = prm->max_correspondence_distance;
    a.thr = radius_thr(a.d);
    a.rel_fit = prm->relative_fitness;
    a.rel_rmse = prm->relative_rmse;
    a.max_iter = prm->max_iteration;
    a.kernel = pl->kernel;
    a.kk = pl->kernel == PCR_KERNEL_L2 ? 1.0 : pl->k;
    a.W = pl->kernel == PCR_KERNEL_GM ? 1.0 / pl->k : 1.0;
    a.order = nullptr;
    a.srcp = nullptr;
    a.grid = GridBatch{};
    if (a.d > 0.0) {
        int rc = build_grids(tgt, n_tgt, P, Mmax, a.d, s, kWsIcpGrid, a.grid);
        if (rc != PCR_OK) return rc;
        if (Nmax > 0) {  // any spatial order serves: it only groups a wave's queries
            rc = spatial_order(src, n_src, P, Nmax, a.grid.cell, s, kWsIcpOrder, &a.order, &a.srcp,
                               kWsIcpPerm);
            if (rc != PCR_OK) return rc;
        }
    } else {
        a.grid.S = 1;
        a.grid.cell = 1.0;
    }
    a.T_out = T_out; a.fit_out = fit_out; a.stats = stats; a.corr_tgt = corr_tgt;
    const size_t hdr = (sizeof(PShared) + 15) & ~size_t(15);
    const size_t gbytes = (a.d > 0.0 && Mmax > 0) ? grid_lds4_bytes(Mmax, a.grid.S, 160 * 1024 - hdr) : 0;
    const bool lds = gbytes > 0;  // else: the grid stays in global memory
    const size_t sm = lds ? hdr + gbytes : hdr;
    const void *fn = plane_fn(lds);
    PCR_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kThreads, sm) != hipSuccess) {
        (void)hipGetLastError();
        per_cu = 0;
    }
    // at most 4, as ICP: an iteration meets at the pair barrier per reduction,
    // and past 4 workgroups their cost outgrows the split sweep
    a.G = coop_groups(P, per_cu, 4);
    const size_t nm = (size_t)(Nmax > 0 ? Nmax : 1);
    // the slots are icp.hip's (workspace.h): the same contents, another ABI call
    a.P3 = (double *)workspace(kWsIcpPoints, sizeof(double) * 3 * (size_t)P * nm + 64);
    PCR_REQUIRE(a.P3, PCR_ERR_NOMEM, "icp_plane: %s", pcr_last_error());
    a.part = nullptr;
    if (a.G > 1) {
        WsLayout l;
        l.take(a.part, 2 * (size_t)a.G * (size_t)P);
        PCR_REQUIRE(workspace_bind(kWsIcpPartials_RadiusNnGrid, l, kWsSlack), PCR_ERR_NOMEM, "icp_plane: %s",
                    pcr_last_error());
    }
    a.bar = nullptr;
    bool *dirty = nullptr;
    if (a.G > 1) {
        // barriers in a slot of their own, zeroed when allocated or after a call
        // that failed between its launches (icp.hip has the reasoning): a
        // completed launch leaves the arrivals zero
        size_t nb = 16384;
        while (nb < 4 * (size_t)P) nb <<= 1;
        bool fresh = false;
        a.bar = (unsigned *)workspace(kWsIcpBarrier, sizeof(unsigned) * nb, &fresh);
        PCR_REQUIRE(a.bar, PCR_ERR_NOMEM, "icp_plane: %s", pcr_last_error());
        dirty = workspace_dirty(kWsIcpBarrier);
        PCR_REQUIRE(dirty, PCR_ERR_ARG, "icp_plane: no workspace slot");
        if (fresh || *dirty) PCR_HIP_CHECK(hipMemsetAsync(a.bar, 0, sizeof(unsigned) * nb, s));
        *dirty = true;  // until the launch below went in
    }
    void *args[] = {&a};
    PCR_HIP_CHECK(coop_launch(fn, P, a.G, kThreads, args, sm, s));
    PCR_LAUNCH_CHECK();
    if (dirty) *dirty = false;
    return PCR_OK;
}

}  // namespace
}  // namespace pcr

extern "C" int pcr_icp_plane_batch(const float *src_xyz, const float *tgt_xyz, const float *tgt_normals,
                                   int32_t P, int32_t Nmax, int32_t Mmax, const int32_t *n_src,
                                   const int32_t *n_tgt, const double *init, const pcr_icp_params *params,
                                   const pcr_icp_plane_params *plane, double *T, double *fitness_rmse,
                                   int32_t *stats, int32_t *corr_tgt, pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(P >= 0 && Nmax >= 0 && Mmax >= 0, PCR_ERR_ARG, "icp_plane: negative size");
    if (P == 0) return PCR_OK;
    PCR_REQUIRE(src_xyz && tgt_xyz && tgt_normals && init && params && plane && T && fitness_rmse && stats,
                PCR_ERR_ARG, "icp_plane: null pointer");
    PCR_REQUIRE(plane->kernel >= PCR_KERNEL_L2 && plane->kernel <= PCR_KERNEL_TUKEY, PCR_ERR_ARG,
                "icp_plane: unknown kernel %d", (int)plane->kernel);
    PCR_REQUIRE(plane->kernel == PCR_KERNEL_L2 || plane->k > 0.0, PCR_ERR_ARG,
                "icp_plane: the kernel's k must be > 0 (k=%g)", plane->k);
    return pcr::icp_plane_impl(src_xyz, tgt_xyz, tgt_normals, P, Nmax, Mmax, n_src, n_tgt, init, params, plane,
                               T, fitness_rmse, stats, corr_tgt, pcr::as_stream(stream));
}
