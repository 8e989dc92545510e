// Coherent Point Drift (Myronenko & Song 2010): the matrix-free E-step and the
// rigid / rigid + scale / affine loop.  Reference use: DataPreparation/CPD.py:26-73
// (probreg.cpd.RigidCPD / AffineCPD / NonRigidCPD on cupy, f32).
//
// probreg forms the (M,N) posterior three times per iteration; only Pt1 (N),
// P1 (M) and PX (M,3) are used.  Here two sweeps give them with no (M,N) array:
//  * column sweep: one lane per target, the transformed sources staged through
//    LDS as SoA chunks (transformed once per workgroup, while staging); writes
//    inv_n = 1 / (den_n + c) and Pt1_n;
//  * row sweep: one lane per source, targets and inv staged through LDS; five
//    accumulators per lane, the moments sum v, sum v (y^ - x) and sum v d of
//    v = k inv: they are of the size of the residual, not of the clouds, so the
//    M-step's sigma2 = (trXPX - 2 tr(A^T R) + tr G) / (3 Np), a difference of
//    sums hundreds of times its size once sigma2 is small, keeps its digits;
//    P1 = sum v and PX = P1 y^ - sum v (y^ - x).
// Both grids are (tiles, slices, pairs).  A small batch of large clouds splits
// the staged axis over workgroups.  Every sum has one association whatever the
// split and the batch size: terms are added in f32 in groups of four
// consecutive staged points, ((k0 + k1) + (k2 + k3)), the groups of one
// 512-point chunk are added in f64 in order from 0, and the chunk sums are added
// in f64 in chunk order.  A split launch writes the chunk sums to scratch and a
// second kernel adds them in that order; there are no float atomics, so a call
// returns the same bytes every time and a pair's result does not depend on what
// else is in the batch.
// Exponential: k = exp2(d * f), f = -log2(e) / (2 sigma2) held as an f32 pair
// (hi, lo) so that the factor's rounding does not scale with the argument:
// arg = fmaf(d, hi, d * lo), one v_exp_f32 per pair evaluation.
// Per pair evaluation the row sweep issues 3 sub, 5 mul/add (d), 2 (arg), 1 exp,
// 1 mul (k inv), 4.75 (group sums: 3 add + 4 mul + 12 fma per 4): 15.75 plain
// f32 issues + 1 exp + 2.5 f64 (5 cvt + 5 f64 add per 4, half rate); the column
// sweep 3 + 5 + 2, 0.75 (3 add per 4): 10.75 plain + 1 exp + 0.5 f64.
#include "pcr_internal.h"
#include "geom.h"
#include "wave.h"
#include <float.h>

namespace pcr {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 512;   // staged points per LDS stage (pcr_api.h documents the sums' chunk)

// per-pair f64 state record (device memory; nothing goes through the host)
enum : int {
    kStT = 0,        // 12: [B | t] row-major 3x4, B = s R or the affine matrix
    kStSigma2 = 12,
    kStScale = 13,
    kStQ = 14,
    kStNp = 15,
    kStIters = 16,
    kStDone = 17,
    kStStatus = 18,
    kStC = 19,       // (2 pi sigma2)^1.5 w / (1 - w) M / N
    kStFhi = 20,     // -log2(e) / (2 sigma2) as an f32 pair
    kStFlo = 21,
    kStWords = 32,
};

__device__ inline void state_derive(double *st, double w, int M, int N) {
    const double s2 = st[kStSigma2];
    const double tp = 6.283185307179586476925 * s2;
    st[kStC] = (tp * __builtin_sqrt(tp)) * (w / (1.0 - w)) * ((double)M / (double)N);
    const double f = -1.442695040888963407360 / (2.0 * s2);
    const float hi = (float)f;
    st[kStFhi] = (double)hi;
    st[kStFlo] = (double)(float)(f - (double)hi);
}

__device__ __forceinline__ int pair_count(const int32_t *n, int p, int nmax) {
    const int v = n ? n[p] : nmax;
    return v < 0 ? 0 : (v > nmax ? nmax : v);
}

__device__ __forceinline__ float kern(float qx, float qy, float qz, float cx, float cy, float cz,
                                      float fhi, float flo) {
    const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    return __builtin_amdgcn_exp2f(__builtin_fmaf(d, fhi, d * flo));
}

struct EArgs {
    const float *src, *tgt;          // (P,Mmax,3), (P,Nmax,3)
    const int32_t *n_src, *n_tgt;    // device, or null
    const double *state;             // (P,kStWords)
    float *inv, *pt1, *p1, *px;      // (P,Nmax) x2, (P,Mmax), (P,Mmax,3)
    double *pden;                    // split: [chunk][P][Nmax]
    double *prow;                    // split: [chunk][P][Mmax][5]
    double *rowm;                    // (P,Mmax,5): the sources' row moments (row_finish)
    double *colw;                    // (P,Nmax): Pt1 of the targets no source reaches, else 0
    int P, Mmax, Nmax;
    int use_T;                       // 0: the sources are already transformed
    int slice_chunks, split;         // chunks per blockIdx.y slice; 1 if partials are written
};

__device__ __forceinline__ void source_point(const EArgs &a, const double *st, const float *y,
                                             float &ox, float &oy, float &oz) {
    if (a.use_T) {
        double x, yy, z;
        xform12(st + kStT, (double)y[0], (double)y[1], (double)y[2], x, yy, z);
        ox = (float)x; oy = (float)yy; oz = (float)z;
    } else {
        ox = y[0]; oy = y[1]; oz = y[2];
    }
}

__device__ __forceinline__ void col_finish(const EArgs &a, const double *st, int p, int n, double den) {
    // den == 0: the FLT_EPSILON rule.  Such a column has v = 0 in every row, so the
    // row moments know nothing of its Pt1 = eps / (eps + c); the M-step adds it from colw
    const bool unreached = den == 0.0;
    if (unreached) den = (double)FLT_EPSILON;
    const double r = den + st[kStC];
    a.inv[(size_t)p * a.Nmax + n] = (float)(1.0 / r);
    a.pt1[(size_t)p * a.Nmax + n] = (float)(den / r);
    a.colw[(size_t)p * a.Nmax + n] = unreached ? den / r : 0.0;
}

__global__ __launch_bounds__(kThreads) void cpd_col_kernel(EArgs a) {
    const int p = blockIdx.z;
    const double *st = a.state + (size_t)p * kStWords;
    if (st[kStDone] != 0.0) return;
    const int M = pair_count(a.n_src, p, a.Mmax), N = pair_count(a.n_tgt, p, a.Nmax);
    const int n0 = blockIdx.x * kThreads;
    const int c0 = blockIdx.y * a.slice_chunks;
    if (n0 >= N || c0 * kChunk >= M) return;   // block-uniform
    const int nchunks = (M + kChunk - 1) / kChunk;
    const int c1 = min(nchunks, c0 + a.slice_chunks);
    __shared__ float4 sx[kChunk / 4], sy[kChunk / 4], sz[kChunk / 4];
    float *fx = reinterpret_cast<float *>(sx), *fy = reinterpret_cast<float *>(sy),
          *fz = reinterpret_cast<float *>(sz);
    const int tid = threadIdx.x, n = n0 + tid;
    const bool live = n < N;
    const float *X = a.tgt + ((size_t)p * a.Nmax + (live ? n : N - 1)) * 3;
    const float qx = X[0], qy = X[1], qz = X[2];
    const float fhi = (float)st[kStFhi], flo = (float)st[kStFlo];
    const float *Y = a.src + (size_t)p * a.Mmax * 3;
    double total = 0.0;
    for (int ci = c0; ci < c1; ++ci) {
        const int m0 = ci * kChunk, kend = min(kChunk, M - m0);
        __syncthreads();
        for (int e = tid; e < kChunk; e += kThreads) {
            float x = 0.f, y = 0.f, z = 0.f;
            if (e < kend) source_point(a, st, Y + (size_t)(m0 + e) * 3, x, y, z);
            fx[e] = x; fy[e] = y; fz[e] = z;
        }
        __syncthreads();
        double acc = 0.0;
        const int k4 = kend >> 2;
        for (int g = 0; g < k4; ++g) {
            const float4 CX = sx[g], CY = sy[g], CZ = sz[g];
            const float k0 = kern(qx, qy, qz, CX.x, CY.x, CZ.x, fhi, flo);
            const float k1 = kern(qx, qy, qz, CX.y, CY.y, CZ.y, fhi, flo);
            const float k2 = kern(qx, qy, qz, CX.z, CY.z, CZ.z, fhi, flo);
            const float k3 = kern(qx, qy, qz, CX.w, CY.w, CZ.w, fhi, flo);
            acc = acc + (double)((k0 + k1) + (k2 + k3));
        }
        if (kend & 3) {   // the chunk's last, short group: absent terms are +0
            float k[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < (kend & 3); ++j) {
                const int e = 4 * k4 + j;
                k[j] = kern(qx, qy, qz, fx[e], fy[e], fz[e], fhi, flo);
            }
            acc = acc + (double)((k[0] + k[1]) + (k[2] + k[3]));
        }
        if (a.split) {
            if (live) a.pden[((size_t)ci * a.P + p) * a.Nmax + n] = acc;
        } else {
            total = total + acc;
        }
    }
    if (!a.split && live) col_finish(a, st, p, n, total);
}

__global__ __launch_bounds__(kThreads) void cpd_col_finish_kernel(EArgs a) {
    const int p = blockIdx.z;
    const double *st = a.state + (size_t)p * kStWords;
    if (st[kStDone] != 0.0) return;
    const int M = pair_count(a.n_src, p, a.Mmax), N = pair_count(a.n_tgt, p, a.Nmax);
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const int nchunks = (M + kChunk - 1) / kChunk;
    double total = 0.0;
    for (int ci = 0; ci < nchunks; ++ci) total = total + a.pden[((size_t)ci * a.P + p) * a.Nmax + n];
    col_finish(a, st, p, n, total);
}

// a source's row moments R = (sum v, sum v dx, sum v dy, sum v dz, sum v d) with
// v = k inv, (dx, dy, dz) = y^ - x and d the f32 squared distance: P1 = R0,
// PX = R0 y^ - R1..3 (f64, then rounded), and sum v |x|^2 = R0 |y^|^2 - 2 y^.R1..3 + R4
__device__ __forceinline__ void row_finish(const EArgs &a, int p, int m, float qx, float qy, float qz,
                                           const double t[5]) {
    double *r = a.rowm + ((size_t)p * a.Mmax + m) * 5;
    for (int c = 0; c < 5; ++c) r[c] = t[c];
    a.p1[(size_t)p * a.Mmax + m] = (float)t[0];
    float *o = a.px + ((size_t)p * a.Mmax + m) * 3;
    o[0] = (float)(t[0] * (double)qx - t[1]);
    o[1] = (float)(t[0] * (double)qy - t[2]);
    o[2] = (float)(t[0] * (double)qz - t[3]);
}

// one group of four targets: the five f32 group sums, added to acc in f64
__device__ __forceinline__ void row_group(double acc[5], float qx, float qy, float qz, const float x[4],
                                          const float y[4], const float z[4], const float iv[4], float fhi,
                                          float flo) {
    float v[4], dx[4], dy[4], dz[4], d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dx[j] = qx - x[j]; dy[j] = qy - y[j]; dz[j] = qz - z[j];
        d[j] = (dx[j] * dx[j] + dy[j] * dy[j]) + dz[j] * dz[j];
        v[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(d[j], fhi, d[j] * flo)) * iv[j];
    }
    acc[0] = acc[0] + (double)((v[0] + v[1]) + (v[2] + v[3]));
    acc[1] = acc[1] + (double)__builtin_fmaf(v[3], dx[3], __builtin_fmaf(v[2], dx[2], __builtin_fmaf(v[1], dx[1], v[0] * dx[0])));
    acc[2] = acc[2] + (double)__builtin_fmaf(v[3], dy[3], __builtin_fmaf(v[2], dy[2], __builtin_fmaf(v[1], dy[1], v[0] * dy[0])));
    acc[3] = acc[3] + (double)__builtin_fmaf(v[3], dz[3], __builtin_fmaf(v[2], dz[2], __builtin_fmaf(v[1], dz[1], v[0] * dz[0])));
    acc[4] = acc[4] + (double)__builtin_fmaf(v[3], d[3], __builtin_fmaf(v[2], d[2], __builtin_fmaf(v[1], d[1], v[0] * d[0])));
}

__global__ __launch_bounds__(kThreads) void cpd_row_kernel(EArgs a) {
    const int p = blockIdx.z;
    const double *st = a.state + (size_t)p * kStWords;
    if (st[kStDone] != 0.0) return;
    const int M = pair_count(a.n_src, p, a.Mmax), N = pair_count(a.n_tgt, p, a.Nmax);
    const int m0 = blockIdx.x * kThreads;
    const int c0 = blockIdx.y * a.slice_chunks;
    if (m0 >= M || c0 * kChunk >= N) return;   // block-uniform
    const int nchunks = (N + kChunk - 1) / kChunk;
    const int c1 = min(nchunks, c0 + a.slice_chunks);
    __shared__ float4 sx[kChunk / 4], sy[kChunk / 4], sz[kChunk / 4], si[kChunk / 4];
    float *fx = reinterpret_cast<float *>(sx), *fy = reinterpret_cast<float *>(sy),
          *fz = reinterpret_cast<float *>(sz), *fi = reinterpret_cast<float *>(si);
    const int tid = threadIdx.x, m = m0 + tid;
    const bool live = m < M;
    float qx, qy, qz;
    source_point(a, st, a.src + ((size_t)p * a.Mmax + (live ? m : M - 1)) * 3, qx, qy, qz);
    const float fhi = (float)st[kStFhi], flo = (float)st[kStFlo];
    const float *X = a.tgt + (size_t)p * a.Nmax * 3;
    const float *I = a.inv + (size_t)p * a.Nmax;
    double total[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int ci = c0; ci < c1; ++ci) {
        const int t0 = ci * kChunk, kend = min(kChunk, N - t0);
        __syncthreads();
        // a chunk's absent targets: inv = 0 and the lane's own distances stay finite, so v = +0
        for (int e = tid; e < kChunk; e += kThreads) {
            float x = 0.f, y = 0.f, z = 0.f, iv = 0.f;
            if (e < kend) {
                const float *q = X + (size_t)(t0 + e) * 3;
                x = q[0]; y = q[1]; z = q[2];
                iv = I[t0 + e];
            }
            fx[e] = x; fy[e] = y; fz[e] = z; fi[e] = iv;
        }
        __syncthreads();
        double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        const int k4 = kend >> 2;
        for (int g = 0; g < k4; ++g) {
            const float4 CX = sx[g], CY = sy[g], CZ = sz[g], CI = si[g];
            const float x[4] = {CX.x, CX.y, CX.z, CX.w}, y[4] = {CY.x, CY.y, CY.z, CY.w},
                        z[4] = {CZ.x, CZ.y, CZ.z, CZ.w}, iv[4] = {CI.x, CI.y, CI.z, CI.w};
            row_group(acc, qx, qy, qz, x, y, z, iv, fhi, flo);
        }
        if (kend & 3) {   // the chunk's last, short group: absent terms are +0 (v = 0 * finite)
            float x[4], y[4], z[4], iv[4];
            for (int j = 0; j < 4; ++j) {
                const bool in = j < (kend & 3);
                const int e = 4 * k4 + j;
                x[j] = in ? fx[e] : qx; y[j] = in ? fy[e] : qy; z[j] = in ? fz[e] : qz;
                iv[j] = in ? fi[e] : 0.f;
            }
            row_group(acc, qx, qy, qz, x, y, z, iv, fhi, flo);
        }
        if (a.split) {
            if (live) {
                double *o = a.prow + (((size_t)ci * a.P + p) * a.Mmax + m) * 5;
                for (int c = 0; c < 5; ++c) o[c] = acc[c];
            }
        } else {
            for (int c = 0; c < 5; ++c) total[c] = total[c] + acc[c];
        }
    }
    if (!a.split && live) row_finish(a, p, m, qx, qy, qz, total);
}

__global__ __launch_bounds__(kThreads) void cpd_row_finish_kernel(EArgs a) {
    const int p = blockIdx.z;
    const double *st = a.state + (size_t)p * kStWords;
    if (st[kStDone] != 0.0) return;
    const int M = pair_count(a.n_src, p, a.Mmax), N = pair_count(a.n_tgt, p, a.Nmax);
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= M) return;
    const int nchunks = (N + kChunk - 1) / kChunk;
    double total[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int ci = 0; ci < nchunks; ++ci) {
        const double *o = a.prow + (((size_t)ci * a.P + p) * a.Mmax + m) * 5;
        for (int c = 0; c < 5; ++c) total[c] = total[c] + o[c];
    }
    float qx, qy, qz;
    source_point(a, st, a.src + ((size_t)p * a.Mmax + m) * 3, qx, qy, qz);
    row_finish(a, p, m, qx, qy, qz, total);
}

// ---- per-pair kernels: one 256-thread workgroup, procrustes.hip's reduction order ----
constexpr int kRedW = 10;

__device__ inline void tree256(double (*red)[kRedW], const double *v, int nv) {
    __syncthreads();   // the previous round's reads of red[0] are over
    for (int k = 0; k < nv; ++k) red[threadIdx.x][k] = v[k];
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < nv; ++k) red[threadIdx.x][k] = red[threadIdx.x][k] + red[threadIdx.x + s][k];
        __syncthreads();
    }
}

struct StateArgs {
    const float *src, *tgt;
    const int32_t *n_src, *n_tgt;
    const double *init;      // (P,16) or null (identity)
    const double *sigma2;    // (P) or null (the initial sigma2 of the contract)
    double *state;
    double *np_out;          // estep: (P) or null
    const float *p1;         // estep: the P1 to sum into np_out
    int32_t *done_count;
    int P, Mmax, Nmax;
    double w;
};

// state of every pair: T = init or identity, sigma2 given or the contract's
// initial value sum |x_n - y_m|^2 / (3 M N) as
// (M sum|x - c|^2 + N sum|y - c|^2 - 2 sum(x - c) . sum(y - c)) / (3 M N), c = x_0, in f64
__global__ __launch_bounds__(kThreads) void cpd_init_kernel(StateArgs a) {
    const int p = blockIdx.x, t = threadIdx.x;
    __shared__ double red[kThreads][kRedW];
    double *st = a.state + (size_t)p * kStWords;
    const int M = pair_count(a.n_src, p, a.Mmax), N = pair_count(a.n_tgt, p, a.Nmax);
    if (M == 0 || N == 0) {
        if (t == 0) {
            for (int k = 0; k < kStWords; ++k) st[k] = 0.0;
            st[kStDone] = 1.0;
            st[kStStatus] = 1.0;
            if (a.done_count) atomicAdd(a.done_count, 1);
        }
        return;
    }
    double s2 = 0.0;
    if (a.sigma2) {
        s2 = a.sigma2[p];
    } else {
        const float *X = a.tgt + (size_t)p * a.Nmax * 3, *Y = a.src + (size_t)p * a.Mmax * 3;
        const double c[3] = {(double)X[0], (double)X[1], (double)X[2]};
        double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = t; i < N; i += kThreads)
            for (int k = 0; k < 3; ++k) {
                const double d = (double)X[3 * i + k] - c[k];
                v[k] = v[k] + d;
                v[6] = v[6] + d * d;
            }
        for (int i = t; i < M; i += kThreads)
            for (int k = 0; k < 3; ++k) {
                const double d = (double)Y[3 * i + k] - c[k];
                v[3 + k] = v[3 + k] + d;
                v[7] = v[7] + d * d;
            }
        tree256(red, v, 8);
        const double *r = red[0];
        const double dot = (r[0] * r[3] + r[1] * r[4]) + r[2] * r[5];
        s2 = (((double)M * r[6] + (double)N * r[7]) - 2.0 * dot) / ((3.0 * (double)M) * (double)N);
    }
    if (t == 0) {
        for (int k = 0; k < kStWords; ++k) st[k] = 0.0;
        if (a.init) {
            for (int k = 0; k < 12; ++k) st[kStT + k] = a.init[(size_t)p * 16 + k];
        } else {
            st[kStT + 0] = 1.0; st[kStT + 5] = 1.0; st[kStT + 10] = 1.0;
        }
        st[kStSigma2] = s2;
        st[kStScale] = 1.0;
        state_derive(st, a.w, M, N);
    }
}

// Np = sum P1 in the M-step's order (lane t adds t, t + 256, ...; halving tree)
__global__ __launch_bounds__(kThreads) void cpd_np_kernel(StateArgs a) {
    const int p = blockIdx.x, t = threadIdx.x;
    __shared__ double red[kThreads][kRedW];
    if (a.state[(size_t)p * kStWords + kStDone] != 0.0) return;
    const int M = pair_count(a.n_src, p, a.Mmax);
    double v = 0.0;
    for (int i = t; i < M; i += kThreads) v = v + (double)a.p1[(size_t)p * a.Mmax + i];
    tree256(red, &v, 1);
    if (t == 0) a.np_out[p] = red[0][0];
}

struct MArgs {
    const float *src, *tgt;
    const int32_t *n_src, *n_tgt;
    const double *rowm;     // (P,Mmax,5): the row sweep's moments at the state's T
    const double *colw;     // (P,Nmax): Pt1 of the targets no source reaches, else 0
    double *state;
    int32_t *done_count;
    int P, Mmax, Nmax;
    int kind;      // 0 rigid, 1 rigid + scale, 2 affine
    double w, tol;
};

// P1, PX and sum_n v |x_n|^2 of source i from its row moments (row_finish), y^ as the sweeps formed it
__device__ __forceinline__ void row_terms(const double *T, const float *y, const double *r, double &w1,
                                          double px[3], double &pxx) {
    double tx, ty, tz;
    xform12(T, (double)y[0], (double)y[1], (double)y[2], tx, ty, tz);
    const double h[3] = {(double)(float)tx, (double)(float)ty, (double)(float)tz};
    w1 = r[0];
    for (int c = 0; c < 3; ++c) px[c] = w1 * h[c] - r[1 + c];
    const double hh = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2];
    const double hd = (h[0] * r[1] + h[1] * r[2]) + h[2] * r[3];
    pxx = (w1 * hh - 2.0 * hd) + r[4];
}

// tr(Xc^T dPt1 Xc) is split by column.  A target some source reaches has
// Pt1_n = sum_m v_mn, and over those the trace is sum_mn v |x_n|^2 - 2 mux . sum PX
// + |mux|^2 Np = sum_mn v |x_n|^2 - Np |mux|^2 with the row sweep's own weights v, so
// that this part of the residual trXPX - 2 tr(A^T B) + tr(B G B^T) is a sum of
// squares under exactly those weights and loses nothing to cancellation when
// sigma2 is far below the clouds' extent.  A target no source reaches (den_n = 0)
// has v = 0 in every row but Pt1_n = eps / (eps + c) by the FLT_EPSILON rule; its
// Pt1_n |x_n - mux|^2 is added in a pass over the targets (colw is 0 elsewhere).
__global__ __launch_bounds__(kThreads) void cpd_mstep_kernel(MArgs a) {
    const int p = blockIdx.x, t = threadIdx.x;
    __shared__ double red[kThreads][kRedW];
    double *st = a.state + (size_t)p * kStWords;
    if (st[kStDone] != 0.0) return;
    const int M = pair_count(a.n_src, p, a.Mmax), N = pair_count(a.n_tgt, p, a.Nmax);
    const float *Y = a.src + (size_t)p * a.Mmax * 3;
    const double *RM = a.rowm + (size_t)p * a.Mmax * 5;
    double T[12];
    for (int k = 0; k < 12; ++k) T[k] = st[kStT + k];

    double v[kRedW];
    for (int k = 0; k < kRedW; ++k) v[k] = 0.0;
    for (int i = t; i < M; i += kThreads) {
        double w1, px[3], pxx;
        row_terms(T, Y + 3 * i, RM + 5 * i, w1, px, pxx);
        v[0] = v[0] + w1;
        for (int c = 0; c < 3; ++c) {
            v[1 + c] = v[1 + c] + px[c];
            v[4 + c] = v[4 + c] + w1 * (double)Y[3 * i + c];
        }
        v[7] = v[7] + pxx;
    }
    tree256(red, v, 8);
    const double Np = red[0][0], sumPXX = red[0][7];
    const double mux[3] = {red[0][1] / Np, red[0][2] / Np, red[0][3] / Np};
    const double muy[3] = {red[0][4] / Np, red[0][5] / Np, red[0][6] / Np};

    // PX^T Yc (9)
    for (int k = 0; k < kRedW; ++k) v[k] = 0.0;
    for (int i = t; i < M; i += kThreads) {
        double w1, px[3], pxx;
        row_terms(T, Y + 3 * i, RM + 5 * i, w1, px, pxx);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) v[3 * r + c] = v[3 * r + c] + px[r] * ((double)Y[3 * i + c] - muy[c]);
    }
    tree256(red, v, 9);
    double PXY[9];
    for (int k = 0; k < 9; ++k) PXY[k] = red[0][k];

    // P1^T Yc (3), Yc^T dP1 Yc (6: xx xy xz yy yz zz)
    for (int k = 0; k < kRedW; ++k) v[k] = 0.0;
    for (int i = t; i < M; i += kThreads) {
        const double w1 = RM[5 * i];
        const double y0 = (double)Y[3 * i] - muy[0], y1 = (double)Y[3 * i + 1] - muy[1],
                     y2 = (double)Y[3 * i + 2] - muy[2];
        v[0] = v[0] + w1 * y0; v[1] = v[1] + w1 * y1; v[2] = v[2] + w1 * y2;
        v[3] = v[3] + (w1 * y0) * y0; v[4] = v[4] + (w1 * y0) * y1; v[5] = v[5] + (w1 * y0) * y2;
        v[6] = v[6] + (w1 * y1) * y1; v[7] = v[7] + (w1 * y1) * y2; v[8] = v[8] + (w1 * y2) * y2;
    }
    const float *X = a.tgt + (size_t)p * a.Nmax * 3;
    const double *CW = a.colw + (size_t)p * a.Nmax;
    for (int i = t; i < N; i += kThreads) {
        const double cw = CW[i];
        if (cw != 0.0) {
            const double x0 = (double)X[3 * i] - mux[0], x1 = (double)X[3 * i + 1] - mux[1],
                         x2 = (double)X[3 * i + 2] - mux[2];
            v[9] = v[9] + cw * ((x0 * x0 + x1 * x1) + x2 * x2);
        }
    }
    tree256(red, v, 10);
    if (t != 0) return;
    const double *r = red[0];
    double A[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[3 * i + j] = PXY[3 * i + j] - mux[i] * r[j];
    const double G[9] = {r[3], r[4], r[5], r[4], r[6], r[7], r[5], r[7], r[8]};   // Yc^T dP1 Yc
    const double trYPY = (r[3] + r[6]) + r[8];
    const double trXPX = (sumPXX - Np * ((mux[0] * mux[0] + mux[1] * mux[1]) + mux[2] * mux[2])) + r[9];
    double B[9], scale = 1.0, s2, resid;
    if (a.kind == 2) {
        // B = A G^-1, G symmetric: the adjugate over the determinant
        const double c00 = G[4] * G[8] - G[5] * G[7], c01 = G[5] * G[6] - G[3] * G[8],
                     c02 = G[3] * G[7] - G[4] * G[6];
        const double det = (G[0] * c00 + G[1] * c01) + G[2] * c02;
        const double Gi[9] = {c00 / det, (G[2] * G[7] - G[1] * G[8]) / det, (G[1] * G[5] - G[2] * G[4]) / det,
                              c01 / det, (G[0] * G[8] - G[2] * G[6]) / det, (G[2] * G[3] - G[0] * G[5]) / det,
                              c02 / det, (G[1] * G[6] - G[0] * G[7]) / det, (G[0] * G[4] - G[1] * G[3]) / det};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                B[3 * i + j] = (A[3 * i] * Gi[j] + A[3 * i + 1] * Gi[3 + j]) + A[3 * i + 2] * Gi[6 + j];
        double trAB = 0.0, trBGB = 0.0;
        for (int k = 0; k < 9; ++k) trAB = trAB + A[k] * B[k];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double bg = (B[3 * i] * G[j] + B[3 * i + 1] * G[3 + j]) + B[3 * i + 2] * G[6 + j];
                trBGB = trBGB + bg * B[3 * i + j];
            }
        s2 = (trXPX - trAB) / (3.0 * Np);
        resid = (trXPX - 2.0 * trAB) + trBGB;
    } else {
        // max tr(A^T R): horn_rotation takes S[src][tgt] = A^T
        double S[9], R[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) S[3 * j + i] = A[3 * i + j];
        horn_rotation(S, R);
        double trAR = 0.0;
        for (int k = 0; k < 9; ++k) trAR = trAR + A[k] * R[k];
        if (a.kind == 1) {
            scale = trAR / trYPY;
            s2 = (trXPX - scale * trAR) / (3.0 * Np);
        } else {
            s2 = ((trXPX - 2.0 * trAR) + trYPY) / (3.0 * Np);
        }
        for (int k = 0; k < 9; ++k) B[k] = scale * R[k];
        resid = (trXPX - (2.0 * scale) * trAR) + (scale * scale) * trYPY;
    }
    if (s2 < (double)FLT_EPSILON) s2 = (double)FLT_EPSILON;
    const double q = resid / (2.0 * s2) + (1.5 * Np) * det_log(s2);
    const double q_prev = st[kStQ];
    const int it = (int)st[kStIters];
    st[kStSigma2] = s2;
    st[kStQ] = q;
    st[kStNp] = Np;
    st[kStIters] = (double)(it + 1);
    const bool finite = (s2 - s2 == 0.0) && (q - q == 0.0);
    bool done = false;
    if (!finite) {
        st[kStStatus] = 2.0;   // T and scale keep the last iterate
        done = true;
    } else {
        for (int i = 0; i < 3; ++i) {
            st[kStT + 4 * i] = B[3 * i]; st[kStT + 4 * i + 1] = B[3 * i + 1]; st[kStT + 4 * i + 2] = B[3 * i + 2];
            st[kStT + 4 * i + 3] = mux[i] - ((B[3 * i] * muy[0] + B[3 * i + 1] * muy[1]) + B[3 * i + 2] * muy[2]);
        }
        st[kStScale] = scale;
        state_derive(st, a.w, M, N);
        if (it >= 1 && __builtin_fabs(q - q_prev) < a.tol) done = true;
    }
    if (done) {
        st[kStDone] = 1.0;
        atomicAdd(a.done_count, 1);
    }
}

struct OutArgs {
    const double *state;
    double *T, *scale, *sigma2, *q;
    int32_t *iters, *status;
};

__global__ void cpd_export_kernel(OutArgs a, int P) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const double *st = a.state + (size_t)p * kStWords;
    const int status = (int)st[kStStatus];
    a.status[p] = status;
    if (status == 1) return;   // an empty cloud: the other outputs are left alone
    double *T = a.T + (size_t)p * 16;
    for (int k = 0; k < 12; ++k) T[k] = st[kStT + k];
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
    a.scale[p] = st[kStScale];
    a.sigma2[p] = st[kStSigma2];
    a.q[p] = st[kStQ];
    a.iters[p] = (int)st[kStIters];
}

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// slices of the staged axis (len points) for a sweep whose lanes cover `lanes`
// points: split until the launch has ~2 workgroups per CU or one chunk per slice
inline int slice_chunks_for(int P, int lanes, int len) {
    const int64_t base = cdiv64(lanes, kThreads) * P;
    const int nchunks = (int)cdiv64(len, kChunk);
    int slices = 1;
    while (base * slices < 2LL * kCUs && slices < nchunks) slices *= 2;
    return (int)cdiv64(nchunks, slices);
}

struct Scratch {
    double *state, *pden, *prow, *rowm, *colw;
    int32_t *done_count;
    float *inv, *pt1, *p1, *px;
    size_t bytes;
    int col_chunks, row_chunks;   // chunks per slice of each sweep
    bool col_split, row_split;
};

Scratch scratch_layout(void *base, int P, int Mmax, int Nmax) {
    Scratch s;
    char *b = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = b + off; off += up256(bytes); return q; };
    const size_t p = (size_t)P, m = (size_t)Mmax, n = (size_t)Nmax;
    s.state = reinterpret_cast<double *>(take(p * kStWords * sizeof(double)));
    s.done_count = reinterpret_cast<int32_t *>(take(sizeof(int32_t)));
    s.inv = reinterpret_cast<float *>(take(p * n * sizeof(float)));
    s.pt1 = reinterpret_cast<float *>(take(p * n * sizeof(float)));
    s.p1 = reinterpret_cast<float *>(take(p * m * sizeof(float)));
    s.px = reinterpret_cast<float *>(take(p * m * 3 * sizeof(float)));
    s.col_chunks = slice_chunks_for(P, Nmax, Mmax);
    s.row_chunks = slice_chunks_for(P, Mmax, Nmax);
    const size_t mch = (size_t)cdiv64(Mmax, kChunk), nch = (size_t)cdiv64(Nmax, kChunk);
    s.col_split = (size_t)s.col_chunks < mch;
    s.row_split = (size_t)s.row_chunks < nch;
    s.pden = reinterpret_cast<double *>(take(s.col_split ? mch * p * n * sizeof(double) : 0));
    s.prow = reinterpret_cast<double *>(take(s.row_split ? nch * p * m * 5 * sizeof(double) : 0));
    s.rowm = reinterpret_cast<double *>(take(p * m * 5 * sizeof(double)));
    s.colw = reinterpret_cast<double *>(take(p * n * sizeof(double)));
    s.bytes = off;
    return s;
}

bool sizes_ok(int P, int Mmax, int Nmax) {
    return P >= 0 && Mmax >= 0 && Nmax >= 0 && P <= 65535 && Mmax <= (1 << 24) && Nmax <= (1 << 24);
}

int launch_estep(const EArgs &e0, const Scratch &sc, hipStream_t s) {
    EArgs e = e0;
    const dim3 blk(kThreads);
    e.slice_chunks = sc.col_chunks;
    e.split = sc.col_split;
    hipLaunchKernelGGL(cpd_col_kernel, dim3((unsigned)cdiv64(e.Nmax, kThreads), (unsigned)cdiv64(cdiv64(e.Mmax, kChunk), sc.col_chunks), e.P),
                       blk, 0, s, e);
    PCR_LAUNCH_CHECK();
    if (sc.col_split) {
        hipLaunchKernelGGL(cpd_col_finish_kernel, dim3((unsigned)cdiv64(e.Nmax, kThreads), 1, e.P), blk, 0, s, e);
        PCR_LAUNCH_CHECK();
    }
    e.slice_chunks = sc.row_chunks;
    e.split = sc.row_split;
    hipLaunchKernelGGL(cpd_row_kernel, dim3((unsigned)cdiv64(e.Mmax, kThreads), (unsigned)cdiv64(cdiv64(e.Nmax, kChunk), sc.row_chunks), e.P),
                       blk, 0, s, e);
    PCR_LAUNCH_CHECK();
    if (sc.row_split) {
        hipLaunchKernelGGL(cpd_row_finish_kernel, dim3((unsigned)cdiv64(e.Mmax, kThreads), 1, e.P), blk, 0, s, e);
        PCR_LAUNCH_CHECK();
    }
    return PCR_OK;
}

}  // namespace
}  // namespace pcr

extern "C" int64_t pcr_cpd_scratch_bytes(int32_t P, int32_t Mmax, int32_t Nmax) {
    pcr::clear_error();
    if (!pcr::sizes_ok(P, Mmax, Nmax)) {
        pcr::set_error("cpd_scratch_bytes: P=%d (0..65535), Mmax=%d, Nmax=%d (0..2^24) out of range", P, Mmax, Nmax);
        return -1;
    }
    return (int64_t)pcr::scratch_layout(nullptr, P, Mmax, Nmax).bytes;
}

extern "C" int pcr_cpd_estep(const float *src, const float *tgt, int32_t P, int32_t Mmax, int32_t Nmax,
                             const int32_t *n_src, const int32_t *n_tgt, const double *T,
                             const double *sigma2, double w, float *pt1, float *p1, float *px, double *n_p,
                             void *scratch, pcr_stream_t stream) {
    using namespace pcr;
    clear_error();
    PCR_REQUIRE(sizes_ok(P, Mmax, Nmax), PCR_ERR_ARG, "cpd_estep: P=%d (0..65535), Mmax=%d, Nmax=%d (0..2^24) out of range", P, Mmax, Nmax);
    PCR_REQUIRE(w >= 0.0 && w < 1.0, PCR_ERR_ARG, "cpd_estep: w=%g outside [0, 1)", w);
    if (P == 0 || Mmax == 0 || Nmax == 0) return PCR_OK;
    PCR_REQUIRE(src && tgt && sigma2 && pt1 && p1 && px && n_p && scratch, PCR_ERR_ARG, "cpd_estep: null pointer");
    PCR_REQUIRE(((uintptr_t)scratch & 255) == 0, PCR_ERR_ARG, "cpd_estep: scratch is not 256-byte aligned");
    hipStream_t s = as_stream(stream);
    const Scratch sc = scratch_layout(scratch, P, Mmax, Nmax);
    StateArgs ia{src, tgt, n_src, n_tgt, T, sigma2, sc.state, n_p, p1, nullptr, P, Mmax, Nmax, w};
    hipLaunchKernelGGL(cpd_init_kernel, dim3(P), dim3(kThreads), 0, s, ia);
    PCR_LAUNCH_CHECK();
    EArgs e{src, tgt, n_src, n_tgt, sc.state, sc.inv, pt1, p1, px, sc.pden, sc.prow, sc.rowm, sc.colw, P, Mmax, Nmax, T != nullptr, 1, 0};
    const int rc = launch_estep(e, sc, s);
    if (rc != PCR_OK) return rc;
    hipLaunchKernelGGL(cpd_np_kernel, dim3(P), dim3(kThreads), 0, s, ia);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

extern "C" int pcr_cpd_register(const float *src, const float *tgt, int32_t P, int32_t Mmax, int32_t Nmax,
                                const int32_t *n_src, const int32_t *n_tgt, int32_t kind, double w,
                                int32_t maxiter, double tol, const double *init, double *T, double *scale,
                                double *sigma2, double *q, int32_t *iters, int32_t *status, void *scratch,
                                pcr_stream_t stream) {
    using namespace pcr;
    clear_error();
    PCR_REQUIRE(sizes_ok(P, Mmax, Nmax), PCR_ERR_ARG, "cpd_register: P=%d (0..65535), Mmax=%d, Nmax=%d (0..2^24) out of range", P, Mmax, Nmax);
    PCR_REQUIRE(kind >= 0 && kind <= 2, PCR_ERR_ARG, "cpd_register: kind=%d outside 0..2", kind);
    PCR_REQUIRE(w >= 0.0 && w < 1.0, PCR_ERR_ARG, "cpd_register: w=%g outside [0, 1)", w);
    PCR_REQUIRE(maxiter >= 0, PCR_ERR_ARG, "cpd_register: maxiter=%d negative", maxiter);
    if (P == 0) return PCR_OK;
    PCR_REQUIRE(T && scale && sigma2 && q && iters && status && scratch, PCR_ERR_ARG, "cpd_register: null pointer");
    PCR_REQUIRE((src || Mmax == 0) && (tgt || Nmax == 0), PCR_ERR_ARG, "cpd_register: null cloud");
    PCR_REQUIRE(((uintptr_t)scratch & 255) == 0, PCR_ERR_ARG, "cpd_register: scratch is not 256-byte aligned");
    hipStream_t s = as_stream(stream);
    const Scratch sc = scratch_layout(scratch, P, Mmax, Nmax);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    PCR_HIP_CHECK(hipStreamIsCapturing(s, &cap));
    const bool capturing = cap != hipStreamCaptureStatusNone;
    PCR_HIP_CHECK(hipMemsetAsync(sc.done_count, 0, sizeof(int32_t), s));
    StateArgs ia{src, tgt, n_src, n_tgt, init, nullptr, sc.state, nullptr, nullptr, sc.done_count, P, Mmax, Nmax, w};
    hipLaunchKernelGGL(cpd_init_kernel, dim3(P), dim3(kThreads), 0, s, ia);
    PCR_LAUNCH_CHECK();
    if (Mmax > 0 && Nmax > 0) {
        EArgs e{src, tgt, n_src, n_tgt, sc.state, sc.inv, sc.pt1, sc.p1, sc.px, sc.pden, sc.prow, sc.rowm, sc.colw, P, Mmax, Nmax, 1, 1, 0};
        MArgs m{src, tgt, n_src, n_tgt, sc.rowm, sc.colw, sc.state, sc.done_count, P, Mmax, Nmax, kind, w, tol};
        for (int it = 0; it < maxiter; ++it) {
            const int rc = launch_estep(e, sc, s);
            if (rc != PCR_OK) return rc;
            hipLaunchKernelGGL(cpd_mstep_kernel, dim3(P), dim3(kThreads), 0, s, m);
            PCR_LAUNCH_CHECK();
            // every pair stopped: the launches left would all return at entry
            if (!capturing && tol > 0.0 && (it & 7) == 7 && it + 1 < maxiter) {
                int32_t done = 0;
                PCR_HIP_CHECK(hipMemcpyAsync(&done, sc.done_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
                PCR_HIP_CHECK(hipStreamSynchronize(s));
                if (done >= P) break;
            }
        }
    }
    OutArgs o{sc.state, T, scale, sigma2, q, iters, status};
    hipLaunchKernelGGL(cpd_export_kernel, dim3((unsigned)cdiv64(P, 64)), dim3(64), 0, s, o, P);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}
