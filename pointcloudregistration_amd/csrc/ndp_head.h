// The branch head of an NDP level, shared by the warp (ndp.hip) and the fused
// training step (ndp_train.hip): the nine (motion, rotation format) heads of
// NDPLayer (c2p-net/deformationpyramid/model/nets.py:111-161, rigid_body.py).
//
// Head code (pcr_ndp_level.head) = rotation format + 4 * motion:
//   format 0 axis_angle, 1 euler, 2 quaternion, 3 6D; motion 0 SE3, 1 Sim3,
//   2 sflow (code 8 only: no rotation branch).
//
// Branch rows (the 32-row branch tile, aux, dO and the branch gradients share
// one row map per head):
//   code 0:       rot 0-2, trn 3-5, nr 6                    (8 rows, 7 gradient rows)
//   codes 1-8:    rot 0-5 (the format's 3, 3, 4 or 6 first), trn 6-8, nr 9,
//                 scale 10, and in aux alone R x of a Sim3 head in 11-13
//                                                            (16 rows, 11 gradient rows)
// Rows a head does not use hold exact zeros.
//
// Forward, f32, o = the rot rows scaled by 1e-3:
//   axis_angle  th = |o|, w = o / th, K = skew(w), R = I + sin th K + (1 - cos th) K K
//   euler       R = Rx(o0) Ry(o1) Rz(o2)
//   quaternion  q = o / |o| (the reference's copysign flips q as a whole, and R
//               is even in q: dropped), two_s = 2 / sum q^2, R = I + two_s B(q),
//               B = [[-(jj+kk), ij-kr, ik+jr], [ij+kr, -(ii+kk), jk-ir],
//                    [ik-jr, jk+ir, -(ii+jj)]], q = (r, i, j, k)
//   6D          a1 = o[0:3], a2 = o[3:6]; b1 = a1 / max(|a1|, 1e-12),
//               u = a2 - (b1.a2) b1, b2 = u / max(|u|, 1e-12), b3 = b1 x b2,
//               R = rows (b1, b2, b3)
//   SE3 y = R x + t;  Sim3 y = c (R x) + t, c = 1e-3 o_s + 1;  sflow y = x + t
//   x' = y, or x + s (y - x) with the nonrigidity branch.
//
// Backward of the rotation: G = dL/dR = g_y (x) x (g_y times c for Sim3), and
//   axis_angle  dth = <G, cos th K + sin th K K>, dK = sin th G + (1 - cos th)
//               (G K^T + K^T G), gw = vee(dK - dK^T), do = (gw - (gw.w) w) / th + dth w
//   euler       M = Rx Ry: dRz = M^T G, dM = G Rz^T, dRy = Rx^T dM, dRx = dM Ry^T,
//               do_k = <dR_k, dR_k/do_k> (the four sin / cos entries of each)
//   quaternion  dts = <G, B>, dB = two_s G, dq = (dB : dB/dq) - two_s^2 dts q
//               (two_s = 2 / ss, dss = -(two_s^2 / 2) dts, dq += 2 q dss),
//               do = (dq - (q.dq) q) / |o|
//   6D          db1 = G0 + b2 x G2, db2 = G1 + G2 x b1,
//               du = (db2 - (b2.db2) b2) / |u|   (db2 / 1e-12 where clamped),
//               da2 = du - (du.b1) b1, db1 -= (du.b1) a2 + (b1.a2) du,
//               da1 = (db1 - (b1.db1) b1) / |a1| (db1 / 1e-12 where clamped)
//   Sim3        dc = g_y . (R x), dO_s = 1e-3 dc
#pragma once
#include <hip/hip_runtime.h>
#include "ndp_tile.h"

namespace pcr {
namespace ndph {

constexpr int kAxis = 0, kEuler = 1, kQuat = 2, k6D = 3;
constexpr int kSE3 = 0, kSim3 = 1, kSflow = 2;
constexpr int kHeads = 9;

__host__ __device__ constexpr bool head_valid(int head) { return head >= 0 && head < kHeads; }
__host__ __device__ constexpr int head_motion(int head) { return head >> 2; }
__host__ __device__ constexpr int head_format(int head) { return head & 3; }
__host__ __device__ constexpr int head_rot_rows(int head) {
    return head_motion(head) == kSflow ? 0 : head_format(head) == kQuat ? 4 : head_format(head) == k6D ? 6 : 3;
}

inline const char *head_name(int head) {
    static const char *const names[kHeads] = {"SE3/axis_angle", "SE3/euler", "SE3/quaternion", "SE3/6D",
                                              "Sim3/axis_angle", "Sim3/euler", "Sim3/quaternion", "Sim3/6D",
                                              "sflow"};
    return head_valid(head) ? names[head] : "unknown";
}

// the row map of a head
struct RowMap {
    int rot, trn, nr, sc, rx, n, nw;  // rot rows; first trn row; nr, scale rows; R x rows; aux / dO rows; gradient rows
};
__host__ __device__ constexpr RowMap row_map(int head) {
    return head == 0 ? RowMap{3, 3, 6, -1, -1, 8, 7} : RowMap{head_rot_rows(head), 6, 9, 10, 11, 16, 11};
}

struct BranchW {
    const float *w_rot, *b_rot, *w_trn, *b_trn, *w_nr, *b_nr, *w_s, *b_s;
};

// row q of the branch weights (null: a row the head does not use) and its bias
template <int HEAD>
__device__ __forceinline__ const float *branch_row(const BranchW &b, int q, int W) {
    constexpr RowMap M = row_map(HEAD);
    if (q < M.rot) return b.w_rot + q * W;
    if (q >= M.trn && q < M.trn + 3) return b.w_trn + (q - M.trn) * W;
    if (q == M.nr && b.w_nr) return b.w_nr;
    if (head_motion(HEAD) == kSim3 && q == M.sc) return b.w_s;
    return nullptr;
}
template <int HEAD>
__device__ __forceinline__ float branch_bias(const BranchW &b, int q) {
    constexpr RowMap M = row_map(HEAD);
    if (q < M.rot) return b.b_rot[q];
    if (q >= M.trn && q < M.trn + 3) return b.b_trn[q - M.trn];
    if (q == M.nr && b.w_nr) return b.b_nr[0];
    if (head_motion(HEAD) == kSim3 && q == M.sc) return b.b_s[0];
    return 0.0f;
}

// row Q of a tile, in every lane: rows 0-3 sit in registers 0-3 of the h = 0
// half, rows 4-7 in the h = 1 half, rows 8-11 in registers 4-7 of h = 0, ...
template <int Q>
__device__ __forceinline__ float tile_row(const ndpt::f32x16 &T, int h) {
    constexpr int reg = (Q & 3) + 4 * (Q >> 3), half = (Q >> 2) & 1;
    const float v = T[reg];
    const float o = __shfl_xor(v, 32, 64);
    return h == half ? v : o;
}

__device__ __forceinline__ float dot3(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const float *a, const float *b, float *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void mat3(const float A[3][3], const float B[3][3], float C[3][3]) {
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) C[u][v] = (A[u][0] * B[0][v] + A[u][1] * B[1][v]) + A[u][2] * B[2][v];
}
// C = A^T B, C = A B^T
__device__ __forceinline__ void mat3_tn(const float A[3][3], const float B[3][3], float C[3][3]) {
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) C[u][v] = (A[0][u] * B[0][v] + A[1][u] * B[1][v]) + A[2][u] * B[2][v];
}
__device__ __forceinline__ void mat3_nt(const float A[3][3], const float B[3][3], float C[3][3]) {
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) C[u][v] = (A[u][0] * B[v][0] + A[u][1] * B[v][1]) + A[u][2] * B[v][2];
}

constexpr float kNormEps = 1e-12f;  // F.normalize's eps

struct Euler {
    float Rx[3][3], Ry[3][3], Rz[3][3], s[3], c[3];
    __device__ __forceinline__ explicit Euler(const float *r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { s[k] = sinf(r[k]); c[k] = cosf(r[k]); }
        const float x[3][3] = {{1.f, 0.f, 0.f}, {0.f, c[0], -s[0]}, {0.f, s[0], c[0]}};
        const float y[3][3] = {{c[1], 0.f, s[1]}, {0.f, 1.f, 0.f}, {-s[1], 0.f, c[1]}};
        const float z[3][3] = {{c[2], -s[2], 0.f}, {s[2], c[2], 0.f}, {0.f, 0.f, 1.f}};
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) { Rx[u][v] = x[u][v]; Ry[u][v] = y[u][v]; Rz[u][v] = z[u][v]; }
    }
};

struct Quat {
    float q[4], n, ts, B[3][3];
    __device__ __forceinline__ explicit Quat(const float *o) {
        n = sqrtf(((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) + o[3] * o[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = o[k] / n;
        const float r = q[0], i = q[1], j = q[2], k = q[3];
        ts = 2.0f / (((r * r + i * i) + j * j) + k * k);
        B[0][0] = -(j * j + k * k); B[0][1] = i * j - k * r;    B[0][2] = i * k + j * r;
        B[1][0] = i * j + k * r;    B[1][1] = -(i * i + k * k); B[1][2] = j * k - i * r;
        B[2][0] = i * k - j * r;    B[2][1] = j * k + i * r;    B[2][2] = -(i * i + j * j);
    }
};

struct SixD {
    float a2[3], b1[3], b2[3], b3[3], d1, d2, dd;
    bool clamp1, clamp2;
    __device__ __forceinline__ explicit SixD(const float *o) {
        const float n1 = sqrtf((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]);
        clamp1 = !(n1 >= kNormEps);
        d1 = n1 < kNormEps ? kNormEps : n1;
        float u[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { b1[k] = o[k] / d1; a2[k] = o[3 + k]; }
        dd = dot3(b1, a2);
#pragma unroll
        for (int k = 0; k < 3; ++k) u[k] = a2[k] - dd * b1[k];
        const float n2 = sqrtf((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
        clamp2 = !(n2 >= kNormEps);
        d2 = n2 < kNormEps ? kNormEps : n2;
#pragma unroll
        for (int k = 0; k < 3; ++k) b2[k] = u[k] / d2;
        cross3(b1, b2, b3);
    }
};

// R of the rotation rows r (already scaled by 1e-3)
template <int FMT>
__device__ __forceinline__ void rotation(const float *r, float R[3][3]) {
    if constexpr (FMT == kAxis) {
        const float r0 = r[0], r1 = r[1], r2 = r[2];
        const float th = sqrtf((r0 * r0 + r1 * r1) + r2 * r2);
        const float w0 = r0 / th, w1 = r1 / th, w2 = r2 / th;
        // K = skew(w): [[0,-w2,w1],[w2,0,-w0],[-w1,w0,0]]
        const float K[3][3] = {{0.f, -w2, w1}, {w2, 0.f, -w0}, {-w1, w0, 0.f}};
        const float sn = sinf(th), cs = 1.0f - cosf(th);
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const float kk = (K[u][0] * K[0][v] + K[u][1] * K[1][v]) + K[u][2] * K[2][v];
                R[u][v] = ((u == v ? 1.0f : 0.0f) + sn * K[u][v]) + cs * kk;
            }
    } else if constexpr (FMT == kEuler) {
        const Euler e(r);
        float M[3][3];
        mat3(e.Rx, e.Ry, M);
        mat3(M, e.Rz, R);
    } else if constexpr (FMT == kQuat) {
        const Quat q(r);
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) R[u][v] = (u == v ? 1.0f : 0.0f) + q.ts * q.B[u][v];
    } else {
        const SixD s(r);
#pragma unroll
        for (int v = 0; v < 3; ++v) { R[0][v] = s.b1[v]; R[1][v] = s.b2[v]; R[2][v] = s.b3[v]; }
    }
}

// dL/dr of the rotation rows from G = dL/dR
template <int FMT>
__device__ __forceinline__ void rotation_bwd(const float *r, const float G[3][3], float *dr) {
    if constexpr (FMT == kAxis) {
        const float r0 = r[0], r1 = r[1], r2 = r[2];
        const float th = sqrtf((r0 * r0 + r1 * r1) + r2 * r2);
        const float w[3] = {r0 / th, r1 / th, r2 / th};
        const float K[3][3] = {{0.f, -w[2], w[1]}, {w[2], 0.f, -w[0]}, {-w[1], w[0], 0.f}};
        const float sn = sinf(th), cs0 = cosf(th), cs = 1.0f - cs0;
        float KK[3][3];
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v)
                KK[u][v] = (K[u][0] * K[0][v] + K[u][1] * K[1][v]) + K[u][2] * K[2][v];
        // R = I + sin(th) K + (1 - cos(th)) K^2
        float dth = 0.0f;
        float dK[3][3];
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                dth += G[u][v] * (cs0 * K[u][v] + sn * KK[u][v]);
                // d<G, K K>/dK = G K^T + K^T G
                float gkt = 0.0f, ktg = 0.0f;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    gkt += G[u][q] * K[v][q];
                    ktg += K[q][u] * G[q][v];
                }
                dK[u][v] = sn * G[u][v] + cs * (gkt + ktg);
            }
        const float gw[3] = {dK[2][1] - dK[1][2], dK[0][2] - dK[2][0], dK[1][0] - dK[0][1]};
        const float gww = (gw[0] * w[0] + gw[1] * w[1]) + gw[2] * w[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) dr[c] = (gw[c] - gww * w[c]) / th + dth * w[c];
    } else if constexpr (FMT == kEuler) {
        const Euler e(r);
        float M[3][3], dRz[3][3], dM[3][3], dRy[3][3], dRx[3][3];
        mat3(e.Rx, e.Ry, M);
        mat3_tn(M, G, dRz);
        mat3_nt(G, e.Rz, dM);
        mat3_tn(e.Rx, dM, dRy);
        mat3_nt(dM, e.Ry, dRx);
        const float *s = e.s, *c = e.c;
        dr[0] = ((dRx[2][1] - dRx[1][2]) * c[0]) - ((dRx[1][1] + dRx[2][2]) * s[0]);
        dr[1] = ((dRy[0][2] - dRy[2][0]) * c[1]) - ((dRy[0][0] + dRy[2][2]) * s[1]);
        dr[2] = ((dRz[1][0] - dRz[0][1]) * c[2]) - ((dRz[0][0] + dRz[1][1]) * s[2]);
    } else if constexpr (FMT == kQuat) {
        const Quat Q(r);
        const float qr = Q.q[0], qi = Q.q[1], qj = Q.q[2], qk = Q.q[3];
        float dts = 0.0f, dB[3][3];
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                dts += G[u][v] * Q.B[u][v];
                dB[u][v] = Q.ts * G[u][v];
            }
        const float a01 = dB[0][1] + dB[1][0], a02 = dB[0][2] + dB[2][0], a12 = dB[1][2] + dB[2][1];
        const float s01 = dB[1][0] - dB[0][1], s02 = dB[0][2] - dB[2][0], s12 = dB[2][1] - dB[1][2];
        float dq[4];
        dq[0] = (s01 * qk + s02 * qj) + s12 * qi;
        dq[1] = ((a01 * qj + a02 * qk) + s12 * qr) - 2.0f * qi * (dB[1][1] + dB[2][2]);
        dq[2] = ((a01 * qi + a12 * qk) + s02 * qr) - 2.0f * qj * (dB[0][0] + dB[2][2]);
        dq[3] = ((a02 * qi + a12 * qj) + s01 * qr) - 2.0f * qk * (dB[0][0] + dB[1][1]);
        const float dss2 = -(Q.ts * Q.ts) * dts;  // 2 dL/dss
        float qd = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dq[k] += Q.q[k] * dss2;
            qd += Q.q[k] * dq[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) dr[k] = (dq[k] - qd * Q.q[k]) / Q.n;
    } else {
        const SixD S(r);
        float db1[3], db2[3], t[3], du[3];
        cross3(S.b2, G[2], t);
#pragma unroll
        for (int k = 0; k < 3; ++k) db1[k] = G[0][k] + t[k];
        cross3(G[2], S.b1, t);
#pragma unroll
        for (int k = 0; k < 3; ++k) db2[k] = G[1][k] + t[k];
        const float p2 = S.clamp2 ? 0.0f : dot3(S.b2, db2);
#pragma unroll
        for (int k = 0; k < 3; ++k) du[k] = (db2[k] - p2 * S.b2[k]) / S.d2;
        const float sb = dot3(du, S.b1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dr[3 + k] = du[k] - sb * S.b1[k];
            db1[k] -= sb * S.a2[k] + S.dd * du[k];
        }
        const float p1 = S.clamp1 ? 0.0f : dot3(S.b1, db1);
#pragma unroll
        for (int k = 0; k < 3; ++k) dr[k] = (db1[k] - p1 * S.b1[k]) / S.d1;
    }
}

// The head of one point: branch outputs o (row map of HEAD) -> y, x', s, c, R x.
template <int HEAD>
struct HeadOut {
    float r[6], y[3], n[3], rx[3], s, c;
};

template <int HEAD>
__device__ __forceinline__ void head_forward(const ndpt::f32x16 &Bo, int h, bool has_nr, float x0, float x1,
                                             float x2, HeadOut<HEAD> &o) {
    constexpr RowMap M = row_map(HEAD);
    constexpr int motion = head_motion(HEAD);
    const float t0 = 0.001f * tile_row<M.trn>(Bo, h), t1 = 0.001f * tile_row<M.trn + 1>(Bo, h);
    const float t2 = 0.001f * tile_row<M.trn + 2>(Bo, h);
    const float nrr = tile_row<M.nr>(Bo, h);
    const float rows[6] = {tile_row<0>(Bo, h), tile_row<1>(Bo, h), tile_row<2>(Bo, h),
                           tile_row<3>(Bo, h), tile_row<4>(Bo, h), tile_row<5>(Bo, h)};
#pragma unroll
    for (int k = 0; k < 6; ++k) o.r[k] = k < M.rot ? 0.001f * rows[k] : 0.0f;
    o.c = 0.0f;
    o.rx[0] = o.rx[1] = o.rx[2] = 0.0f;
    if constexpr (motion == kSflow) {
        o.y[0] = x0 + t0; o.y[1] = x1 + t1; o.y[2] = x2 + t2;
    } else {
        float R[3][3];
        rotation<head_format(HEAD)>(o.r, R);
        const float q0 = (R[0][0] * x0 + R[0][1] * x1) + R[0][2] * x2;
        const float q1 = (R[1][0] * x0 + R[1][1] * x1) + R[1][2] * x2;
        const float q2 = (R[2][0] * x0 + R[2][1] * x1) + R[2][2] * x2;
        if constexpr (motion == kSim3) {
            o.c = 0.001f * tile_row<10>(Bo, h) + 1.0f;
            o.rx[0] = q0; o.rx[1] = q1; o.rx[2] = q2;
            o.y[0] = o.c * q0 + t0; o.y[1] = o.c * q1 + t1; o.y[2] = o.c * q2 + t2;
        } else {
            o.y[0] = q0 + t0; o.y[1] = q1 + t1; o.y[2] = q2 + t2;
        }
    }
    o.n[0] = o.y[0]; o.n[1] = o.y[1]; o.n[2] = o.y[2];
    o.s = 0.0f;
    if (has_nr) {
        o.s = 1.0f / (1.0f + expf(-(0.001f * nrr)));
        o.n[0] = x0 + o.s * (o.y[0] - x0);
        o.n[1] = x1 + o.s * (o.y[1] - x1);
        o.n[2] = x2 + o.s * (o.y[2] - x2);
    }
}

}  // namespace ndph
}  // namespace pcr
