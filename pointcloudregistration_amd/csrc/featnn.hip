// a5: exact feature-space 1-NN for batches of cloud pairs + mutual filter.
//
// Reference semantics: Open3D KDTreeFlann SearchKNN(k=1) over Feature.data
// inside registration_ransac_based_on_feature_matching (call sites
// DataPreparation/RANSAC.py:43-52, dip/demo.py:43-52, ngenet/utils/o3d.py:174-180)
// and torch.cdist + min in c2p-net/ngenet/models/vote.py:6-9.  Contract
// (oracle_featnn): argmin_j D_ij, D_ij = sum_k ((double)f_ik - (double)g_jk)^2
// summed sequentially in f64, lowest index on ties.
//
// MI355X design: screen every (row, column) pair of a
// cloud pair with an MFMA distance tile, keep a top-2 per row and per column,
// certify a winner when its top-2 gap exceeds a rigorous bound on the screen's
// error, and recompute every uncertified row / column exactly in f64.
//
// Units (D <= 64: the f16 x3 split screen on v_mfma_f32_32x32x16_f16):
//   featnn_v5.h        operand layout, bounds, argument structs, cross-unit entry points
//   featnn_pack.hip    scale, packed operands, norms, column terms   (v5_prepare)
//   featnn_dual.hip    both directions in one screen                 (feature_match_v5)
//   featnn_row.hip     one direction's rows: featnn_row7 / row8 / row9 (launch_row*)
//   featnn_thresh.hip  featnn_row9's leftover rows from threshold candidates (launch_thresh9)
//   featnn_rescan.hip  exact f64 rescan of the uncertified           (run_rescan)
//   featnn.hip         this file: the mutual path's driver and kernels, the C entry points
//   featnn_f32.hip     64 < D <= 128: augmented f32 operands on v_mfma_f32_32x32x2_f32
// Call paths:
//   pcr_feature_match            v5_prepare -> feature_match_v5's dual screen -> run_rescan
//   pcr_feature_correspondences  v5_prepare -> row screen pass 1 -> run_rescan (rows) -> featmut_jbuild
//                                -> row screen pass 2 -> featmut_resolve -> run_rescan (columns)
//                                -> featmut_corres        (feature_corres_v5 below)
#include "featnn_v5.h"
#include "scan.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>

namespace pcr {
namespace {

// mutual filter + ordered compaction (one block per pair)
__global__ __launch_bounds__(1024) void corres_build(const int32_t *nn12, const int32_t *nn21,
                                                     const int32_t *n_src, const int32_t *n_tgt,
                                                     int Nmax, int Mmax, int mutual, int ransac_n,
                                                     int *scratch, int32_t *corres,
                                                     int32_t *n_corres) {
    const int p = blockIdx.x;
    const int n = count_of(n_src, p, Nmax);
    const int m = count_of(n_tgt, p, Mmax);
    const int32_t *a12 = nn12 + (size_t)p * Nmax;
    const int32_t *a21 = nn21 + (size_t)p * Mmax;
    int *f = scratch + (size_t)p * (Nmax + 1);
    int32_t *co = corres + (size_t)p * Nmax * 2;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int j = a12[i];
        f[i] = (mutual && j >= 0 && j < m && a21[j] == i) ? 1 : 0;
    }
    __syncthreads();
    block_exclusive_scan_1024(f, f, n, false);
    const int total = f[n];
    const bool use_mutual = mutual && total >= 3 * ransac_n;
    if (use_mutual) {
        for (int i = threadIdx.x; i < n; i += 1024) {
            const int pos = f[i];
            if (f[i + 1] != pos) { co[2 * pos] = i; co[2 * pos + 1] = a12[i]; }
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 1024) { co[2 * i] = i; co[2 * i + 1] = a12[i]; }
    }
    if (threadIdx.x == 0) n_corres[p] = use_mutual ? total : n;
}

// J = {nn12[i]} of each pair, ascending (one workgroup per pair).  kLds: the
// flags and their scan in LDS ((Mmax + 1) ints of dynamic LDS), the used flags
// written once, coalesced, for featmut_resolve; else all in the HBM scratch.
template <bool kLds>
__global__ __launch_bounds__(1024) void featmut_jbuild(MutArgs a) {
    extern __shared__ int jsh[];
    const int p = blockIdx.x;
    const int n = count_of(a.n_src, p, a.Nmax), m = count_of(a.n_tgt, p, a.Mmax);
    int *ug = a.used + (size_t)p * (a.Mmax + 1);
    int *u = kLds ? jsh : ug;
    int *ps = kLds ? jsh : a.pos + (size_t)p * (a.Mmax + 1);
    int *jl = a.jlist + (size_t)p * a.Mmax;
    const int32_t *nn = a.nns + (size_t)p * a.Nmax;
    for (int j = threadIdx.x; j < m; j += 1024) u[j] = 0;
    __syncthreads();
    if constexpr (kLds) {
        for (int i = threadIdx.x; i < n; i += 1024) {
            const int j = nn[i];
            if (j >= 0 && j < m) jsh[j] = 1;
        }
        __syncthreads();
        for (int j = threadIdx.x; j < m; j += 1024) ug[j] = jsh[j];
        // in place: flags -> exclusive starts (the scan reads each flag before it
        // writes that position's start; a flag is set iff start[j + 1] > start[j])
        block_exclusive_scan_1024(jsh, jsh, m, false);
        __syncthreads();
        for (int j = threadIdx.x; j < m; j += 1024)
            if (jsh[j + 1] > jsh[j]) jl[jsh[j]] = j;
        if (threadIdx.x == 0) a.nj[p] = jsh[m];
        return;
    }
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int j = nn[i];
        if (j >= 0 && j < m) u[j] = 1;  // plain stores of one value: no race on the result
    }
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += 1024) ps[j] = u[j];
    __syncthreads();
    block_exclusive_scan_1024(ps, ps, m, false);
    for (int j = threadIdx.x; j < m; j += 1024)
        if (u[j]) jl[ps[j]] = j;
    if (threadIdx.x == 0) a.nj[p] = ps[m];
}

// decide each candidate from the pass-2 values, list the undecidable columns
// (once each) for the exact rescan
__global__ __launch_bounds__(256) void featmut_resolve(MutArgs a) {
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = count_of(a.n_src, p, a.Nmax), m = count_of(a.n_tgt, p, a.Mmax);
    if (i >= n) return;
    const size_t oi = (size_t)p * a.Nmax + i;
    const int j = a.nn12[oi];
    int f = 0;
    int *uj = a.used + (size_t)p * (a.Mmax + 1) + j;
    const double e1 = (double)a.e12[oi];  // 0: rescanned (or a zero bound)
    if (j >= 0 && j < m && e1 == 0.0 && (*uj == 0 || *uj == 3)) {
        // J was built from the screened argmins, beside the exact row rescan:
        // a rescanned row's exact argmin j may have no pass-2 values (pass-1
        // certified rows kept the argmin J was built from).  Its exact column
        // argmin decides (listed once: used 0 -> 3)
        f = 2;
        if (atomicCAS(uj, 0, 3) == 0) a.list21[(size_t)p * a.Mmax + atomicAdd(a.cnt21 + p, 1)] = j;
    } else if (j >= 0 && j < m) {
        const size_t oj = (size_t)p * a.Mmax + j;
        const float4 q = a.wq[oj];  // biased values (exact in f64), the bound, the bias
        const double w1 = (double)q.x - (double)q.w, w2 = (double)q.y - (double)q.w, e2 = (double)q.z;
        const double vi = a.v12[oi];
        // slack: the f64 sums of a rescanned value vs the exact real distance
        const double sl = 1e-9 * (__builtin_fabs(w1) + __builtin_fabs(vi));
        bool done = false;
        if (w2 - w1 > 2.0 * (e2 + e1 + sl)) {
            f = (vi <= w1 + e2 + e1 + sl) ? 1 : 0;
            done = true;
        } else if (e1 != 0.0) {
            // the row's screened value is too coarse for this column's gap (the
            // 1-term screen's bound): its exact distance, the oracle's f64 sum in
            // the rescan's units, decides when the gap alone allows
            const float *fr = a.F + oi * a.D, *gr = a.G + oj * a.D;
            double acc = 0.0;
            for (int k = 0; k < a.D; ++k) {
                const double df = (double)fr[k] - (double)gr[k];
                acc = acc + df * df;
            }
            const double sc = (double)__uint_as_float(a.mx[p]);
            const double vx = acc * sc * sc;
            const double slx = 1e-9 * (__builtin_fabs(w1) + __builtin_fabs(vx));
            if (w2 - w1 > 2.0 * (e2 + slx)) {
                f = (vx <= w1 + e2 + slx) ? 1 : 0;
                done = true;
            }
        }
        if (!done) {
            f = 2;
            if (atomicCAS(uj, 1, 2) == 1)
                a.list21[(size_t)p * a.Mmax + atomicAdd(a.cnt21 + p, 1)] = j;
        }
    }
    a.flag[(size_t)p * (a.Nmax + 1) + i] = f;
}

// the flags (undecided ones from the exact column argmin) -> corres_build's
// ordered compaction and fallback (one workgroup per pair)
__global__ __launch_bounds__(1024) void featmut_corres(MutArgs a) {
    const int p = blockIdx.x;
    const int n = count_of(a.n_src, p, a.Nmax), m = count_of(a.n_tgt, p, a.Mmax);
    const int32_t *a12 = a.nn12 + (size_t)p * a.Nmax;
    int *f = a.flag + (size_t)p * (a.Nmax + 1);
    int32_t *co = a.corres + (size_t)p * a.Nmax * 2;
    if (a.mutual) {
        for (int i = threadIdx.x; i < n; i += 1024) {
            const int v = f[i];
            if (v == 2) f[i] = (a.nn21x[(size_t)p * a.Mmax + a12[i]] == i) ? 1 : 0;
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 1024) f[i] = 0;
    }
    (void)m;
    __syncthreads();
    block_exclusive_scan_1024(f, f, n, false);
    const int total = f[n];
    const bool use_mutual = a.mutual && total >= 3 * a.ransac_n;
    if (use_mutual) {
        for (int i = threadIdx.x; i < n; i += 1024) {
            const int pos = f[i];
            if (f[i + 1] != pos) { co[2 * pos] = i; co[2 * pos + 1] = a12[i]; }
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 1024) { co[2 * i] = i; co[2 * i + 1] = a12[i]; }
    }
    if (threadIdx.x == 0) a.n_corres[p] = use_mutual ? total : n;
}

}  // namespace

// column slices of the 3-term screens' list mode: a pair's short list is
// one workgroup per slice -- at 256 pairs one slice (the chip is full), at
// 32 pairs 8 (one block per pair left 224 CUs idle: ~0.2 ms per launch)
static int list_slices(int P) { return std::max(1, std::min(8, 256 / std::max(P, 1))); }

// PCR_FEAT_ROW9=0: the round-6 featnn_row8 1-term passes (A/B; read per call)
static bool feat_row9() {
    const char *e = getenv("PCR_FEAT_ROW9");
    return !(e && e[0] == '0');
}

// a 3-term fallback screen (list mode), in its profile slot
template <bool kIdx>
static int launch_fallback(const RowArgs5 &r, int S, hipStream_t q, int slot) {
    prof_begin(q, slot);
    const int rc = launch_row8<kIdx, false>(r, S, q);
    prof_end(q, slot);
    return rc;
}

// side(q) then main() on s; with PCR_FEAT_BESIDE=1, side(q) on the second
// side stream beside main() on s, joined back into s.  Measured (featnn_bench,
// mutual): 256 pairs 3.42 ms either way, 32 pairs 0.778 beside vs 0.755 ms in
// order -- the 3-term screen and the regroup compete for the same CUs, so the
// default is in order
template <class Side, class Main>
static int beside(hipStream_t s, Side side, Main main) {
    static const bool off = [] {
        const char *e = getenv("PCR_FEAT_BESIDE");
        return !(e && e[0] == '1');
    }();
    hipStream_t q = s;
    hipEvent_t ef = nullptr, ej = nullptr;
    int rc = off ? PCR_OK : side_stream(&q, &ef, &ej, 2);
    if (rc != PCR_OK) return rc;
    if (q != s) {
        PCR_HIP_CHECK(hipEventRecord(ef, s));
        PCR_HIP_CHECK(hipStreamWaitEvent(q, ef, 0));
    }
    if ((rc = side(q)) != PCR_OK) return rc;
    if (q != s) PCR_HIP_CHECK(hipEventRecord(ej, q));
    prof_begin(s, kProfFeatRegroup);
    rc = main();
    prof_end(s, kProfFeatRegroup);
    if (rc != PCR_OK) return rc;
    if (q != s) PCR_HIP_CHECK(hipStreamWaitEvent(s, ej, 0));
    return PCR_OK;
}

// the threshold route behind featnn_row9 (featnn_thresh.hip): on by default,
// PCR_FEAT_THRESH=0 for the 3-term screens of its leftover rows (A/B, parity;
// read per call)
static bool feat_thresh() {
    const char *e = getenv("PCR_FEAT_THRESH");
    return !(e && e[0] == '0');
}

// PCR_FEAT_IMAGE=full: the full 2S + 1 chunk image on the default route too
// (A/B, the parity tests; read per call)
static bool feat_image_full() {
    const char *e = getenv("PCR_FEAT_IMAGE");
    return e && strcmp(e, "full") == 0;
}

// the 1-term screens in front of the 3-term ones (S <= 2): on by default,
// PCR_FEAT_ONE=0 for the round-5 path (A/B, the parity tests; read per call)
static bool feat_one_term() {
    const char *e = getenv("PCR_FEAT_ONE");
    return !(e && e[0] == '0');
}

// ---------------------------------------------------------------------------
// Mutual correspondences without the column screen (feature_corres_v5).
//
// corres_build reads nn21 only at j = nn12[i], and nn12 hits ~half of the
// targets, so the column direction is screened only for those: pass 1 screens
// the rows (F against every G column, a top-2 per row with the column-tile
// index packed into the value: 3 VALU per distance instead of dual7's ~6.6),
// the uncertified rows are rescanned exactly, then pass 2 screens the rows
// J = {nn12[i]} of G against every F column keeping top-2 VALUES only (2 VALU
// per distance, no index), and the candidate i of column j = nn12[i] is decided
// from values:
//   pass 2 certifies column j when its top-2 gap exceeds 2 (e2 + e1_i), e2 the
//   screen's bound for column j, e1_i that of row i's own value v_i (its pass-1
//   b1 with the code bits' perturbation, or 0 when the row was rescanned); then
//   the exact column argmin w has the screen minimum w1, D_w <= w1 + e2 and
//   every other row is >= w2 - e2, so i is mutual iff v_i <= w1 + e2 + e1_i.
//   A column that cannot be decided is rescanned exactly (featnn_rescan3,
//   direction 1) and its candidates compared with that argmin.
// The result is the same set corres_build forms from the exact nn12 / nn21.
// ---------------------------------------------------------------------------

// One pass of the row screens on s (kIdx: pass 1), timed in `slot`:
//   use9    featnn_row9's sweep, then the 3-term screen of the rows it listed
//           (in `slot_fb`) beside the regroup and finish, whose failing rows go
//           to llist / lcount;
//   one     featnn_row8's 1-term pass, then the 3-term screen of the rows it listed;
//   S <= 2  the 3-term featnn_row8 alone;  S > 2  featnn_row7.
// r: the pass's screen; fb: its 3-term fallback over the list r fills.
// th (use9 only, null with PCR_FEAT_THRESH=0): the threshold route instead of
// the 3-term screen -- the finish appends its failing rows to the sweep's own
// list, then featnn_thresh9 + featnn_exact_cand settle that list (in `slot_fb`),
// all in order on s; th->llist / lcount take the rows they leave (pass 1).
template <bool kIdx>
static int run_pass(const RowArgs5 &r, const RowArgs5 &fb, int S, bool one, bool use9, int slot, int slot_fb,
                    int *llist, int *lcount, hipStream_t s, const RowArgs5 *th = nullptr) {
    int rc;
    prof_begin(s, slot);
    if (use9) {
        PCR_HIP_CHECK(hipMemsetAsync(r.bcnt, 0, sizeof(int) * (size_t)r.P * (r.ntc / 2), s));  // a count per step
        if ((rc = launch_row9<kIdx>(r, S, s)) != PCR_OK) return rc;
        prof_end(s, slot);
        if (th) {
            RowArgs5 rg = r;
            rg.llist = r.list; rg.lcount = r.count; rg.thresh = 1;
            prof_begin(s, kProfFeatRegroup);
            rc = launch_regroup9<kIdx>(rg, S, s);
            prof_end(s, kProfFeatRegroup);
            if (rc != PCR_OK) return rc;
            prof_begin(s, slot_fb);
            rc = launch_thresh9<kIdx>(*th, S, s);
            prof_end(s, slot_fb);
            return rc;
        }
        RowArgs5 rg = r;
        rg.llist = llist; rg.lcount = lcount;
        return beside(s, [&](hipStream_t q) { return launch_fallback<kIdx>(fb, S, q, slot_fb); },
                      [&] { return launch_regroup9<kIdx>(rg, S, s); });
    }
    if (one) rc = launch_row8<kIdx, true>(r, S, s);
    else if (S <= 2) rc = launch_row8<kIdx, false>(r, S, s);
    else rc = launch_row7<kIdx>(r, S, s);
    if (rc != PCR_OK) return rc;
    prof_end(s, slot);
    return one ? launch_fallback<kIdx>(fb, S, s, slot_fb) : PCR_OK;
}

// the 3-term screen (featnn_row8 list mode, row-block-major, fsl column
// slices) of the rows the 1-term screen r listed; what it cannot certify
// either goes to list / count
static RowArgs5 fallback_args(RowArgs5 r, int *list, int *count, int fbdiag, int fsl) {
    r.rlist = r.list; r.rcount = r.count;
    r.list = list; r.count = count;
    r.fbdiag = fbdiag; r.rbmajor = 1; r.csl = fsl;
    return r;
}

// the mutual path (see above): nn12 and the correspondences without the
// column screen of every target
static int feature_corres_v5(const float *F, const float *G, int P, int Nmax, int Mmax, int D,
                             const int32_t *n_src, const int32_t *n_tgt, int mutual, int ransac_n,
                             int32_t *nn12, int32_t *corres, int32_t *n_corres, hipStream_t s) {
    // The route, ahead of the prepare (it decides the images' layout): from S,
    // the tile counts as v5_prepare pads them, and the hooks.
    const int S0 = cdiv(D, 16), rg = std::max(kRow8G, kRow9G);
    const int ntn0 = cdiv(cdiv(Nmax, 32), 16) * 16, ntm0 = cdiv(cdiv(Mmax, 32), rg) * rg;
    const bool one = S0 <= 2 && feat_one_term();
    // (the regroup keeps a pair's per-step prefix in LDS)
    const bool use9 = one && feat_row9() && std::max(ntm0, ntn0) / 2 <= kRegroupMaxSteps;
    const bool thresh = use9 && feat_thresh();
    // featnn_row9 with the threshold route reads the images' hi segment only:
    // the compact image (S chunks per tile); every other route reads lo / norms
    const bool compact = thresh && !feat_image_full();
    V5Buf v;
    int rc = v5_prepare(F, G, P, Nmax, Mmax, D, n_src, n_tgt, s, v, compact);
    if (rc != PCR_OK) return rc;
    const int ntn = v.ntn, ntm = v.ntm;
    PCR_REQUIRE(v.S == S0 && ntn == ntn0 && ntm == ntm0, PCR_ERR_ARG, "feature_corres: tile counts");
    // scratch: v12 [P][Nmax] f64 | e12 [P][Nmax] f32 | wq [P][Mmax] float4 | used, pos
    // [P][Mmax+1] | jlist, nn21x [P][Mmax] | flag [P][Nmax+1] | nj, zero [P] | nns [P][Nmax]
    const size_t pn = (size_t)P * Nmax, pm = (size_t)P * Mmax;
    // featnn_row9's buckets (a pass's rows by winning step): 4x a bucket's mean
    // row count, at least 64 rows; a fuller bucket sends rows to the 3-term screen
    const int nst1 = ntm / 2, nst2 = ntn / 2;
    const int cap1 = std::max(64, 4 * cdiv(Nmax, nst1)), cap2 = std::max(64, 4 * cdiv(Mmax, nst2));
    const size_t pb = (size_t)P * std::max(nst1, nst2);
    const size_t pl = (size_t)P * std::max((size_t)nst1 * cap1, (size_t)nst2 * cap2);
    const size_t pr = (size_t)P * std::max(Nmax, Mmax);
    const int fsl = list_slices(P);
    const size_t pt = fsl > 1 ? (size_t)fsl * pr : 0;  // the sliced 3-term screens' partials
    MutArgs ma;
    double *v12;
    float *e12;
    float4 *wq;
    int *nn21x, *zero, *bcnt, *cand;
    int32_t *nns;
    uint4 *blist, *rec, *part;
    WsLayout l;  // pcr_featmut_debug_copy's readers go by these offsets
    l.take(v12, pn); l.take(e12, pn);
    l.take(wq, pm);  // 16-byte aligned
    l.take(ma.used, pm + P); l.take(ma.pos, pm + P);
    l.take(ma.jlist, pm); l.take(nn21x, pm);
    l.take(ma.flag, pn + P);
    l.take(ma.nj, P); l.take(zero, P);
    l.take(nns, pn);
    l.take(blist, pl);  // 16-byte aligned
    l.take(rec, pr); l.take(part, pt);
    l.take(bcnt, pb);
    l.take(cand, thresh ? pr * kThreshK : 0);  // featnn_thresh9's candidate slots
    bool fresh = false;
    // + 32: the tail also keeps 16 bytes per round-up (wq, blist) beyond the layout's own padding
    PCR_REQUIRE(workspace_bind(kWsFeatMutual, l, kWsSlack + 32, &fresh), PCR_ERR_NOMEM, "feature_corres: %s",
                pcr_last_error());
    // a constant zero count per pair (read only): cleared when the slot is new
    // or was last used for fewer pairs
    static thread_local const void *z_ptr = nullptr;
    static thread_local int z_cnt = 0;
    if (fresh || z_ptr != (const void *)zero || z_cnt < P) {
        PCR_HIP_CHECK(hipMemsetAsync(zero, 0, sizeof(int) * (size_t)P, s));
        z_ptr = zero;
        z_cnt = P;
    }
    ma.nn12 = nn12; ma.n_src = n_src; ma.n_tgt = n_tgt; ma.Nmax = Nmax; ma.Mmax = Mmax;
    ma.mutual = mutual; ma.ransac_n = ransac_n; ma.Kt = 16 * v.NX; ma.D = D; ma.ntm = ntm;
    ma.v12 = v12; ma.e12 = e12; ma.wq = wq; ma.fmax = v.fmax;
    ma.nns = v.S <= 2 ? nns : nn12;  // featnn_row7 (S > 2) writes no copy
    ma.F = F; ma.G = G; ma.mx = v.mx;
    ma.list21 = v.list21; ma.cnt21 = v.cnt21; ma.nn21x = nn21x;
    ma.corres = corres; ma.n_corres = n_corres;
    // pass 1: F rows x all G columns (nrb: each launcher sets its own)
    RowArgs5 r;
    r.Ap = v.Ap; r.Bp = v.Bp; r.ich = v.ich; r.rnr = v.fnr; r.cmax = v.gmax; r.n_rows = n_src; r.n_cols = n_tgt;
    r.rlist = nullptr; r.rcount = nullptr; r.P = P; r.Rmax = Nmax; r.Cmax = Mmax; r.ntr = ntn;
    r.ntc = ntm; r.nrb = 0; r.D = D; r.ctbits = 1;
    while ((1 << r.ctbits) < ntm) ++r.ctbits;
    r.nn = nn12; r.v = v12; r.e = e12;
    // a 1-term screen lists the rows it leaves to the 3-term one
    r.list = one ? v.fbl12 : v.list12; r.count = one ? v.fbc12 : v.cnt12;
    r.wq = nullptr;
    r.Xr = F; r.sc = v.mx; r.role = 0; r.cs = v.sp.cs;  // featnn_row8 builds its rows from F
    r.cemax = v.gemax; r.nns = nns; r.fbdiag = 0; r.rbmajor = 0;
    r.rre = v.fre; r.bcnt = bcnt; r.blist = blist; r.bcap = cap1; r.rec = rec;
    r.cct = v.gct; r.rct = v.fct; r.cbias = v.cbias;
    r.csl = 1; r.part = part; r.llist = nullptr; r.lcount = nullptr;
    r.thresh = 0; r.cand = cand; r.used = nullptr; r.Xc = G; r.fbctr = nullptr; r.dbg = 0;
    auto prep_hook = [&](int at) -> int {
        if (!prep_event || prep_at != at) return PCR_OK;
        PCR_HIP_CHECK(hipEventRecord(prep_event, s));
        const int hrc = prep_fn ? prep_fn(prep_ctx) : PCR_OK;
        if (hrc == PCR_OK) prep_fn = nullptr;
        return hrc;
    };
    if ((rc = prep_hook(2)) != PCR_OK) return rc;
    // (the regroup's failing rows go to the exact rescan's list: the 3-term screen runs beside it)
    // the threshold route's view of a pass: the rows r lists; what it leaves goes to list / count
    auto thresh_args = [](RowArgs5 t, int *list, int *count) {
        t.rlist = t.list; t.rcount = t.count;
        t.llist = list; t.lcount = count;
        return t;
    };
    const RowArgs5 t1 = thresh_args(r, v.list12, v.cnt12);
    rc = run_pass<true>(r, fallback_args(r, v.list12, v.cnt12, 1, fsl), v.S, one, use9, kProfFeatScreen,
                        kProfFeatScreen1b, v.list12, v.cnt12, s, thresh ? &t1 : nullptr);
    if (rc != PCR_OK) return rc;
    if ((rc = prep_hook(1)) != PCR_OK) return rc;
    RescanArgs5 ra = rescan_args(F, G, n_src, n_tgt, Nmax, Mmax, D);
    ra.list12 = v.list12; ra.list21 = v.list21; ra.cnt12 = v.cnt12; ra.cnt21 = zero;
    ra.nn12 = nn12; ra.nn21 = nn21x;
    ra.v12 = v12; ra.e12 = e12; ra.mx = v.mx; ra.T = v.sp.T;
    // mutual: the exact rescan of the uncertified rows runs on a side stream
    // beside J's build and pass 2, which read none of its results (J from the
    // screened argmins; featmut_resolve, after the join, sends a rescanned
    // row's new argmin outside J to the exact column rescan).  Large batches
    // only: at 32-128 pairs it gained nothing.  The side stream is the
    // pipeline's prep stream (its grid builds are enqueued first, prep_fn)
    hipStream_t rs = s;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    if (mutual && P >= 192) {
        rc = side_stream(&rs, &ev_fork, &ev_join, 1);
        if (rc != PCR_OK) return rc;
        PCR_HIP_CHECK(hipEventRecord(ev_fork, s));
        PCR_HIP_CHECK(hipStreamWaitEvent(rs, ev_fork, 0));
    }
    rc = run_rescan(ra, P, D, rs);
    if (rc != PCR_OK) return rc;
    if (rs != s) PCR_HIP_CHECK(hipEventRecord(ev_join, rs));
    if (mutual) {
        // the LDS form when its dynamic (Mmax + 1) ints fit beside the kernel's
        // static LDS (the block scan's wave totals) in 64 KB
        const size_t jsm = sizeof(int) * ((size_t)Mmax + 1);
        static size_t jstatic = [] {
            hipFuncAttributes fa{};
            return hipFuncGetAttributes(&fa, (const void *)featmut_jbuild<true>) == hipSuccess
                       ? fa.sharedSizeBytes : (size_t)1024;
        }();
        if (jsm + jstatic <= 64 * 1024) {
            PCR_HIP_CHECK(hipFuncSetAttribute((const void *)featmut_jbuild<true>,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
            hipLaunchKernelGGL(featmut_jbuild<true>, dim3(P), dim3(1024), jsm, s, ma);
        } else {
            hipLaunchKernelGGL(featmut_jbuild<false>, dim3(P), dim3(1024), 0, s, ma);
        }
        PCR_LAUNCH_CHECK();
        // pass 2: the rows J of G (B-role fragments as the register operand) x all F
        // columns (A-role fragments streamed): the same products, values only
        RowArgs5 r2 = r;
        r2.Ap = v.Bp; r2.Bp = v.Ap; r2.rnr = v.gnr; r2.cmax = v.fmax; r2.n_rows = n_tgt;
        r2.n_cols = n_src; r2.rlist = ma.jlist; r2.rcount = ma.nj; r2.Rmax = Mmax; r2.Cmax = Nmax;
        r2.ntr = ntm; r2.ntc = ntn;
        r2.nn = nullptr; r2.v = nullptr; r2.e = nullptr;
        // values only; the columns whose gap the 1-term screen cannot use go to the 3-term
        r2.list = one ? v.fbl21 : nullptr; r2.count = one ? v.fbc21 : nullptr;
        r2.nns = nullptr;
        r2.wq = wq;
        r2.Xr = G; r2.sc = v.mx; r2.role = 1; r2.cs = v.sp.cs;
        r2.cemax = v.femax;
        const RowArgs5 r2b = fallback_args(r2, nullptr, nullptr, 2, fsl);
        if (use9) { r2.rre = v.gre; r2.bcap = cap2; r2.cct = v.fct; r2.rct = v.gct; }
        // (no list for the finish: the resolve sends an undecided column to the exact column rescan)
        // (the threshold route: the exact argmin of a settled column goes to nn21x, its flag to 2)
        RowArgs5 t2 = thresh_args(r2, nullptr, nullptr);
        t2.nn = nn21x; t2.used = ma.used; t2.Xc = F;
        rc = run_pass<false>(r2, r2b, v.S, one, use9, kProfFeatScreen2, kProfFeatScreen2b, nullptr, nullptr, s,
                             thresh ? &t2 : nullptr);
        if (rc != PCR_OK) return rc;
        if (rs != s) PCR_HIP_CHECK(hipStreamWaitEvent(s, ev_join, 0));
        hipLaunchKernelGGL(featmut_resolve, dim3(cdiv(Nmax, 256), P), dim3(256), 0, s, ma);
        PCR_LAUNCH_CHECK();
        RescanArgs5 rb = rescan_args(F, G, n_src, n_tgt, Nmax, Mmax, D);
        rb.list12 = v.list12; rb.list21 = v.list21; rb.cnt12 = zero; rb.cnt21 = v.cnt21;
        rb.nn12 = nn12; rb.nn21 = nn21x;
        rc = run_rescan(rb, P, D, s);
        if (rc != PCR_OK) return rc;
    }
    hipLaunchKernelGGL(featmut_corres, dim3(P), dim3(1024), 0, s, ma);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

int corres_impl(const int32_t *nn12, const int32_t *nn21, const int32_t *n_src,
                const int32_t *n_tgt, int P, int Nmax, int Mmax, int mutual, int ransac_n,
                int32_t *corres, int32_t *n_corres, hipStream_t s);

int feature_corres_impl(const float *F, const float *G, int P, int Nmax, int Mmax, int D,
                        const int32_t *n_src, const int32_t *n_tgt, int mutual, int ransac_n,
                        int32_t *nn12, int32_t *corres, int32_t *n_corres, hipStream_t s) {
    PCR_REQUIRE(D >= 1 && D <= 128, PCR_ERR_ARG, "feature_corres: D=%d unsupported (1..128)", D);
    if (D <= 64)
        return feature_corres_v5(F, G, P, Nmax, Mmax, D, n_src, n_tgt, mutual, ransac_n, nn12, corres,
                                 n_corres, s);
    // 64 < D <= 128: both directions from the f32 screen, then the filter
    int32_t *nn21 = (int32_t *)workspace(kWsFeatNn21, sizeof(int32_t) * (size_t)P * Mmax + 64);
    PCR_REQUIRE(nn21, PCR_ERR_NOMEM, "feature_corres: %s", pcr_last_error());
    int rc = feature_match_f32(F, G, P, Nmax, Mmax, D, n_src, n_tgt, nn12, nn21, s);
    if (rc != PCR_OK) return rc;
    return corres_impl(nn12, nn21, n_src, n_tgt, P, Nmax, Mmax, mutual, ransac_n, corres, n_corres, s);
}

int feature_match_impl(const float *F, const float *G, int P, int Nmax, int Mmax, int D,
                       const int32_t *n_src, const int32_t *n_tgt, int32_t *nn12, int32_t *nn21,
                       hipStream_t s) {
    PCR_REQUIRE(D >= 1 && D <= 128, PCR_ERR_ARG, "feature_match: D=%d unsupported (1..128)", D);
    if (D <= 64) return feature_match_v5(F, G, P, Nmax, Mmax, D, n_src, n_tgt, nn12, nn21, s);
    return feature_match_f32(F, G, P, Nmax, Mmax, D, n_src, n_tgt, nn12, nn21, s);
}

int corres_impl(const int32_t *nn12, const int32_t *nn21, const int32_t *n_src,
                const int32_t *n_tgt, int P, int Nmax, int Mmax, int mutual, int ransac_n,
                int32_t *corres, int32_t *n_corres, hipStream_t s) {
    int *scratch = (int *)workspace(kWsCorres, sizeof(int) * (size_t)P * (Nmax + 1));
    PCR_REQUIRE(scratch, PCR_ERR_NOMEM, "corres: %s", pcr_last_error());
    hipLaunchKernelGGL(corres_build, dim3(P), dim3(1024), 0, s, nn12, nn21, n_src, n_tgt, Nmax, Mmax,
                       mutual, ransac_n, scratch, corres, n_corres);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

}  // namespace pcr

extern "C" int pcr_feature_match(const float *src_feat, const float *tgt_feat, int32_t P,
                                 int32_t Nmax, int32_t Mmax, int32_t D, const int32_t *n_src,
                                 const int32_t *n_tgt, int32_t *nn12, int32_t *nn21,
                                 pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(P >= 0 && Nmax >= 0 && Mmax >= 0, PCR_ERR_ARG, "feature_match: negative size");
    if (P == 0 || Nmax == 0 || Mmax == 0) return PCR_OK;
    PCR_REQUIRE(src_feat && tgt_feat && nn12 && nn21, PCR_ERR_ARG, "feature_match: null pointer");
    PCR_REQUIRE(P <= 65535, PCR_ERR_ARG, "feature_match: P=%d > 65535", P);
    return pcr::feature_match_impl(src_feat, tgt_feat, P, Nmax, Mmax, D, n_src, n_tgt, nn12, nn21,
                                   pcr::as_stream(stream));
}

extern "C" int pcr_feature_correspondences(const float *src_feat, const float *tgt_feat, int32_t P,
                                           int32_t Nmax, int32_t Mmax, int32_t D, const int32_t *n_src,
                                           const int32_t *n_tgt, int32_t mutual_filter, int32_t ransac_n,
                                           int32_t *nn12, int32_t *corres, int32_t *n_corres,
                                           pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(P >= 0 && Nmax >= 0 && Mmax >= 0, PCR_ERR_ARG, "feature_corres: negative size");
    if (P == 0 || Nmax == 0) return PCR_OK;
    PCR_REQUIRE(src_feat && tgt_feat && nn12 && corres && n_corres, PCR_ERR_ARG,
                "feature_corres: null pointer");
    PCR_REQUIRE(P <= 65535, PCR_ERR_ARG, "feature_corres: P=%d > 65535", P);
    hipStream_t s = pcr::as_stream(stream);
    if (Mmax == 0) {  // no target: nn12 = 0 (the reference loop never runs), no mutual pair
        PCR_HIP_CHECK(hipMemsetAsync(nn12, 0, sizeof(int32_t) * (size_t)P * Nmax, s));
        int32_t *nn21 = (int32_t *)pcr::workspace(pcr::kWsFeatNn21, 64);
        PCR_REQUIRE(nn21, PCR_ERR_NOMEM, "feature_corres: %s", pcr_last_error());
        return pcr::corres_impl(nn12, nn21, n_src, n_tgt, P, Nmax, 0, mutual_filter, ransac_n, corres,
                                n_corres, s);
    }
    return pcr::feature_corres_impl(src_feat, tgt_feat, P, Nmax, Mmax, D, n_src, n_tgt, mutual_filter,
                                    ransac_n, nn12, corres, n_corres, s);
}

// debug: copy the mutual path's scratch (v12 | e12 | wq (16-B aligned) | used | pos | jlist |
// nn21x | flag | nj, feature_corres_v5's layout) of the last call to dst
extern "C" int pcr_featmut_debug_copy(void *dst, int64_t bytes, pcr_stream_t stream) {
    pcr::clear_error();
    void *src = pcr::workspace(pcr::kWsFeatMutual, 16);
    PCR_REQUIRE(src && dst && bytes >= 0, PCR_ERR_ARG, "featmut_debug_copy: bad arguments");
    PCR_HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, pcr::as_stream(stream)));
    return PCR_OK;
}

extern "C" int pcr_correspondences(const int32_t *nn12, const int32_t *nn21, int32_t P,
                                   int32_t Nmax, int32_t Mmax, const int32_t *n_src,
                                   const int32_t *n_tgt, int32_t mutual_filter, int32_t ransac_n,
                                   int32_t *corres, int32_t *n_corres, pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(P >= 0 && Nmax >= 0 && Mmax >= 0, PCR_ERR_ARG, "correspondences: negative size");
    if (P == 0) return PCR_OK;
    PCR_REQUIRE(nn12 && nn21 && corres && n_corres, PCR_ERR_ARG, "correspondences: null pointer");
    return pcr::corres_impl(nn12, nn21, n_src, n_tgt, P, Nmax, Mmax, mutual_filter, ransac_n,
                            corres, n_corres, pcr::as_stream(stream));
}
