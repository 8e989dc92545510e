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
//   featnn_v5.h        operand layout, bounds, argument structs, the per-cloud sides (V5Buf),
//                      cross-unit entry points
//   featnn_route.h     host only: the route's constants, the tile padding, the PCR_FEAT_* hooks (feat_route)
//   featnn_pack.hip    scale, packed operands, norms, column terms   (v5_prepare)
//   featnn_dual.hip    both directions in one screen                 (feature_match_v5)
//   featnn_row.hip     one direction's rows: featnn_row7 / row8 / row9 (launch_row*)
//   featnn_thresh.hip  featnn_row9's leftover rows from threshold candidates (launch_thresh9)
//   featnn_rescan.hip  exact f64 rescan of the uncertified           (run_rescan)
//   featnn.hip         this file: the mutual path's driver and kernels, the C entry points
//   featnn_f32.hip     64 < D <= 128: augmented f32 operands on v_mfma_f32_32x32x2_f32
// Call paths:
//   pcr_feature_match            v5_prepare -> feature_match_v5's dual screen -> run_rescan
//   pcr_feature_correspondences  feat_route -> v5_prepare -> row screen pass 1 (screen_args, run_pass)
//                                -> run_rescan (rows) -> featmut_jbuild -> row screen pass 2 (the sides
//                                exchanged) -> featmut_resolve -> run_rescan (columns) -> featmut_corres
//                                (feature_corres_v5 below)
#include "featnn_v5.h"
#include "scan.h"
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
//
// The driver: feat_route (featnn_route.h) decides the route, v5_prepare packs
// both clouds into V5Buf::side[2], and a pass in direction dir is the rows of
// side[dir] against the columns of side[1 - dir] (screen_args) with that pass's
// outputs -- pass 2 is pass 1 with the sides exchanged.
// ---------------------------------------------------------------------------

// what a pass writes, and the scratch both passes share
struct PassIO {
    int32_t *nn = nullptr, *nns = nullptr;  // pass 1: the screened argmin and its copy for featmut_jbuild,
    double *v = nullptr;                    // its value and error bound
    float *e = nullptr;
    float4 *wq = nullptr;                           // pass 2: top-2 values of its rows,
    const int *rlist = nullptr, *rcount = nullptr;  // the list J
    int *bcnt = nullptr;                    // featnn_row9's bucket counts and entries,
    uint4 *blist = nullptr, *rec = nullptr, *part = nullptr;  // the regroup's records, the slices' partials
    int *cand = nullptr;                    // featnn_thresh9's candidate slots
};

// featnn_row9's buckets (a pass's rows by winning step): 4x a bucket's mean
// row count, at least 64 rows; a fuller bucket sends rows to the 3-term screen
static int bucket_cap(const V5Side &row, const V5Side &col) { return std::max(64, 4 * cdiv(row.Nmax, col.nt / 2)); }

// The screen of one pass: the rows of side[dir] (register operand, role dir)
// against every column of side[1 - dir].  The only place RowArgs5 is filled
// field by field; what is not set keeps its default (nrb: each launcher sets
// its own).
static RowArgs5 screen_args(const V5Buf &v, int dir, const FeatRoute &rt, const PassIO &o) {
    const V5Side &row = v.side[dir], &col = v.side[1 - dir];
    RowArgs5 r;
    r.Ap = row.Xp; r.Bp = col.Xp; r.ich = v.ich;
    r.rnr = row.nr; r.cmax = col.nmax; r.cemax = col.emax;
    r.n_rows = row.n; r.n_cols = col.n;
    r.P = v.P; r.Rmax = row.Nmax; r.Cmax = col.Nmax; r.ntr = row.nt; r.ntc = col.nt; r.D = v.D;
    // the column-tile code in pass 1's values (G's tiles); pass 2 keeps values only and carries the same width
    r.ctbits = 1;
    while ((1 << r.ctbits) < v.side[1].nt) ++r.ctbits;
    r.Xr = row.X; r.Xc = col.X; r.sc = v.mx; r.role = dir; r.cs = v.sp.cs;  // featnn_row8 builds its rows from the cloud
    r.rre = row.re; r.rct = row.ct; r.cct = col.ct; r.cbias = v.cbias;
    r.rlist = o.rlist; r.rcount = o.rcount;
    r.nn = o.nn; r.nns = o.nns; r.v = o.v; r.e = o.e; r.wq = o.wq;
    // a 1-term screen lists the rows it leaves to the 3-term one; the 3-term screen alone lists pass 1's
    // rows for the exact rescan and nothing in pass 2 (values only: the resolve decides)
    r.list = rt.one ? (dir ? v.fbl21 : v.fbl12) : (dir ? nullptr : v.list12);
    r.count = rt.one ? (dir ? v.fbc21 : v.fbc12) : (dir ? nullptr : v.cnt12);
    r.bcnt = o.bcnt; r.bcap = bucket_cap(row, col); r.blist = o.blist; r.rec = o.rec;
    r.csl = 1; r.part = o.part; r.cand = o.cand;
    return r;
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

// the threshold route's view of a pass: the rows r lists; what it leaves goes to list / count
static RowArgs5 thresh_args(RowArgs5 t, int *list, int *count) {
    t.rlist = t.list; t.rcount = t.count;
    t.llist = list; t.lcount = count;
    return t;
}

// One pass as run_pass takes it: the screen r, its 3-term fallback view fb and
// its threshold view th (the table at RowArgs5), the profile slots of the screen
// and of whichever settles its list, and where the rows go that no screen
// settles -- pass 1: the exact rescan's list; pass 2: nowhere, the resolve sends
// an undecided column to the exact column rescan
struct Pass {
    RowArgs5 r, fb, th;
    int slot, slot_fb;
    int *list, *count;
};
static Pass make_pass(const RowArgs5 &r, int dir, const FeatRoute &rt, int *list, int *count) {
    return {r, fallback_args(r, list, count, dir + 1, rt.fsl), thresh_args(r, list, count),
            dir ? kProfFeatScreen2 : kProfFeatScreen, dir ? kProfFeatScreen2b : kProfFeatScreen1b, list, count};
}

// a 3-term fallback screen (list mode), in its profile slot
template <bool kIdx>
static int launch_fallback(const RowArgs5 &r, int S, hipStream_t q, int slot) {
    prof_begin(q, slot);
    const int rc = launch_row8<kIdx, false>(r, S, q);
    prof_end(q, slot);
    return rc;
}

// One pass of the row screens, in order on s (kIdx: pass 1), timed in p.slot:
//   use9, thresh   featnn_row9's sweep; the regroup and finish, which appends its
//                  failing rows to the sweep's own list; featnn_thresh9 +
//                  featnn_exact_cand settle that list (in p.slot_fb)
//   use9           the sweep; the 3-term screen of the rows it listed (p.slot_fb);
//                  the regroup and finish, whose failing rows go to p.list
//   one            featnn_row8's 1-term pass, then the 3-term screen of the rows it listed
//   S <= 2         the 3-term featnn_row8 alone;  S > 2  featnn_row7
template <bool kIdx>
static int run_pass(const FeatRoute &rt, const Pass &p, hipStream_t s) {
    const int S = rt.S;
    int rc;
    prof_begin(s, p.slot);
    if (rt.use9) {
        PCR_HIP_CHECK(hipMemsetAsync(p.r.bcnt, 0, sizeof(int) * (size_t)p.r.P * (p.r.ntc / 2), s));  // a count per step
        if ((rc = launch_row9<kIdx>(p.r, S, s)) != PCR_OK) return rc;
        prof_end(s, p.slot);
        RowArgs5 rg = p.r;
        if (rt.thresh) {
            rg.llist = p.r.list; rg.lcount = p.r.count; rg.thresh = 1;
        } else {
            rg.llist = p.list; rg.lcount = p.count;
            if ((rc = launch_fallback<kIdx>(p.fb, S, s, p.slot_fb)) != PCR_OK) return rc;
        }
        prof_begin(s, kProfFeatRegroup);
        rc = launch_regroup9<kIdx>(rg, S, s);
        prof_end(s, kProfFeatRegroup);
        if (rc != PCR_OK || !rt.thresh) return rc;
        prof_begin(s, p.slot_fb);
        rc = launch_thresh9<kIdx>(p.th, S, s);
        prof_end(s, p.slot_fb);
        return rc;
    }
    if (rt.one) rc = launch_row8<kIdx, true>(p.r, S, s);
    else if (S <= 2) rc = launch_row8<kIdx, false>(p.r, S, s);
    else rc = launch_row7<kIdx>(p.r, S, s);
    if (rc != PCR_OK) return rc;
    prof_end(s, p.slot);
    return rt.one ? launch_fallback<kIdx>(p.fb, S, s, p.slot_fb) : PCR_OK;
}

// the mutual path (see above): nn12 and the correspondences without the
// column screen of every target
static int feature_corres_v5(const float *F, const float *G, int P, int Nmax, int Mmax, int D,
                             const int32_t *n_src, const int32_t *n_tgt, int mutual, int ransac_n,
                             int32_t *nn12, int32_t *corres, int32_t *n_corres, hipStream_t s) {
    const FeatRoute rt = feat_route(P, Nmax, Mmax, D);  // ahead of the prepare: it decides the images' layout
    V5Buf v;
    int rc = v5_prepare(F, G, P, Nmax, Mmax, D, n_src, n_tgt, s, v, rt.compact);
    if (rc != PCR_OK) return rc;
    const V5Side &f = v.side[0], &g = v.side[1];
    // scratch: v12 [P][Nmax] f64 | e12 [P][Nmax] f32 | wq [P][Mmax] float4 | used, pos
    // [P][Mmax+1] | jlist, nn21x [P][Mmax] | flag [P][Nmax+1] | nj, zero [P] | nns [P][Nmax]
    // | featnn_row9's buckets | records | slice partials | bucket counts | candidates
    const size_t pn = (size_t)P * Nmax, pm = (size_t)P * Mmax;
    const int nst1 = g.nt / 2, nst2 = f.nt / 2;  // column steps of pass 1 / pass 2
    const size_t pb = (size_t)P * std::max(nst1, nst2);
    const size_t pl = (size_t)P * std::max((size_t)nst1 * bucket_cap(f, g), (size_t)nst2 * bucket_cap(g, f));
    const size_t pr = (size_t)P * std::max(Nmax, Mmax);
    const size_t pt = rt.fsl > 1 ? (size_t)rt.fsl * pr : 0;  // the sliced 3-term screens' partials
    MutArgs ma;
    PassIO o1, o2;
    int *nn21x, *zero;
    WsLayout l;  // tests/featscreen_cases.py mut_scratch reads by these offsets (pcr_featmut_debug_copy)
    l.take(o1.v, pn); l.take(o1.e, pn);
    l.take(o2.wq, pm);  // 16-byte aligned
    l.take(ma.used, pm + P); l.take(ma.pos, pm + P);
    l.take(ma.jlist, pm); l.take(nn21x, pm);
    l.take(ma.flag, pn + P);
    l.take(ma.nj, P); l.take(zero, P);
    l.take(o1.nns, pn);
    l.take(o1.blist, pl);  // 16-byte aligned
    l.take(o1.rec, pr); l.take(o1.part, pt);
    l.take(o1.bcnt, pb);
    l.take(o1.cand, rt.thresh ? pr * kThreshK : 0);  // featnn_thresh9's candidate slots
    bool fresh = false;
    // + 32: the tail also keeps 16 bytes per round-up (wq, blist) beyond the layout's own padding
    PCR_REQUIRE(workspace_bind(kWsFeatMutual, l, kWsSlack + 32, &fresh), PCR_ERR_NOMEM, "feature_corres: %s",
                pcr_last_error());
    o1.nn = nn12;
    o2.rlist = ma.jlist; o2.rcount = ma.nj;
    o2.blist = o1.blist; o2.rec = o1.rec; o2.part = o1.part; o2.bcnt = o1.bcnt; o2.cand = o1.cand;
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
    ma.mutual = mutual; ma.ransac_n = ransac_n; ma.Kt = 16 * v.NX; ma.D = D; ma.ntm = g.nt;
    ma.v12 = o1.v; ma.e12 = o1.e; ma.wq = o2.wq; ma.fmax = f.nmax;
    ma.nns = v.S <= 2 ? o1.nns : nn12;  // featnn_row7 (S > 2) writes no copy
    ma.F = F; ma.G = G; ma.mx = v.mx;
    ma.list21 = v.list21; ma.cnt21 = v.cnt21; ma.nn21x = nn21x;
    ma.corres = corres; ma.n_corres = n_corres;
    auto prep_hook = [&](int at) -> int {
        if (!prep_event || prep_at != at) return PCR_OK;
        PCR_HIP_CHECK(hipEventRecord(prep_event, s));
        const int hrc = prep_fn ? prep_fn(prep_ctx) : PCR_OK;
        if (hrc == PCR_OK) prep_fn = nullptr;
        return hrc;
    };
    if ((rc = prep_hook(2)) != PCR_OK) return rc;
    // pass 1: F rows x all G columns
    rc = run_pass<true>(rt, make_pass(screen_args(v, 0, rt, o1), 0, rt, v.list12, v.cnt12), s);
    if (rc != PCR_OK) return rc;
    if ((rc = prep_hook(1)) != PCR_OK) return rc;
    RescanArgs5 ra = rescan_args(F, G, n_src, n_tgt, Nmax, Mmax, D);
    ra.list12 = v.list12; ra.list21 = v.list21; ra.cnt12 = v.cnt12; ra.cnt21 = zero;
    ra.nn12 = nn12; ra.nn21 = nn21x;
    ra.v12 = o1.v; ra.e12 = o1.e; ra.mx = v.mx; ra.T = v.sp.T;
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
        // columns (A-role fragments streamed): the same products, values only.  The
        // threshold route writes a settled column's exact argmin to nn21x, its flag to 2
        Pass p2 = make_pass(screen_args(v, 1, rt, o2), 1, rt, nullptr, nullptr);
        p2.th.nn = nn21x; p2.th.used = ma.used;
        rc = run_pass<false>(rt, p2, s);
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

// debug: copy the mutual path's scratch (feature_corres_v5's layout) of the last call to dst
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
