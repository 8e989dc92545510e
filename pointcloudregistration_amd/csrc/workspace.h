// The library workspace's slot names, and the helper that lays several
// sub-buffers out in one slot.  Host only, no HIP: a plain host compiler builds
// it (tests/cpp/ws_layout_check.cpp).  DESIGN.md "Workspace slots" has the
// sharing rule and the procedure for adding a slot.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace pcr {

// One name per slot of workspace() (runtime.cpp).  The values are the table
// index and do not change; a new slot goes before kWsCount.  A name with an
// underscore is one slot with several owners: its comment says why they are
// never live together.  icp_plane.hip (pcr_icp_plane_batch) uses icp.hip's
// slots for the same contents -- grid, order, permuted sources, working copy,
// partial sums (27 per record instead of 15), barriers: another ABI call, and
// the barrier words' protocol is the same.
enum WsSlot : int {
    kWsNone = -1,                 // fpfh.hip run_search: "no list slot" (the caller's own buffers)
    kWsNndPartials = 0,           // nnd.hip: split sweep's partial (dist, idx); pcr_nnd_forward
    kWsNndBackward = 1,           // nnd.hip: counts, starts, sorted lists; pcr_nnd_backward
    kWsFeatPack_NndRagged = 2,    // featnn_pack.hip v5_prepare / featnn_f32.hip: packed descriptors, norms, lists
                                  // (exclusive branches of one call, D <= 64 / D > 64); nnd_ragged.hip:
                                  // partials of pcr_nnd_forward_ragged, another ABI call
    kWsCorres = 3,                // featnn.hip corres_impl: corres_build's scratch; pcr_correspondences, D > 64
    kWsRansacGrid = 4,            // ransac.hip build_ransac_grids: target grids (pipeline: side stream)
    kWsFpsOver_PpfIdx = 5,        // group.hip: pcr_fps's distances past the registers; pcr_group_ppf's
                                  // neighbour indices -- two ABI calls
    kWsFeatRescan = 6,            // featnn_rescan.hip run_rescan: slice partials (d, j); stream-ordered reuse in a call
    kWsIcpGrid = 7,               // icp.hip / pipeline.cpp: ICP's target grid (pipeline: side stream, for icp_impl)
    kWsIcpPoints = 8,             // icp.hip: f64 working copy of the sources
    kWsRegister = 9,              // pipeline.cpp: nn12 | nn21 | corres | n_corres; pcr_register_feature_ransac
    kWsIcpPartials_RadiusNnGrid = 10,  // icp.hip: cooperative partial sums; grid.hip: pcr_radius_nn's grid,
                                       // an ABI call that runs no ICP
    kWsFeatDualCols = 11,         // featnn_dual.hip feature_match_v5 / featnn_f32.hip: dual screen's column partials
                                  // (exclusive branches, D <= 64 / D > 64); pcr_feature_match, D > 64 corres
    kWsIcpTiming = 12,            // icp.hip: PCR_ICP_TIMING clocks
    kWsRansacOrder = 13,          // ransac.hip / pipeline.cpp: spatial order of the sources (pipeline: built on
                                  // the side stream for ransac_impl, reused by icp_impl)
    kWsIcpOrder = 14,             // icp.hip: spatial order of the sources; pcr_icp alone
    kWsNndGrid = 15,              // nnd_grid.hip: points, cells, flags, counts, starts; Chamfer grid path
    kWsSubsample = 16,            // kpconv.hip: pcr_grid_subsample's keys and lists
    kWsSubsampleTmp = 17,         // kpconv.hip: pcr_grid_subsample's rocprim temporary
    kWsNeighbors = 18,            // kpconv.hip: radius neighbours' grid, counts and lists
    kWsNeighborsTmp = 19,         // kpconv.hip: radius neighbours' rocprim temporary
    kWsNeighborsKeys = 20,        // kpconv.hip: radius neighbours' sort keys and sort temporary
    kWsRansacBest = 21,           // ransac.hip: the best hypothesis's target indices
    kWsRansacState = 22,          // ransac.hip: per-pair state
    kWsRansacHypT = 23,           // ransac.hip: a round's transforms
    kWsRansacHypBits_FpfhGrid = 24,   // ransac.hip: a round's pass bits; fpfh.hip: the search grid of
                                      // pcr_hybrid_search / _estimate_normals / _compute_fpfh, no RANSAC calls
    kWsRansacHdr_FpfhLists = 25,  // ransac.hip: headers and task counts; fpfh.hip: neighbour lists (as 24)
    kWsFpfhSpfh = 26,             // fpfh.hip: SPFH when the caller passes none; pcr_compute_fpfh
    kWsVoxel = 27,                // voxel.hip: pcr_voxel_down_sample's keys and lists
    kWsVoxelTmp = 28,             // voxel.hip: its rocprim temporary
    kWsRansacTasks = 29,          // ransac.hip: a round's task list
    kWsRansacRes = 30,            // ransac.hip: task results
    kWsRansacSlots = 31,          // ransac.hip: target slots of the first tasks
    kWsRansacParts = 32,          // ransac.hip: split tasks' parts
    kWsFeatMutual = 33,           // featnn.hip feature_corres_v5: mutual path (pcr_featmut_debug_copy reads it)
    kWsFeatNn21 = 34,             // featnn.hip: nn21 of the D > 64 and Mmax == 0 correspondences
    kWsIcpPerm = 35,              // icp.hip: sources in kWsIcpOrder's order
    kWsRansacPerm = 36,           // ransac.hip / pipeline.cpp: sources in kWsRansacOrder's order
    kWsIcpTail = 37,              // icp.hip: two-phase tail's saved state, control words and pair list
    kWsIcpCst = 38,               // icp.hip: per-point correspondence state
    kWsIcpBarrier = 39,           // icp.hip: pair barriers, zeroed when fresh or dirty
    kWsCount
};

// What a multi-buffer request adds past its layout, as the hand-written sums did.
constexpr size_t kWsSlack = 256;

// Lays sub-buffers out in one slot: declare each once with take(), ask the
// slot for bytes(), then bind(base) sets every declared pointer.
//   WsLayout l;  l.take(a.d2, pn * K);  l.take(a.idx, pn * K);
//   workspace_bind(slot, l, kWsSlack)   (pcr_internal.h)
// min_align 1 packs: each sub-buffer at the next multiple of its own alignment,
// a zero count takes no bytes.  min_align > 1 pads: every sub-buffer starts on
// a min_align boundary and a zero count still reserves one element, so
// sub-buffers are distinct and non-null.
class WsLayout {
public:
    explicit WsLayout(size_t min_align = 1) : min_(min_align) {
        if (!pow2(min_align)) bad_ = true;
    }
    // offset of a sub-buffer of count T's
    template <class T> size_t take(size_t count, size_t align = alignof(T)) { return place(count, sizeof(T), align); }
    // the same, and bind() points dst at it (dst must outlive bind)
    template <class T> size_t take(T *&dst, size_t count, size_t align = alignof(T)) {
        const size_t at = place(count, sizeof(T), align);
        dst = nullptr;
        if (n_ == kMaxBound) bad_ = true;
        if (bad_) return 0;
        dst_[n_] = &dst;
        off_[n_++] = at;
        return at;
    }
    bool ok() const { return !bad_; }  // false: a size overflowed size_t, or a bad alignment
    size_t bytes() const { return up(used_, min_); }
    size_t alignment() const { return max_; }  // the largest requested
    // false (nothing written) when the layout is not ok or base is null or misaligned
    bool bind(void *base) const {
        if (bad_ || !base || ((uintptr_t)base & (max_ - 1)) != 0) return false;
        for (int i = 0; i < n_; ++i) {
            char *p = (char *)base + off_[i];
            memcpy(dst_[i], &p, sizeof(p));  // dst_[i] is a T *'s address
        }
        return true;
    }

private:
    static constexpr int kMaxBound = 32;
    static bool pow2(size_t x) { return x != 0 && (x & (x - 1)) == 0; }
    static size_t up(size_t x, size_t a) { return (x + (a - 1)) & ~(a - 1); }
    size_t place(size_t count, size_t elem, size_t align) {
        if (min_ > 1 && count == 0) count = 1;
        if (align < min_) align = min_;
        // at + size, rounded up to min_ by bytes(), must fit size_t
        const size_t at = !pow2(align) || used_ > SIZE_MAX - (align - 1) ? SIZE_MAX : up(used_, align);
        const size_t room = SIZE_MAX - at;
        if (bad_ || room < min_ || count > (room - (min_ - 1)) / elem) {
            bad_ = true;
            return 0;
        }
        used_ = at + count * elem;
        if (align > max_) max_ = align;
        return at;
    }
    size_t min_, used_ = 0, max_ = 1;
    bool bad_ = false;
    int n_ = 0;
    void *dst_[kMaxBound];
    size_t off_[kMaxBound];
};

}  // namespace pcr
