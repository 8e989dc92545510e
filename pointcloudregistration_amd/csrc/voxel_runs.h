// The voxel runs of a batch of clouds, shared by grid_subsample (kpconv.hip)
// and voxel_down_sample (voxel.hip): a stable sort of the points by (cloud,
// voxel key), the runs of equal (cloud, key), and those runs listed in the
// order their first points come in the input -- the insertion sequence of the
// references' unordered_map, which the callers replay on the host.
#pragma once
#include "pcr_internal.h"
#include "wave.h"

namespace pcr {

// Device pointers out of the caller's own WsLayout; N entries each unless noted.
struct VoxelRuns {
    int *v;               // out: sorted position -> input index
    int *start;           // out: [V + 1] run r is v[start[r] .. start[r + 1])
    int *list;            // out: [V] runs in first-occurrence order
    u64 *okey;            // out: [V] their keys
    int *ocloud;          // out: [V] their clouds (only with cloud ids)
    u64 *ck, *ck2;        // sort keys in (only with cloud ids) / out
    int *v2;              // only when key and cloud bits exceed 64 (two passes)
    unsigned char *head;
    int *mark, *dcnt;     // dcnt: [2]
};

// key: per-point voxel keys of kbits bits.  cloud: per-point cloud ids of bbits
// bits, or null when the key already carries the cloud in its top bits.  One
// composite sort when kbits + bbits <= 64, two stable least-significant-digit
// passes otherwise.  tmp_slot: the caller's rocprim temp slot; who: the entry
// point's name for error texts.  N > 0.  One host synchronisation (the fetch of *V).
int voxel_runs(const u64 *key, unsigned kbits, const int *cloud, unsigned bbits, int N,
               const VoxelRuns &r, WsSlot tmp_slot, const char *who, hipStream_t st, int *V);

}  // namespace pcr
