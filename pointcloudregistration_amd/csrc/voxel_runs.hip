// f2: sort-to-runs pipeline of the two voxel-grid entry points (voxel_runs.h).
#include "voxel_runs.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>

namespace pcr {
namespace {

// sort keys with the cloud: the (cloud, key) composite of point i, or -- second
// of two passes, v = the first pass's order -- the cloud of point v[i] alone
__global__ void vr_cloud_key(const u64 *key, const int *cloud, const int *v, int n, int kbits, u64 *ck) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ck[i] = v ? (u64)cloud[v[i]] : ((u64)cloud[i] << kbits) | key[i];
}

// run heads of the (cloud, key)-sorted points: neighbouring sorted entries
// differ.  sorted: the single pass's sorted composites; null after two passes,
// when (cloud, key) is read through v
__global__ void vr_heads(const u64 *sorted, const u64 *key, const int *cloud, const int *v, int n,
                         unsigned char *head) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool h = i == 0;
    if (i && sorted) h = sorted[i] != sorted[i - 1];
    if (i && !sorted) h = cloud[v[i]] != cloud[v[i - 1]] || key[v[i]] != key[v[i - 1]];
    head[i] = h;
}

// mark[first point of run r] = r (the sort is stable: a run's first entry is
// its lowest input index); start[V] = n closes the last run
__global__ void vr_mark(int *start, const int *v, int V, int n, int *mark) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < V) mark[v[start[r]]] = r;
    if (r == 0) start[V] = n;
}

// keys (and clouds) of the listed runs, for the callers' host replay
__global__ void vr_okey(VoxelRuns r, const u64 *key, const int *cloud, int V) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const int first = r.v[r.start[r.list[i]]];
    r.okey[i] = key[first];
    if (cloud) r.ocloud[i] = cloud[first];
}

struct NonNeg {
    __device__ bool operator()(int x) const { return x >= 0; }
};

}  // namespace

int voxel_runs(const u64 *key, unsigned kbits, const int *cloud, unsigned bbits, int N,
               const VoxelRuns &r, WsSlot tmp_slot, const char *who, hipStream_t st, int *V) {
    const bool two = cloud && kbits + bbits > 64;   // keys wider than the composite
    const bool compose = cloud && bbits && !two;
    const u64 *k1 = compose ? r.ck : key;           // the first (or only) pass
    int *v1 = two ? r.v2 : r.v;
    const unsigned bits1 = compose ? kbits + bbits : kbits;
    const rocprim::counting_iterator<int> iota(0);
    // the four rocprim steps: called with null for their temporary's size, then to run
    auto sort1 = [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, k1, r.ck2, iota, v1, N, 0, bits1, st); };
    auto sort2 = [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, r.ck, r.ck2, r.v2, r.v, N, 0, bbits, st); };
    auto starts = [&](void *t, size_t &b) { return rocprim::select(t, b, iota, r.head, r.start, r.dcnt, (size_t)N, st); };
    auto order = [&](void *t, size_t &b) { return rocprim::select(t, b, r.mark, r.list, r.dcnt + 1, (size_t)N, NonNeg(), st); };
    size_t tb = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
    PCR_HIP_CHECK(sort1(nullptr, t1));
    if (two) PCR_HIP_CHECK(sort2(nullptr, t2));
    PCR_HIP_CHECK(starts(nullptr, t3));
    PCR_HIP_CHECK(order(nullptr, t4));
    tb = std::max(std::max(t1, t2), std::max(t3, t4));
    void *tmp = workspace(tmp_slot, tb);
    PCR_REQUIRE(tmp, PCR_ERR_NOMEM, "%s: %s", who, pcr_last_error());

    // stable radix sort by (cloud, key): input order kept inside a voxel
    const dim3 gN((N + 255) / 256), blk(256);
    if (compose) hipLaunchKernelGGL(vr_cloud_key, gN, blk, 0, st, key, cloud, (const int *)nullptr, N, (int)kbits, r.ck);
    PCR_LAUNCH_CHECK();
    PCR_HIP_CHECK(sort1(tmp, t1 = tb));
    if (two) {
        hipLaunchKernelGGL(vr_cloud_key, gN, blk, 0, st, key, cloud, (const int *)r.v2, N, 0, r.ck);
        PCR_LAUNCH_CHECK();
        PCR_HIP_CHECK(sort2(tmp, t2 = tb));
    }
    hipLaunchKernelGGL(vr_heads, gN, blk, 0, st, two ? nullptr : (const u64 *)r.ck2, key, cloud, (const int *)r.v, N,
                       r.head);
    PCR_LAUNCH_CHECK();
    PCR_HIP_CHECK(starts(tmp, t3 = tb));
    PCR_HIP_CHECK(hipMemcpyAsync(V, r.dcnt, sizeof(int), hipMemcpyDeviceToHost, st));
    PCR_HIP_CHECK(hipStreamSynchronize(st));
    PCR_HIP_CHECK(hipMemsetAsync(r.mark, 0xFF, sizeof(int) * N, st));
    hipLaunchKernelGGL(vr_mark, dim3((*V + 255) / 256), blk, 0, st, r.start, (const int *)r.v, *V, N, r.mark);
    PCR_LAUNCH_CHECK();
    PCR_HIP_CHECK(order(tmp, t4 = tb));
    hipLaunchKernelGGL(vr_okey, dim3((*V + 255) / 256), blk, 0, st, r, key, cloud, *V);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

}  // namespace pcr
