// Host check of thresh_flush_count (csrc/featnn_thresh.h), the arithmetic of
// featnn_thresh9's flush of a row's block-local hits to its global slots,
// against a plain model: the blocks (column slices) of a pair flush one after
// the other in some order, each adding its local count to the row's total and
// copying the local slots that land below K.  Plain C++, no HIP.
#include "featnn_thresh.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL line %d: %s\n", __LINE__, #c);            \
            ++fails;                                               \
        }                                                          \
    } while (0)

constexpr int K = 8;             // kThreshK
constexpr int kLaneCap = K + 1;  // hits one lane counts in one slice
constexpr int kGuard = 4;        // slots on either side of the row's: never written

// One row, its slices' local counts in flush order.  A slice's local slot i
// holds the tag (slice, i); the row's global slots sit between guard slots.
static void run_row(const std::vector<uint32_t> &local) {
    std::vector<int> slots(K + 2 * kGuard, -1);  // heap: ASan sees a write past either end
    int *row = slots.data() + kGuard;
    uint32_t total = 0;  // rec.x
    int model_filled = 0;
    for (size_t s = 0; s < local.size(); ++s) {
        const uint32_t lc = local[s];
        if (lc == 0) continue;  // the kernel flushes rows with a non-zero local count
        const uint32_t base = total;  // what the returning add gives
        total += lc;
        const int stored = (int)std::min<uint32_t>(lc, K);  // the local slots that exist
        const int n = pcr::thresh_flush_count(base, lc, K);
        CHECK(n >= 0 && n <= stored);
        // the model: local hit i lands at base + i while that is a slot
        int want = 0;
        for (int i = 0; i < stored; ++i)
            if (base + (uint32_t)i < (uint32_t)K) ++want;
        CHECK(n == want);
        for (int i = 0; i < n; ++i) {
            const uint32_t pos = base + (uint32_t)i;
            CHECK(pos < (uint32_t)K);
            if (pos >= (uint32_t)K) continue;  // (counted above; never write past the row's slots)
            CHECK(row[pos] == -1);             // no slot is written twice
            row[pos] = (int)(s * 64 + i);
            ++model_filled;
        }
    }
    uint32_t sum = 0;
    for (uint32_t lc : local) sum += lc;
    CHECK(total == sum);
    // overflow exactly when the total exceeds K; below that every hit has its slot
    const bool over = total > (uint32_t)K;
    CHECK(over == (sum > (uint32_t)K));
    if (!over) {
        CHECK(model_filled == (int)total);
        for (int i = 0; i < K; ++i) CHECK((row[i] != -1) == (i < (int)total));
    } else {
        // an overflowing row's slots may hold anything: featnn_exact_cand reads none of them
        CHECK(std::min<uint32_t>(total, K + 1) == (uint32_t)K + 1);
    }
    for (int i = 0; i < kGuard; ++i) CHECK(slots[i] == -1 && slots[kGuard + K + i] == -1);
}

int main() {
    // the boundary the GPU tests place: 8 = 3 + 3 + 2 fits, 9 = 3 + 3 + 3 overflows
    run_row({3, 3, 2});
    run_row({3, 3, 3});
    run_row({8});
    run_row({9});
    run_row({0, 8, 0});
    run_row({8, 1});
    run_row({1, 8});
    run_row({7, 2});
    run_row({});
    // a local count past K: two lanes (the row's halves) at the per-lane cap
    run_row({2 * kLaneCap});
    run_row({1, 2 * kLaneCap, 1});
    CHECK(pcr::thresh_flush_count(0u, 0u, K) == 0);
    CHECK(pcr::thresh_flush_count(0u, 8u, K) == 8);
    CHECK(pcr::thresh_flush_count(0u, 9u, K) == 8);
    CHECK(pcr::thresh_flush_count(7u, 5u, K) == 1);
    CHECK(pcr::thresh_flush_count(8u, 5u, K) == 0);
    CHECK(pcr::thresh_flush_count(0xfffffff0u, 5u, K) == 0);  // a base far past K: nothing copied
    // random local counts per slice, 1 to 32 slices, weighted to the edges
    std::mt19937_64 rng(10);
    const uint32_t edge[] = {0u, 0u, 0u, 1u, 2u, 3u, (uint32_t)K - 1, (uint32_t)K, (uint32_t)K + 1,
                             (uint32_t)kLaneCap, 2u * kLaneCap};
    for (int it = 0; it < 200000; ++it) {
        const int ns = 1 + (int)(rng() % 32);
        std::vector<uint32_t> local(ns);
        const int mode = (int)(rng() % 3);
        for (auto &lc : local)
            lc = mode == 0 ? edge[rng() % (sizeof(edge) / sizeof(edge[0]))]
                           : (mode == 1 ? (uint32_t)(rng() % 3) : (uint32_t)(rng() % (2 * kLaneCap + 1)));
        run_row(local);
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok: thresh_flush_count\n");
    return 0;
}
