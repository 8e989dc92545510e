// Host check of the workspace slot table and the layout helper
// (csrc/workspace.h): offsets against the formulas their readers use, alignment,
// no overlap, bounds, and the refusals of bind() and of an overflowing count.
// Meant to be compiled with -fsanitize=address,undefined and run as a plain
// program (exit status 0 = ok).
#include "workspace.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pcr;

namespace {

int g_checks = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(cond)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

struct alignas(16) Q16 { float v[4]; };  // float4 / uint4 stand-in

struct Sub { size_t off, bytes, align; };

// every sub-buffer aligned as asked, inside bytes(), none overlapping another
void check_general(const WsLayout &l, const std::vector<Sub> &subs) {
    CHECK(l.ok());
    for (size_t i = 0; i < subs.size(); ++i) {
        CHECK(subs[i].off % subs[i].align == 0);
        CHECK(subs[i].off + subs[i].bytes <= l.bytes());
        CHECK(subs[i].align <= l.alignment());
        for (size_t j = 0; j < i; ++j)
            CHECK(subs[j].off + subs[j].bytes <= subs[i].off || subs[i].off + subs[i].bytes <= subs[j].off);
    }
}

// feature_corres_v5's first four sub-buffers: v12 f64 [P][N] | e12 f32 [P][N] |
// wq 16-byte [P][M] | used int [P][M+1], by the formula
// tests/test_featcorres_gpu.py::_mut_scratch reads them with
void natural_offsets(size_t P, size_t N, size_t M) {
    WsLayout l;
    double *v12;
    float *e12;
    Q16 *wq;
    int *used;
    const size_t o0 = l.take(v12, P * N), o1 = l.take(e12, P * N), o2 = l.take(wq, P * M),
                 o3 = l.take(used, P * (M + 1));
    CHECK(o0 == 0);
    CHECK(o1 == 8 * P * N);  // not rounded to 16
    CHECK(o2 == (12 * P * N + 15) / 16 * 16);
    CHECK(o3 == o2 + 16 * P * M);
    CHECK(l.bytes() == o3 + 4 * P * (M + 1));
    CHECK(l.alignment() == 16);
    check_general(l, {{o0, 8 * P * N, 8}, {o1, 4 * P * N, 4}, {o2, 16 * P * M, 16}, {o3, 4 * P * (M + 1), 4}});
    CHECK(!l.bind(nullptr) && v12 == nullptr);
    if (l.bytes() > (1u << 20)) return;
    // bind: a 16-aligned base is taken, every pointer set, and both ends of every
    // sub-buffer are inside the allocation; base + 8 is refused
    char *base = (char *)aligned_alloc(16, (l.bytes() + 15) / 16 * 16);
    CHECK(base && l.bind(base));
    CHECK((char *)v12 == base && (char *)e12 == base + o1 && (char *)wq == base + o2 && (char *)used == base + o3);
    v12[0] = v12[P * N - 1] = 1.0;
    e12[0] = e12[P * N - 1] = 1.0f;
    wq[0] = wq[P * M - 1] = Q16{};
    used[0] = used[P * (M + 1) - 1] = 1;
    v12 = nullptr;
    CHECK(!l.bind(base + 8) && v12 == nullptr);
    free(base);
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// min_align 256: used = align256(used + sizeof(T) * max(count, 1))
void padded_offsets() {
    WsLayout l(256);
    struct { size_t elem, count; } seq[] = {{4, 7}, {8, 3}, {1, 300}, {4, 0}, {16, 5}, {8, 0}, {1, 1}, {4, 64}, {8, 31}};
    std::vector<Sub> subs;
    size_t used = 0;
    for (const auto &s : seq) {
        size_t at = 0;
        switch (s.elem) {
            case 1: at = l.take<unsigned char>(s.count); break;
            case 4: at = l.take<int>(s.count); break;
            case 8: at = l.take<double>(s.count); break;
            default: at = l.take<Q16>(s.count); break;
        }
        CHECK(at == used);
        const size_t bytes = s.elem * (s.count > 0 ? s.count : 1);
        subs.push_back({at, bytes, 256});
        used = align256(used + bytes);
        CHECK(l.bytes() == used);
    }
    CHECK(l.alignment() == 256);
    check_general(l, subs);
    // a zero count is still a buffer of its own
    int *a, *b;
    WsLayout z(256);
    z.take(a, 0);
    z.take(b, 0);
    alignas(256) static char base[512];
    CHECK(z.bytes() == 512 && z.bind(base) && a && b && a != b);
    CHECK(!z.bind(base + 128));
    // packed, a zero count takes nothing (the next sub-buffer starts there)
    WsLayout n;
    CHECK(n.take<Q16>(3) == 0 && n.take<Q16>(0) == 48 && n.take<int>(2) == 48 && n.bytes() == 56);
    // an explicit alignment above the type's
    WsLayout e;
    CHECK(e.take<int>(1) == 0 && e.take<char>(5, 16) == 16 && e.take<int>(1) == 24 && e.alignment() == 16);
}

void refusals() {
    WsLayout l;
    double *d;
    l.take<int>(3);
    CHECK(l.ok());
    l.take(d, SIZE_MAX / 8 + 1);  // count * sizeof(T) overflows
    CHECK(!l.ok());
    alignas(16) static char base[16];
    CHECK(!l.bind(base) && d == nullptr);
    WsLayout m(256);
    m.take<char>(SIZE_MAX - 100);  // fits, but not rounded up to 256
    CHECK(!m.ok());
    WsLayout s;
    s.take<char>(SIZE_MAX - 4);
    CHECK(s.ok());
    s.take<double>(1);  // the round-up to 8 overflows
    CHECK(!s.ok());
    WsLayout a;
    a.take<int>(1, 12);  // not a power of two
    CHECK(!a.ok());
    CHECK(!WsLayout(0).ok() && !WsLayout(48).ok());
    WsLayout many;  // more bound pointers than the helper holds
    int *p[64];
    for (int i = 0; i < 64; ++i) many.take(p[i], 1);
    CHECK(!many.ok());
}

void slot_table() {
    const WsSlot all[] = {kWsNndPartials, kWsNndBackward, kWsFeatPack_NndRagged, kWsCorres, kWsRansacGrid,
                          kWsFpsOver_PpfIdx, kWsFeatRescan, kWsIcpGrid, kWsIcpPoints, kWsRegister,
                          kWsIcpPartials_RadiusNnGrid, kWsFeatDualCols, kWsIcpTiming, kWsRansacOrder, kWsIcpOrder,
                          kWsNndGrid, kWsSubsample, kWsSubsampleTmp, kWsNeighbors, kWsNeighborsTmp,
                          kWsNeighborsKeys, kWsRansacBest, kWsRansacState, kWsRansacHypT,
                          kWsRansacHypBits_FpfhGrid, kWsRansacHdr_FpfhLists, kWsFpfhSpfh, kWsVoxel, kWsVoxelTmp,
                          kWsRansacTasks, kWsRansacRes, kWsRansacSlots, kWsRansacParts, kWsFeatMutual,
                          kWsFeatNn21, kWsIcpPerm, kWsRansacPerm, kWsIcpTail, kWsIcpCst, kWsIcpBarrier};
    const int n = (int)(sizeof(all) / sizeof(all[0]));
    CHECK(n == kWsCount && kWsCount == 40);  // runtime.cpp sizes its table by kWsCount
    for (int i = 0; i < n; ++i) CHECK((int)all[i] == i);  // dense from 0, so pairwise distinct
    CHECK(kWsNone < 0);
    CHECK(kWsSlack == 256);
}

}  // namespace

int main() {
    const size_t shapes[][3] = {{1, 1, 1}, {1, 3, 5}, {3, 7, 2}, {192, 160, 340}, {256, 8192, 8192}};
    for (const auto &s : shapes) natural_offsets(s[0], s[1], s[2]);
    padded_offsets();
    refusals();
    slot_table();
    printf("ok: %d checks\n", g_checks);
    return 0;
}
