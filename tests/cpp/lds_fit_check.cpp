// Host-only check of the fit rule of a grid's LDS copy (csrc/lds_fit.h), which
// decides whether the batch Chamfer's LDS query, RANSAC and ICP may stage a
// cloud's grid.  Compiled with -fsanitize=address,undefined and run as a plain
// executable (tests/test_lds_fit_cpu.py).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lds_fit.h"

static int fails = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                    \
        }                                                               \
    } while (0)

int main() {
    using pcr::lds4_fit_bytes;
    const size_t kAll = 160 * 1024;
    // the C4 cloud: 8192 float4 points + 8193 u16 starts = 147,458 B, rounded to 16
    CHECK(lds4_fit_bytes(8192, 8192, kAll) == 147472);
    CHECK((131072 + 16386 + 15) / 16 * 16 == 147472);
    // exactly the budget fits; one byte less does not
    CHECK(lds4_fit_bytes(8192, 8192, 147472) == 147472);
    CHECK(lds4_fit_bytes(8192, 8192, 147471) == 0);
    CHECK(lds4_fit_bytes(8192, 8192, 0) == 0);
    // u16 slot starts: at most 65535 points, at most 65536 table entries
    const size_t kHuge = size_t(1) << 40;
    CHECK(lds4_fit_bytes(65535, 256, kHuge) == (size_t(65535) * 16 + 257 * 2 + 15) / 16 * 16);
    CHECK(lds4_fit_bytes(65536, 256, kHuge) == 0);
    CHECK(lds4_fit_bytes(1 << 30, 256, kHuge) == 0);
    CHECK(lds4_fit_bytes(256, 65535, kHuge) == (size_t(256) * 16 + 65536 * 2 + 15) / 16 * 16);
    CHECK(lds4_fit_bytes(256, 65536, kHuge) == 0);
    CHECK(lds4_fit_bytes(256, 0x7fffffff, kHuge) == 0);  // S + 1 must not be formed in int
    CHECK(lds4_fit_bytes(-1, 256, kHuge) == 0);
    CHECK(lds4_fit_bytes(256, -1, kHuge) == 0);
    // the Chamfer's table sizes (power of two >= nmax, >= 256): the largest
    // cloud that fits 160 KiB, and the answer is a whole layout -- every byte
    // of a buffer of the returned size that the layout addresses lies inside it
    for (int nmax = 1; nmax <= 20000; nmax += 97) {
        int S = 256;
        while (S < nmax) S <<= 1;
        const size_t b = lds4_fit_bytes(nmax, S, kAll);
        const size_t need = size_t(nmax) * 16 + size_t(S + 1) * 2;
        CHECK((b != 0) == (need <= kAll));  // kAll is a multiple of 16
        if (!b) continue;
        CHECK(b % 16 == 0 && b >= need && b < need + 16 && b <= kAll);
        std::vector<unsigned char> lds(b);
        uint16_t *starts = reinterpret_cast<uint16_t *>(lds.data() + size_t(nmax) * 16);
        lds[size_t(nmax) * 16 - 1] = 1;   // the last point's last byte
        starts[S] = 2;                    // the last slot start
        CHECK(starts[S] == 2);
    }
    CHECK(lds4_fit_bytes(8192, 8192, kAll) != 0);
    CHECK(lds4_fit_bytes(9000, 16384, kAll) == 0);  // 144,000 + 32,770 B
    if (fails) return 1;
    std::printf("ok: lds fit rule\n");
    return 0;
}
