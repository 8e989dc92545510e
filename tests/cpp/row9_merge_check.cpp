// Host check of row9_close / row9_merge (csrc/row9_merge.h): the columns-
// stationary sweep of featnn_row9 gives step s to wave s mod W, each wave
// closes its steps in ascending order, and the waves' triples merge at the end.
// For random and adversarial sequences of group minima the merged (B1, B2, I)
// must equal, bit for bit, what one wave closing every step in order keeps.
// Plain C++, no HIP.
#include "row9_merge.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
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

struct Triple {
    unsigned b1 = pcr::kRow9Inf, b2 = pcr::kRow9Inf, i = 0u;
    bool operator==(const Triple &o) const { return b1 == o.b1 && b2 == o.b2 && i == o.i; }
};

static unsigned bits(float v) {
    unsigned u;
    memcpy(&u, &v, sizeof(u));
    return u;
}

// the sequential loop: every step in ascending order
static Triple sequential(const std::vector<unsigned> &mn) {
    Triple t;
    for (size_t s = 0; s < mn.size(); ++s) pcr::row9_close(t.b1, t.b2, t.i, mn[s], (unsigned)s);
    return t;
}

// W waves, wave w the steps w, w + W, ..., merged in the order `order` gives
static Triple split(const std::vector<unsigned> &mn, int W, const std::vector<int> &order) {
    std::vector<Triple> wave(W);  // heap: ASan sees an index past either end
    for (int w = 0; w < W; ++w)
        for (size_t s = (size_t)w; s < mn.size(); s += (size_t)W)
            pcr::row9_close(wave[w].b1, wave[w].b2, wave[w].i, mn[s], (unsigned)s);
    Triple t;
    for (int w : order) pcr::row9_merge(t.b1, t.b2, t.i, wave[w].b1, wave[w].b2, wave[w].i);
    return t;
}

static void run(const std::vector<unsigned> &mn, std::mt19937_64 &rng) {
    const Triple want = sequential(mn);
    // the plain definition beside the loop's: the two smallest of the multiset
    // with two +inf, and the first step at the smallest below +inf
    unsigned m1 = pcr::kRow9Inf, m2 = pcr::kRow9Inf, mi = 0u;
    for (size_t s = 0; s < mn.size(); ++s) {
        if (mn[s] < m1) { m2 = m1; m1 = mn[s]; mi = (unsigned)s; }
        else if (mn[s] < m2) m2 = mn[s];
    }
    CHECK(want.b1 == m1 && want.b2 == m2 && want.i == mi);
    for (int W : {4, 8}) {
        std::vector<int> order(W);
        for (int w = 0; w < W; ++w) order[w] = w;
        CHECK(split(mn, W, order) == want);  // the kernel's order
        for (int k = 0; k < 3; ++k) {        // any order gives the same
            for (int w = W - 1; w > 0; --w) std::swap(order[w], order[rng() % (unsigned)(w + 1)]);
            CHECK(split(mn, W, order) == want);
        }
    }
}

int main() {
    std::mt19937_64 rng(14);
    const unsigned inf = pcr::kRow9Inf, nan = 0x7fc00000u, pad = bits(3.0e38f);
    const unsigned a = bits(1048576.0f), b = bits(1048577.0f), c = bits(2097152.0f);
    for (int n : {0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 24, 64, 65}) {
        run(std::vector<unsigned>(n, a), rng);    // all equal
        run(std::vector<unsigned>(n, inf), rng);  // +inf everywhere
        run(std::vector<unsigned>(n, nan), rng);  // patterns above +inf never enter
        for (int s = 0; s < n; ++s) {             // one real step among padding
            std::vector<unsigned> v(n, pad);
            v[s] = a;
            run(v, rng);
            std::vector<unsigned> w(n, inf);
            w[s] = a;
            run(w, rng);
        }
        // the equal smallest twice, at every pair of steps: different waves
        // (s2 - s1 not a multiple of W) and the same wave (s2 = s1 + W, + 2 W)
        for (int s1 = 0; s1 < n; ++s1)
            for (int s2 = s1 + 1; s2 < n; ++s2) {
                std::vector<unsigned> v(n, c);
                v[s1] = a;
                v[s2] = a;
                run(v, rng);
                v[s2] = b;  // a near second: B2 from another wave's B1, or the same wave's B2
                run(v, rng);
                v[s1] = b;
                v[s2] = a;
                run(v, rng);
            }
    }
    // random: few distinct values (many ties), some +inf and NaN patterns
    for (int it = 0; it < 200000; ++it) {
        const int n = (int)(rng() % 70);
        const int nv = 1 + (int)(rng() % 6);
        std::vector<unsigned> v(n);
        for (auto &x : v) {
            const unsigned r = (unsigned)(rng() % 16);
            x = r == 0 ? inf : (r == 1 ? nan : bits(1048576.0f + (float)(rng() % (unsigned)nv)));
        }
        run(v, rng);
    }
    // random: full patterns
    for (int it = 0; it < 100000; ++it) {
        const int n = 1 + (int)(rng() % 70);
        std::vector<unsigned> v(n);
        for (auto &x : v) x = (unsigned)rng() & 0x7fffffffu;
        run(v, rng);
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok: row9_merge\n");
    return 0;
}
