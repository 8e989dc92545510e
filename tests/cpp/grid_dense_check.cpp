// Host check of the dense r-cell grid's index arithmetic (csrc/grid_dense.h):
// builds bitmap, rank and start arrays the way the build kernel does, then
// checks for many queries that the candidate ranges of dense_ranges are valid
// and contain every point with d2 < thr.  Meant to be compiled with
// -fsanitize=address,undefined and run as a plain program (exit status 0 = ok).
#include "grid_dense.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace pcr;

namespace {

struct P3 { float x, y, z; };

struct Host {
    std::vector<uint32_t> bits;
    std::vector<uint16_t> rank, start;
    std::vector<int> order;  // sorted position -> point
    DenseTab tab{};
    bool dense = false;
};

int cell_of(float v, double cell) { return (int)std::floor((double)v / cell); }

Host build(const std::vector<P3> &pts, double r) {
    Host h;
    const double cell = kDenseCellFactor * r;
    const int m = (int)pts.size();
    h.tab.inv_cell = 1.0 / cell;
    h.tab.cellf = (float)cell;
    if (m == 0) {
        h.bits.assign(1, 0u);
        h.rank.assign(1, 0);
        h.start.assign(1, 0);
        h.dense = true;
    } else {
        int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
        for (const P3 &p : pts) {
            const int c[3] = {cell_of(p.x, cell), cell_of(p.y, cell), cell_of(p.z, cell)};
            for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], c[k]); hi[k] = std::max(hi[k], c[k]); }
        }
        const int cells = dense_cells((long long)hi[0] - lo[0] + 1, (long long)hi[1] - lo[1] + 1,
                                      (long long)hi[2] - lo[2] + 1);
        if (cells < 0 || m > kDenseMaxPoints) return h;
        h.dense = true;
        h.tab.ox = lo[0]; h.tab.oy = lo[1]; h.tab.oz = lo[2];
        h.tab.DX = hi[0] - lo[0] + 1; h.tab.DY = hi[1] - lo[1] + 1; h.tab.DZ = hi[2] - lo[2] + 1;
        const int words = (cells + 31) >> 5;
        std::vector<int> id(m), cnt(cells, 0);
        for (int j = 0; j < m; ++j) {
            id[j] = dense_id(cell_of(pts[j].x, cell) - lo[0], cell_of(pts[j].y, cell) - lo[1],
                             cell_of(pts[j].z, cell) - lo[2], h.tab.DX, h.tab.DY);
            ++cnt[id[j]];
        }
        h.order.resize(m);
        for (int j = 0; j < m; ++j) h.order[j] = j;
        std::stable_sort(h.order.begin(), h.order.end(), [&](int a, int b) { return id[a] < id[b]; });
        h.bits.assign(words, 0u);
        h.rank.assign(words, 0);
        int occ = 0, at = 0;
        for (int c = 0; c < cells; ++c) {
            if ((c & 31) == 0) h.rank[c >> 5] = (uint16_t)occ;
            if (cnt[c]) {
                h.bits[c >> 5] |= 1u << (c & 31);
                h.start.push_back((uint16_t)at);
                at += cnt[c];
                ++occ;
            }
        }
        h.start.push_back((uint16_t)m);
    }
    h.tab.bits = h.bits.data();
    h.tab.rank = h.rank.data();
    h.tab.start = h.start.data();
    return h;
}

long long g_queries = 0, g_cands = 0;

bool check_query(const std::vector<P3> &pts, const Host &h, double r, const double q[3]) {
    const double thr = (double)(float)(r * r);
    const int m = (int)pts.size();
    std::vector<char> cand(m, 0);
    bool ok = true;
    int nr = 0;
    dense_ranges(h.tab, r, thr, q[0], q[1], q[2], [&](int s, int e) {
        ++nr;
        if (s < 0 || e < s || e > m) { ok = false; return; }
        for (int k = s; k < e; ++k) {
            if (cand[h.order[k]]) ok = false;  // ranges must not overlap
            cand[h.order[k]] = 1;
            ++g_cands;
        }
    });
    ++g_queries;
    if (nr != 9) ok = false;
    for (int j = 0; j < m; ++j) {
        const double dx = (double)pts[j].x - q[0], dy = (double)pts[j].y - q[1], dz = (double)pts[j].z - q[2];
        if ((dx * dx + dy * dy) + dz * dz < thr && !cand[j]) ok = false;
    }
    if (!ok) std::fprintf(stderr, "FAIL query (%.17g, %.17g, %.17g) r=%g m=%d\n", q[0], q[1], q[2], r, m);
    return ok;
}

std::mt19937_64 rng(12345);
double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }

bool check_cloud(const char *name, const std::vector<P3> &pts, double r, bool expect_dense = true) {
    const Host h = build(pts, r);
    if (h.dense != expect_dense) {
        std::fprintf(stderr, "FAIL %s: dense=%d\n", name, (int)h.dense);
        return false;
    }
    if (!h.dense) return true;
    bool ok = true;
    std::vector<std::vector<double>> qs;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (size_t j = 0; j < pts.size(); ++j) {
        const double v[3] = {pts[j].x, pts[j].y, pts[j].z};
        for (int k = 0; k < 3; ++k) {
            lo[k] = j ? std::min(lo[k], v[k]) : v[k];
            hi[k] = j ? std::max(hi[k], v[k]) : v[k];
        }
    }
    const size_t stride = std::max<size_t>(1, pts.size() / 200);
    for (size_t j = 0; j < pts.size(); j += stride) {
        const double c[3] = {pts[j].x, pts[j].y, pts[j].z};
        qs.push_back({c[0], c[1], c[2]});
        for (int k = 0; k < 3; ++k)
            for (double d : {r, std::nextafter(r, 0.0), std::nextafter(r, 1.0), std::sqrt((double)(float)(r * r)),
                             0.999 * r, -r, -0.5 * r}) {
                std::vector<double> q = {c[0], c[1], c[2]};
                q[k] += d;
                qs.push_back(q);
            }
        for (int t = 0; t < 4; ++t) {  // random directions, lengths up to 1.2 r
            double d[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
            const double n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 1e-300, len = uni(0, 1.2) * r;
            qs.push_back({c[0] + d[0] / n * len, c[1] + d[1] / n * len, c[2] + d[2] / n * len});
        }
    }
    for (double gap : {0.5 * r, 1.5 * r, 100 * r, 1e12, 1e300})  // outside the bounding box
        for (int k = 0; k < 3; ++k) {
            std::vector<double> q = {uni(lo[0], hi[0]), uni(lo[1], hi[1]), uni(lo[2], hi[2])};
            q[k] = hi[k] + gap;
            qs.push_back(q);
            q[k] = lo[k] - gap;
            qs.push_back(q);
        }
    for (const auto &q : qs) ok = check_query(pts, h, r, q.data()) && ok;
    if (!ok) std::fprintf(stderr, "FAIL cloud %s\n", name);
    return ok;
}

std::vector<P3> lattice(int nx, int ny, int nz, double cell, int ox, int oy, int oz, double pitch = 1.0) {
    std::vector<P3> v;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x)
                v.push_back(P3{(float)((x * pitch + 0.5 + ox) * cell), (float)((y * pitch + 0.5 + oy) * cell),
                               (float)((z * pitch + 0.5 + oz) * cell)});
    return v;
}

}  // namespace

int main() {
    const double r = 0.04, cell = kDenseCellFactor * r;
    bool ok = true;
    // dense_range against a naive count, every interval of <= 3 cells over three words
    {
        std::vector<uint32_t> bits = {0x80000001u, 0xffffffffu, 0x00018000u, 0u};
        for (int t = 0; t < 50; ++t) bits.push_back((uint32_t)rng());
        std::vector<int> rank(bits.size());
        int occ = 0;
        for (size_t w = 0; w < bits.size(); ++w) { rank[w] = occ; occ += __builtin_popcount(bits[w]); }
        auto bit = [&](int id) { return (int)((bits[id >> 5] >> (id & 31)) & 1u); };
        const int ncell = (int)bits.size() * 32;
        for (int a = 0; a < ncell; ++a)
            for (int b = a; b < std::min(ncell, a + 3); ++b) {
                int lo, n, wl = 0, wn = 0;
                dense_range(bits[a >> 5], bits[b >> 5], rank[a >> 5], a, b, lo, n);
                for (int c = 0; c < a; ++c) wl += bit(c);
                for (int c = a; c <= b; ++c) wn += bit(c);
                if (lo != wl || n != wn) { std::fprintf(stderr, "FAIL dense_range %d %d\n", a, b); ok = false; }
            }
    }
    ok = check_cloud("empty", {}, r) && ok;
    ok = check_cloud("one", {P3{0.3f, -0.2f, 0.1f}}, r) && ok;
    {
        std::vector<P3> v;
        for (int j = 0; j < 50; ++j)
            v.push_back(P3{(float)((5.5 + uni(-0.4, 0.4)) * cell), (float)((5.5 + uni(-0.4, 0.4)) * cell),
                           (float)((5.5 + uni(-0.4, 0.4)) * cell)});
        ok = check_cloud("one cell", v, r) && ok;
    }
    ok = check_cloud("distinct cells", lattice(9, 7, 5, cell, 0, 0, 0, 2.0), r) && ok;
    for (int DX : {31, 32, 33, 65}) {
        ok = check_cloud("row", lattice(DX, 1, 1, cell, 0, 0, 0), r) && ok;
        ok = check_cloud("rows", lattice(DX, 3, 2, cell, -7, 2, -40), r) && ok;
    }
    ok = check_cloud("flat", lattice(20, 30, 1, cell, -3, -3, 9), r) && ok;
    ok = check_cloud("line z", lattice(1, 1, 40, cell, 0, 0, 0), r) && ok;
    for (int t = 0; t < 6; ++t) {  // random clouds, some far from the origin
        const double off = t < 3 ? 0.0 : (t == 3 ? -37.0 : (t == 4 ? 1000.0 : -2000.0));
        std::vector<P3> v;
        const int m = 300 + 500 * t;
        for (int j = 0; j < m; ++j)
            v.push_back(P3{(float)(off + uni(-0.4, 0.4)), (float)(off / 2 + uni(-0.3, 0.3)), (float)(uni(-0.2, 0.2) - off)});
        ok = check_cloud("random", v, r) && ok;
    }
    {  // targets on cell boundaries and one f32 ulp to either side, duplicates
        std::vector<P3> v;
        for (int off : {0, -17, 400})
            for (int x = 0; x < 5; ++x)
                for (int y = 0; y < 4; ++y)
                    for (int z = 0; z < 3; ++z) {
                        const float b[3] = {(float)((off + x) * cell), (float)((off + y) * cell), (float)((off + z) * cell)};
                        v.push_back(P3{b[0], b[1], b[2]});
                        v.push_back(P3{std::nextafterf(b[0], 1e30f), std::nextafterf(b[1], 1e30f), std::nextafterf(b[2], 1e30f)});
                        v.push_back(P3{std::nextafterf(b[0], -1e30f), std::nextafterf(b[1], -1e30f), std::nextafterf(b[2], -1e30f)});
                        v.push_back(P3{b[0], b[1], b[2]});
                    }
        ok = check_cloud("boundaries", std::vector<P3>(v.begin(), v.begin() + 240), r) && ok;
        ok = check_cloud("boundaries far", std::vector<P3>(v.begin() + 480, v.end()), r) && ok;
        ok = check_cloud("boundaries spread", v, r, false) && ok;  // 417 cells per axis: not dense
    }
    ok = check_cloud("too wide", {P3{0, 0, 0}, P3{(float)(1000 * cell), (float)(1000 * cell), (float)(1000 * cell)}}, r, false) && ok;
    std::printf("%s: %lld queries, %.2f candidates per query\n", ok ? "ok" : "FAILED", g_queries,
                g_queries ? (double)g_cands / (double)g_queries : 0.0);
    return ok ? 0 : 1;
}
