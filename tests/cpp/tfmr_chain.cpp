// The similarity of the TFMR matching contract (include/pcr_api.h) on the host:
// S[i][j] = the f32 fmaf chain over c = 0 .. C-1 ascending, from +0.  numpy has
// no fmaf, so tests/tfmr_ref.py compiles this (-O2 -ffp-contract=off) and loads
// it with ctypes.  x (n,c), y (m,c) row-major, out (n,m).  Eight columns run
// side by side (independent chains, each in its own order) to hide the latency.
#include <math.h>
#include <stdint.h>

extern "C" void tfmr_chain(const float *x, const float *y, int64_t n, int64_t m, int64_t c, float *out) {
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j0 = 0; j0 < m; j0 += 8) {
            const int64_t w = m - j0 < 8 ? m - j0 : 8;
            const float *xi = x + i * c;
            float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int64_t k = 0; k < c; ++k)
                for (int64_t t = 0; t < w; ++t) s[t] = fmaf(xi[k], y[(j0 + t) * c + k], s[t]);
            for (int64_t t = 0; t < w; ++t) out[i * m + j0 + t] = s[t];
        }
}
