// The mutual feature path's route (pcr_feature_correspondences at D <= 64): the
// constants it depends on, the tile padding, and the one function that reads
// the PCR_FEAT_* hooks.  Host only, no HIP: tests/cpp/feat_route_check.cpp
// includes nothing else.
#pragma once
#include <stdlib.h>
#include <string.h>

namespace pcr {

// column tiles per LDS group of featnn_row8 / featnn_row9 (the column images
// are padded to whole groups of both)
constexpr int kRow8G = 8;      // column tiles per LDS group (16: the whole LDS, measured no faster)
#ifndef PCR_ROW9_G
#define PCR_ROW9_G 16  // 8: pass 1 1.12 vs 1.09 ms, pass 2 0.76 vs 0.74 (C4, featnn_bench)
#endif
#ifndef PCR_ROW9_G1
#define PCR_ROW9_G1 PCR_ROW9_G
#endif
constexpr int kRow9G = PCR_ROW9_G;     // featnn_row9's: pass 2 (and the padding)
constexpr int kRow9G1 = PCR_ROW9_G1;   // pass 1 (<= kRow9G)
constexpr int kRegroupMaxSteps = 4096;  // featnn_regroup9 keeps a pair's per-step prefix in LDS

// column slices of the 3-term screens' list mode: a pair's short list is
// one workgroup per slice -- at 256 pairs one slice (the chip is full), at
// 32 pairs 8 (one block per pair left 224 CUs idle: ~0.2 ms per launch)
inline int list_slices(int P) {
    const int s = 256 / (P > 1 ? P : 1);
    return s < 1 ? 1 : (s > 8 ? 8 : s);
}

// 32-row tiles of the packed images.  F's (ntn): whole blocks of the dual
// screen (8 tiles) and of the row screens (8 waves x up to 2 tiles).  G's
// (ntm): whole LDS groups of featnn_row8 and featnn_row9.  The padding rows are
// valid encodings of +inf rows.
struct FeatTiles {
    int ntn, ntm;
};
inline FeatTiles feat_tiles(int Nmax, int Mmax) {
    constexpr int g = kRow8G > kRow9G ? kRow8G : kRow9G;
    const int tn = (Nmax + 31) / 32, tm = (Mmax + 31) / 32;
    return {(tn + 15) / 16 * 16, (tm + g - 1) / g * g};
}

// Which screens a call runs and which image they read:
//   one      a 1-term screen in front of the 3-term one (S <= 2); PCR_FEAT_ONE=0: the
//            3-term featnn_row8 alone (S > 2: featnn_row7 whatever the hooks)
//   use9     the 1-term screen is featnn_row9 + regroup; PCR_FEAT_ROW9=0, or more column
//            steps than the regroup's LDS prefix holds: featnn_row8's 1-term pass
//   thresh   featnn_row9's leftover rows go to the threshold route; PCR_FEAT_THRESH=0:
//            to the 3-term screen
//   compact  the images hold the hi segment only (S chunks per tile), all the threshold
//            route reads; PCR_FEAT_IMAGE=full keeps the 2S + 1 chunks there too
//   fsl      column slices of the 3-term list screens
// The hooks are A/B and parity switches, read on every call.
struct FeatRoute {
    int S;
    bool one, use9, thresh, compact;
    int fsl, ntn, ntm;
};
inline FeatRoute feat_route(int P, int Nmax, int Mmax, int D) {
    auto off = [](const char *name) {
        const char *e = getenv(name);
        return e && e[0] == '0';
    };
    const char *img = getenv("PCR_FEAT_IMAGE");
    const FeatTiles t = feat_tiles(Nmax, Mmax);
    FeatRoute r{};
    r.S = (D + 15) / 16;
    r.ntn = t.ntn;
    r.ntm = t.ntm;
    r.fsl = list_slices(P);
    r.one = r.S <= 2 && !off("PCR_FEAT_ONE");
    r.use9 = r.one && !off("PCR_FEAT_ROW9") && (t.ntm > t.ntn ? t.ntm : t.ntn) / 2 <= kRegroupMaxSteps;
    r.thresh = r.use9 && !off("PCR_FEAT_THRESH");
    r.compact = r.thresh && !(img && strcmp(img, "full") == 0);
    return r;
}

}  // namespace pcr
