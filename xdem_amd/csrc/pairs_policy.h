// pairs_policy.h -- the host decisions of the bracketed exact-median selection over point pairs (variogram.hip:
// pairs_medians_typed): which sets take the route, the design effect of each attempt, the bracket ends from the two sampled
// selection states, the candidate capacity, the rebase origins of the candidate keys and the ranks among the candidates.  Plain
// C++ without a HIP include: the CPU tests (tests/test_pairs_host.py) compile it with g++.  The constants of select.h it needs
// (design effects, half widths) come in as arguments.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "pairs_classes.h"

namespace xd {

constexpr int64_t PAIRS_BRACKET_MIN = (int64_t)4000000000ll;  // pairs; below this the sample units are too few

// The bracketed route: not switched off (context option "selection_mode" = 1), every class in one histogram sweep, enough pairs for
// the 1/64 sample and enough units for the resident workgroups of the sampled passes.
inline bool pairs_route_brackets(int selection_mode, int nb, int64_t n_pairs, int64_t n_wg_big) {
    return selection_mode != 1 && nb <= HIST_BINS_PER_SWEEP && n_pairs >= PAIRS_BRACKET_MIN && n_wg_big >= 256;
}

// Design effect assumed for the sample (select.h): every-a-with-every-b blocks are sampled with per-lane B slots (few pairs
// per point: `deff_spread`), i < j blocks with 4 B slots against all A points (`deff_wide`).  A bracket that misses its rank (the
// integer counts tell) costs one more attempt with 16 x the assumed design effect (4 x the width), then one with the wide rule,
// before the plain digit passes take over; with a reduction hook the counts are global, so every rank retries alike.
// Returns the design effect of attempt 0, 1, 2 given the previous attempt's (`deff`; ignored for attempt 0), or 0: no such attempt.
inline uint32_t pairs_attempt_deff(int attempt, uint32_t deff, bool pdist, uint32_t deff_wide, uint32_t deff_spread) {
    if (attempt == 0) return pdist ? deff_wide : deff_spread;
    if (attempt > 2 || deff >= deff_wide) return 0;
    return (attempt == 1 && deff * 16 < deff_wide) ? deff * 16 : deff_wide;
}

// Ends of a class's bracket, as keys, from the two sampled states: the low state's prefix, and the high state's prefix with the
// digits the sampled passes did not resolve (`low_mask`) set.  A class without a sampled pair gets the bracket that holds
// everything; test mode (context option "selection_mode" = 2): brackets that (almost surely) miss.
template <typename K> inline void pairs_bracket_ends(uint64_t sample_count, K lo_prefix, K hi_prefix, K low_mask, int selection_mode, K& klo, K& khi) {
    const bool have = sample_count > 0;
    klo = have ? lo_prefix : (K)0;
    khi = have ? (K)(hi_prefix | low_mask) : (K)~(K)0;
    if (selection_mode == 2 && have) khi = klo;
}

// Candidates a class's bracket should hold: the pairs one sample rank stands for (`per_rank`: 64 on i < j blocks, the tile's
// points per sampled slot otherwise) x its width in sample ranks (2 half widths + 2), at most the class.
inline double pairs_expected_candidates(uint64_t sample_count, uint64_t halfwidth, double per_rank) {
    const double m = (double)sample_count, w = 2.0 * (double)halfwidth + 2.0;
    return per_rank * (w < m ? w : m);
}
// candidate buffers sized from the brackets (x1.5 + slack), not from the pair count: 5e13 pairs (SURVEY 8d, C5 reading
// A) need ~2e10 slots, not n_pairs / 64.
inline long long pairs_candidate_capacity(double expected, int64_t n_pairs) {
    const double want = expected * 1.5 + (double)(1 << 20);
    const double most = (double)n_pairs + 1024.0;
    return (long long)(want < most ? want : most);
}

// Candidate keys are rebased for their selection (select_run.h, hist_pass_kernel): per class the origin in key_of()'s key space
// (|dv| >= 0: key = bits | top bit; the pair passes use bits << 1); returns the widest range of a class (the common shift follows
// from it).  An empty bracket (khi < klo) has range 0.
// WIDE (K = uint32_t, KC = uint64_t): candidates are the exact differences d with fl32(d) in [L, H] (L, H the float32 ends, raw
// bits klo >> 1 / khi >> 1): every such d lies in (pred(L), succ(H)) -- the origin and the range of the rebased float64 keys.
template <bool WIDE, typename K, typename KC> inline KC pairs_rebase_origins(const std::vector<K>& klo, const std::vector<K>& khi, std::vector<KC>& origin) {
    static_assert(WIDE ? (sizeof(K) == 4 && sizeof(KC) == 8) : sizeof(K) == sizeof(KC), "WIDE: float32 ends, float64 candidates");
    const KC top = (KC)1 << (8 * sizeof(KC) - 1);
    origin.resize(klo.size());
    KC widest = 0;
    for (size_t k = 0; k < klo.size(); ++k) {
        KC r;
        if constexpr (WIDE) {
            const uint32_t lb = (uint32_t)(klo[k] >> 1), hb = (uint32_t)(khi[k] >> 1);
            const uint32_t lp = lb > 0 ? lb - 1 : 0u, hs = hb < 0x7f800000u ? hb + 1 : 0x7f800000u;
            float lf, hf;
            memcpy(&lf, &lp, 4);
            memcpy(&hf, &hs, 4);
            const double ld = (double)lf, hd = (double)hf;
            uint64_t lk, hk;
            memcpy(&lk, &ld, 8);
            memcpy(&hk, &hd, 8);
            origin[k] = (KC)(lk | top);
            r = (khi[k] >= klo[k] && hk >= lk) ? (KC)(hk - lk) : (KC)0;
        } else {
            origin[k] = (KC)((klo[k] >> 1) | top);
            r = khi[k] >= klo[k] ? (KC)((khi[k] >> 1) - (klo[k] >> 1)) : (KC)0;
        }
        widest = r > widest ? r : widest;
    }
    return widest;
}

// From the counting pass's integers per class -- total, pairs below the bracket, pairs inside it -- the rank of the wanted order
// statistic AMONG THE CANDIDATES (given[k]; all-ones: an empty class, nothing to select): the lower median, rank (total - 1) / 2,
// and for an even total its upper neighbour must both lie inside.  Returns the first class whose bracket missed (later entries of
// `given` are then not filled), -2 when the candidate buffer overflowed (nothing filled), -1 when every class has its rank.
inline int pairs_ranks_from_counts(const uint64_t* total, const uint64_t* below, const uint64_t* inside, int nb, bool overflow, uint64_t* given) {
    if (overflow) return -2;
    for (int k = 0; k < nb; ++k) {
        given[k] = ~(uint64_t)0;
        if (total[k] == 0) continue;
        const uint64_t r = (total[k] - 1) / 2;
        const uint64_t need = (total[k] & 1) ? r : r + 1;
        if (below[k] > r || need - below[k] >= inside[k]) return k;
        given[k] = r - below[k];
    }
    return -1;
}

}  // namespace xd
