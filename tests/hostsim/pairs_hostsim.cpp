// Host harness of the pair kernel's host side (xdem_amd/csrc/pairs_classes.h, pairs_layout.h, pairs_policy.h) -- test tool only,
// driven through ctypes by tests/test_pairs_host.py.
#include "../../xdem_amd/csrc/pairs_classes.h"
#include "../../xdem_amd/csrc/pairs_layout.h"
#include "../../xdem_amd/csrc/pairs_policy.h"

using namespace xd;

namespace {

template <typename T, int OP, bool WIDE> int table_of(int nb, int nbs, int64_t* out, uint64_t* total) {
    const PairsLdsTable t = pairs_lds_table<T, OP, WIDE>(nb, nbs);
    for (int k = 0; k < t.n; ++k) {
        out[5 * k] = t.r[k].id; out[5 * k + 1] = (int64_t)t.r[k].offset; out[5 * k + 2] = (int64_t)t.r[k].elem;
        out[5 * k + 3] = (int64_t)t.r[k].count; out[5 * k + 4] = (int64_t)t.r[k].align;
    }
    *total = pairs_lds_bytes<T, OP, WIDE>(nb, nbs);
    return t.n;
}
template <typename T> int table_of_op(int op, bool wide, int nb, int nbs, int64_t* out, uint64_t* total) {
    switch (op) {
        case OP_SUMS_SQ: return table_of<T, OP_SUMS_SQ, false>(nb, nbs, out, total);
        case OP_SUMS_SQRT: return table_of<T, OP_SUMS_SQRT, false>(nb, nbs, out, total);
        case OP_HIST: return table_of<T, OP_HIST, false>(nb, nbs, out, total);
        case OP_SUCC: return table_of<T, OP_SUCC, false>(nb, nbs, out, total);
        case OP_BRACKET:
            if constexpr (sizeof(T) == 4) { if (wide) return table_of<T, OP_BRACKET, true>(nb, nbs, out, total); }
            return table_of<T, OP_BRACKET, false>(nb, nbs, out, total);
    }
    return -1;
}

}  // namespace

extern "C" {

// ---- pairs_classes.h ----
void ph_constants(int* out) {
    out[0] = PT; out[1] = BCHUNK; out[2] = LUT_N; out[3] = LUT_G; out[4] = LUT_G0; out[5] = NCOPY; out[6] = HIST_BINS_PER_SWEEP;
    out[7] = LDS_ACC_FIRST; out[8] = PAIRS_STAGE_CAP; out[9] = PAIRS_REC;
}
void ph_thresholds(const double* edges, int n, int strict, double* thr) {
    for (int k = 0; k < n; ++k) thr[k] = strict ? sq_threshold_strict(edges[k]) : sq_threshold(edges[k]);
}
// lut [LUT_N]; returns whether the table is taken
int ph_binade_lut(const double* thr, int n, uint8_t* lut, int* emin) {
    std::vector<uint8_t> t;
    const bool ok = build_binade_lut(std::vector<double>(thr, thr + n), t, *emin);
    for (int i = 0; i < LUT_N; ++i) lut[i] = t[i];
    return ok ? 1 : 0;
}
// class of every s2 as the table kernels compute it: cell -> class lower bound, one compare where the cell holds a threshold
void ph_binade_classes(const double* thr, int n, const uint8_t* lut, int emin, const double* s2, int64_t m, int32_t* cls) {
    for (int64_t i = 0; i < m; ++i) {
        uint64_t b;
        memcpy(&b, &s2[i], 8);
        int e = (int)(b >> 49) - emin;
        e = e < 0 ? 0 : (e > LUT_N - 1 ? LUT_N - 1 : e);
        const int c = lut[e];
        int l = c >> 1;
        if (c & 1) l += (l < n ? thr[l] : INFINITY) <= s2[i] ? 1 : 0;
        cls[i] = l;
    }
}
int ph_cell_of_u32(uint32_t d2) { return cell_of_u32(d2); }
// bx == null: an i < j set.  a_xy [na], b_xy [nbt], thr_i [n], lut [LUT_G]; returns whether the lattice route is taken
int ph_make_grid(const double* ax, const double* ay, int64_t na, const double* bx, const double* by, int64_t nbt, const double* thr, int n,
                 uint32_t* a_xy, uint32_t* b_xy, uint32_t* thr_i, uint8_t* lut) {
    GridInfo g;
    if (!make_grid(ax, ay, na, bx, by, nbt, std::vector<double>(thr, thr + n), g)) return 0;
    for (size_t i = 0; i < g.a_xy.size(); ++i) a_xy[i] = g.a_xy[i];
    for (size_t i = 0; i < g.b_xy.size(); ++i) b_xy[i] = g.b_xy[i];
    for (int i = 0; i < n; ++i) thr_i[i] = g.thr_i[i];
    for (int i = 0; i < LUT_G; ++i) lut[i] = g.lut[i];
    return 1;
}
int ph_host_threads() { return host_threads(); }

// ---- pairs_layout.h ----
// out: [regions][5] = id, offset, elem, count, align; returns the number of regions
int ph_lds_table(int f64, int op, int wide, int nb, int nbs, int64_t* out, uint64_t* total) {
    return f64 ? table_of_op<double>(op, false, nb, nbs, out, total) : table_of_op<float>(op, wide != 0, nb, nbs, out, total);
}
// the kernel's walker over a real block: byte offsets of the regions' pointers from the base (-1: a region of another operation)
void ph_lds_pointers(int nb, unsigned char* base, int64_t* off) {
    PairsLdsPointers w(base);
    PAIRS_LDS_WALK(w, float, OP_BRACKET, false, nb, 0);
    for (int k = 0; k < LDS_REGIONS; ++k) off[k] = w.p[k] ? (int64_t)(static_cast<unsigned char*>(w.p[k]) - base) : -1;
}

// ---- pairs_policy.h ----
int ph_route(int selection_mode, int nb, int64_t n_pairs, int64_t n_wg_big) { return pairs_route_brackets(selection_mode, nb, n_pairs, n_wg_big) ? 1 : 0; }
int64_t ph_bracket_min() { return PAIRS_BRACKET_MIN; }
uint32_t ph_attempt_deff(int attempt, uint32_t deff, int pdist, uint32_t wide, uint32_t spread) { return pairs_attempt_deff(attempt, deff, pdist != 0, wide, spread); }
void ph_bracket_ends32(uint64_t count, uint32_t lo, uint32_t hi, uint32_t mask, int mode, uint32_t* out) { pairs_bracket_ends<uint32_t>(count, lo, hi, mask, mode, out[0], out[1]); }
void ph_bracket_ends64(uint64_t count, uint64_t lo, uint64_t hi, uint64_t mask, int mode, uint64_t* out) { pairs_bracket_ends<uint64_t>(count, lo, hi, mask, mode, out[0], out[1]); }
double ph_expected(uint64_t count, uint64_t halfwidth, double per_rank) { return pairs_expected_candidates(count, halfwidth, per_rank); }
long long ph_capacity(double expected, int64_t n_pairs) { return pairs_candidate_capacity(expected, n_pairs); }
uint32_t ph_rebase32(const uint32_t* klo, const uint32_t* khi, int n, uint32_t* origin) {
    std::vector<uint32_t> o;
    const uint32_t w = pairs_rebase_origins<false, uint32_t, uint32_t>(std::vector<uint32_t>(klo, klo + n), std::vector<uint32_t>(khi, khi + n), o);
    for (int k = 0; k < n; ++k) origin[k] = o[k];
    return w;
}
uint64_t ph_rebase64(const uint64_t* klo, const uint64_t* khi, int n, uint64_t* origin) {
    std::vector<uint64_t> o;
    const uint64_t w = pairs_rebase_origins<false, uint64_t, uint64_t>(std::vector<uint64_t>(klo, klo + n), std::vector<uint64_t>(khi, khi + n), o);
    for (int k = 0; k < n; ++k) origin[k] = o[k];
    return w;
}
uint64_t ph_rebase_wide(const uint32_t* klo, const uint32_t* khi, int n, uint64_t* origin) {
    std::vector<uint64_t> o;
    const uint64_t w = pairs_rebase_origins<true, uint32_t, uint64_t>(std::vector<uint32_t>(klo, klo + n), std::vector<uint32_t>(khi, khi + n), o);
    for (int k = 0; k < n; ++k) origin[k] = o[k];
    return w;
}
int ph_ranks(const uint64_t* total, const uint64_t* below, const uint64_t* inside, int nb, int overflow, uint64_t* given) {
    return pairs_ranks_from_counts(total, below, inside, nb, overflow != 0, given);
}

}  // extern "C"
