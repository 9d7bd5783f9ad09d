// nk_layout.h -- ONE description of each small device block of the one-pass Nuth-Kaab step: where every region lies and how large
// the block is.  The plan allocates from it (nuthkaab.hip: nk_create_impl, nk_mr_alloc), the step's host code takes its pointers
// from it, and the kernels of nk_onepass.h are handed those pointers.  Every region is a whole number of 64-bit words, whatever the
// sample type; a region grows with the plan's largest bin count (nb_max), not with the step's.  No HIP include: the CPU tests
// evaluate the sizes with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace xd {

constexpr int BINSEG_CTR_STRIDE = 16;   // the per-bin place counters sit one 128-byte line apart (same-line atomics serialise)
constexpr int DSEL_BUCKETS = 4096;      // value buckets of the selection of the median of dh among its candidates
constexpr int DSEL_CAP = 8192;          // keys of the chosen bucket (more -- ties en masse -- send the step to the plain route)
constexpr int DSEL_HDR_WORDS = 4;       // 64-bit words: [0] ~(smallest key IN the bucket), [1] keys appended, [2] ~(smallest key above the bucket), [3] largest key in the bucket; then the histogram

template <typename T> struct KeyT;   // (select.h)

// word offsets of the step's device block `fz`; all of it but the key list at its end is zeroed at the start of a step
struct NkFzWords {
    // head: fixed places
    static constexpr int64_t CTR = 0;      // [8] counters and flags: [1] dh candidates, [2] overflow, [3] miss, [5] y candidates, [6] no survivor in an EXT list
    static constexpr int64_t RBS_D = 8;    // rebase shift of the dh candidates' keys (32 bits)
    static constexpr int64_t RBS_Y = 9;    // ... of the bin candidates' keys (32 bits)
    static constexpr int64_t CNT_D = 10;   // [3] total, below, inside of the bracket of the median of dh
    // (13: ranks of the dh selection, written and read on the device only)
    static constexpr int64_t KLO_D = 14, KHI_D = 15;   // bracket of the median of dh, keys
    static constexpr int64_t VHAT = 16, DELTA = 17;    // its midpoint and half width, values
    static constexpr int64_t SUMS = 18;    // [5] float64 sums of the pass
    // (23: unused)
    static constexpr int64_t HEAD = 24;
    static constexpr int64_t HEAD_FETCHED = 16;   // the step fetches words [0, 16) as one item: counters, rebase shifts, cnt_d
    // per bin, from HEAD on: each region follows the one before it
    static constexpr int64_t klo_y_w(int64_t) { return HEAD; }                              // [nbm] brackets of the bin medians, keys
    static constexpr int64_t khi_y_w(int64_t nbm) { return klo_y_w(nbm) + nbm; }              // [nbm]
    static constexpr int64_t rank_y_w(int64_t nbm) { return khi_y_w(nbm) + nbm; }             // [nbm] ranks of the bin selections, device only
    static constexpr int64_t cls_y_w(int64_t nbm) { return rank_y_w(nbm) + nbm; }             // [3][nbm] classes counted by the pass
    static constexpr int64_t res_y_w(int64_t nbm) { return cls_y_w(nbm) + 3 * nbm; }          // [2][nbm] counters of the resolved candidates
    static constexpr int64_t cnt_y_w(int64_t nbm) { return res_y_w(nbm) + 2 * nbm; }          // [3][nbm] total, below, inside of the bins' brackets
    static constexpr int64_t seg_ctr_w(int64_t nbm) { return cnt_y_w(nbm) + 3 * nbm; }        // [nbm] x BINSEG_CTR_STRIDE places taken in the candidate segments
    static constexpr int64_t dsel_w(int64_t nbm) { return seg_ctr_w(nbm) + BINSEG_CTR_STRIDE * nbm; }   // header + histogram of the dh selection
    static constexpr int64_t zeroed_words(int64_t nbm) { return dsel_w(nbm) + DSEL_HDR_WORDS + DSEL_BUCKETS / 2; }
    static constexpr int64_t dsel_keys_w(int64_t nbm) { return zeroed_words(nbm); }         // [DSEL_CAP] keys of the chosen bucket (not zeroed)
    static constexpr size_t total_bytes(int64_t nbm) { return (size_t)(dsel_keys_w(nbm) + DSEL_CAP) * 8; }
};
static_assert(NkFzWords::CNT_D + 3 <= NkFzWords::HEAD_FETCHED && NkFzWords::RBS_Y < NkFzWords::HEAD_FETCHED, "counters, rebase shifts and cnt_d arrive in the one head item");
static_assert(NkFzWords::KLO_D >= NkFzWords::CNT_D + 4 && NkFzWords::SUMS + 5 <= NkFzWords::HEAD, "the head regions do not overlap");
static_assert(DSEL_BUCKETS % 2 == 0, "the 32-bit histogram fills whole words");
static_assert(BINSEG_CTR_STRIDE * 8 == 128, "one 128-byte line per bin's place counter");

template <typename T, typename K = typename KeyT<T>::type> struct NkFzLayout : NkFzWords {
    unsigned long long* ctr;
    uint32_t *rbs_d, *rbs_y;
    uint64_t* cnt_d;
    K *klo_d, *khi_d;
    T *vhat, *delta;
    double* sums;
    K *klo_y, *khi_y;
    uint64_t *cls_y, *res_y, *cnt_y;
    unsigned long long* seg_ctr;
    uint32_t* dsel;   // DSEL_HDR_WORDS 64-bit words, then the histogram [DSEL_BUCKETS]
    K* dsel_keys;
    uint64_t* base;
    int64_t nbm;
    NkFzLayout(uint64_t* fz, int64_t nb_max) : base(fz), nbm(nb_max) {
        ctr = at<unsigned long long>(CTR);
        rbs_d = at<uint32_t>(RBS_D);
        rbs_y = at<uint32_t>(RBS_Y);
        cnt_d = at<uint64_t>(CNT_D);
        klo_d = at<K>(KLO_D);
        khi_d = at<K>(KHI_D);
        vhat = at<T>(VHAT);
        delta = at<T>(DELTA);
        sums = at<double>(SUMS);
        klo_y = at<K>(klo_y_w(nbm));
        khi_y = at<K>(khi_y_w(nbm));
        cls_y = at<uint64_t>(cls_y_w(nbm));
        res_y = at<uint64_t>(res_y_w(nbm));
        cnt_y = at<uint64_t>(cnt_y_w(nbm));
        seg_ctr = at<unsigned long long>(seg_ctr_w(nbm));
        dsel = at<uint32_t>(dsel_w(nbm));
        dsel_keys = at<K>(dsel_keys_w(nbm));
    }
    uint32_t* dsel_hist() const { return dsel ? dsel + 2 * DSEL_HDR_WORDS : nullptr; }
    static int64_t zeroed_words(int64_t nb_max) { return NkFzWords::zeroed_words(nb_max); }
    static size_t total_bytes(int64_t nb_max) { return NkFzWords::total_bytes(nb_max); }

private:
    // (a layout over no block -- sizes only -- has null members)
    template <typename U> U* at(int64_t word) const { return base ? reinterpret_cast<U*>(base + word) : nullptr; }
};

// the small block of PARTITIONED plans: this rank's own classes, the counters rewritten for the gathered bucket values and the true
// counters of the bins (nk_mr_* kernels); each region follows the one before it
struct NkMrSmallLayout {
    static constexpr int64_t cls_loc_w(int64_t) { return 0; }                                          // [3][nbm]
    static constexpr int64_t cls_f_w(int64_t nbm) { return cls_loc_w(nbm) + 3 * nbm; }                 // [3][nbm]
    static constexpr int64_t res_f_w(int64_t nbm) { return cls_f_w(nbm) + 3 * nbm; }                   // [2][nbm]
    static constexpr int64_t cnt_true_w(int64_t nbm) { return res_f_w(nbm) + 2 * nbm; }                // [3][nbm]
    static constexpr int64_t segf_ctr_w(int64_t nbm) { return cnt_true_w(nbm) + 3 * nbm; }             // [nbm] x BINSEG_CTR_STRIDE words
    static constexpr int64_t total_words(int64_t nbm) { return segf_ctr_w(nbm) + BINSEG_CTR_STRIDE * nbm; }
    uint64_t *cls_loc, *cls_f, *res_f, *cnt_true;
    unsigned long long* segf_ctr;
    NkMrSmallLayout(uint64_t* mr_small, int64_t nbm) {   // (no block: null members)
        cls_loc = mr_small ? mr_small + cls_loc_w(nbm) : nullptr;
        cls_f = mr_small ? mr_small + cls_f_w(nbm) : nullptr;
        res_f = mr_small ? mr_small + res_f_w(nbm) : nullptr;
        cnt_true = mr_small ? mr_small + cnt_true_w(nbm) : nullptr;
        segf_ctr = mr_small ? reinterpret_cast<unsigned long long*>(mr_small + segf_ctr_w(nbm)) : nullptr;
    }
};

// The step's small results: what the host keeps of them, and the ONE table of {host destination, device source, bytes} that says
// where each comes from.  A step packs the table's items into one block on the device and fetches it with one copy; the plan sizes
// that block from the same table at its largest bin count (nk_fetch_bytes).  S: the selection state of a bin (select.h: SelState<K>).
struct NkFetchItem { void* dst; const void* src; size_t bytes; };
constexpr int NK_FETCH_MAX = 14;
// the items that do not live in the two blocks above (the step's scratch buffer; null: sizes only)
struct NkScratchSrc { const void *info, *edges, *state, *succ; };
template <typename T, typename K, typename S> struct NkStepResults {
    std::vector<uint64_t> cnt;        // [3][nb] total, below, inside of the bins' brackets (partitioned plans: rewritten for the gathered bucket values)
    std::vector<K> klo, khi;          // the bins' brackets
    unsigned long long head[NkFzWords::HEAD_FETCHED];   // ctr[8] | rbs_d | rbs_y | cnt_d[3] (total, below, inside) | ...
    uint64_t rbs = 0;
    unsigned char info[32];           // the step's info block: T vshift | n_valid | flags | double vshift
    double sums[5];
    T vhat = (T)0;
    std::vector<T> edges;
    std::vector<S> st;
    std::vector<uint64_t> succ;
    K kd[2] = {0, 0};                 // bracket of the median of dh (the next step's prediction keeps the widths of the last sampled brackets)
    std::vector<uint64_t> cnt_t;      // partitioned plans: (total, below, inside) of the bins' brackets
    void resize(int nb, bool mr) {
        cnt.resize(3 * (size_t)nb); klo.resize(nb); khi.resize(nb); edges.resize(nb + 1); st.resize(nb); succ.resize(nb);
        cnt_t.resize(mr ? 3 * (size_t)nb : 0);
    }
    const unsigned long long* ctr() const { return head + NkFzWords::CTR; }
    const unsigned long long* cnt_d() const { return head + NkFzWords::CNT_D; }
    int table(const NkFzLayout<T, K>& fz, const NkMrSmallLayout& mrs, const NkScratchSrc& sc, int nb, bool mr, NkFetchItem (&t)[NK_FETCH_MAX]) {
        int k = 0;
        t[k++] = {cnt.data(), fz.cnt_y, 8 * 3 * (size_t)nb};
        t[k++] = {klo.data(), fz.klo_y, sizeof(K) * nb};
        t[k++] = {head, fz.ctr, sizeof head};
        t[k++] = {&rbs, fz.rbs_y, 8};
        t[k++] = {info, sc.info, sizeof info};
        t[k++] = {sums, fz.sums, sizeof sums};
        t[k++] = {&vhat, fz.vhat, sizeof(T)};
        t[k++] = {edges.data(), sc.edges, sizeof(T) * (nb + 1)};
        t[k++] = {st.data(), sc.state, sizeof(S) * nb};
        t[k++] = {succ.data(), sc.succ, 8 * (size_t)nb};
        t[k++] = {khi.data(), fz.khi_y, sizeof(K) * nb};
        t[k++] = {&kd[0], fz.klo_d, sizeof(K)};
        t[k++] = {&kd[1], fz.khi_d, sizeof(K)};
        if (mr) t[k++] = {cnt_t.data(), mrs.cnt_true, 8 * 3 * (size_t)nb};
        return k;
    }
};
// offsets of the items in the packed block (16-byte aligned); returns its size
inline size_t nk_fetch_offsets(const NkFetchItem* t, int n, uint32_t* off) {
    uint32_t o = 0;
    for (int k = 0; k < n; ++k) {
        if (off) off[k] = o;
        o += (uint32_t)((t[k].bytes + 15) & ~(size_t)15);
    }
    return o;
}
// size of the packed block of a plan: the table at the plan's largest bin count, partitioned form
template <typename T, typename K, typename S> size_t nk_fetch_bytes(int nb_max) {
    NkStepResults<T, K, S> h;
    h.resize(nb_max, true);
    NkFetchItem t[NK_FETCH_MAX];
    const int n = h.table(NkFzLayout<T, K>(nullptr, nb_max), NkMrSmallLayout(nullptr, nb_max), NkScratchSrc{nullptr, nullptr, nullptr, nullptr}, nb_max, true, t);
    return nk_fetch_offsets(t, n, nullptr);
}

}  // namespace xd
