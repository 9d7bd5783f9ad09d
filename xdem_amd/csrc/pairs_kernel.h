// pairs_kernel.h -- the pair kernel of the empirical variogram (variogram.hip holds the pair set, the launch and the drivers): its
// arguments, its small device helpers and pairs_kernel itself.  The lag classes come from the host tables of pairs_classes.h, the
// dynamic LDS block from pairs_layout.h.
#pragma once
#include <math.h>
#include <type_traits>

#include "common.h"
#include "select.h"
#include "select_run.h"
#include "pairs_classes.h"
#include "pairs_layout.h"

namespace xd {

#pragma clang fp contract(off)

// spread pair sample (every-a-with-every-b blocks): B slots per lane and tile -> SPREAD_SLOTS / 256 of the pairs of every unit.
// (4 = 1/64 was the first setting; the brackets scale with 1 / sqrt(sample), the three sampled passes with the sample: 2 slots
// cost 0.1 % more candidates and save a third of the sampled passes' time on SURVEY 8d's C5)
constexpr int SPREAD_SLOTS = 2;
// (a lane's SPREAD_SLOTS slots lie PT / SPREAD_SLOTS apart, so one wave covers SPREAD_SLOTS of the tile's four 64-slot groups:
// consecutive waves start in different groups and the waves of a workgroup together cover every B point of the tile -- with one
// common start the 2-slot sample used half of the B points of a unit and its ranks scattered three times as far)
static_assert(SPREAD_SLOTS == 1 || SPREAD_SLOTS == 2 || SPREAD_SLOTS == 4, "64-slot groups");
__device__ __forceinline__ int spread_wave_offset(int tid) { return 64 * ((tid >> 6) % (4 / SPREAD_SLOTS)); }
static_assert(PAIRS_RADIX == SEL_RADIX && PAIRS_STAGE_CAP == SEL_STAGE_CAP, "pairs_layout.h restates two constants of the selection headers");

template <typename T> struct PairArgs {
    const double *ax, *ay, *bx, *by;
    const T *av, *bv;
    const int64_t *a_off, *b_off;  // per block [nblk + 1]
    const int64_t* wg_off;         // workgroups before each block [nblk + 1] (for this kernel's NT)
    int nblk, nb, pdist;
    const double* thr;  // nb thresholds on d^2
    const uint8_t* lut;  // [LUT_N] (class lower bound << 1 | cell holds a threshold) per 1/8 binade of d^2; nullptr: binary search
    int lut_emin;        // (biased exponent << 3 | top 3 mantissa bits) of LUT entry 0
    // integer-lattice path (GRID kernels): points as packed int16 lattice indexes (x | y << 16), thresholds on the integer
    // squared lattice distance, class lower bound per 1/8 binade of float(d2)
    const uint32_t *a_xy, *b_xy;
    const uint32_t* thr_i;   // [nb]
    const uint8_t* lut_i;    // [LUT_G]
    long long : 64;          // (no member: the 8 bytes a never-read table origin took.  Closing the gap moves every later argument and
                             // the implicit ones behind them -- 30 kernels then load their arguments from other offsets, the lattice sum
                             // kernels with other scalar registers -- so the block keeps the layout the kernels were measured with)
    // outputs / state
    double* sums;                  // [nb]
    unsigned long long* counts;    // [nb]
    unsigned long long* hist;      // [nb][256]
    const typename KeyT<T>::type* prefix;  // [nb] selection prefix (hist) or selected key (succ)
    unsigned long long* succ;              // [nb] 8-byte slots, all-ones = none
    int shift, first, bin0, nbs;   // hist digit, first pass flag, LDS sweep window [bin0, bin0 + nbs)
    int64_t wg_base, wg_end;       // units [wg_base, wg_end) belong to this launch (a pass over very many tiles takes several launches)
    int sample;                    // OP_HIST: only the pseudo-randomly chosen 1/64 of the (A tile x B tile) units
    // OP_HIST, dual: TWO selection states per class advance in the same pass (both ends of a bracket): a second prefix array and
    // a second histogram; an element is counted under each prefix it matches
    int dual;
    const typename KeyT<T>::type* prefix2;
    unsigned long long* hist2;
    int has_nan;                   // some value is NaN (unknown for device-resident inputs: assumed): full tiles keep the NaN test
    // OP_BRACKET (bracketed selection, select_run.h): keys in [prefix[k], khi[k]] are candidates
    const typename KeyT<T>::type* khi;
    unsigned long long* cnt3;      // [3][nb]: pairs per class at or above the bracket's low end, below it, inside the bracket
    void* cand_v;                  // candidate |dv| (T; WIDE kernels: the EXACT float64 difference of two float32 values)
    uint16_t* cand_b;              // and their class
    unsigned long long* cand_ctr;  // [0] count, [1] overflow flag
    long long cand_cap;
    int runs;                      // OP_BRACKET on the lattice: the points come in Morton order (xdemhip_pairs_link_sorted) -- run-length counting
};

// Sampled digit passes (bracketed selection): EVERY (A tile x B tile) unit contributes exactly 1/64 of its pairs.  (Round 2
// sampled whole units with probability 1/64: for values of a spatially correlated field the class distributions differ from
// block to block, the number of sampled units per block was binomial (3 +- 1.7), and the mixture weights -- hence the sample
// medians -- were too noisy for any affordable bracket.)
//  * every-a-with-every-b blocks: thread t (A point t of the tile) takes SPREAD_SLOTS B slots (h + lane + u 256 / SPREAD_SLOTS) mod
//    256, h hashed from the unit: the sampled pairs of a unit use each of its 1024 A points SPREAD_SLOTS times and each of its
//    256 B points 4 SPREAD_SLOTS times.  EVERY tile takes part: sampling every 4th tile with 16 slots per lane (a quarter of the tile loads and barriers
//    for the same pairs) was measured -- the wanted ranks then sat 0.63 half widths off the bracket centres instead of 0.04: B
//    points arrive ring by ring, a tile is one distance class of one block, and the class mixtures over the blocks get noisy.  (The first form of this round took 4 B slots for ALL A points: 1024 pairs per sampled B point, and since |v_a - v_b|
//    of a correlated field moves with v_b for all of them at once, a class of 8.5e7 sampled pairs behaved like 2e4 independent
//    draws -- brackets 8 x wider, 5 % of all pairs candidates.)
//  * i < j blocks keep 4 adjacent slots [4 h, 4 h + 4) against all A points (the diagonal test needs the uniform slot index) and
//    the wide brackets that go with them.
__device__ __forceinline__ int unit_sample_slot(int64_t wg, int tile) {
    return (int)(((uint64_t)(wg * 16 + tile) * 0x9E3779B97F4A7C15ull) >> 58);   // 0 .. 63
}

template <typename K> __device__ __forceinline__ void lds_min(K* p, K v);
template <> __device__ __forceinline__ void lds_min<uint32_t>(uint32_t* p, uint32_t v) { atomicMin(p, v); }
template <> __device__ __forceinline__ void lds_min<uint64_t>(uint64_t* p, uint64_t v) {
    atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// |dv| >= 0: its IEEE bits are already order-preserving; shifting the (always zero) sign bit out gives the first radix
// digit the full 8 exponent bits instead of sign + 7 (twice the spread of the LDS counters it hits).
__device__ __forceinline__ uint32_t key_abs(float v) { return __float_as_uint(v) << 1; }
__device__ __forceinline__ uint64_t key_abs(double v) { return (uint64_t)__double_as_longlong(v) << 1; }

typedef short v2s16 __attribute__((ext_vector_type(2)));

// r = (mask bit of this lane) ? b : a, the lane mask held in an SGPR pair (a divergent `bool` carried around a loop is
// legalised into a 0/1 VGPR and costs a compare per use; an explicit 64-bit mask stays scalar)
__device__ __forceinline__ uint32_t select_by_mask(uint32_t a, uint32_t b, unsigned long long mask) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(mask));
    return r;
}
__device__ __forceinline__ float select_by_mask(float a, float b, unsigned long long mask) {
    return __uint_as_float(select_by_mask(__float_as_uint(a), __float_as_uint(b), mask));
}
__device__ __forceinline__ double select_by_mask(double a, double b, unsigned long long mask) {
    const unsigned long long ua = (unsigned long long)__double_as_longlong(a), ub = (unsigned long long)__double_as_longlong(b);
    const uint32_t lo = select_by_mask((uint32_t)ua, (uint32_t)ub, mask), hi = select_by_mask((uint32_t)(ua >> 32), (uint32_t)(ub >> 32), mask);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <typename T> struct alignas(8) FzEnds { T lo, hi; };   // a class's bracket as values: one 8 / 16-byte LDS read

// n + (mask bit of this lane): one v_addc with the lane mask as the carry-in
__device__ __forceinline__ uint32_t add_mask_bit(uint32_t n, unsigned long long mask) {
    uint32_t r;
    unsigned long long carry_out;
    asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(r), "=s"(carry_out) : "v"(n), "s"(mask));
    return r;
}

// squared lattice distance of two packed int16 index pairs (x | y << 16): one v_pk_sub_i16 + one v_dot2_i32_i16, exact in 32 bits
// (the three-operand form with the inline constant 0: the builtin picks v_dot2c, which needs a zeroed accumulator)
__device__ __forceinline__ uint32_t lattice_d2(uint32_t pxy, uint32_t bxy) {
    const v2s16 d = __builtin_bit_cast(v2s16, pxy) - __builtin_bit_cast(v2s16, bxy);
    uint32_t d2;
    asm("v_dot2_i32_i16 %0, %1, %1, 0" : "=v"(d2) : "v"(d));
    return d2;
}
// ... of this lane's A point with tile slots j .. j + 3, and the four raw value differences (the B-point reads issued back to back)
template <typename T>
__device__ __forceinline__ void lattice_d2x4(uint32_t pxy, T pv, const uint32_t* s_bxy, const T* s_bv, int j, uint32_t (&d2)[4], T (&dv)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        d2[u] = lattice_d2(pxy, s_bxy[j + u]);
        dv[u] = pv - s_bv[j + u];
    }
}

// OP_HIST, one pair of class l (row lb of the sweep's LDS table): its key's digit counts under each selection prefix it matches --
// the class's prefix, and in a dual pass the second one too (table nbs + lb); the first digit has no prefix yet
template <typename K> struct HistDigits {
    uint32_t* s_hist;
    const K *s_pref, *s_khi;
    K himask;
    int shift, first, nbs;
    bool dual;
    __device__ __forceinline__ void add(K key, int l, int lb) const {
        const int digit = (int)((key >> shift) & 0xFF);
        if (first || (key & himask) == s_pref[l]) atomicAdd(&s_hist[lb * SEL_RADIX + digit], 1u);
        if (dual && (key & himask) == s_khi[l]) atomicAdd(&s_hist[(nbs + lb) * SEL_RADIX + digit], 1u);
    }
};

// GRID (implies FAST): the points lie on an integer lattice (raster pixel centres -- the reference's cdist / pdist samplers
// draw raster pixels, xdem/spatialstats.py:1413-1416): coordinates are packed int16 lattice indexes, the squared lattice
// distance of a pair is ONE v_pk_sub_i16 + ONE v_dot2_i32_i16, exact in 32 bits, and the class follows from integer
// thresholds that are the exact pre-images of the float64 thresholds (host: make_grid) -- identical classes, a third fewer
// instructions per pair than the float64 coordinates (5 float64 operations + a 64-bit compare).
// WIDE (float32 values only; context option "vario_diff" = 1 on float32 inputs, round 5): the pass classifies every pair by its
// float32 difference fl(a - b) exactly as the default kernel does -- same instructions in the hot loop --, but a CANDIDATE leaves
// as the exact float64 difference |double(a) - double(b)| (the B value is read again from the LDS tile when, rarely, a pair is a
// candidate).  Rounding is monotone -- fl(d1) < fl(d2) implies d1 < d2 -- so the integer counts of the float32 classification
// are exact counts below / inside / above the bracket for the exact differences too, and the order statistic selected among
// the float64 candidates at rank (r - below) IS the exact float64 one: scikit-gstat's pdist-style float64 differences at the
// speed of the float32 kernels (the float64 kernels spend 60 ms on this pass against 38).
template <typename T, bool WIDE> struct CandT { typedef T type; };
template <> struct CandT<float, true> { typedef double type; };
template <typename T, int OP, bool FAST, int NT, bool GRID = false, bool WIDE = false>
// (1024-thread workgroups: two of them per CU -- 8 waves per SIMD -- need at most 64 VGPRs: second launch-bound = waves per SIMD; float32 values only, the float64
// kernels do not fit that budget without spilling)
__global__ __launch_bounds__(NT, (NT == 1024 && sizeof(T) == 4) ? 8 : 1) void pairs_kernel(const PairArgs<T> a) {
    typedef typename KeyT<T>::type K;
    typedef typename CandT<T, WIDE>::type TC;   // what a candidate is stored as
    static_assert(!WIDE || (sizeof(T) == 4 && OP == OP_BRACKET), "WIDE: float32 values, counting pass only");
    TC* const cand_out = static_cast<TC*>(a.cand_v);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // every region of the block, what it holds and where it lies: pairs_layout.h
    PairsLdsPointers lds(smem);
    PAIRS_LDS_WALK(lds, T, OP, WIDE, a.nb, 0);   // (nbs sizes the last region only: the launch's business, no pointer depends on it)
    double* s_bx = lds.at<double>(LDS_BX);
    double* s_by = lds.at<double>(LDS_BY);
    double* s_thr = lds.at<double>(LDS_THR);
    K* s_pref = lds.at<K>(LDS_PREF);
    K* s_khi = lds.at<K>(LDS_KHI);
    T* s_bv = lds.at<T>(LDS_BV);
    uint32_t* s_bxy = lds.at<uint32_t>(LDS_BXY);
    uint32_t* s_thr_i = lds.at<uint32_t>(LDS_THR_I);
    // OP_SUMS: NCOPY privatised copies per class, copy = lane % 32: lanes of a wave that hit the same class land on
    // different banks (at most 2 lanes per address) instead of serialising 64-way on one LDS word
    constexpr int REC = PAIRS_REC;
    unsigned char* s_rec = lds.at<unsigned char>(LDS_REC);
    uint32_t* s_hist = lds.at<uint32_t>(LDS_HIST);
    K* s_min = lds.at<K>(LDS_MIN);
    unsigned long long* s_c3 = lds.at<unsigned long long>(LDS_C3);
    K* s_lh = lds.at<K>(LDS_LH);
    T* s_lhf = lds.at<T>(LDS_LHF);
    uint32_t* s_in = lds.at<uint32_t>(LDS_IN);
    constexpr int STAGE_CAP = pairs_stage_cap<WIDE>();
    BlockStage<TC, STAGE_CAP> stage;
    if (OP == OP_BRACKET) {
        stage.v = lds.at<TC>(LDS_STAGE_V);
        stage.b = lds.at<uint16_t>(LDS_STAGE_B);
        stage.base = lds.at<unsigned long long>(LDS_STAGE_BASE);
        stage.held = lds.at<int>(LDS_STAGE_HELD);
    }

    __shared__ uint8_t s_lut[GRID ? LUT_G : LUT_N];
    // GRID: class of a cell's lower bound and the one threshold above it fused into one 8-byte entry (one LDS read per pair
    // instead of a byte read and a dependent threshold read -- the Matheron pass is bound by the LDS array)
    __shared__ uint2 s_lut2[GRID ? LUT_G : 1];
    // sums on the lattice (round 4): {class of the cell's lower bound c, threshold c, threshold c - 1 (0 for c = 0), threshold c + 1}: the
    // class of a d^2 AND the d^2 interval of that class from one 16-byte read (see the run-length loop)
    __shared__ uint4 s_lut4[(GRID && (OP == OP_SUMS_SQ || OP == OP_SUMS_SQRT || OP == OP_BRACKET)) ? LUT_G : 1];
    // run-length counting pass, float32 values (round 5): everything a lane loads when its run enters class l -- the class's d^2
    // interval {low, width} and its bracket {low, high} as float bits -- in ONE 16-byte record (the interval used to be rebuilt from the
    // cell's table entry with two selects and a subtract next to the 8-byte read of the bracket)
    constexpr bool CLSREC = GRID && OP == OP_BRACKET && sizeof(T) == 4;
    __shared__ uint4 s_clsrec[CLSREC ? HIST_BINS_PER_SWEEP + 2 : 1];
    const int tid = threadIdx.x;
    if (FAST)  // (NT may be smaller than the table: round 1 loaded only its first NT entries -- wrong classes beyond 32 binades of d^2)
        for (int k = tid; k < (GRID ? LUT_G : LUT_N); k += NT) s_lut[k] = GRID ? a.lut_i[k] : a.lut[k];
    for (int k = tid; k < a.nb + LUT_STEPS + 1; k += NT) s_thr[k] = k < a.nb ? a.thr[k] : (double)INFINITY;
    if (GRID) {
        for (int k = tid; k < a.nb + 2; k += NT) s_thr_i[k] = k < a.nb ? a.thr_i[k] : 0xFFFFFFFFu;
        for (int k = tid; k < LUT_G; k += NT) {
            const uint32_t c = a.lut_i[k];
            s_lut2[k] = make_uint2(c, c < (uint32_t)a.nb ? a.thr_i[c] : 0xFFFFFFFFu);
            if (OP == OP_SUMS_SQ || OP == OP_SUMS_SQRT || OP == OP_BRACKET)
                s_lut4[k] = make_uint4(c, c < (uint32_t)a.nb ? a.thr_i[c] : 0xFFFFFFFFu, (c > 0 && c - 1 < (uint32_t)a.nb) ? a.thr_i[c - 1] : (c > 0 ? 0xFFFFFFFFu : 0u),
                                       c + 1 < (uint32_t)a.nb ? a.thr_i[c + 1] : 0xFFFFFFFFu);
        }
    }
    if (OP == OP_SUMS_SQ || OP == OP_SUMS_SQRT)
        for (int k = tid; k < (a.nb + 1) * REC / 4; k += NT) reinterpret_cast<uint32_t*>(s_rec)[k] = 0u;
    unsigned char* const s_sum_cp = s_rec + (tid & (NCOPY - 1)) * 8;              // this lane's privatised copies
    unsigned char* const s_cnt_cp = s_rec + NCOPY * 8 + (tid & (NCOPY - 1)) * 4;
    auto rec_add = [&](int l, double term) {
        const int off = l * REC;
        atomicAdd(reinterpret_cast<double*>(s_sum_cp + off), term);
        atomicAdd(reinterpret_cast<uint32_t*>(s_cnt_cp + off), 1u);
    };
    // (the first digit's histogram is the same for both states: only table A is filled, the host copies it)
    const bool dual = OP == OP_HIST && a.dual && !a.first;
    if (OP == OP_HIST)
        for (int k = tid; k < a.nbs * SEL_RADIX * (dual ? 2 : 1); k += NT) s_hist[k] = 0;
    if (dual)
        for (int k = tid; k < a.nb; k += NT) s_khi[k] = a.prefix2[k];
    if (OP == OP_SUCC)
        for (int k = tid; k < a.nb; k += NT) s_min[k] = ~(K)0;
    if ((OP == OP_HIST && !a.first) || OP == OP_SUCC || OP == OP_BRACKET)
        for (int k = tid; k < a.nb; k += NT) s_pref[k] = a.prefix[k];
    if (OP == OP_BRACKET) {
        for (int k = tid; k < a.nb; k += NT) s_khi[k] = a.khi[k];
        // (the fast loop compares the raw bits of |d| -- key_abs(d) >> 1 -- so the ends are stored halved: key >= lo <=> bits >=
        // ceil(lo / 2), key <= hi <=> bits <= floor(hi / 2); the spare class gets an unreachable low end)
        for (int k = tid; k <= a.nb; k += NT) {
            const K lo = k < a.nb ? a.prefix[k] : ~(K)0, hi = k < a.nb ? a.khi[k] : (K)0;
            const K lo_h = (K)((lo >> 1) + (lo & 1)), hi_h = (K)(hi >> 1);
            s_lh[2 * k] = lo_h;
            s_lh[2 * k + 1] = hi_h;
            // (lo_h can be 2^(bits - 1) -- the bit pattern of -0 -- when the low end is unreachable: NaN, never >= anything)
            K lo_bits = lo_h, hi_bits = hi_h;
            if (lo_h >> (8 * sizeof(K) - 1)) lo_bits = (K)~(K)0 >> 1;
            T lo_f, hi_f;
            __builtin_memcpy(&lo_f, &lo_bits, sizeof(T));
            __builtin_memcpy(&hi_f, &hi_bits, sizeof(T));
            s_lhf[2 * k] = lo_f;
            s_lhf[2 * k + 1] = hi_f;
            if constexpr (CLSREC) {
                if (k <= HIST_BINS_PER_SWEEP) {
                    const uint32_t lo_d2 = k > 0 ? a.thr_i[k - 1] : 0u, hi_d2 = k < a.nb ? a.thr_i[k] : 0xFFFFFFFFu;
                    uint32_t lb, hb;
                    __builtin_memcpy(&lb, &lo_f, 4);
                    __builtin_memcpy(&hb, &hi_f, 4);
                    s_clsrec[k] = make_uint4(lo_d2, hi_d2 - lo_d2, lb, hb);
                }
            }
        }
        for (int k = tid; k < (a.nb + 1) * NCOPY; k += NT) s_c3[k] = 0ull;
        for (int k = tid; k < a.nb + 1; k += NT) s_in[k] = 0u;
        if (tid == 0) *stage.held = 0;
    }

    const int nb = a.nb;
    const K himask = (OP == OP_HIST && !a.first) ? (K)(~(K)0 << (a.shift + 8)) : (K)0;
    const HistDigits<K> hist = {s_hist, s_pref, s_khi, himask, a.shift, a.first, a.nbs, dual};
    int run_l = a.nb;          // spare class: flushing the empty initial run adds (0, 0) to the record nobody reads
    double run_s = 0.0;
    uint32_t run_start = 0;    // position (count of plain-tile pairs so far, the same for every lane) at which the lane's run began
    uint32_t run_pos = 0;      // ... and the current position: a run's length is their difference, no per-pair counter
    uint32_t run_lo = 1u, run_w = 0u;   // GRID: d^2 interval of the run's class (empty: the first pair looks its class up)
    uint32_t run_ge = 0u;               // OP_BRACKET runs: pairs of the run at or above the bracket's low end
    T run_blo = (T)0, run_bhi = (T)0;   // ... and the bracket of the run's class
    // One workgroup = one (A tile x B chunk) unit, except in the SAMPLED digit passes: there a unit is 16 tile loads and 16 k pairs,
    // while zeroing and flushing the [classes][256] LDS tables costs ~25 k LDS writes and thousands of global atomics -- a
    // resident set of workgroups therefore walks over all units (grid-stride) and flushes once.
    __syncthreads();   // the tables above are complete (the barrier-free sampled path below reads them at once)
    for (int64_t wg = a.wg_base + blockIdx.x; wg < a.wg_end; wg += gridDim.x) {
        // which block / A tile / B chunk is this unit?
        int lo = 0, hi = a.nblk;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.wg_off[mid] <= wg) lo = mid; else hi = mid;
        }
        const int r = lo;
        const int64_t a0 = a.a_off[r], na = a.a_off[r + 1] - a0;
        const int64_t b0 = a.pdist ? a0 : a.b_off[r], nbp = a.pdist ? na : a.b_off[r + 1] - b0;
        const int64_t nchunk = (nbp + BCHUNK - 1) / BCHUNK;
        const int64_t local = wg - a.wg_off[r];
        const int64_t ta = local / nchunk, cb = local - ta * nchunk;
        const int64_t ia = ta * NT + tid;  // index inside the block's A set
        const int64_t jb0 = cb * BCHUNK, jb1 = (jb0 + BCHUNK < nbp) ? jb0 + BCHUNK : nbp;
        const bool have_a = ia < na;
        const bool skip_wg = a.pdist && (jb1 <= ta * NT + 1);  // whole chunk at or below the diagonal: no i < j pair
        double px = 0.0, py = 0.0;
        T pv = 0;
        uint32_t pxy = 0;
        if (have_a) {
            if (GRID) pxy = a.a_xy[a0 + ia];
            else { px = a.ax[a0 + ia]; py = a.ay[a0 + ia]; }
            pv = a.av[a0 + ia];
        }
        const double* gbx = a.pdist ? a.ax : a.bx;
        const double* gby = a.pdist ? a.ay : a.by;
        const uint32_t* gbxy = a.pdist ? a.a_xy : a.b_xy;
        const T* gbv = a.pdist ? a.av : a.bv;

        // OP_BRACKET, fast path: a lane keeps at most ONE candidate pending in registers; every 8 pairs the wave moves its pending
        // candidates into the staging buffer with one LDS reservation (the per-pair form -- ballot, leader atomic with return and
        // its round trip whenever any lane of the wave had a candidate, i.e. for half of all wave-pairs -- was most of the 22
        // vector instructions per pair this pass spent beyond the class lookup).  A second candidate while one is pending (a few
        // per thousand lane-octets) is appended directly.
        // OP_SUMS, full tiles: RUN-LENGTH accumulation.  The point sets are uploaded in Morton order (PairSet: neighbouring slots are
        // neighbouring points), so consecutive B points of a tile mostly fall into the same lag class of a lane's A point: the lane
        // keeps the running sum and count of its current class in registers and touches the LDS record -- two atomics -- only when
        // the class changes.  (Round 2 paid both atomics for every pair and the LDS array was busy for the whole kernel.)
        TC pend_v = (TC)0;
        uint32_t pend_l = 0;
        // the value a candidate is stored as: the pair's |dv| as classified, or (WIDE) the exact float64 difference with tile slot j
        auto cand_value = [&](T abs_dv, int j) -> TC {
            if constexpr (WIDE) return (TC)__builtin_fabs((double)pv - (double)s_bv[j]);
            else return abs_dv;
        };
        unsigned long long pend_m = 0;  // lanes with a pending candidate (wave-uniform scalar)
        // Candidates that find the staging buffer full go straight to the global candidate buffer, one global atomic per wave and
        // call.  (Values of a spatially correlated field cluster: all 262144 pairs of a tile -- 1024 neighbouring A points x 256 B
        // points -- can fall into a class's bracket at once, far more than the 8192 staging slots a tile may fill; round 2's "flag
        // an overflow and redo everything with plain passes" made the C5 input of SURVEY 8d five times slower than uniform noise.)
        auto spill = [&](bool mine, TC v, uint32_t l) {   // every lane of the wave calls this
            const unsigned long long ov = __builtin_amdgcn_ballot_w64(mine);
            if (!ov) return;
            const int lane = tid & 63;
            const int leader = __ffsll((long long)ov) - 1;
            unsigned long long base = 0;
            if (lane == leader) base = atomicAdd(&a.cand_ctr[0], (unsigned long long)__popcll(ov));
            base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(base >> 32), leader) << 32) |
                   (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)base, leader);
            if (mine) {
                const unsigned long long pos = base + (unsigned long long)__builtin_amdgcn_mbcnt_hi((uint32_t)(ov >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ov, 0u));
                if ((long long)pos < a.cand_cap) { cand_out[pos] = v; a.cand_b[pos] = (uint16_t)l; }
                else a.cand_ctr[1] = 1ull;
            }
        };
        auto flush_pending = [&](bool tally = false) {
            const unsigned long long m = pend_m;
            if (m) {  // (wave-uniform)
                const int lane = tid & 63;
                const int leader = __ffsll((long long)m) - 1;
                int pos0 = 0;
                if (lane == leader) pos0 = atomicAdd(stage.held, __popcll(m));
                pos0 = __builtin_amdgcn_readlane(pos0, leader);
                const bool has = (m >> lane) & 1ull;
                const int pos = pos0 + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (has && pos < STAGE_CAP) { stage.v[pos] = pend_v; stage.b[pos] = (uint16_t)pend_l; }
                if (tally && has) atomicAdd(&s_in[pend_l], 1u);
                if (__builtin_expect(pos0 + __popcll(m) > STAGE_CAP, 0)) spill(has && pos >= STAGE_CAP, pend_v, pend_l);   // (wave-uniform test)
                pend_m = 0;
            }
        };
        // Sampled pass over every-a-with-every-b blocks on the integer lattice, straight from global memory: a lane needs 4 B points
        // of each tile (slots h + lane + 64 u: consecutive over the lanes, so the loads coalesce), which is not worth a 256-point
        // LDS tile and two barriers -- that form left a workgroup waiting for one tile load at a time, 2.6 us per tile and 3.4 ms
        // per pass.  Four tiles per trip: 16 independent pairs (32 loads) per lane in flight, no barrier, waves run on their own.
        if constexpr (GRID && OP == OP_HIST) {
            if (a.sample && !a.pdist) {   // (uniform over the launch)
                const int lane = tid & 63;
                for (int64_t j0 = jb0; j0 < jb1; j0 += 4 * PT) {
                    uint32_t bxy[4 * SPREAD_SLOTS];
                    T bvv[4 * SPREAD_SLOTS];
                    bool okk[4 * SPREAD_SLOTS];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int64_t jt = j0 + (int64_t)t * PT;
                        const int h = unit_sample_slot(wg, (int)((jt - jb0) / PT));
                        const int64_t cnt_t = jb1 - jt;   // (<= 0: no such tile)
#pragma unroll
                        for (int u = 0; u < SPREAD_SLOTS; ++u) {
                            const int sj = (h + lane + spread_wave_offset(tid) + (PT / SPREAD_SLOTS) * u) & (PT - 1);
                            const bool ok = have_a && sj < cnt_t;
                            const int64_t src = b0 + (ok ? jt + sj : jb0);
                            okk[SPREAD_SLOTS * t + u] = ok;
                            bxy[SPREAD_SLOTS * t + u] = gbxy[src];
                            bvv[SPREAD_SLOTS * t + u] = gbv[src];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 4 * SPREAD_SLOTS; ++q) {
                        const uint32_t d2 = lattice_d2(pxy, bxy[q]);
                        const uint32_t cell = __float_as_uint((float)d2) >> 20;
                        const uint2 e = s_lut2[(cell > LUT_G0 ? cell : (uint32_t)LUT_G0) - LUT_G0];
                        const int lu = (int)e.x + ((e.y <= d2) ? 1 : 0);
                        T dd = pv - bvv[q];
                        dd = dd < 0 ? -dd : dd;
                        const int lb = lu - a.bin0;
                        if (okk[q] && lu < nb && dd == dd && lb >= 0 && lb < a.nbs) {
                            hist.add(key_abs(dd), lu, lb);
                        }
                    }
                }
                continue;   // next unit
            }
        }
        if (!skip_wg)
            for (int64_t j0 = jb0; j0 < jb1; j0 += PT) {
                // sampled pass: only slots [jbeg, jend) of this tile (uniform over the workgroup)
                const bool sampled = OP == OP_HIST && a.sample;
                const int jslot = sampled ? 4 * unit_sample_slot(wg, (int)((j0 - jb0) / PT)) : 0;
                if (OP == OP_BRACKET)  // (starts with the barrier the tile reload needs); flush the staged candidates when half full
                    stage.sync_and_flush_at(STAGE_CAP / 2, cand_out, a.cand_b, &a.cand_ctr[0], a.cand_cap, &a.cand_ctr[1]);
                else
                    __syncthreads();
                const int cnt = (int)((jb1 - j0) < PT ? (jb1 - j0) : PT);
                // sampled pass over every-a-with-every-b blocks: per-lane slots (see unit_sample_slot), the whole tile is loaded
                const bool spread = sampled && !a.pdist;
                const int hslot = jslot >> 2;
                if (tid < cnt) {
                    if (GRID) s_bxy[tid] = gbxy[b0 + j0 + tid];
                    else { s_bx[tid] = gbx[b0 + j0 + tid]; s_by[tid] = gby[b0 + j0 + tid]; }
                    s_bv[tid] = gbv[b0 + j0 + tid];
                }
                __syncthreads();
                if (!have_a && OP != OP_BRACKET) continue;   // (OP_BRACKET: every thread stays for the mid-tile flush barriers)
                // OP_BRACKET, one pair: counters + staged candidate (every lane of the wave must reach the append)
                auto bracket_pair = [&](bool ok, int l, T d, int j) {
                    bool cand = false;
                    if (ok) {
                        const K key = key_abs(d);
                        const int cp = tid & (NCOPY - 1);
                        // one packed counter update per pair (see s_c3)
                        const bool below = key < s_pref[l];
                        cand = !below && key <= s_khi[l];
                        atomicAdd(&s_c3[l * NCOPY + cp], 1ull | (below ? 0ull : (1ull << 21)) | ((below || cand) ? 0ull : (1ull << 42)));
                    }
                    {   // staged append (one LDS reservation per wave); what does not fit the staging buffer spills to global memory
                        const unsigned long long cm = __builtin_amdgcn_ballot_w64(cand);
                        if (cm) {
                            const int lane = tid & 63, leader = __ffsll((long long)cm) - 1;
                            int pos0 = 0;
                            if (lane == leader) pos0 = atomicAdd(stage.held, __popcll(cm));
                            pos0 = __builtin_amdgcn_readlane(pos0, leader);
                            const int pos = pos0 + __popcll(cm & ((1ull << lane) - 1ull));
                            const TC dw = cand ? cand_value(d, j) : (TC)0;
                            if (cand && pos < STAGE_CAP) { stage.v[pos] = dw; stage.b[pos] = (uint16_t)l; }
                            if (pos0 + __popcll(cm) > STAGE_CAP) spill(cand && pos >= STAGE_CAP, dw, (uint32_t)l);
                        }
                    }
                };
                // One pair: class lookup + accumulate.  `ok` folds every skip rule so the fast path stays branch-free
                // up to the (exec-masked) LDS atomics.
                auto pair = [&](int j, bool ok) {
                    const double dx = px - s_bx[j], dy = py - s_by[j];
                    const double s2 = dx * dx + dy * dy;  // not contracted: same rounding as NumPy's dx**2 + dy**2
                    int l;  // class = number of thresholds <= s2
                    if (FAST) {
                        // 1/8-binade cell of s2 -> class lower bound; only cells that contain a threshold (1 in 8 for the
                        // reference's sqrt(2)-geometric edges) need the one exact compare against it
                        int e = (int)((unsigned long long)__double_as_longlong(s2) >> 49) - a.lut_emin;
                        e = e < 0 ? 0 : (e > LUT_N - 1 ? LUT_N - 1 : e);
                        const int c = s_lut[e];
                        l = c >> 1;
                        if (c & 1) l += (s_thr[l] <= s2) ? 1 : 0;
                    } else {
                        l = 0;
                        int h = nb;
                        while (l < h) {
                            const int m = (l + h) >> 1;
                            if (s_thr[m] <= s2) l = m + 1; else h = m;
                        }
                    }
                    T d = pv - s_bv[j];
                    d = d < 0 ? -d : d;
                    ok = ok && (l < nb) && (d == d);  // beyond the last edge (maxlag) / NaN values never form a pair
                    if (OP == OP_BRACKET) { bracket_pair(ok, l, d, j); return; }
                    if (!ok) return;
                    if (OP == OP_SUMS_SQ) {
                        rec_add(l, (double)d * (double)d);
                    } else if (OP == OP_SUMS_SQRT) {
                        rec_add(l, sqrt((double)d));
                    } else if (OP == OP_HIST) {
                        const int lb = l - a.bin0;
                        if (lb < 0 || lb >= a.nbs) return;
                        hist.add(key_abs(d), l, lb);
                    } else if (OP == OP_SUCC) {
                        const K key = key_abs(d);
                        if (key > s_pref[l] && key < s_min[l]) lds_min<K>(&s_min[l], key);
                    }
                };

                // classes of the 4 pairs (this lane's A point) x (tile slots j .. j + 3) and their raw value differences, written
                // stage by stage so that the B-point reads, the table reads and the threshold reads are each issued back to back
                auto classify4 = [&](const int (&js)[4], int (&lu)[4], T (&dv)[4]) {
                    if constexpr (GRID) {
                        uint32_t d2[4];
    #pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            d2[u] = lattice_d2(pxy, s_bxy[js[u]]);
                            dv[u] = pv - s_bv[js[u]];
                        }
                        uint2 e[4];
    #pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            // 1/8-binade cell of float(d2) (monotone in d2); d2 = 0 (coincident points) clamps onto the first cell
                            const uint32_t cell = __float_as_uint((float)d2[u]) >> 20;
                            e[u] = s_lut2[(cell > LUT_G0 ? cell : (uint32_t)LUT_G0) - LUT_G0];
                        }
    #pragma unroll
                        for (int u = 0; u < 4; ++u) lu[u] = (int)e[u].x + ((e[u].y <= d2[u]) ? 1 : 0);
                    } else {
                        double s2[4];
    #pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const double dx = px - s_bx[js[u]], dy = py - s_by[js[u]];
                            s2[u] = dx * dx + dy * dy;  // not contracted: same rounding as NumPy's dx**2 + dy**2
                            dv[u] = pv - s_bv[js[u]];
                        }
                        int l[4];
    #pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            int e = (int)((unsigned long long)__double_as_longlong(s2[u]) >> 49) - a.lut_emin;
                            e = e < 0 ? 0 : (e > LUT_N - 1 ? LUT_N - 1 : e);
                            l[u] = s_lut[e] >> 1;
                        }
                        double th[4];
    #pragma unroll
                        for (int u = 0; u < 4; ++u) th[u] = s_thr[l[u]];  // next threshold above the cell's lower bound
    #pragma unroll
                        for (int u = 0; u < 4; ++u) lu[u] = l[u] + ((th[u] <= s2[u]) ? 1 : 0);  // class = number of thresholds <= s2
                    }
                };
                if (FAST) {
                    // 4 pairs per trip, written stage by stage so that the 4 B-point reads, the 4 table reads and the 4
                    // threshold reads are each issued back to back (one LDS round trip per stage instead of per pair).
                    // Tile slots beyond cnt hold stale data and are masked by `ok`.
                    const int64_t rel = ia - j0;  // pdist: only B indices j > rel pair with this lane's A point
                    // (a thread without an A point -- last A tile of a block -- pairs with nothing: every slot masked)
                    const int ia_rel = !have_a ? PT : (a.pdist ? (int)(rel < -1 ? -1 : (rel > PT ? PT : rel)) : -1);
                    // Full tiles (the bulk of the pairs): every slot is a pair -- no index, diagonal, class or NaN test and no
                    // exec masking; the class beyond the last edge lands in the spare record.
                    const bool plain_tile = (OP == OP_SUMS_SQ || OP == OP_SUMS_SQRT) && cnt == PT && !a.has_nan &&
                                            (!a.pdist || j0 >= (ta + 1) * (int64_t)NT);
                    if (plain_tile) {
                        if constexpr (GRID) {
                            // Round 4: no class lookup per pair.  A lane keeps the d^2 interval [run_lo, run_lo + run_w) of the lag class
                            // its run is in (integer thresholds: exact pre-images of the float64 edges) -- a pair that stays in the
                            // class costs one subtract and one unsigned compare instead of the table lookup (convert, cell, table
                            // read, threshold compare, class compare: 9 vector instructions); only a pair that LEAVES the class
                            // -- 5 % of the pairs of a lane, a third of the wave-pairs on SURVEY 8d's C5 geometry -- looks its
                            // class up, flushes the run (the run's length is the distance of its positions: no counter per pair)
                            // and loads the new bounds.
                            for (int j = 0; j < PT; j += 4) {
                                uint32_t d2[4];
                                T dv[4];
                                lattice_d2x4<T>(pxy, pv, s_bxy, s_bv, j, d2, dv);
    #pragma unroll
                                for (int u = 0; u < 4; ++u) {
                                    if (!((uint32_t)(d2[u] - run_lo) < run_w)) {   // (exec-masked; skipped by the whole wave while every lane stays in its class)
                                        const uint32_t cell = __float_as_uint((float)d2[u]) >> 20;
                                        const uint4 e = s_lut4[(cell > LUT_G0 ? cell : (uint32_t)LUT_G0) - LUT_G0];
                                        const bool up = e.y <= d2[u];   // the cell's one threshold lies at or below d^2: the class above it
                                        const int off = (int)__umul24((unsigned)run_l, (unsigned)REC);
                                        atomicAdd(reinterpret_cast<double*>(s_sum_cp + off), run_s);
                                        atomicAdd(reinterpret_cast<uint32_t*>(s_cnt_cp + off), run_pos - run_start);
                                        run_l = (int)e.x + (up ? 1 : 0);
                                        run_s = 0.0;
                                        run_start = run_pos;
                                        run_lo = up ? e.y : e.z;
                                        run_w = (up ? e.w : e.y) - run_lo;   // (beyond the last edge: thresholds padded with all ones)
                                    }
                                    const double dd = (double)dv[u];
                                    run_s = OP == OP_SUMS_SQ ? __builtin_fma(dd, dd, run_s) : run_s + sqrt(fabs(dd));
                                    run_pos += 1;   // (uniform: a scalar counter)
                                }
                            }
                            continue;
                        }
                        for (int j = 0; j < PT; j += 4) {
                            int lu[4];
                            T dv[4];
                            const int js[4] = {j, j + 1, j + 2, j + 3};
                            classify4(js, lu, dv);
    #pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const double dd = (double)dv[u];
                                if (lu[u] != run_l) {   // (exec-masked; skipped by the whole wave while every lane stays in its class)
                                    const int off = run_l * REC;
                                    atomicAdd(reinterpret_cast<double*>(s_sum_cp + off), run_s);
                                    atomicAdd(reinterpret_cast<uint32_t*>(s_cnt_cp + off), run_pos - run_start);
                                    run_l = lu[u];
                                    run_s = 0.0;
                                    run_start = run_pos;
                                }
                                run_s = OP == OP_SUMS_SQ ? __builtin_fma(dd, dd, run_s) : run_s + sqrt(fabs(dd));
                                run_pos += 1;
                            }
                        }
                        continue;
                    }
                    if constexpr (OP == OP_BRACKET && GRID) {
                        // Round 4: run-length counting.  With the points in Morton order a lane's pairs stay in one lag class for ~20
                        // pairs at a stretch: the lane keeps the class's d^2 interval and bracket in registers and counts in registers
                        // (two compares of |dv| against the bracket ends, two carry adds); the packed LDS counter gets ONE ds_add_u64
                        // per run instead of one per pair, and the class lookup and the read of the bracket ends happen once per run
                        // (19 -> 9 vector instructions and 4 -> 2 LDS operations per pair that stays in its class).
                        // (a lane without an A point -- last A tile of a block -- sits in the spare class for good: an interval nothing leaves,
                        // a low end nothing reaches)
                        if (a.runs && cnt == PT && !a.has_nan && (!a.pdist || j0 >= (ta + 1) * (int64_t)NT)) {
                            if (!have_a && run_w != 0xFFFFFFFFu) {
                                const unsigned long long inc = (unsigned long long)(run_pos - run_start) | ((unsigned long long)run_ge << 21) | ((unsigned long long)run_ge << 42);
                                atomicAdd(s_c3 + (size_t)run_l * NCOPY + (tid & (NCOPY - 1)), inc);
                                run_l = nb; run_ge = 0u; run_start = run_pos; run_lo = 0u; run_w = 0xFFFFFFFFu;
                                run_blo = s_lhf[2 * nb]; run_bhi = s_lhf[2 * nb + 1];
                            }
                            static_assert(NCOPY * 8 == 256, "counter records are 256 bytes");
                            unsigned char* const c3_mine = reinterpret_cast<unsigned char*>(s_c3 + (tid & (NCOPY - 1)));
                            // every fourth tile all lanes look their class up again: a run then holds at most 4 PT = 2^10 pairs and its
                            // counts pack with two shifts (no 64-bit arithmetic)
                            static_assert(4 * PT <= 1024, "a run's count of pairs >= the low end must fit 11 bits");
                            if ((((j0 - jb0) / PT) & 3) == 0 && have_a) run_w = 0u;
                            for (int j = 0; j < PT; j += 4) {
                                uint32_t d2[4];
                                T dv[4];
                                lattice_d2x4<T>(pxy, pv, s_bxy, s_bv, j, d2, dv);
    #pragma unroll
                                for (int u = 0; u < 4; ++u) {
                                    if (!((uint32_t)(d2[u] - run_lo) < run_w)) {   // (exec-masked; skipped by the whole wave while every lane stays in its class)
                                        const uint32_t cell = __float_as_uint((float)d2[u]) >> 20;
                                        const uint4 e = s_lut4[(cell > LUT_G0 ? cell : (uint32_t)LUT_G0) - LUT_G0];
                                        const bool up = e.y <= d2[u];
                                        // packed counter: pairs | >= low end | "above" (here: >= low end as well -- the candidates among
                                        // them are tallied in s_in and taken off at the end); a run holds <= 1024 pairs (see below)
                                        const uint32_t inc_lo = (run_ge << 21) | (run_pos - run_start), inc_hi = run_ge << 10;
                                        atomicAdd(reinterpret_cast<unsigned long long*>(c3_mine + ((uint32_t)run_l << 8)), ((unsigned long long)inc_hi << 32) | inc_lo);
                                        run_l = (int)e.x + (up ? 1 : 0);
                                        run_ge = 0u;
                                        run_start = run_pos;
                                        if constexpr (CLSREC) {
                                            const uint4 cr = s_clsrec[run_l];
                                            run_lo = cr.x;
                                            run_w = cr.y;
                                            __builtin_memcpy(&run_blo, &cr.z, 4);
                                            __builtin_memcpy(&run_bhi, &cr.w, 4);
                                        } else {
                                            run_lo = up ? e.y : e.z;
                                            run_w = (up ? e.w : e.y) - run_lo;
                                            const FzEnds<T> be = *reinterpret_cast<const FzEnds<T>*>(s_lhf + 2 * run_l);
                                            run_blo = be.lo;
                                            run_bhi = be.hi;
                                        }
                                    }
                                    const T ad = sizeof(T) == 4 ? (T)__builtin_fabsf((float)dv[u]) : (T)__builtin_fabs((double)dv[u]);
                                    const unsigned long long m_ge = __builtin_amdgcn_ballot_w64(ad >= run_blo);
                                    const unsigned long long in = m_ge & ~__builtin_amdgcn_ballot_w64(ad > run_bhi);   // (an empty bracket, hi < lo: nothing inside)
                                    run_ge = add_mask_bit(run_ge, m_ge);
                                    if (in != 0) {   // (wave-uniform: a fifth of the wave-pairs hold a candidate)
                                        if (__builtin_expect((in & pend_m) != 0, 0)) flush_pending(true);
                                        const unsigned long long take = in & ~pend_m;
                                        pend_v = select_by_mask(pend_v, cand_value(ad, j + u), take);
                                        pend_l = select_by_mask(pend_l, (uint32_t)run_l, take);
                                        pend_m |= take;
                                    }
                                    run_pos += 1;
                                }
                                if ((j & 28) == 28) flush_pending(true);   // every 32 pairs (a second candidate of a lane before that flushes at once)
                                if ((j & 63) == 60 && j + 4 < PT)
                                    stage.sync_and_flush_at(STAGE_CAP / 4, cand_out, a.cand_b, &a.cand_ctr[0], a.cand_cap, &a.cand_ctr[1]);
                            }
                            continue;
                        }
                    }
                    auto run4 = [&](auto plain_tag) {
                        constexpr bool PLAIN = decltype(plain_tag)::value;  // every slot of the tile is a pair: no index / diagonal / NaN tests
                        const int jbeg = spread ? 0 : jslot;
                        const int jend = spread ? 4 : (sampled ? (jslot + 4 < cnt ? jslot + 4 : cnt) : cnt);
                        const int cnt_m = cnt;   // slots at or beyond this hold no point of the tile
                        for (int j = jbeg; j < jend; j += 4) {
                            int lus[4];
                            T dv[4];
                            int js[4];
    #pragma unroll
                            for (int u = 0; u < 4; ++u) js[u] = spread ? ((hslot + (tid & 63) + spread_wave_offset(tid) + (PT / SPREAD_SLOTS) * (j + u)) & (PT - 1)) : j + u;
                            classify4(js, lus, dv);
                            if constexpr (OP == OP_BRACKET) {
                                static_assert(NCOPY * 8 == 256, "counter records are 256 bytes");
                                unsigned char* const c3_mine = reinterpret_cast<unsigned char*>(s_c3 + (tid & (NCOPY - 1)));
                                int lc[4];
                                K lo4[4], hi4[4];
                                unsigned long long in4[4];
        #pragma unroll
                                for (int u = 0; u < 4; ++u) {
                                    dv[u] = fabs(dv[u]);
                                    // everything that is no pair goes to the spare class nb (the class lookup itself never exceeds nb:
                                    // "beyond the last edge" IS class nb, so full tiles need no test at all)
                                    if constexpr (PLAIN) lc[u] = lus[u];
                                    else lc[u] = (js[u] < cnt_m && js[u] > ia_rel && dv[u] == dv[u]) ? lus[u] : nb;
                                    if constexpr (sizeof(K) == 4) {   // one 8-byte read (its constant offset folds into the instruction)
                                        const uint2 lh = *reinterpret_cast<const uint2*>(s_lh + 2 * lc[u]);
                                        lo4[u] = lh.x;
                                        hi4[u] = lh.y;
                                    } else {
                                        lo4[u] = s_lh[2 * lc[u]];
                                        hi4[u] = s_lh[2 * lc[u] + 1];
                                    }
                                }
        #pragma unroll
                                for (int u = 0; u < 4; ++u) {
                                    const K bits = key_abs(dv[u]) >> 1;  // (|d| has no sign bit: its raw bits order like the keys)
                                    // counter plane = (bits >= lo) + (bits > hi): 0 below the bracket, 1 inside, 2 above -- two compares,
                                    // two carry adds, one multiply-add for the address (no selects)
                                    const bool ge_lo = bits >= lo4[u], gt_hi = bits > hi4[u];
                                    // (lane masks handled as scalars: a `bool` combined in C++ comes back as a 0/1 VGPR and a compare)
                                    const unsigned long long m_ge = __builtin_amdgcn_ballot_w64(ge_lo), m_gt = __builtin_amdgcn_ballot_w64(gt_hi);
                                    const unsigned long long m_gt2 = m_ge & m_gt;  // (an empty bracket, hi < lo: everything below or above)
                                    in4[u] = m_ge & ~m_gt;
                                    const unsigned long long inc = (unsigned long long)select_by_mask(1u, 1u | (1u << 21), m_ge) |
                                                                   ((unsigned long long)select_by_mask(0u, 1u << 10, m_gt2) << 32);
                                    atomicAdd(reinterpret_cast<unsigned long long*>(c3_mine + ((uint32_t)lc[u] << 8)), inc);
                                }
                                // Candidates (0.3 % of the pairs): nearly half of the wave-trips hold none in their 256 lane-pairs and
                                // skip this altogether (one scalar test per trip instead of two selects per pair)
                                if ((in4[0] | in4[1] | in4[2] | in4[3]) != 0) {
        #pragma unroll
                                    for (int u = 0; u < 4; ++u) {
                                        // (wave-uniform, rare: a second candidate of some lane before the next flush -- the pending ones
                                        // leave first, one LDS reservation for the wave, and the lane keeps the new one)
                                        if (__builtin_expect((in4[u] & pend_m) != 0, 0)) flush_pending();
                                        const unsigned long long take = in4[u] & ~pend_m;
                                        pend_v = select_by_mask(pend_v, cand_value(dv[u], js[u]), take);
                                        pend_l = select_by_mask(pend_l, (uint32_t)lc[u], take);
                                        pend_m |= take;
                                    }
                                }
                                if ((j & 12) == 12) flush_pending();  // every fourth stage = 16 pairs (brackets hold < 1 % of the pairs)
                                // every 64 B slots (65536 pairs of the workgroup) the staged candidates leave if the buffer is a quarter full:
                                // the brackets of spatially correlated values hold a few per cent of the pairs, a whole tile's worth
                                // would not fit (j and cnt are uniform over the workgroup: every thread meets this barrier)
                                if ((j & 63) == 60 && j + 4 < jend)
                                    stage.sync_and_flush_at(STAGE_CAP / 4, cand_out, a.cand_b, &a.cand_ctr[0], a.cand_cap, &a.cand_ctr[1]);
                                continue;
                            }
        #pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const int lu = lus[u];
                                dv[u] = dv[u] < 0 ? -dv[u] : dv[u];
                                const T d = dv[u];
                                const bool ok = (PLAIN || (js[u] < cnt_m && js[u] > ia_rel && d == d)) && lu < nb && (!spread || u < SPREAD_SLOTS);   // (a trip = 4 pairs: the first SPREAD_SLOTS are the sampled ones)
                                if (OP == OP_BRACKET) {
                                    bracket_pair(ok, lu, d, js[u]);
                                } else if (ok) {
                                    if (OP == OP_SUMS_SQ) {
                                        rec_add(lu, (double)d * (double)d);
                                    } else if (OP == OP_SUMS_SQRT) {
                                        rec_add(lu, sqrt((double)d));
                                    } else if (OP == OP_HIST) {
                                        const int lb = lu - a.bin0;
                                        const K key = key_abs(d);
                                        if (lb >= 0 && lb < a.nbs) hist.add(key, lu, lb);
                                    } else if (OP == OP_SUCC) {
                                        const K key = key_abs(d);
                                        if (key > s_pref[lu] && key < s_min[lu]) lds_min<K>(&s_min[lu], key);
                                    }
                                }
                            }
                        }
                    };
                    // (PLAIN needs every thread of the workgroup to hold an A point: uniform, the mid-tile barriers sit inside run4)
                    if (cnt == PT && !a.has_nan && (!a.pdist || j0 >= (ta + 1) * (int64_t)NT) && (ta + 1) * (int64_t)NT <= na) run4(std::true_type());
                    else run4(std::false_type());
                    if (OP == OP_BRACKET) flush_pending();  // (a tile's pair count need not be a multiple of 8)
                } else {
                    if (spread) {
                        for (int u = 0; u < SPREAD_SLOTS; ++u) {
                            const int sj = (hslot + (tid & 63) + spread_wave_offset(tid) + (PT / SPREAD_SLOTS) * u) & (PT - 1);
                            pair(sj, have_a && sj < cnt);
                        }
                    } else {
                        const int jend = sampled ? (jslot + 4 < cnt ? jslot + 4 : cnt) : cnt;
                        for (int j = jslot; j < jend; ++j) pair(j, have_a && (!a.pdist || (j0 + j) > ia));
                    }
                }
            }
    }
    if ((OP == OP_SUMS_SQ || OP == OP_SUMS_SQRT) && run_pos != run_start) {   // the open run of every lane
        const int off = run_l * REC;
        atomicAdd(reinterpret_cast<double*>(s_sum_cp + off), run_s);
        atomicAdd(reinterpret_cast<uint32_t*>(s_cnt_cp + off), run_pos - run_start);
    }
    if (OP == OP_BRACKET && run_pos != run_start) {   // (run-length counting: the open run of every lane)
        const unsigned long long inc = (unsigned long long)(run_pos - run_start) | ((unsigned long long)run_ge << 21) | ((unsigned long long)run_ge << 42);
        atomicAdd(s_c3 + (size_t)run_l * NCOPY + (tid & (NCOPY - 1)), inc);
    }
    __syncthreads();
    if (OP == OP_SUMS_SQ || OP == OP_SUMS_SQRT) {
        for (int k = tid; k < nb; k += NT) {
            unsigned long long c = 0;
            double sm = 0.0;
            for (int q = 0; q < NCOPY; ++q) {
                const unsigned char* r = s_rec + k * REC;
                c += reinterpret_cast<const uint32_t*>(r + NCOPY * 8)[q];
                sm += reinterpret_cast<const double*>(r)[q];
            }
            if (c) { atomicAdd(&a.counts[k], c); atomicAdd(&a.sums[k], sm); }
        }
    } else if (OP == OP_HIST) {
        for (int k = tid; k < a.nbs * SEL_RADIX; k += NT)
            if (s_hist[k]) atomicAdd(&a.hist[(size_t)a.bin0 * SEL_RADIX + k], (unsigned long long)s_hist[k]);
        if (dual)
            for (int k = tid; k < a.nbs * SEL_RADIX; k += NT) {
                const uint32_t c = s_hist[a.nbs * SEL_RADIX + k];
                if (c) atomicAdd(&a.hist2[(size_t)a.bin0 * SEL_RADIX + k], (unsigned long long)c);
            }
    } else if (OP == OP_BRACKET) {
        stage.sync_and_flush_at(0, cand_out, a.cand_b, &a.cand_ctr[0], a.cand_cap, &a.cand_ctr[1]);
        for (int k = tid; k < nb; k += NT) {
            unsigned long long above = 0, below = 0, inside = 0;
            for (int q = 0; q < NCOPY; ++q) {
                const unsigned long long c = s_c3[k * NCOPY + q];
                const unsigned long long total = c & 0x1FFFFFull, ge = (c >> 21) & 0x1FFFFFull, gt = (c >> 42) & 0x1FFFFFull;
                below += total - ge;
                inside += ge - gt;
                above += gt;
            }
            // (run-length loop: its pairs at or above the low end sit in BOTH upper fields; the candidates among them were tallied)
            inside += s_in[k];
            above -= s_in[k];
            if (above + inside) atomicAdd(&a.cnt3[k], above + inside);  // [0]: at or above the bracket's low end
            if (below) atomicAdd(&a.cnt3[nb + k], below);
            if (inside) atomicAdd(&a.cnt3[2 * nb + k], inside);
        }
    } else {
        for (int k = tid; k < nb; k += NT)
            if (s_min[k] != ~(K)0) atomicMin(&a.succ[k], (unsigned long long)s_min[k]);
    }
}

}  // namespace xd
