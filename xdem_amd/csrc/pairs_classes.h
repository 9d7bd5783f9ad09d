// pairs_classes.h -- the host arithmetic that decides every pair's lag class (variogram.hip: xdemhip_pairs_create), and the constants
// the pair kernel (pairs_kernel.h) shares with it: thresholds on the squared distance that are exact images of the edges under
// sqrt, the binade table over d^2, and the integer-lattice analysis of a pair set (make_grid).  No HIP include: the CPU tests
// (tests/test_pairs_host.py) compile it with g++ and compare every rule with its restatement in NumPy.
#pragma once
#include <math.h>
#include <sched.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <vector>

namespace xd {

constexpr int PT = 256;      // B points per LDS tile; A points per workgroup = NT (256 for sums / succ, 1024 for histograms)
constexpr int BCHUNK = 4096;  // B points per workgroup
constexpr int LUT_N = 512;    // cells (1/8 binade of d^2 each) of the class lookup table
constexpr int LUT_G = 256;    // GRID: cells of float(d2) from LUT_G0 on (d2 = 1 is cell 1016, d2 < 2^32 ends at 1272): 64 dwords = one per LDS bank
constexpr int LUT_G0 = 1016;
constexpr int LUT_STEPS = 1;  // a cell holds at most ONE threshold (host-checked), flagged in the entry's low bit
constexpr int NCOPY = 32;     // privatised accumulator copies (copy = lane % 32 -> one LDS bank per copy)
constexpr int HIST_BINS_PER_SWEEP = 128;   // classes of one histogram sweep's LDS table = the most lag classes a bracketed selection takes

// smallest double t with sqrt(t) >= e (round-to-nearest sqrt is monotone): d >= e  <=>  d^2-sum >= t
inline double sq_threshold(double e) {
    if (!(e > 0)) return 0.0;
    double t = e * e;
    while (sqrt(t) >= e) t = nextafter(t, 0.0);
    while (sqrt(t) < e) t = nextafter(t, INFINITY);
    return t;
}

// right-closed classes (context option "vario_edge" = 1): smallest double t with sqrt(t) > e
inline double sq_threshold_strict(double e) {
    if (!(e > 0)) return nextafter(0.0, INFINITY);
    double t = e * e;
    while (sqrt(t) > e) t = nextafter(t, 0.0);
    while (!(sqrt(t) > e)) t = nextafter(t, INFINITY);
    return t;
}

// Class lookup table over d^2: cell i covers [lo_i, lo_{i+1}) with lo_i the double whose top 15 bits (biased
// exponent, first 3 mantissa bits) are emin + i; entry = (number of thresholds <= lo_i) << 1 | (a threshold lies
// inside the cell).  Used only if no cell holds more than one threshold and there are < 128 classes (true for the
// reference's sqrt(2)-geometric edges: one threshold per binade = per 8 cells); otherwise (false) binary search.
// `lut` gets LUT_N entries; `emin` is set either way.
inline bool build_binade_lut(const std::vector<double>& thr, std::vector<uint8_t>& lut, int& emin) {
    const int n_bins = (int)thr.size();
    lut.assign(LUT_N, 0);
    emin = 0;
    if (n_bins < 1 || n_bins > 127) return false;
    bool lut_ok = true;
    uint64_t bits;
    memcpy(&bits, &thr[0], 8);
    emin = (int)(bits >> 49) - 1;  // cell 0 lies strictly below every threshold: smaller d^2 clamp onto it
    if (emin < 8) emin = 8;
    auto cell_lo = [&](int i) { uint64_t b = (uint64_t)(emin + i) << 49; double v; memcpy(&v, &b, 8); return v; };
    for (int i = 0; i < LUT_N; ++i) {
        const double lo = cell_lo(i), hi2 = cell_lo(i + 1);
        int below = 0, inside = 0;
        for (int k = 0; k < n_bins; ++k) { below += thr[k] <= lo; inside += (thr[k] > lo && (i == LUT_N - 1 || thr[k] < hi2)); }
        lut[i] = (uint8_t)((below << 1) | (inside ? 1 : 0));
        if (inside > 1) lut_ok = false;  // (the last cell also serves every larger d^2)
    }
    if (!(thr[0] > cell_lo(0))) lut_ok = false;
    return lut_ok;
}

// 1/8-binade cell of float(d2) as the GRID kernels compute it (round-to-nearest conversion: monotone in d2)
inline int cell_of_u32(uint32_t d2) {
    const float f = (float)d2;
    uint32_t b;
    memcpy(&b, &f, 4);
    return (int)(b >> 20);
}

// Integer-lattice analysis of a pair set (host coordinates).  Succeeds when every coordinate is x0 + g * i (same g for x and
// y, g = G * 2^-k with an integer G) with lattice indexes i < 32768, and when the float64 kernels' arithmetic is exact on
// such points -- (g dx)^2 + (g dy)^2 < 2^53 -- so that their squared distance IS g^2 * d2 with d2 = dx^2 + dy^2 the integer
// squared lattice distance.  Then class(d2) = #{k : T_k <= d2}, T_k = the smallest integer with g^2 T_k >= thr_k, is
// identical to the float64 classification, pair by pair.
struct GridInfo {
    std::vector<uint32_t> a_xy, b_xy, thr_i;
    std::vector<uint8_t> lut;
};
// (host threads of the scans below: the cores this process may use, at most 16; XDEM_HOST_THREADS overrides -- the same rule as
//  xdem_amd/spatialstats.py: _host_threads)
inline int host_threads() {
    if (const char* e = getenv("XDEM_HOST_THREADS")) { const int v = atoi(e); if (v >= 1) return v; }
    cpu_set_t set;
    int n = 1;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    return n < 1 ? 1 : (n > 16 ? 16 : n);
}
// f(first, last, thread) over [0, n) cut into one contiguous piece per thread
template <class F> inline void host_chunks(int64_t n, int threads, F f) {
    threads = (int)std::max<int64_t>(1, std::min<int64_t>(threads, (n + (1 << 16) - 1) >> 16));   // (pieces of at least 64 K elements)
    if (threads == 1) { f((int64_t)0, n, 0); return; }
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) pool.emplace_back([=]() { f(n * t / threads, n * (t + 1) / threads, t); });
    for (auto& th : pool) th.join();
}

// The scans of make_grid run over every coordinate of the set (6e8 values for SURVEY 8d's C5 reading A): each is a reduction --
// all-of, min, gcd, max -- done in pieces on the host's threads and combined.
struct GridScan {
    const double* arr[4];
    int64_t len[4];
    int threads;
    // 1. the smallest power-of-two scale 2^k, k <= 20, that makes every coordinate an integer below 2^52 (-1: none)
    int scale_exponent() const {
        for (int kk = 0; kk <= 20; ++kk) {
            const double sc = ldexp(1.0, kk);
            std::atomic<int> bad(0);
            for (int q = 0; q < 4; ++q)
                host_chunks(len[q], threads, [&, q](int64_t i0, int64_t i1, int) {
                    const double* v = arr[q];
                    bool ok = true;
                    for (int64_t i = i0; i < i1 && ok; ++i) { const double w = v[i] * sc; ok = std::isfinite(v[i]) && fabs(w) < 4.5e15 && w == floor(w); }
                    if (!ok) bad.store(1);
                });
            if (!bad.load()) return kk;
        }
        return -1;
    }
    // combine(part of every piece) of reduce(first, last, array) over the four arrays; x arrays feed out[0], y arrays out[1]
    template <class V, class R, class C> void reduce(V init, V (&out)[2], R piece, C combine) const {
        out[0] = out[1] = init;
        for (int q = 0; q < 4; ++q) {
            std::vector<V> part((size_t)threads, init);
            host_chunks(len[q], threads, [&, q](int64_t i0, int64_t i1, int t) { part[(size_t)t] = piece(arr[q], i0, i1, q & 1); });
            for (V p : part) out[q & 1] = combine(out[q & 1], p);
        }
    }
};

inline unsigned long long gcd_u64(unsigned long long a_, unsigned long long b_) {
    while (b_) { const unsigned long long t = a_ % b_; a_ = b_; b_ = t; }
    return a_;
}

// 4. integer thresholds: smallest n with g2 * n >= thr, g2 = G^2 * 2^-2k (g2 * n is exact in float64 for n <= 2 imax^2)
inline void grid_thresholds(const std::vector<double>& thr, double g2, unsigned long long nmax, std::vector<uint32_t>& thr_i) {
    thr_i.resize(thr.size());
    for (size_t q = 0; q < thr.size(); ++q) {
        const long double est = (long double)thr[q] / (long double)g2;
        unsigned long long n = est >= 4.0e9L ? 0xFFFFFFFFull : (unsigned long long)ceill(est);
        if (n <= nmax + 2) {  // refine with exact products (n inside the exactly representable range)
            while (n > 0 && g2 * (double)(n - 1) >= thr[q]) --n;
            while (g2 * (double)n < thr[q]) ++n;
        } else if (n > 0xFFFFFFFFull) {
            n = 0xFFFFFFFFull;
        }
        thr_i[q] = (uint32_t)(n > 0xFFFFFFFFull ? 0xFFFFFFFFull : n);
    }
}

// 5. class table over the cells of float(d2), indexed directly by the cell: entry = classes whose threshold lies at or below
// the cell's first d2; a cell may hold at most one more threshold (checked: false), which the kernel resolves with one integer compare
inline bool grid_cell_table(const std::vector<uint32_t>& thr_i, std::vector<uint8_t>& lut) {
    lut.assign(LUT_G, 0);
    auto first_in_cell = [&](int c) -> unsigned long long {  // smallest d2 with cell(d2) >= c (2^32 if none)
        unsigned long long lo = 0, hi = 0x100000000ull;
        while (lo < hi) {
            const unsigned long long mid = (lo + hi) >> 1;
            if (cell_of_u32((uint32_t)mid) >= c) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    for (int i = 0; i < LUT_G; ++i) {
        // (entry 0 also serves d2 = 0: coincident points belong to the class of the smallest distances)
        const unsigned long long lo = i == 0 ? 0 : first_in_cell(LUT_G0 + i), hi = first_in_cell(LUT_G0 + i + 1);
        if (lo >= 0x100000000ull || lo == hi) { lut[i] = (uint8_t)(i ? lut[i - 1] : 0); continue; }  // no d2 maps here
        int below = 0, inside = 0;
        for (size_t q = 0; q < thr_i.size(); ++q) {
            below += (unsigned long long)thr_i[q] <= lo;
            inside += ((unsigned long long)thr_i[q] > lo && (unsigned long long)thr_i[q] < hi);
        }
        if (inside > 1) return false;
        lut[i] = (uint8_t)below;
    }
    return true;
}

// (bx == nullptr: an i < j set, only A)
inline bool make_grid(const double* ax, const double* ay, int64_t na, const double* bx, const double* by, int64_t nbt, const std::vector<double>& thr,
                      GridInfo& out) {
    const int T = host_threads();
    const GridScan scan = {{ax, ay, bx, by}, {na, na, bx ? nbt : 0, by ? nbt : 0}, T};
    if (na + nbt == 0) return false;
    const int k = scan.scale_exponent();
    if (k < 0) return false;
    const double sc = ldexp(1.0, k);
    double mn[2];
    scan.reduce((double)INFINITY, mn,
                [&](const double* v, int64_t i0, int64_t i1, int) {
                    double m = INFINITY;
                    for (int64_t i = i0; i < i1; ++i) { const double w = v[i] * sc; m = w < m ? w : m; }
                    return m;
                },
                [](double a_, double b_) { return b_ < a_ ? b_ : a_; });
    // 2. lattice constant: gcd of all offsets from the minima; 3. index range
    unsigned long long g2v[2];
    scan.reduce(0ull, g2v,
                [&](const double* v, int64_t i0, int64_t i1, int xy) {
                    const double m0 = mn[xy];
                    unsigned long long g = 0;
                    for (int64_t i = i0; i < i1; ++i) {
                        const unsigned long long u = (unsigned long long)(v[i] * sc - m0);
                        if (g != 1 && (g == 0 || u % g != 0)) g = gcd_u64(g, u);   // (most offsets are multiples of the running gcd: one modulo each)
                    }
                    return g;
                },
                gcd_u64);
    unsigned long long G = gcd_u64(g2v[0], g2v[1]);
    if (G == 0) G = 1;
    unsigned long long mx[2];
    scan.reduce(0ull, mx,
                [&](const double* v, int64_t i0, int64_t i1, int xy) {
                    const double m0 = mn[xy];
                    unsigned long long m = 0;
                    for (int64_t i = i0; i < i1; ++i) { const unsigned long long u = (unsigned long long)(v[i] * sc - m0) / G; m = u > m ? u : m; }
                    return m;
                },
                [](unsigned long long a_, unsigned long long b_) { return b_ > a_ ? b_ : a_; });
    const unsigned long long imax = mx[0] > mx[1] ? mx[0] : mx[1];
    if (imax > 32767ull) return false;
    if ((long double)G * (long double)imax >= 67108864.0L) return false;  // (G dx)^2 + (G dy)^2 < 2^53
    auto pack = [&](const double* x, const double* y, int64_t n, std::vector<uint32_t>& o) {
        o.resize((size_t)n);
        host_chunks(n, T, [&](int64_t i0, int64_t i1, int) {
            for (int64_t i = i0; i < i1; ++i) {
                const uint32_t ix = (uint32_t)((unsigned long long)(x[i] * sc - mn[0]) / G), iy = (uint32_t)((unsigned long long)(y[i] * sc - mn[1]) / G);
                o[(size_t)i] = ix | (iy << 16);
            }
        });
    };
    pack(ax, ay, na, out.a_xy);
    if (bx) pack(bx, by, nbt, out.b_xy);
    const double g2 = ldexp((double)G * (double)G, -2 * k);
    const unsigned long long nmax = 2ull * imax * imax;
    grid_thresholds(thr, g2, nmax, out.thr_i);
    out.lut.assign(LUT_G, 0);
    if (thr.size() > 255 || cell_of_u32(nmax > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)nmax) >= LUT_G0 + LUT_G) return false;
    return grid_cell_table(out.thr_i, out.lut);
}

}  // namespace xd
