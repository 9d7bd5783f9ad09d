// pairs_layout.h -- ONE description of the dynamic LDS block of the pair kernel (pairs_kernel.h) per (value type, operation, WIDE),
// as a function of the class count nb (and, for the size, of the histogram sweep width nbs): PAIRS_LDS_WALK names the regions
// in their order, each with its element type, count and alignment; a region starts where the one before it ends.  Three walkers
// read it: the kernel takes its pointers from it (PairsLdsPointers), the launch asks it for the size of the block
// (pairs_lds_bytes, variogram.hip: launch_pairs), and the CPU tests list it (PairsLdsTable) -- a table added to the kernel
// without a region here has no pointer to write through.  Plain C++, no HIP include.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pairs_classes.h"
#include "sel_narrow.h"   // XD_HD: host + device where a HIP compiler reads this, plain inline elsewhere

namespace xd {

enum { OP_SUMS_SQ = 0, OP_SUMS_SQRT = 1, OP_HIST = 2, OP_SUCC = 3, OP_BRACKET = 4 };

constexpr int PAIRS_RADIX = 256;        // counters of one histogram row (= select.h: SEL_RADIX, asserted in pairs_kernel.h)
constexpr int PAIRS_STAGE_CAP = 8192;   // staging slots of a workgroup's candidates (= select_run.h: SEL_STAGE_CAP, asserted there too)
// OP_SUMS: per class a 384-byte record: NCOPY float64 sums (256 B = all 64 LDS banks, one copy per lane % 32: conflict-free), then
// NCOPY uint32 counts.  Record nb collects the pairs beyond the last edge and is never read back, so full tiles need no
// class test.  Both atomics of a pair address the record with the same `l * 384` term.
// (An interleaved 16-byte (sum, count) slot per copy would save an address computation but puts four lanes of every
// 32-lane group on one bank pair: measured slower.)
constexpr int PAIRS_REC = NCOPY * 12;
// (WIDE: 8-byte candidates in half as many slots -- the staging buffer keeps its size, and with it two workgroups per CU)
template <bool WIDE> constexpr int pairs_stage_cap() { return WIDE ? PAIRS_STAGE_CAP / 2 : PAIRS_STAGE_CAP; }

template <int N> struct PairsBytes { unsigned char b[N]; };   // an element of N bytes without a type of its own
template <int N> struct PairsUint;                            // ... and the unsigned integer of 4 / 8 bytes
template <> struct PairsUint<4> { typedef uint32_t type; };
template <> struct PairsUint<8> { typedef uint64_t type; };

enum PairsLdsRegion {
    // every operation: the B tile and the class tables
    LDS_BX, LDS_BY, LDS_THR, LDS_THR_PAD, LDS_PREF, LDS_KHI, LDS_BV, LDS_BXY, LDS_THR_I,
    // the accumulator area: ONE place (it starts where LDS_THR_I ends, 8-byte aligned), used by each operation for its own regions
    LDS_REC,    // OP_SUMS_*
    LDS_HIST,   // OP_HIST
    LDS_MIN,    // OP_SUCC
    LDS_C3, LDS_LH, LDS_LHF, LDS_IN, LDS_STAGE_V, LDS_STAGE_B, LDS_STAGE_BASE, LDS_STAGE_HELD,   // OP_BRACKET
    LDS_REGIONS
};
constexpr int LDS_ACC_FIRST = LDS_REC;   // regions from here on lie in the accumulator area

// The regions, in their order.  w: a walker with region<element type>(id, name, count, alignment); T: the value type (a key is as
// wide as its value, select.h: KeyT); nb, nbs: int expressions.
//   bx, by      float64 B coordinates of the tile
//   thr         nb thresholds on d^2, then thr_pad: their +inf padding (the lookup reads one entry past the class)
//   pref        nb selection prefixes / selected keys / bracket lows (8-byte slots)
//   khi         nb bracket highs; dual digit passes: the second prefixes (8-byte slots)
//   bv          B values of the tile
//   bxy         packed lattice indexes (GRID)
//   thr_i       nb + 2 integer thresholds (GRID), padded with all-ones; an even count: what follows is 8-byte aligned
//   rec         OP_SUMS: [nb + 1] records (PAIRS_REC)
//   hist        OP_HIST: [nbs][256] counters (dual passes: nbs counts both tables)
//   min         OP_SUCC: nb keys
//   c3          OP_BRACKET: [nb + 1][NCOPY], one PACKED 64-bit counter per class and copy -- bits 0..20 pairs of the class, 21..41
//               those at or above the bracket's low end, 42..62 those above its high end (a workgroup gives a copy at most 1024 x
//               4096 / 32 = 2^17 pairs): ONE ds_add_u64 of (1 | ge << 21 | gt << 42) per pair, its value two selects on the compare
//               masks, its address one shift-add (three separate planes needed a plane index, a multiply-add and two more adds).
//               Class nb = spare: pairs that are no pairs -- beyond the last edge, diagonal, NaN -- count there, so the hot loop
//               needs no predicate.
//   lh          then the bracket ends interleaved {low, high} per class as halved keys (one 8 / 16-byte read per pair; the spare
//               class holds {all-ones, 0}: always "below", never a candidate),
//   lhf         ... the same ends as VALUES {low, high} per class for the run-length loop (float compares of |dv|; an end whose
//               bits are no number compares false with everything, which is what an unreachable end means),
//   in          ... per class the number of candidates the run-length loop staged (tallied when the wave hands its pending
//               candidates to the staging buffer: the runs count only total and >= low end per pair); nb + 1 counters, an even count,
//   stage_*     ... and the staging buffer (select_run.h: BlockStage): values (as a candidate is stored: T, WIDE: the exact float64
//               difference), classes, the reserved base, the fill count
// (A macro, not a function template: as a function the walk left the six table / lattice counting kernels with other LDS address
// immediates in their tile loops -- the compiler splits the same addresses differently between base register and offset when the
// counts reach it already simplified.  Expanded in place, the kernel sees the chain of typed pointer steps it had when it carved
// the block by hand, and 42 of the 45 kernels of variogram.hip compile to the instructions they had.)
#define PAIRS_LDS_WALK(w, T, OP, WIDE, nb, nbs)                                                                                        \
    do {                                                                                                                               \
        static_assert(!(WIDE) || (sizeof(T) == 4 && (OP) == OP_BRACKET), "WIDE: float32 values, counting pass only");                  \
        (w).template region<double>(LDS_BX, "bx", PT, 16);                                                                             \
        (w).template region<double>(LDS_BY, "by", PT, 8);                                                                              \
        (w).template region<double>(LDS_THR, "thr", (nb), 8);                                                                          \
        (w).template region<double>(LDS_THR_PAD, "thr_pad", LUT_STEPS + 1, 8);                                                         \
        (w).template region<uint64_t>(LDS_PREF, "pref", (nb), 8);                                                                      \
        (w).template region<uint64_t>(LDS_KHI, "khi", (nb), 8);                                                                        \
        (w).template region<T>(LDS_BV, "bv", PT, sizeof(T));                                                                           \
        (w).template region<uint32_t>(LDS_BXY, "bxy", PT, 4);                                                                          \
        (w).template region<uint32_t>(LDS_THR_I, "thr_i", ((nb) + 2 + 1) & ~1, 4);                                                     \
        if ((OP) == OP_SUMS_SQ || (OP) == OP_SUMS_SQRT) (w).template region<PairsBytes<PAIRS_REC>>(LDS_REC, "rec", (nb) + 1, 8);       \
        if ((OP) == OP_HIST) (w).template region<uint32_t>(LDS_HIST, "hist", (nbs) * PAIRS_RADIX, 4);                                  \
        if ((OP) == OP_SUCC) (w).template region<typename PairsUint<sizeof(T)>::type>(LDS_MIN, "min", (nb), sizeof(T));                \
        if ((OP) == OP_BRACKET) {                                                                                                      \
            (w).template region<unsigned long long>(LDS_C3, "c3", ((nb) + 1) * NCOPY, 8);                                              \
            (w).template region<typename PairsUint<sizeof(T)>::type>(LDS_LH, "lh", 2 * ((nb) + 1), 8);                                 \
            (w).template region<T>(LDS_LHF, "lhf", 2 * ((nb) + 1), 8);                                                                 \
            (w).template region<uint32_t>(LDS_IN, "in", ((nb) + 2) & ~1, 4);                                                           \
            (w).template region<typename PairsUint<((WIDE) ? 8 : sizeof(T))>::type>(LDS_STAGE_V, "stage_v", pairs_stage_cap<(WIDE)>(), \
                                                                                    (WIDE) ? 8 : sizeof(T));                           \
            (w).template region<uint16_t>(LDS_STAGE_B, "stage_b", pairs_stage_cap<(WIDE)>(), 2);                                       \
            (w).template region<unsigned long long>(LDS_STAGE_BASE, "stage_base", 1, 8);                                               \
            (w).template region<int>(LDS_STAGE_HELD, "stage_held", 1, 4);                                                              \
        }                                                                                                                              \
    } while (0)

// walker of the kernel: the start of every region of the block at `base` (regions of other operations: null)
struct PairsLdsPointers {
    unsigned char* cur;
    void* p[LDS_REGIONS] = {};
    XD_HD explicit PairsLdsPointers(unsigned char* base) : cur(base) {}
    template <typename U> XD_HD void region(int id, const char*, int count, size_t) {
        U* const q = reinterpret_cast<U*>(cur);
        p[id] = q;
        cur = reinterpret_cast<unsigned char*>(q + count);
    }
    template <typename U> XD_HD U* at(int id) const { return static_cast<U*>(p[id]); }
};

// walker of the launch: the size of the block; it also checks the description against itself -- every region starts at a multiple
// of the alignment it declares (`aligned`; the kernel's walker, which adds no padding of its own, then meets it too)
struct PairsLdsSize {
    size_t bytes = 0;
    bool aligned = true;
    template <typename U> XD_HD void region(int, const char*, int count, size_t align) {
        aligned = aligned && bytes % align == 0 && align % alignof(U) == 0;
        bytes += sizeof(U) * (size_t)count;
    }
};
// dynamic LDS of a launch with nb classes (nbs: classes of the histogram sweep's table, both tables of a dual pass); all ones: the
// description breaks its own alignments at this nb -- no launch can get that much LDS, so the launch fails instead of running
template <typename T, int OP, bool WIDE = false> inline size_t pairs_lds_bytes(int nb, int nbs) {
    PairsLdsSize s;
    PAIRS_LDS_WALK(s, T, OP, WIDE, nb, nbs);
    return s.aligned ? s.bytes : ~(size_t)0;
}

// walker of the tests: the regions as a table
struct PairsRegion {
    int id;
    const char* name;
    size_t offset, elem, count, align;   // bytes, bytes, elements, bytes
};
struct PairsLdsTable {
    PairsRegion r[LDS_REGIONS];
    int n = 0;
    size_t bytes = 0;
    template <typename U> XD_HD void region(int id, const char* name, int count, size_t align) {
        r[n++] = {id, name, bytes, sizeof(U), (size_t)count, align};
        bytes += sizeof(U) * (size_t)count;
    }
};
template <typename T, int OP, bool WIDE = false> inline PairsLdsTable pairs_lds_table(int nb, int nbs) {
    PairsLdsTable t;
    PAIRS_LDS_WALK(t, T, OP, WIDE, nb, nbs);
    return t;
}

}  // namespace xd
