// sel_narrow.h -- the narrow codes of the bracketed selection (select.h), free of any HIP include: shared by the device code that
// applies them (select.h: advance of the bracket ends) and by the host policy that chooses them (nk_policy.h), which a plain C++
// compiler builds for the CPU tests.
#pragma once
#include <stdint.h>

#ifndef XD_HD   // (terrain_math.h's convention; a translation unit that includes both sees one definition)
#if defined(__HIPCC__)
#define XD_HD __host__ __device__ __forceinline__
#else
#define XD_HD inline
#endif
#endif

namespace xd {

// Narrowed half widths (callers that MEASURE how well their samples centre: the one-pass Nuth-Kaab step).  `narrow` is a code: below
// 16 a right shift of the rule's width (0 = the full rule, 1 = half, 2 = a quarter), 16 + q = q sixteenths of it (q = 1 .. 16).
constexpr uint32_t SEL_NARROW_16THS = 16;
XD_HD uint64_t sel_narrowed(uint64_t h_full, uint32_t narrow) {
    const uint64_t w = h_full - 32;
    return (narrow < SEL_NARROW_16THS ? (w >> narrow) : ((w * (uint64_t)(narrow - SEL_NARROW_16THS)) >> 4)) + 32;
}
XD_HD double sel_narrow_unit(uint32_t narrow) {   // the fraction of the full rule a code stands for
    return narrow < SEL_NARROW_16THS ? 1.0 / (double)(1u << narrow) : (double)(narrow - SEL_NARROW_16THS) / 16.0;
}

}  // namespace xd
