// spline_line.h -- one line of the mirror spline prefilter as bands or segments of it compute it (spline.hip has the derivation): the
// walk down (causal recursion from a warm-up halo or SciPy's mirror start, the anticausal start summed forward through the halo
// behind the band) and the walk back.  Host and device: the kernels of spline.hip and xdemhip_spline_host_line run these functions.
#pragma once
#include <math.h>
#include <stdint.h>

#define SP_HD __host__ __device__

constexpr int SP_HALO = 64;

struct SpPole {
    double z, gain, zn1;   // the pole, the gain its pass applies to what it reads (1 after the first pole), z^(n-1) of the line length
    int exact;             // n - 1 <= SP_HALO: the causal start sums the whole mirrored line as SciPy does
};

SP_HD inline int sp_poles(int order, double* z) {
    if (order == 3) { z[0] = -0.267949192431122706472553658494127633; return 1; }   // sqrt(3) - 2
    z[0] = -0.430575347099973791851434783493520110;   // sqrt(67.5 - sqrt(4436.25)) + sqrt(26.25) - 6.5: the closed forms lose digits
    z[1] = -0.043096288203264653822712376822550182;   // sqrt(67.5 + sqrt(4436.25)) - sqrt(26.25) - 6.5
    return 2;
}

SP_HD inline SpPole sp_pole(int order, int k, int64_t n) {
    double z[2];
    const int np = sp_poles(order, z);
    SpPole p;
    p.z = z[k];
    p.gain = 1.0;
    if (k == 0)
        for (int j = 0; j < np; ++j) p.gain *= (1.0 - z[j]) * (1.0 - 1.0 / z[j]);
    p.exact = n - 1 <= SP_HALO;
    p.zn1 = p.exact ? pow(p.z, (double)(n - 1)) : 0.0;
    return p;
}

// ---- one line of the prefilter --------------------------------------------------------------------------------------------------------
template <class In>
SP_HD inline double sp_causal_init(const In& in, int64_t n, const SpPole& p) {
    double zi = p.z, c0;
    if (p.exact) {
        c0 = in(0) + p.zn1 * in(n - 1);
        for (int64_t i = 1; i < n - 1; ++i) {
            c0 += zi * (in(i) + p.zn1 * in(n - 1 - i));
            zi *= p.z;
        }
        c0 /= 1.0 - p.zn1 * p.zn1;
    } else {
        c0 = in(0);
        for (int i = 1; i <= SP_HALO; ++i) {   // (n - 1 > SP_HALO)
            c0 += zi * in(i);
            zi *= p.z;
        }
    }
    return c0;
}

struct SpWarm {
    double c;      // c+[i0 - 1]
    int64_t i0;    // the first sample the band's causal loop computes (y0, or 1 for the band that holds sample 0)
};

// The walk down over samples [y0, y1) of a line of n: the causal recursion from its warm-up through the band (stored if STORE) and
// on through the halo behind it.  cm = c-[y1], or c-[n-1] itself when the band ends the line (last).
template <bool STORE, class In, class Out>
SP_HD inline void sp_forward(const In& in, Out& out, int64_t n, int64_t y0, int64_t y1, const SpPole& p, SpWarm& warm, double& cm, bool& last) {
    const double z = p.z;
    const int64_t a = y0 - SP_HALO;
    double c, cprev = 0.0;
    int64_t i0 = y0;
    if (a <= 0) {
        c = sp_causal_init(in, n, p);
        if (y0 == 0) i0 = 1;
        for (int64_t i = 1; i < y0; ++i) { cprev = c; c = in(i) + z * c; }
    } else {
        c = in(a);
        for (int64_t i = a + 1; i < y0; ++i) { cprev = c; c = in(i) + z * c; }
    }
    warm.c = c;
    warm.i0 = i0;
    if (STORE && i0 > y0) out.put(y0, c);
    for (int64_t i = i0; i < y1; ++i) {
        cprev = c;
        c = in(i) + z * c;
        if (STORE) out.put(i, c);
    }
    const double edge = z / (z * z - 1.0);
    last = y1 == n;
    if (last) {
        cm = (z * cprev + c) * edge;
        return;
    }
    int64_t b = y1 + SP_HALO;
    const bool real = b >= n;
    if (real) b = n - 1;
    double acc = 0.0, zj = 1.0;
    for (int64_t i = y1; i < b; ++i) {
        cprev = c;
        c = in(i) + z * c;
        acc += zj * c;
        zj *= z;
    }
    cm = -z * acc;
    if (real) {
        cprev = c;
        c = in(n - 1) + z * c;
        cm += zj * ((z * cprev + c) * edge);
    }
}

// the causal loop of the band again from its warm state, stored (the LDS route: its first walk stores nothing)
template <class In, class Out>
SP_HD inline void sp_replay(const In& in, Out& out, int64_t y0, int64_t y1, const SpPole& p, const SpWarm& warm) {
    double c = warm.c;
    if (warm.i0 > y0) out.put(y0, c);
    for (int64_t i = warm.i0; i < y1; ++i) {
        c = in(i) + p.z * c;
        out.put(i, c);
    }
}

// the walk back over [y0, y1): out holds c+ and receives c-
template <class Out>
SP_HD inline void sp_backward(Out& out, int64_t y0, int64_t y1, double cm, bool last, double z) {
    int64_t top = y1 - 1;
    if (last) {
        out.put(y1 - 1, cm);
        top = y1 - 2;
    }
    for (int64_t i = top; i >= y0; --i) {
        cm = z * (cm - out.get(i));
        out.put(i, cm);
    }
}
