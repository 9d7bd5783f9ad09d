// nk_policy.h -- the two host policies of the one-pass Nuth-Kaab step (nuthkaab.hip: nk_step_onepass) as plain C++: how narrow the
// NEXT step's sample brackets may be (NkNarrowing) and whether THIS step's brackets are predicted from the previous step instead
// of sampled (NkPrediction).  Float64 arithmetic on host state only; no HIP include, so the CPU tests build it with g++
// (tests/hostsim/nk_policy_hostsim.cpp).  Compiled without fused multiply-add contraction, like its includer.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <cmath>
#include <vector>

#include "sel_narrow.h"

namespace xd {

// ---- bracket narrowing -------------------------------------------------------------------------------------------------------
// The sample brackets of the NEXT step are a fraction (code `narrow`, sel_narrow.h) of what the rule for fully correlated sample
// lines asks (select.h: sel_bracket_halfwidth); set from how far off the bracket centres the wanted ranks lay in the steps so far,
// never below unit_min (raised by a miss).
struct NkNarrowing {
    int narrow = 0;
    double unit_min = 0.25;
    double worst = 0.0;   // largest |wanted rank - bracket centre| seen, in half widths of the FULL rule
    double off2 = 0.0;    // sum of squares of those offsets over all brackets of all steps so far
    int64_t offn = 0;

    void reset() { *this = NkNarrowing(); }

    // How centred was a bracket?  |wanted rank - centre| in half widths of the bracket that was used (`unit`: the fraction of the
    // full rule it was), kept in units of the FULL rule.  Lines of a sample that are not fully correlated (the rule's worst case)
    // leave the ranks within a small fraction of it: the next step then takes narrower brackets -- fewer candidates staged,
    // resolved and selected from (measured on C3: 1.88 -> 1.73 -> 1.62 ms per step); a miss costs that step the plain route and
    // caps the narrowing (exact either way).
    void observe(uint64_t tot, uint64_t lt, uint64_t in, double unit) {
        if (tot < 4096 || in < 64 || in >= tot) return;
        const double o = fabs(((double)(tot - 1) * 0.5 - (double)lt) - 0.5 * (double)in) / (0.5 * (double)in) * unit;
        worst = o > worst ? o : worst;
        off2 += o * o;
        offn += 1;
    }

    // rms offset = one standard deviation of the sample ranks in units of the full half width (independent sample elements:
    // 1 / 17, the rule being 6 sigma of 8-element lines that are fully correlated; 0.062-0.068 measured on C3): the next brackets
    // keep >= 4.8 sigma (a miss in 1e-4 of the steps with 73 brackets each -- it costs that step the plain route, nothing else) and
    // >= 1.5 x the worst offset ever seen, in sixteenths of the rule.  (Rounds 4-5 halved or quartered only, at 7 sigma and 2.2 x:
    // C3 sat at one half with 7.7 sigma of room; five sixteenths stage 38 % fewer candidates.)
    // `option`: the context's "nk_narrow" -- -1 = this rule, 0 / 1 / 2 fixed.
    int choose_next(int option) {
        int next = 0;
        if (offn >= 24) {
            const double sigma = sqrt(off2 / (double)offn);
            static const int qs[] = {4, 5, 6, 7, 8, 10, 12};
            for (int q : qs) {
                const double u = (double)q / 16.0;
                if (4.8 * sigma <= u && 1.5 * worst <= u && u >= unit_min) { next = q == 8 ? 1 : (q == 4 ? 2 : (int)SEL_NARROW_16THS + q); break; }
            }
        }
        if (option >= 0) next = option;
        if (getenv("XDEMHIP_DEBUG"))
            fprintf(stderr, "[xdemhip] one-pass step: brackets x %.4f, offsets rms %.3f worst %.3f of the full half width (%lld brackets) -> next x %.4f\n",
                    sel_narrow_unit((uint32_t)narrow), offn ? sqrt(off2 / (double)offn) : 0.0, worst, (long long)offn, sel_narrow_unit((uint32_t)next));
        narrow = next;
        return next;
    }

    // a step with brackets of code `used` fell through (narrowed brackets may be what missed: not that narrow again)
    void on_miss(int used) {
        if (used > 0) {
            unit_min = fmin(1.0, 1.5 * sel_narrow_unit((uint32_t)used));
            narrow = 0;
        }
    }
};

// ---- predicted brackets ------------------------------------------------------------------------------------------------------
// Once a fit has settled its offsets move by a few thousandths of a pixel per step and the exact medians of the previous step,
// moved by what the Nuth-Kaab model says the shift does to them, bracket this step's medians better than a fresh 1/64 sample does
// -- the two sample kernels and their six digit passes (~0.26 ms of a 1.66 ms step at C3) are skipped.  A bin median of
// y = (dh - vshift) / slope_tan moves by -(dE sin(aspect) + dN cos(aspect)) when the tap position moves by (dE, dN) pixels -- the
// Nuth-Kaab model itself -- and the median of dh stays to first order; how well that held is MEASURED at every step (err: the worst
// miss of the centres in half widths of the sampled brackets, for the step just finished), and a step is predicted only when the
// last one would have been hit with room to spare and the shift change has not grown.  The brackets are then 0.25 ... 1 sampled
// widths around the predicted centres; the integer counts of the pass prove them like any sampled bracket, a miss reruns THIS step
// sampled (and the next one): exact either way.  Identical decisions on every rank of a partitioned plan (everything is derived
// from reduced results and the call's arguments).
constexpr int NK_PREDICT_MAX_BINS = 128;

// what NkPrediction::plan decides for one step
struct NkStepBrackets {
    bool predict = false;     // every bracket predicted
    bool predict_d = false;   // the bracket of the median of dh alone
    double dE = 0, dN = 0, dpx = 0;   // the change of the tap offsets since the previous step (pixels) and its length
    double h = 1.0;           // bracket half widths of this step in sampled half widths
    double hd = 0.0;          // half width (value) of the bracket of the median of dh around the previous median
    std::vector<double> lo, hi;   // predict: the bins' brackets; an empty bin gets (1, 0)
};

struct NkPrediction {
    // what the previous step left (identical on every rank of a partitioned plan)
    bool have = false;             // ... it answered on the one-pass route and everything below is its record
    int nb = 0;
    double sx = 0, sy = 0;         // its tap offsets, pixels (column, row)
    double v = 0, wd = 0;          // its vshift; half width (value) of the last SAMPLED bracket of the median of dh
    std::vector<double> med, w, mid;   // per bin: exact median of y, half width of the last sampled bracket, centre aspect
    std::vector<unsigned char> ok;     // ... the bin had a median
    double err = 1e30, err_d = 1e30;   // how far the prediction of the LAST step would have been off (or was), in sampled half widths: bins / median of dh
    double dpx = 1e30;             // the shift change of the last step, pixels
    int cooldown = 0;              // sampled steps still to run after a predicted bracket missed
    int64_t n_predicted = 0, n_predicted_d = 0, n_predict_miss = 0;   // steps with every bracket predicted / with the bracket of the median of dh predicted / reruns after a miss

    void forget() { have = false; }

    // `allow`: false on the rerun after a miss; `option`: the context's "nk_predict"
    NkStepBrackets plan(double dE, double dN, int nb_now, bool allow, int option) {
        NkStepBrackets s;
        s.dE = dE;
        s.dN = dN;
        const double dpx_now = sqrt(dE * dE + dN * dN);
        s.dpx = dpx_now;
        // (the measured miss of the centres is proportional to the shift change -- 0.90 / 0.11 / 0.012 half widths at 0.2 / 0.02 / 0.002 px
        //  on C3: the model's error is its second-order term -- so the miss to EXPECT at this step is the last one scaled by the ratio of
        //  the shift changes, with a floor for the jitter of the medians themselves)
        const bool scaled = dpx > 0 && dpx < 1e29;
        const double expect = scaled ? fmax(0.02, err * (dpx_now / dpx)) : 1e30;      // bin medians
        const double expect_d = scaled ? fmax(0.02, err_d * (dpx_now / dpx)) : 1e30;  // median of dh (assumed not to move)
        s.predict = allow && option != 0 && have && nb == nb_now && nb_now <= NK_PREDICT_MAX_BINS && cooldown == 0 &&
                    expect <= 0.20 && expect_d <= 0.20 && dpx_now <= 0.05 && wd > 0;
        // ... and on steps that still move too far for the bins, the bracket of the MEDIAN OF DH alone may be predicted: that median
        // hardly follows the shift (0.19 / 0.29 sampled half widths off at 0.1 / 0.5 px on C3), and without its three digit passes the y^
        // sample can be taken straight away (the bins' brackets are sampled as ever)
        s.predict_d = !s.predict && allow && option != 0 && have && nb == nb_now && cooldown == 0 &&
                      expect_d <= 0.35 && dpx_now <= 0.6 && wd > 0;
        if (cooldown > 0 && allow) --cooldown;
        // (the bracket of the median of dh may not be padded: its half width is the margin delta / slope_tan of EVERY pixel's y, and on
        //  flat ground a centimetre of it turns whole waves into bin candidates -- overflow flag at 0.04 px)
        if (s.predict || s.predict_d) s.hd = fmin(1.0, fmax(0.25, 2.0 * expect_d + 0.15)) * wd;
        if (s.predict) {
            s.h = fmin(1.0, fmax(0.25, 2.0 * expect + 0.15));
            s.lo.resize(nb_now);
            s.hi.resize(nb_now);
            for (int b = 0; b < nb_now; ++b) {
                if (!ok[b]) { s.lo[b] = 1; s.hi[b] = 0; continue; }   // (an empty bin stays empty: the aspects do not move)
                const double c = med[b] - (dE * sin(mid[b]) + dN * cos(mid[b]));
                const double hw = s.h * w[b] + 0.05 * dpx_now;
                s.lo[b] = c - hw;
                s.hi[b] = c + hw;
            }
        }
        return s;
    }

    // a PREDICTED bracket missed (or overflowed): this step once more with sampled brackets, and the next one sampled too; the
    // prediction has to earn its way back through a measured error
    void on_miss() {
        ++n_predict_miss;
        cooldown = 1;
        err = err_d = 1e30;
    }

    // What the NEXT step's prediction rests on, and how well THIS step was (or would have been) predicted by the model "a bin median
    // moves by -(dE sin(aspect) + dN cos(aspect))" (dE = change of the column offset of the taps, dN = minus the change of their row
    // offset, pixels) and "the median of dh stays".  (Were the signs wrong for some layout, the measured misses would be large and no
    // step would ever be predicted.)
    // `s`: this step's decision; (dc, dr): its tap offsets; vs, medians, counts, edges [nb + 1]: what it returns; (lo, hi) [nb] and
    // (dlo, dhi): the ends of the brackets it used, as values; `narrow`: the code its sample brackets were taken with.
    // (The ends are compared as values where the step's host code used to compare their keys.  The two differ only for ends that are
    //  no numbers -- the bracket {0, all-ones} of a bin without sample elements -- whose width is then recorded as 0 instead of NaN;
    //  such a bin has ok = 0 either way, and ok, w > 0 and wd > 0 gate every use of a width.)
    void record(const NkStepBrackets& s, double dc, double dr, int nb_now, double vs, const double* medians, const int64_t* counts, const double* edges,
                const double* lo, const double* hi, double dlo, double dhi, int narrow) {
        std::vector<double> mid_now(nb_now);
        for (int b = 0; b < nb_now; ++b) mid_now[b] = 0.5 * (edges[b] + edges[b + 1]);
        if (have && nb == nb_now) {
            double worst = 0.0;
            for (int b = 0; b < nb_now; ++b) {
                if (!ok[b] || counts[b] == 0 || !(w[b] > 0)) continue;
                const double e = fabs(medians[b] - (med[b] - (s.dE * sin(mid[b]) + s.dN * cos(mid[b])))) / w[b];
                worst = e > worst ? e : worst;
            }
            err = worst;
            err_d = wd > 0 ? fabs(vs - v) / wd : 1e30;
            dpx = fmax(s.dpx, 1e-5);   // (a repeated step measures the jitter floor: the ratio rule then stays conservative)
            if (getenv("XDEMHIP_DEBUG"))
                fprintf(stderr, "[xdemhip] one-pass step (%s, half widths x %.2f): shift change %.2e px, centres off by %.3f (bins) / %.3f (dh) sampled half widths\n",
                        s.predict ? "PREDICTED brackets" : (s.predict_d ? "sampled brackets, PREDICTED bracket of the median of dh" : "sampled brackets"), s.h, s.dpx, err, err_d);
        } else {
            err = err_d = 1e30;
            dpx = 1e30;
        }
        if (!s.predict || (int)w.size() != nb_now) {   // the widths of SAMPLED brackets only (predicted ones are fractions of them)
            // (kept in units of HALF the rule, the brackets the prediction's thresholds were tuned on: narrower sample brackets -- the
            //  sixteenths of NkNarrowing -- must not make the prediction shyer or its brackets thinner)
            const double norm = narrow >= (int)SEL_NARROW_16THS ? 0.5 / sel_narrow_unit((uint32_t)narrow) : 1.0;
            w.assign(nb_now, 0.0);
            for (int b = 0; b < nb_now; ++b)
                if (counts[b] > 0 && hi[b] >= lo[b]) w[b] = norm * 0.5 * (hi[b] - lo[b]);
            if (!s.predict_d) wd = dhi >= dlo ? norm * 0.5 * (dhi - dlo) : 0.0;
        }
        med.assign(medians, medians + nb_now);
        mid = mid_now;
        ok.assign(nb_now, 0);
        for (int b = 0; b < nb_now; ++b) ok[b] = (counts[b] > 0 && w[b] > 0 && std::isfinite(w[b]) && std::isfinite(medians[b])) ? 1 : 0;
        v = vs;
        sx = dc;
        sy = dr;
        nb = nb_now;
        have = true;
        if (s.predict) ++n_predicted;
        if (s.predict_d) ++n_predicted_d;
    }
};

}  // namespace xd
