// Host harness of the two policies of the one-pass Nuth-Kaab step (xdem_amd/csrc/nk_policy.h) and of the sizes of its device
// blocks (nk_layout.h) -- test tool only, driven through ctypes by tests/test_nk_policy_host.py.
#include "../../xdem_amd/csrc/nk_layout.h"
#include "../../xdem_amd/csrc/nk_policy.h"

using namespace xd;

// the selection state of a bin, with select.h's members
template <typename K> struct State { K prefix; uint64_t rank, count, n_le, group; };

extern "C" {

// ---- NkNarrowing ----
void* nkp_narrow_new() { return new NkNarrowing(); }
void nkp_narrow_free(void* p) { delete static_cast<NkNarrowing*>(p); }
void nkp_narrow_observe(void* p, uint64_t tot, uint64_t lt, uint64_t in, double unit) { static_cast<NkNarrowing*>(p)->observe(tot, lt, in, unit); }
int nkp_narrow_choose_next(void* p, int option) { return static_cast<NkNarrowing*>(p)->choose_next(option); }
void nkp_narrow_on_miss(void* p, int used) { static_cast<NkNarrowing*>(p)->on_miss(used); }
void nkp_narrow_reset(void* p) { static_cast<NkNarrowing*>(p)->reset(); }
// out: unit_min, worst, off2; returns the code, *offn the number of observations
int nkp_narrow_get(void* p, double* out, int64_t* offn) {
    const NkNarrowing* s = static_cast<NkNarrowing*>(p);
    out[0] = s->unit_min; out[1] = s->worst; out[2] = s->off2;
    *offn = s->offn;
    return s->narrow;
}
double nkp_narrow_unit(uint32_t code) { return sel_narrow_unit(code); }
uint64_t nkp_narrowed(uint64_t h_full, uint32_t code) { return sel_narrowed(h_full, code); }

// ---- NkPrediction ----
void* nkp_pred_new() { return new NkPrediction(); }
void nkp_pred_free(void* p) { delete static_cast<NkPrediction*>(p); }
// sc: sx, sy, v, wd, err, err_d, dpx
void nkp_pred_set(void* p, int have, int nb, int cooldown, const double* sc, const double* med, const double* w, const double* mid, const unsigned char* ok) {
    NkPrediction* s = static_cast<NkPrediction*>(p);
    s->have = have != 0; s->nb = nb; s->cooldown = cooldown;
    s->sx = sc[0]; s->sy = sc[1]; s->v = sc[2]; s->wd = sc[3]; s->err = sc[4]; s->err_d = sc[5]; s->dpx = sc[6];
    s->med.assign(med, med + nb); s->w.assign(w, w + nb); s->mid.assign(mid, mid + nb); s->ok.assign(ok, ok + nb);
}
// ints: have, nb, cooldown, n_predicted, n_predicted_d, n_predict_miss, size of the per-bin record; the per-bin arrays hold >= that many
void nkp_pred_get(void* p, int64_t* ints, double* sc, double* med, double* w, double* mid, unsigned char* ok) {
    const NkPrediction* s = static_cast<NkPrediction*>(p);
    ints[0] = s->have; ints[1] = s->nb; ints[2] = s->cooldown; ints[3] = s->n_predicted; ints[4] = s->n_predicted_d; ints[5] = s->n_predict_miss;
    ints[6] = (int64_t)s->w.size();
    sc[0] = s->sx; sc[1] = s->sy; sc[2] = s->v; sc[3] = s->wd; sc[4] = s->err; sc[5] = s->err_d; sc[6] = s->dpx;
    for (size_t b = 0; b < s->med.size(); ++b) med[b] = s->med[b];
    for (size_t b = 0; b < s->w.size(); ++b) w[b] = s->w[b];
    for (size_t b = 0; b < s->mid.size(); ++b) mid[b] = s->mid[b];
    for (size_t b = 0; b < s->ok.size(); ++b) ok[b] = s->ok[b];
}
// the decision of a step, kept for the record() that follows it.  flags: predict, predict_d; sc: dpx, h, hd; lo / hi [nb] filled when predict
static NkStepBrackets g_last;
void nkp_pred_plan(void* p, double dE, double dN, int nb, int allow, int option, int* flags, double* sc, double* lo, double* hi) {
    g_last = static_cast<NkPrediction*>(p)->plan(dE, dN, nb, allow != 0, option);
    flags[0] = g_last.predict; flags[1] = g_last.predict_d;
    sc[0] = g_last.dpx; sc[1] = g_last.h; sc[2] = g_last.hd;
    for (size_t b = 0; b < g_last.lo.size(); ++b) { lo[b] = g_last.lo[b]; hi[b] = g_last.hi[b]; }
}
void nkp_pred_on_miss(void* p) { static_cast<NkPrediction*>(p)->on_miss(); }
void nkp_pred_forget(void* p) { static_cast<NkPrediction*>(p)->forget(); }
void nkp_pred_record(void* p, double dc, double dr, int nb, double vs, const double* medians, const int64_t* counts, const double* edges, const double* lo,
                     const double* hi, double dlo, double dhi, int narrow) {
    static_cast<NkPrediction*>(p)->record(g_last, dc, dr, nb, vs, medians, counts, edges, lo, hi, dlo, dhi, narrow);
}

// ---- sizes of the device blocks ----
int64_t nkp_fz_zeroed_words(int64_t nb_max) { return NkFzWords::zeroed_words(nb_max); }
uint64_t nkp_fz_total_bytes(int64_t nb_max) { return NkFzWords::total_bytes(nb_max); }
int64_t nkp_mr_small_words(int64_t nb_max) { return NkMrSmallLayout::total_words(nb_max); }
// size of the step's packed result block, from the step's own table
uint64_t nkp_fetch_bytes(int dtype_is_f64, int nb_max) {
    return dtype_is_f64 ? nk_fetch_bytes<double, uint64_t, State<uint64_t>>(nb_max) : nk_fetch_bytes<float, uint32_t, State<uint32_t>>(nb_max);
}
// word offsets of the per-bin regions: klo_y, khi_y, cls_y, res_y, cnt_y, seg_ctr, dsel, dsel_keys
void nkp_fz_offsets(int64_t nb_max, int64_t* out) {
    out[0] = NkFzWords::klo_y_w(nb_max); out[1] = NkFzWords::khi_y_w(nb_max); out[2] = NkFzWords::cls_y_w(nb_max); out[3] = NkFzWords::res_y_w(nb_max);
    out[4] = NkFzWords::cnt_y_w(nb_max); out[5] = NkFzWords::seg_ctr_w(nb_max); out[6] = NkFzWords::dsel_w(nb_max); out[7] = NkFzWords::dsel_keys_w(nb_max);
}

}  // extern "C"
