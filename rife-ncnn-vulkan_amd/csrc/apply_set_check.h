// apply_set_check.h: the host-only rules of a rife_hip_apply_set_t (include/rife_hip.h "apply motion at another resolution") - what rife_hip_apply_set_check answers and
// what every sets call repeats per set, prefixed "set k:", before it touches anything.  Plain C++, no HIP include: the engine (engine_apply_sets.h) and the stand-alone
// sanitizer program (tests/sanitize/apply_set_check_main.cpp) compile this one statement.  The rules of the three descriptors are apply_check.h's.
#pragma once
#include "apply_check.h"

namespace rife_apply {

static inline bool shift_admitted(int sx, int sy) { return (sx == 0 && sy == 0) || (sx == -1 && (sy == -1 || sy == 0)) || (sx == 1 && sy == 1); }
// the plane size one axis must have at shift s over m motion samples: [lo, hi]
static inline void shift_size(int s, int m, long long& lo, long long& hi) {
    if (s == 0) lo = hi = m;
    else if (s < 0) lo = hi = ((long long)m + 1) / 2;
    else { lo = 2ll * m - 1; hi = 2ll * m; }
}
static inline std::string shift_words(int sx, int sy) { return "(" + std::to_string(sx) + ", " + std::to_string(sy) + ")"; }

// one set against a motion field of mw x mh: 0, or 1 with the fault in `err`
static inline int check_set(const rife_hip_apply_set_t* s, int mw, int mh, std::string& err) {
    if (!s) { err = "null set"; return 1; }
    if (mw <= 0 || mh <= 0) { err = "bad motion size"; return 1; }
    const rife_hip_planes_t* d[3] = {s->p0, s->p1, s->out};
    static const char* const nm[3] = {"planes 0: ", "planes 1: ", "planes out: "};
    for (int i = 0; i < 3; i++) if (check(d[i], err)) { err = nm[i] + err; return 1; }
    if (!agree(*s->p0, *s->p1) || !agree(*s->p0, *s->out)) { err = "the three plane sets differ in w, h, n, sample or maxval"; return 1; }
    const int w = s->p0->w, h = s->p0->h;
    if ((long long)w * h > (1ll << 27)) { err = "planes too large (more than 2^27 pixels)"; return 1; }
    if (!shift_admitted(s->shift_x, s->shift_y)) {
        err = "the shift pair " + shift_words(s->shift_x, s->shift_y) + " is not one of (0, 0), (-1, -1), (-1, 0), (1, 1)";
        return 1;
    }
    long long wlo, whi, hlo, hhi;
    shift_size(s->shift_x, mw, wlo, whi); shift_size(s->shift_y, mh, hlo, hhi);
    if (w < wlo || w > whi || h < hlo || h > hhi) {
        const std::string ww = wlo == whi ? std::to_string(wlo) : std::to_string(wlo) + " or " + std::to_string(whi);
        const std::string hh = hlo == hhi ? std::to_string(hlo) : std::to_string(hlo) + " or " + std::to_string(hhi);
        err = "the plane size (" + std::to_string(w) + " x " + std::to_string(h) + ") does not fit a motion of " + std::to_string(mw) + " x " + std::to_string(mh) +
              " at shift " + shift_words(s->shift_x, s->shift_y) + ", which takes planes of " + ww + " x " + hh;
        return 1;
    }
    return check_extent(w, h, s->wp, s->hp, err);
}

// the sets of a call: the count, then every set by its number
static inline int check_sets(int nsets, const rife_hip_apply_set_t* sets, int mw, int mh, std::string& err) {
    if (nsets < 1 || nsets > 4) { err = "the set count (" + std::to_string(nsets) + ") is not in 1..4"; return 1; }
    if (!sets) { err = "null sets"; return 1; }
    for (int k = 0; k < nsets; k++) if (check_set(&sets[k], mw, mh, err)) { err = "set " + std::to_string(k) + ": " + err; return 1; }
    return 0;
}
// the motion of an apply call: the rules of rife_hip_motion_check for mw x mh, both buffers present
static inline int check_sets_motion(const rife_hip_motion_t* m, int mw, int mh, std::string& err) {
    if (rife_motion::check(m, mw, mh, err)) { err = "motion: " + err; return 1; }
    if (!m->flow || !m->mask) { err = "motion: an apply call needs both flow and mask"; return 1; }
    return 0;
}

}  // namespace rife_apply
