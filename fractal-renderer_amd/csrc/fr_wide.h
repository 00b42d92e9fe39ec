/*
 * fr_wide.h — internal: the fixed-point view centre of WIDE PT (include/fractal_hip.h, "WIDE PT") and its reference
 * orbits, host arithmetic only (fr_wide.hip).  fr_pt.hip keeps the orbits on the device; fr_api.hip checks the domain.
 */
#ifndef FR_WIDE_H
#define FR_WIDE_H

#include <cstdint>
#include <vector>

#include "../../include/fractal_hip.h"

namespace fr {

/* an orbit's last stored entry as integers: what continuing the recurrence needs (the role OrbitEnd's dd pair plays) */
struct WideTail {
    std::vector<uint64_t> re, im; /* n words each; empty: no wide orbit */
};

/* WIDE PT's domain (include/fractal_hip.h), or — `scaled` — SCALED PT's: limit <= 2^20, the axes of scale within 2^32 of
 * each other, and no 2^440 rule (F >= e + 64 bounds the scale); no device needed */
int check_pt_wide(const fr_config *cfg, const fr_wide_centre *centre, bool scaled = false);

/* Orbit `which` (0: R or V, 1: K) of the view as re, im pairs of the stored f64 entries, appended to `out`; at most
 * iterations + 2 entries in all.  from == nullptr: the whole orbit, entry 0 first.  Otherwise entries 0 .. last of an orbit
 * CUT BY THE CAP exist already (`last` = its kmax, *from its last entry) and the recurrence goes on from entry last + 1.
 * `ended` / `tail`: how the orbit's last entry came about, and that entry.  Arguments already checked. */
void wide_reference_orbit(const fr_config *cfg, const fr_wide_centre *centre, int which, std::vector<double> &out, bool &ended,
                          WideTail &tail, const WideTail *from = nullptr, uint32_t last = 0);

/* the view's identity for the orbit cache: n, then the words of re and of im */
void wide_key(const fr_wide_centre *centre, std::vector<uint64_t> &key);

}  // namespace fr

#endif
