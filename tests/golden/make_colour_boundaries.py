#!/usr/bin/env python3
"""Regenerates tests/golden/colour_boundaries.npz: inputs of the colour map (calc/src/lib.rs:214-234) AIMED at byte boundaries.

The colour filter (fr_colour.h, fr_kernels.hip: colour_fast32) decides a pixel's bytes from an f32 or f64 bracket around nu and
is right only if every window is wide enough; natural images put about one pixel in 10^5 near a boundary.  The recolour calls
take any (z, iters), so this file computes, with mpmath at 70 digits, inputs whose true colour value lies at a chosen distance
from a chosen byte boundary:

  rungs   for a configuration (iterations n, exposure E, stored primary fields, stable_limit), an output channel k (which
          shows the stored field p_k = primary[CH[k]], CH = (0, 2, 1)), a boundary B and an offset d, solve over the reals
              p_k * (i + 1 - nu) * E / n = B + d,
          with i such that nu lies in (3, 4] — where real escapes at the default limit lie —, dist = 2^(4 * 2^nu) and
          z = (sqrt(dist), 0) rounded to f64.  The real value is then RE-EVALUATED from the rounded z; the fixture stores what
          was found.  Offsets are in units of W_k = p_k * |E / n| * 2^-18 (FR_NU_BRACKET in byte units of that channel): one W
          is 2^-18 in nu whatever the configuration.
  gates   pixels at the ends of the filter's range of dist (2 and 2^120 exactly, and one f64 step outside each), unaimed: each
          channel's real value at least 1e-3 from an integer.
  order   known answers for the OPERATION ORDER of the exact paths: an exposure (or, for the inside colour, a position) at which
          the reference's association col * (((iters + (1 - nu)) / n) * E) truncates to one byte and another association of the
          same real expression to the other.  log2 is correctly rounded here (mpmath), and a KAT is kept only if the oracle gives
          the same byte with its software log2.

Every rung must be placed: within a quarter of the intended offset, and with |d| at least 1000 times what the oracle's own f64
arithmetic (libm log2) misses the real value by — so the expected byte does not depend on whose log2 or whose rounding order
computed it.  A rung that fails either makes this script fail; nothing is skipped.  Deterministic: fixed seeds, no clock.

    python3 tests/golden/make_colour_boundaries.py [--check]
"""
import json
import math
import os
import random
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import colour_model as CM  # noqa: E402
import oracle_lib as O  # noqa: E402

mp.mp.dps = 70
OUT = os.path.join(HERE, "colour_boundaries.npz")
CH = CM.CH

BOUNDARIES = (1, 2, 17, 64, 128, 200, 254, 255, 256)  # 256: no byte flips there (saturation), a control
LADDER = (2.0 ** -12, 0.25, 0.75, 1.5, 4.0, 64.0, 256.0, 1024.0)  # the last two: so that the f32 stage decides some rung too
UP, DOWN = math.inf, -math.inf
CAP = (1 << 24) - 1

# At the cap (i + 1 - nu of the order 2^23, K = 255 / 2^24) the f64 spacing of the value, 2^-45 byte near 255, is 5e-4 W: with a
# dyadic K a target 2^-12 W from B rounds to B itself, so that one rung cannot stand 1000 times clear of the oracle's own
# rounding and W / 8 takes its place.  The two far rungs are for the f32 stage, whose i + 1 - nu32 has a spacing of 1 there: it
# can decide nothing closer than |v| * 2^-21, some 2^21 W (2^31 W is an eighth of a byte per unit of p_k).
LADDER_CAP = (0.125,) + LADDER[1:] + (2.0 ** 22, 2.0 ** 31)
ZERO = (0,)  # the configurations whose bytes are 0 (or 0 | 255) throughout: the boundary is 0, from both sides

# name, iterations, exposure, stored primary fields (r, g, b), stable_limit, boundaries, ladder
CONFIGS = [
    ("default-colours", 1024, 2.0, (40, 255, 40), 2.0, BOUNDARIES, LADDER),  # RGB::new(40, 40, 255): the fields differ
    ("255-40-7", 1024, 2.0, (255, 40, 7), 2.0, BOUNDARIES, LADDER),
    ("zero-field", 1000, 3.0, (200, 0, 90), 2.0, BOUNDARIES, LADDER),  # without the swap channel 1 would get the width 0
    ("steep-fields", 1024, 2.0, (7, 255, 1), 2.0, BOUNDARIES, LADDER),  # ... and here channel 2 one 255 times too narrow
    ("negative-exposure", 1024, -2.0, (255, 40, 7), 2.0, ZERO, LADDER),
    ("n-1000", 1000, 5.0, (255, 40, 7), 2.0, BOUNDARIES, LADDER),
    ("n-77", 77, 2.0, (200, 255, 128), 2.0, BOUNDARIES, LADDER),
    ("n-cap", CAP, 255.0 * CAP / 2.0 ** 24, (1, 2, 1), 2.0, (200, 254, 255), LADDER_CAP),  # K = 255 / 2^24, i + 1 >= 2^23
    ("n-2^24", 1 << 24, 2.0 ** 15, (255, 40, 7), 2.0, BOUNDARIES, LADDER),  # the f32 stage is off
    ("K-2^-60", 1024, 2.0 ** -50, (255, 40, 7), 2.0, ZERO, LADDER),
    ("K-under-2^-60", 1024, math.nextafter(2.0 ** -50, DOWN), (255, 40, 7), 2.0, ZERO, LADDER),  # the f32 stage is off
    ("K-2^60", 1024, 2.0 ** 70, (255, 40, 7), 2.0, ZERO, LADDER),
    ("K-over-2^60", 1024, math.nextafter(2.0 ** 70, UP), (255, 40, 7), 2.0, ZERO, LADDER),  # the f32 stage is off
    ("K-1e100", 1024, 1e100 * 1024.0, (255, 40, 7), 2.0, ZERO, LADDER),  # the f32 stage is off, the f64 stage on
    ("K-over-1e100", 1024, math.nextafter(1e100, UP) * 1024.0, (255, 40, 7), 2.0, ZERO, LADDER),  # the filter is off
    ("negative-stable-limit", 1024, 2.0, (255, 40, 7), -1.0, BOUNDARIES, LADDER),  # the filter is off
]
GATE_CONFIG = ("range-ends", 1024, 2.0, (255, 40, 7), 0.5, (), ())  # stable_limit 0.5: a dist near 2 is "outside"


def M(x):
    return mp.mpf(x)


def real_nu(re, im=0.0):
    return mp.log(mp.log(mp.sqrt(M(re) ** 2 + M(im) ** 2), 2) / 2, 2)


def real_value(p, i, n, exposure, re, im=0.0):
    return M(p) * (i + 1 - real_nu(re, im)) * (M(exposure) / n)


def libm_value(p, i, n, exposure, re, im=0.0):
    """the oracle's arithmetic (oracle/fractal_oracle.c: colour_of) with the platform's log2"""
    dist = re * re + im * im
    nu = math.log2(math.log2(math.sqrt(dist)) / 2.0)
    return float(p) * ((float(i) + (1.0 - nu)) / float(n) * exposure)


def sat(v):
    return int(min(255, max(0, mp.floor(v))))


def place(cfg, k, B, mult):
    """one rung: (iters, re, real value - B, |oracle's value - real value|, expected byte), or None if B is out of p_k's reach"""
    name, n, exposure, prim, _sl, _b, _l = cfg
    p = prim[CH[k]]
    if p == 0:
        return None
    K = M(exposure) / n
    W = p * abs(K) * M(2) ** -18
    delta = mult * W
    reach = mp.floor(M(B) / (p * K) + 3)
    if B != 0 and not 3 <= reach <= n - 2:
        return None  # the boundary itself, not the offset, decides: a boundary is in for every rung of the ladder or for none
    t = (M(B) + delta) / (p * K)  # i + 1 - nu
    i = int(mp.floor(t + 3))
    nu = i + 1 - t
    assert 0 <= i <= n - 1 and 3 < nu <= 4, (name, k, B, mult, i, float(nu))
    re = float(mp.sqrt(mp.power(2, 4 * mp.power(2, nu))))
    real = real_value(p, i, n, exposure, re)
    off = real - B
    if abs(off - delta) > abs(delta) / 4:
        raise SystemExit("cannot place %s channel %d B %d at %g W: landed at %g W" % (name, k, B, mult, float(off / W)))
    err = abs(M(libm_value(p, i, n, exposure, re)) - real)
    if abs(delta) < 1000 * err:
        raise SystemExit("%s channel %d B %d at %g W: the oracle's own error %g W is within 1/1000 of the offset"
                         % (name, k, B, mult, float(err / W)))
    return i, re, float(off), float(err), sat(real), float(err / W)


def make_rungs():
    rows, meta = [], {}
    for c, cfg in enumerate(CONFIGS):
        name, n, exposure, prim, sl, bounds, ladder = cfg
        worst_abs = worst_w = 0.0
        groups = {}
        for k in range(3):
            for B in bounds:
                for mult in ladder:
                    for sgn in (1.0, -1.0):
                        r = place(cfg, k, B, sgn * mult)
                        if r is None:
                            continue
                        i, re, off, err, byte, err_w = r
                        rows.append((c, k, B, sgn * mult, i, re, off, err, byte))
                        worst_abs, worst_w = max(worst_abs, err), max(worst_w, err_w)
                        groups.setdefault(k, []).append((re * re, i, byte))
        roads = {}
        for form in ("packed", "fast32"):
            consts = CM.Consts(n, exposure, prim, sl)
            for k, rungs in groups.items():
                count = {"f32": 0, "f64": 0, "exact": 0}
                for dist, i, byte in rungs:
                    where, b = CM.road(consts, dist, i, form)
                    count[where] += 1
                    assert b is None or b[k] == byte, (name, form, k, dist, i, b, byte)
                roads["%s/%d" % (form, k)] = count
        meta[name] = {"rungs": sum(len(g) for g in groups.values()), "oracle_error_bytes": worst_abs, "oracle_error_W": worst_w,
                      "roads": roads}
    return rows, meta


def make_gates():
    """dist = re^2 + im^2 in f64 EXACTLY at 2, one step under, 2^120, one step over; iters such that no channel is near a boundary"""
    name, n, exposure, prim, sl, _b, _l = GATE_CONFIG
    pts = [(1.0, 1.0, 2.0), (1.0, 1.0 - 2.0 ** -53, math.nextafter(2.0, DOWN)), (2.0 ** 60, 0.0, 2.0 ** 120),
           (2.0 ** 60, 2.0 ** 34, math.nextafter(2.0 ** 120, UP))]
    rows = []
    for re, im, want in pts:
        assert re * re + im * im == want and M(re) ** 2 + M(im) ** 2 != 0
        for i in (7, 100, 333, 501):
            vals = [real_value(prim[CH[k]], i, n, exposure, re, im) for k in range(3)]
            if all(abs(v - mp.nint(v)) > 1e-3 for v in vals):
                rows.append((re, im, i, [sat(v) for v in vals]))
    assert len(rows) >= 8
    return rows


# ---- order KATs ----------------------------------------------------------------------------------------------------------------


def cr_log2(x):
    return float(mp.log(M(x), 2))


def oracle_byte(n, exposure, col, sl, smooth, re, im, i, channel=0):
    """the oracle's byte with its SOFTWARE log2 — plain f64 arithmetic, the same on every host.  (That libm's log2 gives the same
    byte is asserted by tests/test_colour_boundaries_cpu.py, not used here: the fixture must not depend on the host's libm.)"""
    cfg = O.config_new(iterations=n, exposure=exposure, primary_color=col, secondary_color=col, stable_limit=sl, smooth=smooth, inside=1)
    try:
        O.set_log2_mode(O.LOG2_SOFT)
        return int(O.colour_rows(cfg, np.array([[re, im]]), np.array([i], dtype=np.uint32), threads=1)[0, channel])
    finally:
        O.set_log2_mode(O.LOG2_LIBM)


def steps(x, s):
    for _ in range(abs(s)):
        x = math.nextafter(x, UP if s > 0 else DOWN)
    return x


def trunc(v):
    return CM.sat_trunc(v)


def order_kats(per=8):
    rng = random.Random(20261019)
    rows = []

    def search(path, alt, n_choices, make):
        found, tries = 0, 0
        while found < per:
            tries += 1
            assert tries < 20000, (path, alt)
            n = rng.choice(n_choices)
            # the two forms of log_zn differ by an ulp of nu at the most, which i + (1 - nu) keeps only while i is small
            # ... and the flat KATs also go through a small render, which must hold a pixel with that escape index
            i = rng.randrange(3, 9) if alt == "log_dist_4" else rng.randrange(3, 20) if path == "flat" else rng.randrange(3, n)
            p = rng.choice((255, 200, 129, 40, 7))
            B = rng.randrange(1, 256)
            got = make(n, i, p, B)
            if got is None:
                continue
            exposure, re, im, byte, alt_byte = got
            smooth = 0 if path == "flat" else 1
            sl = 0.5 if alt == "log_dist_4" else 2.0
            if oracle_byte(n, exposure, (p, p, p), sl, smooth, re, im, i) != byte:
                continue
            rows.append((path, alt, n, exposure, p, sl, re, im, i, byte, alt_byte))
            found += 1

    def smooth_make(alt):
        def make(n, i, p, B):
            # 1 - nu is exact for nu in [0.5, 8), and then both orders of i + 1 - nu round the same real number once: only a
            # nu under 0.5 (a dist under 2^5.7, which a small `limit` leaves) can tell them apart
            nu = rng.uniform(-1.5, 0.45) if alt == "ip1_nu" else rng.uniform(3.0, 4.0)
            re, im = float(mp.sqrt(mp.power(2, 4 * mp.power(2, M(nu))))), 0.0
            if alt == "log_dist_4":
                # a logarithm swallows its argument's last bit unless it is small: only for a dist close to 1 (under a small
                # stable_limit) does sqrt's rounding reach log_zn, and off the axis sqrt(dist) is not simply |re| again
                re = math.sqrt(rng.uniform(1.02, 1.5))
                re, im = re * 0.8, re * 0.6
            dist = re * re + im * im
            ref_q = CM.smooth_value(1.0, i, n, 1.0, dist, cr_log2)
            if ref_q <= 0 or (alt in ("ip1_nu", "log_dist_4") and ref_q == CM.smooth_value(1.0, i, n, 1.0, dist, cr_log2, alt)):
                return None
            e0 = B / (p * ref_q)
            for s in range(-16, 17):
                e = steps(e0, s)
                a = trunc(CM.smooth_value(float(p), i, n, e, dist, cr_log2))
                b = trunc(CM.smooth_value(float(p), i, n, e, dist, cr_log2, alt))
                if a != b:
                    return e, re, im, a, b
            return None
        return make

    def flat_make(alt):
        def make(n, i, p, B):
            e0 = B / (p * (i / n))
            for s in range(-16, 17):
                e = steps(e0, s)
                a, b = trunc(CM.flat_value(float(p), float(i), n, e)), trunc(CM.flat_value(float(p), float(i), n, e, alt))
                if a != b:
                    return e, 300.0, 0.0, a, b  # any dist > stable_limit
            return None
        return make

    def inside_make(n, i, p, B):
        d = B / p
        if d > 2.0:
            return None
        re = math.sqrt(d) * rng.uniform(0.2, 0.9)
        im0 = math.sqrt(d - re * re)
        for s in range(-8, 9):
            im = steps(im0, s)
            a, b = trunc(p * CM.inside_dist(re, im)), trunc(p * CM.inside_dist(re, im, "fma_dist"))
            if a != b and re * re + im * im <= 2.0:
                return 2.0, re, im, a, b
        return None

    for alt in CM.SMOOTH_ALTS:
        search("smooth", alt, (1024, 1000, 300, 77, 4096), smooth_make(alt))
    search("flat", "colq_e", (1024, 256), flat_make("colq_e"))
    search("flat", "colq_e", (1000, 300, 77), flat_make("colq_e"))
    search("flat", "i_en", (1000, 300, 77), flat_make("i_en"))  # with n = 2^k both forms scale exactly: no such exposure exists
    search("inside", "fma_dist", (50,), inside_make)
    return rows


def build():
    rungs, meta = make_rungs()
    gates = make_gates()
    kats = order_kats()
    cfgs = CONFIGS + [GATE_CONFIG]
    ordinary = [m for name, m in meta.items() if not name.startswith("K-")]
    summary = {
        "rungs": len(rungs), "gates": len(gates), "kats": len(kats), "omitted": 0,
        "largest_oracle_error_W": max(m["oracle_error_W"] for m in meta.values()),
        "largest_oracle_error_bytes_ordinary": max(m["oracle_error_bytes"] for m in ordinary),
        "roads_packed": {r: sum(m["roads"][g][r] for m in meta.values() for g in m["roads"] if g.startswith("packed"))
                         for r in ("f32", "f64", "exact")},
        "roads_fast32": {r: sum(m["roads"][g][r] for m in meta.values() for g in m["roads"] if g.startswith("fast32"))
                         for r in ("f32", "f64", "exact")},
        "configurations": meta,
    }
    arrays = {
        "cfg_name": np.array([c[0] for c in cfgs]),
        "cfg_iterations": np.array([c[1] for c in cfgs], dtype=np.uint32),
        "cfg_exposure": np.array([c[2] for c in cfgs], dtype=np.float64),
        "cfg_primary": np.array([c[3] for c in cfgs], dtype=np.uint8),
        "cfg_stable_limit": np.array([c[4] for c in cfgs], dtype=np.float64),
        "rung_cfg": np.array([r[0] for r in rungs], dtype=np.uint8),
        "rung_channel": np.array([r[1] for r in rungs], dtype=np.uint8),
        "rung_boundary": np.array([r[2] for r in rungs], dtype=np.int16),
        "rung_offset_W": np.array([r[3] for r in rungs], dtype=np.float64),
        "rung_iters": np.array([r[4] for r in rungs], dtype=np.uint32),
        "rung_re": np.array([r[5] for r in rungs], dtype=np.float64),
        "rung_real_offset": np.array([r[6] for r in rungs], dtype=np.float64),
        "rung_oracle_error": np.array([r[7] for r in rungs], dtype=np.float64),
        "rung_byte": np.array([r[8] for r in rungs], dtype=np.uint8),
        "gate_z": np.array([[g[0], g[1]] for g in gates], dtype=np.float64),
        "gate_iters": np.array([g[2] for g in gates], dtype=np.uint32),
        "gate_bytes": np.array([g[3] for g in gates], dtype=np.uint8),
        "kat_path": np.array([k[0] for k in kats]),
        "kat_alt": np.array([k[1] for k in kats]),
        "kat_iterations": np.array([k[2] for k in kats], dtype=np.uint32),
        "kat_exposure": np.array([k[3] for k in kats], dtype=np.float64),
        "kat_colour": np.array([k[4] for k in kats], dtype=np.uint8),
        "kat_stable_limit": np.array([k[5] for k in kats], dtype=np.float64),
        "kat_z": np.array([[k[6], k[7]] for k in kats], dtype=np.float64),
        "kat_iters": np.array([k[8] for k in kats], dtype=np.uint32),
        "kat_byte": np.array([k[9] for k in kats], dtype=np.uint8),
        "kat_alt_byte": np.array([k[10] for k in kats], dtype=np.uint8),
        "meta": np.array(json.dumps(summary, sort_keys=True)),
    }
    return arrays


def measured(key):
    return "oracle_error" in key


def without_measured(meta):
    """the metadata without the figures that depend on the host's libm (what the oracle's f64 arithmetic misses the real value by)"""
    if isinstance(meta, dict):
        return {k: without_measured(v) for k, v in meta.items() if not measured(k)}
    return meta


def same(a, b):
    """are two builds the same fixture?  Every input, expected byte and count exactly; the measured libm figures, which another
    host's libm may give an ulp differently, are left to the 1000-times bound that build() itself enforces"""
    if sorted(a) != sorted(b):
        return False
    exact = all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a if k != "meta" and not measured(k))
    return exact and without_measured(json.loads(str(a["meta"]))) == without_measured(json.loads(str(b["meta"])))


if __name__ == "__main__":
    arrays = build()
    if "--check" in sys.argv:
        with np.load(OUT) as old:
            ok = same(arrays, {k: old[k] for k in old.files})
        print("colour_boundaries.npz", "is current" if ok else "DIFFERS from a fresh run")
        sys.exit(0 if ok else 1)
    np.savez_compressed(OUT, **arrays)
    m = json.loads(str(arrays["meta"]))
    print("wrote %s: %d rungs, %d gates, %d KATs, %d bytes" % (OUT, m["rungs"], m["gates"], m["kats"], os.path.getsize(OUT)))
    print(json.dumps({k: v for k, v in m.items() if k != "configurations"}, indent=1))
    for name, c in m["configurations"].items():
        print(name, c["rungs"], "%.3g" % c["oracle_error_W"], c["roads"])
