"""A numpy model of the colour filter's three roads (fractal-renderer_amd/csrc/fr_colour.h: colour_filter_stage1_packed and
colour_outside_filtered; fr_kernels.hip: colour_fast32) and of the host's constants (fr_api.hip: fill_params), operation for
operation — test infrastructure only.  A correctly rounded f32 log2 stands in for v_log_f32, so what the model says about an input is a
statement about the INPUT (how far its value lies from a byte boundary, measured in the filter's own windows), not about the
hardware.  tests/golden/make_colour_boundaries.py counts roads with it; tests/test_colour_boundaries_cpu.py shows that the
fixture's rungs convict a filter whose windows are too narrow or indexed without color_multiply's swap.
"""
import functools
import math
from fractions import Fraction

import numpy as np

f32 = np.float32
CH = (0, 2, 1)  # color_multiply's RGB::new(r, b, g): output channel k shows the stored field CH[k]
NU_BRACKET = 2.0 ** -18  # FR_NU_BRACKET (fr_kernels.h)
F32_RANGE_TOP = float.fromhex("0x1.ffffep119")


def fma64(a, b, c):
    """fl64(a * b + c), one rounding"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fma32(a, b, c):
    """fl32(a * b + c) for f32 a, b, c: the f64 product of two f32 is exact, and the f64 sum is too whenever the exponents lie
    within 29 bits of each other; beyond that the smaller term only decides a tie, which the exact form below settles"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return f32(a * b + c)
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    lo = f32(float(exact))
    # repair a double rounding: compare the two f32 neighbours of the f64-rounded sum exactly
    best = lo
    for cand in (np.nextafter(lo, f32(-np.inf)), np.nextafter(lo, f32(np.inf))):
        if math.isfinite(float(cand)) and abs(Fraction(float(cand)) - exact) < abs(Fraction(float(best)) - exact):
            best = cand
    return f32(best)


def sat_trunc(v):
    """Rust's `as u8`: truncate toward zero, saturate, NaN -> 0 (sat_u8_dev)"""
    v = float(v)
    if v != v or v <= 0.0:
        return 0
    return 255 if v >= 255.0 else int(v)


def sat_floor_pack(v):
    """sat_u8_pack: v_floor_f32, then v_cvt_pk_u8_f32 (round to nearest even, saturate, NaN -> 0)"""
    v = float(v)
    if v != v:
        return 0
    return int(min(255.0, max(0.0, math.floor(v)))) if math.isfinite(v) else (255 if v > 0 else 0)


def sat_rne_pack(v):
    """v_cvt_pk_u8_f32 alone"""
    v = float(v)
    if v != v:
        return 0
    if not math.isfinite(v):
        return 255 if v > 0 else 0
    return int(min(255.0, max(0.0, float(np.rint(v)))))


class Consts:
    """fill_params' colour-filter constants for (iterations n, exposure, stored primary fields, stable_limit) with
    fr_set_colour_filter(knob); zero_windows / unswapped_widths are the two broken filters the CPU tests convict (unswapped:
    filt_d and filt_d32 indexed by the output channel, in colour_filter_stage1_packed and in the f64 stage)."""

    def __init__(self, n, exposure, prim, stable_limit, knob=1, zero_windows=False, unswapped_widths=False):
        self.n, self.exposure, self.prim, self.stable_limit = int(n), float(exposure), tuple(float(p) for p in prim), float(stable_limit)
        self.filt_k = self.exposure / float(n) if n else 0.0
        ak = abs(self.filt_k)
        self.filter = bool(knob) and n != 0 and math.isfinite(self.exposure) and ak <= 1e100 and self.stable_limit >= 0.0
        self.filter32 = self.filter and knob == 1 and n < (1 << 24) and 2.0 ** -60 <= ak <= 2.0 ** 60
        with np.errstate(all="ignore"):
            self.filt_k32 = f32(self.filt_k)
        up = lambda x: np.nextafter(f32(x), f32(np.inf))  # noqa: E731
        self.filt_c32 = up(ak * NU_BRACKET * (1.0 + 2.0 ** -9)) if self.filter32 else f32(0)
        self.filt_d = [p * ak * NU_BRACKET * (1.0 + 2.0 ** -20) for p in self.prim]
        self.filt_d32 = [up(p * ak * NU_BRACKET * (1.0 + 2.0 ** -10)) if self.filter32 else f32(0) for p in self.prim]
        self.prim32 = [f32(p) for p in self.prim]
        lo = max(self.stable_limit, 2.0) * (1.0 + 2.0 ** -20)
        self.filt_lo32 = up(lo) if (self.filter32 and lo < 1e30) else f32(np.inf)
        self.rel32, self.rel32_fast, self.rel64 = f32(2.0 ** -21), f32(2.0 ** -20), 2.0 ** -46
        if zero_windows:
            self.filt_c32 = f32(0)
            self.filt_d = [0.0] * 3
            self.filt_d32 = [f32(0)] * 3
            self.rel32 = self.rel32_fast = f32(0)
            self.rel64 = 0.0
        self.width_of = (lambda k: k) if unswapped_widths else (lambda k: CH[k])


@functools.lru_cache(maxsize=None)
def _log2_f32(x):
    import mpmath  # here, not at the top: the GPU tests load the fixture through this module and need no mpmath

    with mpmath.workprec(120):
        return f32(float(mpmath.log(mpmath.mpf(x), 2)))  # 120 bits, then f64, then f32: a double rounding needs a 2^-29 tie


def log2_f32(x):
    """the correctly rounded f32 log2 of an f32, the same on every host (numpy's f32 loop and libm differ between CPUs)"""
    x = float(x)
    if x != x or x < 0.0:
        return f32(np.nan)
    if x == 0.0:
        return f32(-np.inf)
    return _log2_f32(x) if math.isfinite(x) else f32(np.inf)


def nu32_of(d32):
    with np.errstate(all="ignore"):
        return log2_f32(f32(log2_f32(f32(d32)) * f32(0.25)))


def stage1_packed(c, dist, iters):
    """colour_filter_stage1 on (float)dist: (decided, bytes)"""
    in_range = 2.0 <= dist <= 2.0 ** 120
    nu32 = nu32_of(f32(dist))
    with np.errstate(all="ignore"):
        m32 = f32(f32(f32(iters + 1) - nu32) * c.filt_k32)
        lo, hi = [], []
        for k in range(3):
            v = f32(c.prim32[CH[k]] * m32)
            w = fma32(abs(v), c.rel32, c.filt_d32[c.width_of(k)])
            lo.append(sat_floor_pack(f32(v - w)))
            hi.append(sat_floor_pack(f32(v + w)))
    return in_range and lo == hi, tuple(lo)


def fast32(c, dist, iters):
    """colour_packed's rule 1 (colour_fast32 and its range test) on (float)dist: (decided, bytes).  This form has ONE window, on
    m, and no width per channel: unswapped_widths changes nothing here, only the f64 stage behind it."""
    d32 = f32(dist)
    sure = bool(d32 >= c.filt_lo32) and bool(d32 <= f32(F32_RANGE_TOP))
    nu32 = nu32_of(d32)
    with np.errstate(all="ignore"):
        m = f32(f32(f32(iters + 1) - nu32) * c.filt_k32)
        w = fma32(abs(m), c.rel32_fast, c.filt_c32)
        ml, mh = f32(m - w), f32(m + w)
        lo, hi = [], []
        for k in range(3):
            p = c.prim32[CH[k]]
            lo.append(sat_rne_pack(fma32(p, ml, f32(-0.5))))
            hi.append(sat_rne_pack(fma32(p, mh, f32(-0.5))))
    return sure and lo == hi, tuple(lo)


def stage2(c, dist, iters):
    """colour_outside_filtered's f64 stage: (decided, bytes)"""
    in_range = 2.0 <= dist <= 2.0 ** 120
    nu32 = nu32_of(f32(dist))
    it2 = (float(iters) + 1.0) - float(nu32)
    m = it2 * c.filt_k
    lo, hi = [], []
    for k in range(3):
        v = c.prim[CH[k]] * m
        w = fma64(abs(v), c.rel64, c.filt_d[c.width_of(k)])
        lo.append(sat_trunc(v - w))
        hi.append(sat_trunc(v + w))
    return in_range and lo == hi, tuple(lo)


def road(c, dist, iters, form="packed"):
    """('f32' | 'f64' | 'exact', bytes or None) for a pixel with dist > stable_limit under smooth colouring"""
    if c.filter32:
        ok, b = (stage1_packed if form == "packed" else fast32)(c, dist, iters)
        if ok:
            return "f32", b
    if c.filter:
        ok, b = stage2(c, dist, iters)
        if ok:
            return "f64", b
    return "exact", None


# ---- the associations of the order KATs (plain IEEE f64; log2 and sqrt supplied by the caller) --------------------------------

SMOOTH_ALTS = ("colq_e", "i_en", "ip1_nu", "log_dist_4")
FLAT_ALTS = ("colq_e", "i_en")
INSIDE_ALTS = ("fma_dist",)


def smooth_value(col, iters, n, exposure, dist, log2, alt=None):
    """col * (((iters + (1 - nu)) / n) * exposure) with nu = log2(log2(sqrt(dist)) / 2), or one other association of it"""
    nu = log2(log2(dist) / 4.0) if alt == "log_dist_4" else log2(log2(math.sqrt(dist)) / 2.0)
    it = (float(iters) + 1.0) - nu if alt == "ip1_nu" else float(iters) + (1.0 - nu)
    return flat_value(col, it, n, exposure, alt)


def flat_value(col, it, n, exposure, alt=None):
    if alt == "colq_e":
        return (col * (it / float(n))) * exposure
    if alt == "i_en":
        return col * (it * (exposure / float(n)))
    return col * ((it / float(n)) * exposure)


def inside_dist(re, im, alt=None):
    return fma64(re, re, im * im) if alt == "fma_dist" else re * re + im * im


# ---- the fixture tests/golden/colour_boundaries.npz --------------------------------------------------------------------------


class Fixture:
    def __init__(self, path=None):
        import json
        import os

        path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colour_boundaries.npz")
        with np.load(path) as f:
            for k in f.files:
                setattr(self, k, f[k])
        self.meta = json.loads(str(self.meta))
        self.names = [str(s) for s in self.cfg_name]

    def consts(self, c, **kw):
        return Consts(int(self.cfg_iterations[c]), float(self.cfg_exposure[c]), [int(v) for v in self.cfg_primary[c]],
                      float(self.cfg_stable_limit[c]), **kw)

    def oracle_config(self, O, c, **kw):
        """the oracle's Config of configuration c (the default secondary colour, smooth, inside)"""
        return O.config_new(iterations=int(self.cfg_iterations[c]), exposure=float(self.cfg_exposure[c]),
                            primary_color=tuple(int(v) for v in self.cfg_primary[c]), stable_limit=float(self.cfg_stable_limit[c]), **kw)

    def rungs_of(self, c):
        """(z [m, 2], iters [m], index into the rung arrays [m]) of configuration c"""
        at = np.flatnonzero(self.rung_cfg == c)
        z = np.zeros((at.size, 2))
        z[:, 0] = self.rung_re[at]
        return z, self.rung_iters[at].copy(), at

    def kat_config(self, O, j):
        p = int(self.kat_colour[j])
        return O.config_new(iterations=int(self.kat_iterations[j]), exposure=float(self.kat_exposure[j]), primary_color=(p, p, p),
                            secondary_color=(p, p, p), stable_limit=float(self.kat_stable_limit[j]),
                            smooth=0 if str(self.kat_path[j]) == "flat" else 1, inside=1)
