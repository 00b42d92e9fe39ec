"""The exact per-pixel orbits that the deep roads (WIDE PT, BLA-PT, SCALED PT, their state and extend forms, and PT and DD on a
dd centre) are checked against, and the views they are checked on.

Everything here is plain Python integers: z <- z^2 + c in fixed point with P fraction bits, `>>` the floor, recursive()'s
index convention (calc/src/lib.rs:245-257).  It shares nothing with the library or with the C models of the other test
files; from tests/pt_wide_model.py it takes only the centres (mpmath at 1200 bits), frac_bits and floor_scaled, and from
tests/pt_scaled_model.py the minibrot's centre and the specs of the four existing views.

A pixel's point is the view's centre plus the pixel's offset, both exact: the centre is the wide centre's integers over 2^F
(or pos + pos_lo of a dd centre), the offset is woff 2^-e with woff from the header's f64 operations ("SCALED PT", constants
of a view).  Inside the common domain off == woff 2^-e as numbers, which View asserts.

Per pixel: iters; z, the f64 nearest to the exact value; settled, true when the four points displaced by +-delta on either
axis, delta = 2^-(e+34), give the same iters; move, the largest component-wise distance between z and the z of those four
points (on the f64 values).  A pixel that is not settled is chaotic at the resolution of its own f64 offset: no method that
starts from an f64 offset can be asked for its index.

P = 2e + 320, and everything is computed a second time at P + 320: tests/golden/make_deep_truth.py refuses to write the
fixture unless both give the same iters, z, settled and move on every pixel, and unless every view leaves at least 95 % of
its pixels settled with at least 10 distinct escape indices.  The (f), (g) and (h) views met that as first written; no centre
was moved and no cap lowered.

View also takes a Spec, or a generated record of tests/deep_random_views.py, in place of a name (tests/test_deep_random_cpu.py
computes such views' pixels when it runs; nothing of them is in the fixture).  A centre with spare words has F > 2e + 320, and P is
then F, so that the centre is still held exactly; for every view of VIEWS P is 2e + 320 as before."""
import math
import os
from collections import namedtuple
from fractions import Fraction

import numpy as np

import pt_scaled_model as S
import pt_wide_model as W

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "deep_truth.npz")
EXTRA = 320  # the second precision is P + EXTRA
DELTA_LOG2 = 34  # delta = 2^-(e + 34)
MIN_SETTLED = 0.95
MIN_INDICES = 10

# |z_model - z| <= move + Z_FLOOR max(|z|, 1) per component on a settled pixel whose index agrees.  The floor is there because
# an interior pixel can have move == 0 while a model is a few units in the last place off the rounded exact z.  Measured on the
# CPU over every wide-centre view, model and bits in -1, 40, 53 (tests/test_deep_truth_cpu.py prints it with -s and checks the
# constants): the largest excess (|z_model - z| - move) / max(|z|, 1) is Z_EXCESS_MEASURED, on MINI_OFF_860; the floor is 4 times
# that, rounded up to a power of two.
Z_EXCESS_MEASURED = 1.9507658047129975e-16
Z_FLOOR = 2.0 ** -50
# A table at 40 bits (eps = 2^-40) has a floor of its own on the generated views of tests/deep_random_views.py.  Each skip keeps z
# within a relative eps of what the plain loop gives, and the final steps of an escape at a large limit square that error: on a
# view with limit 2^20 the model at 40 bits is 1.5e-11 max(|z|, 1) past move (Z_EXCESS_MEASURED_40, on seed 10 view 1 of the
# generator, a Julia view at 2^921 with limit 2^20 on the fixed point of -0.12 + 0.75i, pixel (12, 0); 1.2e-11 at pixel (44, 1), where |z| = 2.8e7) while the
# plain loop and the table at 53 bits stay inside `move` there, and the error follows eps from 24 to 48 bits: the definition is
# met and the seven hand-written views, with limits 2 and 65536, had measured too narrowly.  The same 4 times rule.  Z_FLOOR
# itself, which every existing assertion uses, stays: bits -1 and 53 stay under it on every generated view.
Z_EXCESS_MEASURED_40 = 1.471859911378064e-11
Z_FLOOR_40 = 2.0 ** -33


def z_floor(bits):
    """the floor of the generated views' spot check: Z_FLOOR, and Z_FLOOR_40 for a table at 40 bits (bits 0 is 40)"""
    return Z_FLOOR_40 if bits in (0, 40) else Z_FLOOR


# The dd-centre view has constants of its own.  Its roads iterate the reference orbit (PT, BLA-PT) or the pixel itself (DD) in
# dd arithmetic, whose operations are good to about 2^-104 of their value: every step moves the point by what a displacement of
# some 2^-104 would, while delta there is 2^-(84 + 34) = 2^-118.  So z is off by thousands of `move`, by design of a dd centre
# and not by a fault of the models: measured, at most 7.4e3 move (DD; PT and BLA-PT 5.2e3), an excess over move of
# Z_EXCESS_MEASURED_DD max(|z|, 1).  Kept apart so that the wide-centre floor stays at 2^-50; both bounds are asserted there:
# the floor by the same recipe, and |z_model - z| <= DD_MOVE_RATIO move wherever move > 0, 4 times the measured ratio rounded up
# to a power of two, which follows each pixel's own sensitivity.
Z_EXCESS_MEASURED_DD = 0.030711534082116958
Z_FLOOR_DD = 2.0 ** -3
DD_RATIO_MEASURED = 7.4e3
DD_MOVE_RATIO = 2.0 ** 15

# kind "wide": a wide centre of n words, `centre` one of pt_wide_model's M, N, J or pt_scaled_model's MINI; kind "dd": the
# same point rounded to pos + pos_lo.  shift = (a, b, k): the centre is moved by (a + b i) 2^-k.  scale = (re, im).
Spec = namedtuple("Spec", "kind centre n shift scale limit width height cap")


def _existing(spec):
    """one of pt_scaled_model's views: on the centre itself, scale 2^k on both axes, limit 2"""
    name, n, scale_log2, width, height, cap = spec
    return Spec("wide", name, n, (0, 0, 0), (math.ldexp(1.0, scale_log2),) * 2, 2.0, width, height, cap)


VIEWS = {
    "M_440": _existing(S.M_440),  # (a) 37 x 21, ragged against the 16 x 16 workgroup; the edge of WIDE PT's domain
    "M_900": _existing(S.M_900),  # (b)
    "J_900": _existing(S.J_900),  # (c)
    "MINI_861": _existing(S.MINI_861),  # (d)
    # (e) off the minibrot's nucleus, an odd scale with a negative axis, the default limit
    "MINI_OFF_860": Spec("wide", "MINI", 16, (5, -3, 864), (math.ldexp(1.37, 860), math.ldexp(-0.81, 860)), 65536.0, 24, 16, 3204),
    # (f) the same kind inside WIDE PT's domain
    "M_OFF_299": Spec("wide", "M", 6, (3, -2, 304), (math.ldexp(-1.9, 299), math.ldexp(0.53, 299)), 65536.0, 37, 21, 5000),
    # (g) a Julia view off the fixed point
    "J_OFF_300": Spec("wide", "J", 6, (3, 2, 304), (math.ldexp(0.77, 300), math.ldexp(1.21, 300)), 65536.0, 16, 12, 5000),
    # (h) a dd centre around 10^25: pos + pos_lo is M + (3 - 2i) 2^-87 rounded to a dd, pos_lo normalised and nonzero
    "DD_1E25": Spec("dd", "M", None, (3, -2, 87), (1.3e25, -0.9e25), 65536.0, 32, 24, 2000),
}
# not in the fixture: the Julia view of DESIGN.md's BLA-PT table (64 x 48), on which BLA-PT at 40 bits and PT disagree at 13
# pixels; tests/test_deep_truth_cpu.py computes the exact orbits of those pixels when it runs
UNRECORDED = {"J_300_64": Spec("wide", "J", 6, (0, 0, 0), (math.ldexp(1.0, 300),) * 2, 2.0, 64, 48, 5000)}
WIDE_DOMAIN = ("M_440", "M_OFF_299", "J_OFF_300")  # inside WIDE PT's domain: the common domain of the scaled and unscaled roads
PAST = ("M_900", "J_900", "MINI_861", "MINI_OFF_860")
DD = ("DD_1E25",)


def _as_fraction(value):
    """an mpmath number as its exact binary value"""
    sign, man, exp, _ = value._mpf_
    return Fraction(-int(man) if sign else int(man)) * Fraction(2) ** int(exp)


class View:
    """One of VIEWS with everything exact that a pixel's point needs, and what the library's calls need.  Instead of a name it
    takes a Spec itself, or any record with Spec's fields (tests/deep_random_views.py's); such a record may carry `julia_set`, the
    constant of a Julia view on a centre other than J, and with it the centre "F": that constant's repelling fixed point."""

    def __init__(self, name):
        if isinstance(name, str):
            spec = VIEWS[name] if name in VIEWS else UNRECORDED[name]
            common = name not in PAST
        else:
            spec, name = name, repr(tuple(name))
            common = max(abs(s) for s in spec.scale) <= 2.0 ** 440  # WIDE PT's rule
        self.name, self.spec, self.kind, self.n = name, spec, spec.kind, spec.n
        self.width, self.height, self.cap, self.limit = spec.width, spec.height, spec.cap, spec.limit
        self.shape = (spec.height, spec.width)
        self.scale = spec.scale
        constant = getattr(spec, "julia_set", None)
        self.julia = spec.centre == "J" or constant is not None
        self.julia_set = (W.JULIA_SET if constant is None else tuple(constant)) if self.julia else None
        self.e = math.frexp(max(abs(spec.scale[0]), abs(spec.scale[1])))[1]  # max |scale| = f 2^e, 0.5 <= f < 1
        self.common = common  # inside the common domain of the scaled and unscaled roads
        self.P = 2 * self.e + 320
        a, b, k = spec.shift
        if spec.kind == "wide":
            f = W.frac_bits(spec.n)
            assert f >= self.e + 64 and k <= f, "the domain rule F >= e + 64"
            self.P = max(self.P, f)  # a centre with spare words (every view of VIEWS has the fewest: F < 2e + 320) is held exactly
            if spec.centre == "F":  # the repelling fixed point of the record's own constant
                import pt_scaled_state_model as R

                cre, cim = R._fixed_point_ints(self.julia_set, spec.n)
            else:
                cre, cim = S.centre_ints(spec.centre, spec.n)
            self.ints = (cre + (a << (f - k)), cim + (b << (f - k)))
            self.words = W.to_words(self.ints[0], spec.n), W.to_words(self.ints[1], spec.n)
            self.centre = (Fraction(self.ints[0], 1 << f), Fraction(self.ints[1], 1 << f))
            self.pos, self.pos_lo = (123.0, -77.0), None  # pos is not read
        else:
            re, im = (_as_fraction(c) for c in W.centre(spec.centre))
            re, im = re + Fraction(a, 1 << k), im + Fraction(b, 1 << k)
            self.pos = (float(re), float(im))
            self.pos_lo = (float(re - Fraction(self.pos[0])), float(im - Fraction(self.pos[1])))
            assert all(lo != 0.0 and hi + lo == hi for hi, lo in zip(self.pos, self.pos_lo)), "pos_lo normalised and nonzero"
            self.centre = (Fraction(self.pos[0]) + Fraction(self.pos_lo[0]), Fraction(self.pos[1]) + Fraction(self.pos_lo[1]))

    # ---- the pixel's offset, by the header's f64 operations -----------------------------------------------------------

    def woff(self, x, y):
        """(woff_re, woff_im) of "SCALED PT", constants of a view"""
        w, h = float(self.width), float(self.height)
        sinv = math.ldexp(1.0, -self.e)
        sre, sim = self.scale[0] * sinv, self.scale[1] * sinv  # exact
        return ((float(x) / h) - ((w / h) / 2.0)) / sre, ((float(y) / h) - 0.5) / sim

    def off(self, x, y):
        """(off_re, off_im) of DD's start, the offset of the unscaled roads"""
        w, h = float(self.width), float(self.height)
        return ((float(x) / h) - ((w / h) / 2.0)) / self.scale[0], ((float(y) / h) - 0.5) / self.scale[1]

    def offset(self, x, y):
        """the pixel's exact offset (re, im) as Fractions"""
        wre, wim = self.woff(x, y)
        got = (Fraction(wre) / (1 << self.e), Fraction(wim) / (1 << self.e))
        if self.common:  # the common domain: the two definitions of the offset are one number
            ore, oim = self.off(x, y)
            assert got == (Fraction(ore), Fraction(oim)), (self.name, x, y)
        return got

    def fixed(self, value, P):
        """an exact value as an integer over 2^P; it has to be one"""
        v = Fraction(value) * (1 << P)
        assert v.denominator == 1, "P fraction bits hold the point exactly"
        return v.numerator

    # ---- one pixel ------------------------------------------------------------------------------------------------------

    def pixel(self, x, y, extra=0):
        """-> (iters, (z.re, z.im) as f64, settled, move) at P + extra fraction bits"""
        P = self.P + extra
        ore, oim = self.offset(x, y)
        pre, pim = self.fixed(self.centre[0] + ore, P), self.fixed(self.centre[1] + oim, P)
        lim = self.fixed(Fraction(self.limit) ** 2, 2 * P)
        if self.julia:
            add = (self.fixed(self.julia_set[0], P), self.fixed(self.julia_set[1], P))
        else:
            add = None
        d = 1 << (P - self.e - DELTA_LOG2)
        it, z = _orbit(pre, pim, add, P, lim, self.cap)
        settled, move = True, 0.0
        for dre, dim in ((d, 0), (-d, 0), (0, d), (0, -d)):
            it2, z2 = _orbit(pre + dre, pim + dim, add, P, lim, self.cap)
            settled = settled and it2 == it
            move = max(move, abs(z2[0] - z[0]), abs(z2[1] - z[1]))
        return it, z, settled, move

    # ---- what the calls of the library and of the models take ------------------------------------------------------------

    def fill(self, cfg, cap=None):
        """fill a default Config (the library's or the oracle's) with this view, at its cap or at another"""
        cfg.algo = 2 if self.julia else 0
        cfg.width, cfg.height = self.width, self.height
        cfg.iterations = self.cap if cap is None else cap
        cfg.limit = self.limit
        cfg.scale.re, cfg.scale.im = self.scale
        cfg.pos.re, cfg.pos.im = self.pos
        if self.julia:
            cfg.julia_set.re, cfg.julia_set.im = self.julia_set
        return cfg


def _orbit(zr, zi, add, P, lim, cap):
    """recursive(cap, start, c, limit) on integers over 2^P: Mandelbrot (add None) is start = c = the point, Julia adds `add`.
    -> (index, z as f64s, each the nearest to the exact value)"""
    ar, ai = (zr, zi) if add is None else add
    rr, ii = zr * zr, zi * zi
    index = cap
    for i in range(cap):
        zr, zi = (rr >> P) - (ii >> P) + ar, ((zr * zi) >> (P - 1)) + ai
        rr, ii = zr * zr, zi * zi
        if rr + ii > lim:
            index = i
            break
    return index, (float(Fraction(zr, 1 << P)), float(Fraction(zi, 1 << P)))


_views = {}


def view(name):
    """the View of one of VIEWS, or of a Spec or record given in place of a name, made once per process"""
    if isinstance(name, View):
        return name
    if name not in _views:
        _views[name] = View(name)
    return _views[name]


def _pixel_job(job):
    name, x, y, extra = job
    return view(name).pixel(x, y, extra)


def view_truth(name, extra=0, pool=None):
    """every pixel of a view -> {"iters": uint32 [h, w], "z": float64 [h, w, 2], "settled": bool [h, w], "move": float64 [h, w]}"""
    v = view(name)
    jobs = [(name, x, y, extra) for y in range(v.height) for x in range(v.width)]
    res = pool.map(_pixel_job, jobs, chunksize=4) if pool is not None else list(map(_pixel_job, jobs))
    return {
        "iters": np.array([r[0] for r in res], dtype=np.uint32).reshape(v.shape),
        "z": np.array([r[1] for r in res], dtype=np.float64).reshape(v.shape + (2,)),
        "settled": np.array([r[2] for r in res], dtype=np.bool_).reshape(v.shape),
        "move": np.array([r[3] for r in res], dtype=np.float64).reshape(v.shape),
    }


def bounds(name):
    """the keyword arguments of assert_rows for a view: the floor of its kind of centre"""
    if VIEWS[name].kind == "dd":
        return {"floor": Z_FLOOR_DD, "max_ratio": DD_MOVE_RATIO}
    return {"floor": Z_FLOOR}


# (view, mode, bits) -> settled pixels on which a definition is off the exact index (mode: "wide", "bla", "scaled", "pt", "dd";
# bits -1 without a table).  Findings about the definitions, each described in DESIGN.md, "Accuracy against exact orbits"; an
# entry has to stay below 1 % of the view's pixels.  There is none: every model and every kernel has the exact index on every
# settled pixel of every view for bits -1, 40 and 53.
ALLOWED = {}


def allowed(name, mode, bits):
    n = ALLOWED.get((name, mode, 40 if bits == 0 else bits), 0)
    assert n < 0.01 * VIEWS[name].width * VIEWS[name].height
    return n


def splits(name):
    """the caps at which the resumable runs of a view are split in two links: cap / 3, and the median of the exact indices,
    which cuts through every view (on some of them every pixel has escaped before cap / 3)"""
    return sorted({VIEWS[name].cap // 3, int(np.median(load(name)["iters"]))})


def same_truth(a, b):
    """two results of view_truth equal, the doubles as bits"""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in a)


def condition(t):
    """(share of settled pixels, distinct escape indices) of a result: the generator asserts >= MIN_SETTLED and >= MIN_INDICES"""
    return float(t["settled"].mean()), len(np.unique(t["iters"]))


FIELDS = ("iters", "z", "settled", "move")


def load(name):
    """the fixture's record of a view, read-only, with "precision" = (P, P + EXTRA)"""
    with np.load(FIXTURE) as f:
        t = {k: f["%s/%s" % (name, k)] for k in FIELDS + ("precision",)}
    for a in t.values():
        a.setflags(write=False)
    return t


def sample_pixels(t):
    """the (x, y) that the freshness test recomputes: the largest escape index, an unsettled pixel where the view has one, two
    corners, the centre and one more"""
    h, w = t["iters"].shape
    y, x = np.unravel_index(int(np.argmax(t["iters"])), (h, w))
    out = [(int(x), int(y))]
    bad = np.argwhere(~t["settled"])
    if len(bad):
        out.append((int(bad[0][1]), int(bad[0][0])))
    for p in ((0, 0), (w - 1, h - 1), (w // 2, h // 2), (w // 3, (2 * h) // 3)):
        if p not in out:
            out.append(p)
    return out[:6]


# ---- the comparison of a model's or a kernel's rows with the truth ------------------------------------------------------------


def compare(t, z, iters, cap=None):
    """-> (settled pixels whose index differs from the exact one, the largest |z - z_exact| / move over the agreeing settled
    pixels with move > 0, the largest excess (|z - z_exact| - move) / max(|z|, 1) over the agreeing settled pixels).  With a cap
    below the view's the index is compared with min(exact, cap) and z is not compared (the two stop at different entries)."""
    want = t["iters"] if cap is None else np.minimum(t["iters"], cap)
    settled = t["settled"]
    differ = int(((iters != want) & settled).sum())
    if cap is not None:
        return differ, 0.0, 0.0
    ok = settled & (iters == want)
    err = np.abs(np.asarray(z, dtype=np.float64) - t["z"])[ok]  # [pixels, 2]
    move = t["move"][ok][:, None]
    size = np.maximum(np.hypot(t["z"][..., 0], t["z"][..., 1])[ok], 1.0)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(move > 0, err / move, 0.0)
    return differ, float(ratio.max(initial=0.0)), float(((err - move) / size).max(initial=-np.inf))


def assert_rows(t, z, iters, what, cap=None, allowed=0, floor=None, max_ratio=None):
    """the assertion of the truth tests: every settled pixel has the exact index (but for `allowed` of them, a recorded
    finding), and where it has, z is within move + floor max(|z|, 1) of the exact z, per component (floor: Z_FLOOR unless given;
    max_ratio: also |z - z_exact| <= max_ratio move where move > 0)"""
    floor = Z_FLOOR if floor is None else floor
    differ, ratio, excess = compare(t, z, iters, cap)
    assert differ <= allowed, "%s: %d settled pixels off the exact escape index (allowed: %d)" % (what, differ, allowed)
    assert excess <= floor, "%s: z is %.3g max(|z|, 1) past the exact z's own movement (floor %.3g)" % (what, excess, floor)
    assert max_ratio is None or ratio <= max_ratio, "%s: z is %.3g move off the exact z (allowed: %.3g)" % (what, ratio, max_ratio)
    return differ, ratio, excess
