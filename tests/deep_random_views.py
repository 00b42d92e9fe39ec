"""Generated and edge views of the wide-centre deep roads (WIDE PT, BLA-PT, SCALED PT, their state and extend forms, DE on each),
shared by tests/test_deep_random_cpu.py (the models alone: is the generated set worth running, and are the models right on it)
and tests/test_gpu_deep_random.py (the kernels against the models on the same views).  No device and no library: numpy's seeded
generator, Python integers, and tests/deep_truth.py's View for everything exact.

A view is a record with deep_truth.Spec's fields and three more: `julia_set` (the constant of a Julia view on a centre that is
not J; None otherwise), `bits` (-1, 0 or 24 .. 53, as SCALED PT takes them) and `look` (the colour fields).  draw(rng) draws:
  centre  M, N, J or MINI (pt_scaled_model.centre_ints), moved by (a + b i) 2^-k with |a|, |b| <= 4 and k in e .. e + 5 — the
          special point lies from mid-image to a few image widths outside — or not moved at all (one draw in five); J is a Julia
          view with pt_wide_model.JULIA_SET; one draw in ten is a Julia view on M or N with a constant of JULIA_CONSTANTS, and
          one in five a Julia view on "F", the repelling fixed point of a constant of FILLED_CONSTANTS;
  scale   f 2^e with f uniform in (0.5, 1), e in 60 .. 951 (views(seed) takes the first view of a seed from 60 .. 440, the
          second from 441 .. 951 and the third from the whole range; with MINI three draws in four past 2^440 lie in 855 .. 866,
          where the minibrot fills the image); the other axis is the first times one of RATIOS; either sign, either axis larger;
  n       pt_wide_model.words_for_scale half of the time, otherwise anything from there to 16;
  size    1 .. 48 by 1 .. 40;  cap from CAPS, one below 300 in a third of the draws;  limit from LIMITS;  bits from BITS;
  look    smooth, inside, exposure, stable_limit and the two colours as test_gpu_deep_edges.random_config draws them.
EDGES are fixed views, each just inside a domain rule of include/fractal_hip.h."""
import math
from collections import namedtuple

import numpy as np

import deep_truth as T
import pt_wide_model as W

SEEDS = range(16)
BASE_SEED = 9500
PER_SEED = 3
E_MIN, E_MAX, E_WIDE = 60, 951, 440
RATIOS = (1.0, 0.7, 0.53, 1.0 / 3.0, 2.0 ** -5)
CAPS = (0, 1, 2, 3, 17, 300, 1000, 3000, 6000)
LIMITS = (2.0, 4.0, 1000.5, 65536.0, 2.0 ** 20)
BITS = (-1, 0, 24, 40, 53)
JULIA_CONSTANTS = ((0.0, 1.0), (-1.0, 0.0), (0.0, 0.0), (1e-310, -3e-320), (1e-200, 1e-170), (0.285, 0.01))
# beyond the four centres: "F", the repelling fixed point (1 + sqrt(1 - 4c)) / 2 of a constant whose filled Julia set has an
# interior that reaches the fixed point (the basilica, a rabbit, the disc).  A view there shows capped pixels beside escaping ones
# at every depth, which of the four only MINI does, and only around 2^861.
FILLED_CONSTANTS = ((-1.0, 0.0), (-0.12, 0.75), (0.0, 0.0))
RESOLVED_CAP = 300  # the conditions of tests/test_deep_random_cpu.py count the views with at least this cap
RESOLVED_INDICES = 4

Look = namedtuple("Look", "smooth inside exposure stable_limit primary secondary")
Draw = namedtuple("Draw", T.Spec._fields + ("julia_set", "bits", "look"))
PLAIN = Look(1, 1, 5.0, 2.0, (255, 255, 255), (0, 0, 0))


def _look(rng):
    stable = float(rng.choice([2.0, 0.5, 0.0, -1.0, 100.0]))
    exposure = float(rng.choice([5.0, 2.0, 0.3, 50.0, -1.0]))
    inside, smooth = int(rng.random() < 0.7), int(rng.random() < 0.7)
    primary = tuple(int(v) for v in rng.integers(0, 256, 3))
    secondary = tuple(int(v) for v in rng.integers(0, 256, 3))
    return Look(smooth, inside, exposure, stable, primary, secondary)


def draw(rng, e_range=(E_MIN, E_MAX)):
    """one view from a numpy Generator; every number in the record is a Python int or float"""
    r = rng.random()
    centre, constant = "M", None
    if r < 0.22:
        centre = "M"
    elif r < 0.44:
        centre = "J"
    elif r < 0.64:
        centre = "MINI"
    elif r < 0.68:
        centre = "N"
    elif r < 0.90:
        centre, constant = "F", FILLED_CONSTANTS[int(rng.integers(len(FILLED_CONSTANTS)))]
    else:
        centre = "M" if rng.random() < 0.5 else "N"
        if rng.random() < 0.25:
            constant = (float(rng.uniform(-1.2, 0.6)), float(rng.uniform(-0.8, 0.8)))
        else:
            constant = JULIA_CONSTANTS[int(rng.integers(len(JULIA_CONSTANTS)))]
    e = int(rng.integers(e_range[0], e_range[1] + 1))
    if centre == "MINI" and e > E_WIDE and rng.random() < 0.75:
        e = int(rng.integers(855, 867))
    f = 0.5
    while f == 0.5:  # never a power of two
        f = 0.5 + 0.5 * float(rng.random())
    first = math.ldexp(f, e)
    other = first * float(RATIOS[int(rng.integers(len(RATIOS)))])
    first = math.copysign(first, 1.0 if rng.random() < 0.5 else -1.0)
    other = math.copysign(other, 1.0 if rng.random() < 0.5 else -1.0)
    scale = (first, other) if rng.random() < 0.5 else (other, first)
    least = W.words_for_scale(math.ldexp(f, e))
    n = least if rng.random() < 0.5 else int(rng.integers(least, W.MAX_WORDS + 1))
    if rng.random() < 0.2:
        shift = (0, 0, 0)
    else:
        a, b = 0, 0
        while a == 0 and b == 0:
            a, b = int(rng.integers(-4, 5)), int(rng.integers(-4, 5))
        shift = (a, b, e + int(rng.integers(0, 6)))
    width, height = int(rng.integers(1, 49)), int(rng.integers(1, 41))
    small = [c for c in CAPS if c < RESOLVED_CAP]
    large = [c for c in CAPS if c >= RESOLVED_CAP]
    cap = int(small[int(rng.integers(len(small)))]) if rng.random() < 1.0 / 3.0 else int(large[int(rng.integers(len(large)))])
    limit = float(LIMITS[int(rng.integers(len(LIMITS)))])
    bits = int(BITS[int(rng.integers(len(BITS)))])
    return Draw("wide", centre, n, shift, scale, limit, width, height, cap, constant, bits, _look(rng))


class Generated:
    """a drawn or an edge view: the record, deep_truth's exact View of it, the centre's integers and words, e, the roads whose
    domain it lies in, and what the models and the calls need"""

    def __init__(self, record, label):
        self.draw, self.label = record, label
        self.v = v = T.view(record)
        self.n, self.ints, self.words, self.e, self.julia = v.n, v.ints, v.words, v.e, v.julia
        self.shape, self.cap = v.shape, v.cap
        self.bits = record.bits
        self.table_bits = record.bits if record.bits > 0 else 40  # what the models take for a table run (0 is the default, 40)
        self.call_bits = max(record.bits, 0)  # what a table call of the library takes where the view's bits say "no table"
        self.wide = v.common  # WIDE PT's, BLA-PT's and their DE's domain; SCALED PT's holds for every view here
        self.roads = ("wide", "bla", "scaled") if self.wide else ("scaled",)
        lo, hi = sorted(abs(s) for s in record.scale)
        assert E_MIN <= self.e <= 952 and lo >= 2.0 ** -32 * hi and record.limit <= 2.0 ** 20 and 2 <= self.n <= W.MAX_WORDS
        assert W.frac_bits(self.n) >= self.e + 64

    def cfg(self, new_config, cap=None):
        """a Config of the library or of the oracle filled with the view and its look, at its cap or at another"""
        return self.dress(self.v.fill(new_config(), cap))

    def dress(self, cfg):
        """set the view's look on a config that deep_truth.View.fill has filled"""
        look = self.draw.look
        cfg.smooth, cfg.inside, cfg.exposure, cfg.stable_limit = look.smooth, look.inside, look.exposure, look.stable_limit
        cfg.primary_color.r, cfg.primary_color.g, cfg.primary_color.b = look.primary
        cfg.secondary_color.r, cfg.secondary_color.g, cfg.secondary_color.b = look.secondary
        return cfg

    def orbits(self, cfg):
        """pt_wide_model's orbits of (cfg, centre): Python integers"""
        return W.Orbits(cfg, *self.ints, self.n)

    def describe(self, cfg):
        """everything that replays the view: the config's bytes, n and the centre's words, in hex"""
        return "%s: config %s, n %d, re %s, im %s, bits %d" % (
            self.label, bytes(cfg).hex(), self.n, " ".join("%016x" % int(w) for w in self.words[0]),
            " ".join("%016x" % int(w) for w in self.words[1]), self.bits)


def views(seed):
    """the views of one seed, the same on every machine: inside 2^440, past it, anywhere"""
    rng = np.random.default_rng(BASE_SEED + seed)
    ranges = ((E_MIN, E_WIDE), (E_WIDE + 1, E_MAX), (E_MIN, E_MAX))
    return [Generated(draw(rng, ranges[k % 3]), "seed %d view %d" % (seed, k)) for k in range(PER_SEED)]


def pixels(seed, k, view):
    """the sampled pixels of view k of a seed: eight drawn from the seed (with repeats on a small image) plus the centre pixel"""
    rng = np.random.default_rng([BASE_SEED + seed, k])
    h, w = view.shape
    out = [(int(rng.integers(w)), int(rng.integers(h))) for _ in range(8)] + [(w // 2, h // 2)]
    return list(dict.fromkeys(out))


# ---- the edge views -------------------------------------------------------------------------------------------------------------


def _edge(centre, n, shift, scale, limit, width, height, cap, bits=40, julia_set=None):
    return Draw("wide", centre, n, shift, scale, limit, width, height, cap, julia_set, bits, PLAIN)


BELOW_2_440 = math.nextafter(2.0 ** 440, 0.0)
EDGES = {
    # max |scale| the largest f64 below 2^440: inside WIDE PT's domain, run on the wide and the scaled roads
    "below_2^440": _edge("M", 9, (3, -2, 443), (BELOW_2_440, -0.7 * BELOW_2_440), 65536.0, 33, 31, 6000, 53),
    # e = 951 with n = 16: F = 1016 >= 1015
    "e_951": _edge("M", 16, (-2, 5, 953), (math.ldexp(0.81, 951), math.ldexp(0.77, 951)), 65536.0, 31, 33, 6000, 0),
    # min |scale| = 2^-32 max |scale| exactly
    "ratio_2^-32": _edge("M", 16, (1, 1, 702), (math.ldexp(0.6, 700), -math.ldexp(0.6, 668)), 4.0, 17, 1, 3000, 40),
    # F = e + 64 exactly: n = 8 at e = 440 (F = 504), and n = 3 at e = 120 (F = 184)
    "F_e+64_n8": _edge("J", 8, (3, 2, 442), (math.ldexp(0.93, 440), math.ldexp(-0.93, 440)), 65536.0, 1, 17, 3000, 24),
    "F_e+64_n3": _edge("M", 3, (-1, 2, 122), (math.ldexp(-0.55, 120), math.ldexp(0.55 * 0.53, 120)), 2.0, 17, 1, 1000, 0),
    # spare words: n = 16 at e = 70
    "n16_e70": _edge("M", 16, (2, 3, 72), (math.ldexp(0.75, 70), math.ldexp(0.75, 70)), 1000.5, 31, 33, 1000, 40),
    # limit = 2^20, past 2^440 and inside it
    "limit_2^20": _edge("MINI", 16, (1, -1, 864), (math.ldexp(0.9, 861), math.ldexp(0.9, 861)), 2.0 ** 20, 33, 31, 3204, 53),
    "limit_2^20_J": _edge("J", 6, (0, 0, 0), (math.ldexp(0.66, 300), math.ldexp(0.66 / 3, 300)), 2.0 ** 20, 33, 31, 3000, 0),
    # one lane
    "1x1": _edge("M", 6, (1, 0, 303), (math.ldexp(0.7, 300), math.ldexp(0.7, 300)), 65536.0, 1, 1, 3000, 40),
    # a Mandelbrot centre outside the set: M + (1 + i) / 2, whose reference orbit ends by escape within a few entries
    "outside": _edge("M", 4, (1, 1, 1), (math.ldexp(0.9, 100), math.ldexp(-0.63, 100)), 65536.0, 17, 17, 3000, 40),
    # the special point exactly on pixel (5, 3) of 24 x 16: its offset is (5/16 - 3/4, 3/16 - 1/2) 2^-600 = -(7 + 5i) 2^-604
    "on_a_pixel": _edge("M", 12, (7, 5, 604), (2.0 ** 600, 2.0 ** 600), 65536.0, 24, 16, 6000, 40),
    "on_a_pixel_J": _edge("J", 6, (7, 5, 304), (2.0 ** 300, 2.0 ** 300), 2.0, 24, 16, 3000, 53),
}


def edge(name):
    return Generated(EDGES[name], "edge view " + name)


# ---- the dd-centre views: test_gpu_deep_edges.random_config's, for BLA-PT and DE ---------------------------------------------------

DD_BASE_SEED = 9700
DD_PER_SEED = 3
F64_MAX_SCALE = 1e13  # past it an f64 pixel spacing near a centre of size 1 is below a few hundred ulps: the F64 road is not run


def dd_domain(cfg, call):
    """whether a dd-centre view of random_config (inside PT's domain as drawn) lies in the domain of a call of the GPU file:
    "bla" fr_escape_rows_pt_bla with pos_lo (PT's domain), "de_pt" fr_escape_rows_de and fr_escape_rows_de_pt_bla on
    FR_PRECISION_PT (DE's limit <= 2^20), "de_f64" fr_escape_rows_de on FR_PRECISION_F64 (the same, where the scale permits)"""
    if call == "bla":
        return True
    if call == "de_pt":
        return cfg.limit <= 2.0 ** 20
    if call == "de_f64":
        return cfg.limit <= 2.0 ** 20 and max(abs(cfg.scale.re), abs(cfg.scale.im)) <= F64_MAX_SCALE
    raise KeyError(call)
