"""The exact orbit derivatives that DE ON SCALED PT (include/fractal_hip.h, "DE ON SCALED PT") is checked against.

Beside tests/deep_truth.py's integer orbit z <- z^2 + c (fixed point with P fraction bits, `>>` the floor, on deep_truth.View's
exact points) runs d' = 2 z d + b0 on Python integers, d0 = 1, b0 = 1 for Mandelbrot and 0 for Julia, from the z before the
step; it returns what DE's definition returns: the derivative of the returned position.  The fixture records, per pixel, the
escape index and u = d 2^-e as the f64 nearest to the exact value (+-inf where that is past f64, which only capped pixels reach),
e the exponent of the view's scale: the scaled derivative the road carries.  It shares nothing with the library or with the C
models.

P = 2e + 320 as in deep_truth, and everything is computed a second time at P + 320: tests/golden/make_de_scaled_truth.py writes
nothing unless both give the same iters and u on every pixel of every view.

The exact distance of a pixel is DE's distance (tests/de_model.py) over deep_truth's z (the f64 nearest to the exact z), the
index and this u, on the scaled view: the f64 evaluation of |z| ln|z| / |u| is a few units in the last place off, far below every
figure here.  COMPARED PIXELS of a view and a model run: settled in deep_truth's fixture, the model's index equal to the exact
one, escaped, exact D >= 2^-10 pixels.  At least half of every image has to be compared."""
import math
import os
from fractions import Fraction

import numpy as np

import deep_truth as T

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "de_scaled_truth.npz")
VIEWS = T.PAST + T.WIDE_DOMAIN
FIELDS = ("iters", "u")
MIN_D = 2.0 ** -10
MIN_COMPARED = 0.5

# The worst |D_model - D_exact| / D_exact over the compared pixels of all seven views that tests/de_scaled_model.c gave on the
# CPU, per bits (tests/test_de_scaled_cpu.py prints the figures per view with -s and checks these constants), and the tolerance:
# 4 times that, rounded up to a power of two.  DESIGN.md 3.24 carries the table.
D_ERROR_MEASURED = {-1: 1.75625e-10, 40: 6.40976e-10, 53: 2.89599e-10}  # on MINI_861, J_900 and MINI_861
D_TOLERANCE = {-1: 2.0 ** -30, 40: 2.0 ** -28, 53: 2.0 ** -29}


def tolerance_for(measured):
    """4 x measured, rounded up to a power of two"""
    return 2.0 ** math.ceil(math.log2(4.0 * measured))


def _nearest(num, shift):
    """num / 2^shift as the nearest f64, +-inf past the range"""
    try:
        return float(Fraction(num, 1 << shift))
    except OverflowError:
        return float("inf") if num > 0 else float("-inf")


def _orbit(zr, zi, add, P, lim, cap, b0):
    """deep_truth._orbit with the derivative beside it -> (index, (d.re, d.im) as integers over 2^P)"""
    ar, ai = (zr, zi) if add is None else add
    dr, di = 1 << P, 0
    rr, ii = zr * zr, zi * zi
    index = cap
    for i in range(cap):
        dr, di = ((zr * dr - zi * di) >> (P - 1)) + b0, (zr * di + zi * dr) >> (P - 1)  # from the z before the step
        zr, zi = (rr >> P) - (ii >> P) + ar, ((zr * zi) >> (P - 1)) + ai
        rr, ii = zr * zr, zi * zi
        if rr + ii > lim:
            index = i
            break
    return index, (dr, di)


def pixel(name, x, y, extra=0):
    """-> (iters, (u.re, u.im) as f64) of pixel (x, y) of a deep_truth view at P + extra fraction bits"""
    v = T.view(name)
    P = v.P + extra
    ore, oim = v.offset(x, y)
    pre, pim = v.fixed(v.centre[0] + ore, P), v.fixed(v.centre[1] + oim, P)
    lim = v.fixed(Fraction(v.limit) ** 2, 2 * P)
    add = (v.fixed(v.julia_set[0], P), v.fixed(v.julia_set[1], P)) if v.julia else None
    it, (dr, di) = _orbit(pre, pim, add, P, lim, v.cap, 0 if v.julia else 1 << P)
    return it, (_nearest(dr, P + v.e), _nearest(di, P + v.e))


def _pixel_job(job):
    return pixel(*job)


def view_truth(name, extra=0, pool=None):
    """every pixel of a view -> {"iters": uint32 [h, w], "u": float64 [h, w, 2]}"""
    v = T.view(name)
    jobs = [(name, x, y, extra) for y in range(v.height) for x in range(v.width)]
    res = pool.map(_pixel_job, jobs, chunksize=4) if pool is not None else list(map(_pixel_job, jobs))
    return {"iters": np.array([r[0] for r in res], dtype=np.uint32).reshape(v.shape),
            "u": np.array([r[1] for r in res], dtype=np.float64).reshape(v.shape + (2,))}


def load(name):
    """the fixture's record of a view, read-only, with "precision" = (P, P + EXTRA)"""
    with np.load(FIXTURE) as f:
        t = {k: f["%s/%s" % (name, k)] for k in FIELDS + ("precision",)}
    for a in t.values():
        a.setflags(write=False)
    return t


def compare(name, cfg_v, distance, z, iters, der):
    """One model or kernel run of a view against the exact distance.  cfg_v: the run's scaled view; distance: tests/de_model.py's
    distance(cfg, z, iters, der) -> (compared pixels, all pixels, the worst |D - D_exact| / D_exact over the compared ones)"""
    t, tu = T.load(name), load(name)
    assert np.array_equal(t["iters"], tu["iters"]), "the two fixtures are of one orbit"
    exact = distance(cfg_v, t["z"], tu["iters"], tu["u"])
    got = distance(cfg_v, z, iters, der)
    escaped = tu["iters"] < cfg_v.iterations
    compared = t["settled"] & (np.asarray(iters) == tu["iters"]) & escaped & (exact >= MIN_D) & np.isfinite(exact)
    err = np.abs(got - exact)[compared] / exact[compared]
    return int(compared.sum()), int(compared.size), float(err.max(initial=0.0))
