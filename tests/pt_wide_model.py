"""The model of WIDE PT (include/fractal_hip.h, fr_precision: "WIDE PT"), written from the definition alone.

Reference orbits come from plain Python integers: `>>` is the floor of the definition and Fraction(I, 1 << F) -> float is its
rounding (correct, ties to even), so nothing here shares code or method with the library's limb arithmetic.  The pixel, state
and extend loops are tests/pt_wide_model.c (PT's step sequence over orbit arrays that are passed in; Python 3.10 has no fma),
compiled on first use into a fresh temporary directory: gcc -O2 -ffp-contract=off -fno-fast-math -shared.

Also here: the three centres of the tests, computed with mpmath at 1200 bits and floored, and the views built on them."""
import atexit
import ctypes as C
import functools
import math
import os
import shutil
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pt_wide_model.c")
ON_K = 0x80000000
MAX_WORDS = 16

# ---- wide numbers on Python integers ----------------------------------------------------------------------------


def frac_bits(n):
    return 64 * n - 8


def to_words(i, n):
    """the integer I as n little-endian uint64 words, two's complement"""
    assert -(1 << (64 * n - 1)) <= i < (1 << (64 * n - 1))
    return np.array([(i >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(n)], dtype=np.uint64)


def from_words(w):
    n = len(w)
    i = sum(int(x) << (64 * k) for k, x in enumerate(w))
    return i - (1 << (64 * n)) if i >> (64 * n - 1) else i


def floor_scaled(value, n):
    """floor(value 2^F) for an exact value: int, float, Fraction, or an mpmath mpf (through its exact binary value)"""
    if hasattr(value, "_mpf_"):
        sign, man, exp, _ = value._mpf_  # (-1)^sign man 2^exp, exactly
        value = Fraction(-int(man) if sign else int(man)) * Fraction(2) ** int(exp)
    return math.floor(Fraction(value) * (1 << frac_bits(n)))


def to_f64(i, n):
    """the f64 nearest to I / 2^F, ties to even"""
    return float(Fraction(i, 1 << frac_bits(n)))


def split(i, n):
    """(hi, lo): the f64 nearest to the value, and the f64 nearest to the rest"""
    v = Fraction(i, 1 << frac_bits(n))
    hi = float(v)
    return hi, float(v - Fraction(hi))


# ---- reference orbits ----------------------------------------------------------------------------------------------


def orbit(cre, cim, n, algo, iterations, julia_set=(0.0, 0.0), which=0):
    """Orbit `which` (0: R or V, 1: K) of the view centred on the integers (cre, cim) -> (float64 [entries, 2] of the stored
    entries, ended by escape, the last entry as integers)"""
    f = frac_bits(n)
    julia = algo == 2
    kmin = 1 if julia else 2
    kmax = max(iterations, 1) if julia else iterations + 1
    if julia:
        are, aim = floor_scaled(julia_set[0], n), floor_scaled(julia_set[1], n)
    else:
        are, aim = cre, cim
    zr, zi = (cre, cim) if julia and which == 0 else (0, 0)
    out = []
    k = 0
    while True:
        re, im = to_f64(zr, n), to_f64(zi, n)
        out.append((re, im))
        ended = k >= kmin and re * re + im * im > 4.0
        if ended or k == kmax:
            break
        if not julia and k == 0:
            zr, zi = cre, cim
        else:
            assert abs(zr) < (16 << f) and abs(zi) < (16 << f), "the overflow argument of the definition"
            zr, zi = ((zr * zr) >> f) - ((zi * zi) >> f) + are, ((2 * zr * zi) >> f) + aim
        k += 1
    return np.array(out, dtype=np.float64), ended, (zr, zi)


# ---- the pixel loop ------------------------------------------------------------------------------------------------


class _View(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("julia", C.c_int),
                ("limit", C.c_double), ("scale_re", C.c_double), ("scale_im", C.c_double)]


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler for tests/pt_wide_model.c")
    d = tempfile.mkdtemp(prefix="pt_wide_model_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libpt_wide_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", so, SRC, "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.ptwm_rows.restype = None
    L.ptwm_rows.argtypes = [C.POINTER(_View), C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32,
                            C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.POINTER(C.c_uint64)]
    _lib = L
    return L


class Orbits:
    """the orbits of (cfg, centre) at cfg's cap: x (R or V) and k (K; Mandelbrot: x again), each (entries, ended, tail)"""

    def __init__(self, cfg, cre, cim, n):
        js = (cfg.julia_set.re, cfg.julia_set.im)
        self.julia = cfg.algo == 2
        self.x = orbit(cre, cim, n, cfg.algo, cfg.iterations, js, 0)
        self.k = orbit(cre, cim, n, cfg.algo, cfg.iterations, js, 1) if self.julia else self.x


def _run(cfg, orbits, y0, y1, from_iterations, fresh, rule, state):
    y1 = cfg.height if y1 is None else y1
    v = _View(cfg.width, cfg.height, cfg.iterations, int(orbits.julia), cfg.limit, cfg.scale.re, cfg.scale.im)
    z, it, dz, m = state
    reb = np.zeros(it.shape, dtype=np.uint32)
    viol = C.c_uint64(0)
    (xa, xe, _), (ka, ke, _) = orbits.x, orbits.k
    lib().ptwm_rows(C.byref(v), xa.ctypes.data, len(xa) - 1, int(xe), ka.ctypes.data, len(ka) - 1, int(ke), y0, y1,
                    from_iterations, int(fresh), rule, z.ctypes.data, it.ctypes.data, dz.ctypes.data, m.ctypes.data,
                    reb.ctypes.data, C.byref(viol))
    assert viol.value == 0, "a step began with m >= last of the orbit followed"
    return (z, it, dz, m), reb


def state_rows(cfg, orbits, y0=0, y1=None, rule=0):
    """the state after cfg.iterations steps: ((z float64 [rows, width, 2], iters uint32 [rows, width], dz, m), rebases per
    pixel).  rule 0: the state rule; rule 1: PT's own — its z and iters are what plain WIDE PT gives."""
    y1 = cfg.height if y1 is None else y1
    shape = (y1 - y0, cfg.width)
    st = (np.empty(shape + (2,), dtype=np.float64), np.empty(shape, dtype=np.uint32), np.empty(shape + (2,), dtype=np.float64),
          np.empty(shape, dtype=np.uint32))
    return _run(cfg, orbits, y0, y1, 0, True, rule, st)


def continue_rows(cfg, orbits, state, from_iterations, y0=0, y1=None):
    """`state` at the cap from_iterations continued to cfg.iterations on `orbits` (those of cfg's cap) -> the new state (copies)"""
    st = tuple(np.array(a, order="C") for a in state)
    return _run(cfg, orbits, y0, y1, from_iterations, False, 0, st)[0]


def same_state(a, b):
    """all four arrays equal, the doubles as bits"""
    return (np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
            and np.array_equal(np.ascontiguousarray(a[0]).view(np.uint64), np.ascontiguousarray(b[0]).view(np.uint64))
            and np.array_equal(np.ascontiguousarray(a[2]).view(np.uint64), np.ascontiguousarray(b[2]).view(np.uint64)))


# ---- the centres of the tests, at 1200 bits ---------------------------------------------------------------------------

PREC = 1200
JULIA_SET = (-0.8, 0.156)


def _newton(f, df, x):
    import mpmath

    for _ in range(40):  # quadratic: 12 steps from 8 digits reach 1200 bits; the rest are fixed points
        x = x - f(x) / df(x)
    assert abs(f(x)) < mpmath.mpf(2) ** (20 - PREC)
    return x


@functools.lru_cache(maxsize=None)
def centre(name):
    """(re, im) as mpmath numbers of 1200 bits:
    M  the Misiurewicz point, root of c^3 + 2c^2 + 2c + 2 near -0.22815549 + 1.11514251i;
    N  the period-3 nucleus, the real root of c^3 + 2c^2 + c + 1 near -1.75487767;
    J  for julia_set = -0.8 + 0.156i (its f64 values), the repelling fixed point (1 + sqrt(1 - 4J)) / 2."""
    import mpmath

    with mpmath.workprec(PREC):
        if name == "M":
            c = _newton(lambda c: ((c + 2) * c + 2) * c + 2, lambda c: (3 * c + 4) * c + 2, mpmath.mpc("-0.22815549", "1.11514251"))
        elif name == "N":
            c = mpmath.mpc(_newton(lambda c: ((c + 2) * c + 1) * c + 1, lambda c: (3 * c + 4) * c + 1, mpmath.mpf("-1.75487767")), 0)
        elif name == "J":
            j = mpmath.mpc(mpmath.mpf(JULIA_SET[0]), mpmath.mpf(JULIA_SET[1]))
            c = (1 + mpmath.sqrt(1 - 4 * j)) / 2
            assert abs(c * c + j - c) < mpmath.mpf(2) ** (20 - PREC) and abs(2 * c) > 1
        else:
            raise KeyError(name)
        return +c.real, +c.imag


def centre_ints(name, n):
    """the centre floored to n words: (Cre, Cim) as integers"""
    re, im = centre(name)
    return floor_scaled(re, n), floor_scaled(im, n)


def decimal_text(value, digits):
    """an mpmath number as a plain decimal string of `digits` fractional digits, truncated toward zero"""
    import mpmath

    with mpmath.workprec(PREC + 4 * digits):
        q = int(mpmath.floor(abs(value) * mpmath.mpf(10) ** digits))
    s = str(q).rjust(digits + 1, "0")
    return ("-" if value < 0 else "") + s[:-digits] + "." + s[-digits:]


def view(cfg, name, scale_log2, width, height, iterations):
    """fill cfg (a default Config of the library or of the oracle) with the view of the tests centred on `name`; limit = 2"""
    cfg.algo = 2 if name == "J" else 0
    cfg.width, cfg.height, cfg.iterations = width, height, iterations
    cfg.limit = 2.0
    cfg.scale.re = cfg.scale.im = math.ldexp(1.0, scale_log2)
    cfg.pos.re, cfg.pos.im = 123.0, -77.0  # not read
    if name == "J":
        cfg.julia_set.re, cfg.julia_set.im = JULIA_SET
    return cfg


def words_for_scale(scale):
    """the smallest n of the domain rule F >= e + 64, max |scale| = f 2^e with 0.5 <= f < 1"""
    e = math.frexp(abs(scale))[1]
    return max(2, -(-(e + 64 + 8) // 64))
