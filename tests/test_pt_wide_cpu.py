"""WIDE PT without a device (include/fractal_hip.h, fr_precision: "WIDE PT"):
  - the host helpers fr_wide_from_double / _add_double / _to_double / _from_decimal against Python integers and Fractions:
    negatives (floor toward -inf), carries across every word boundary, n = 2 and n = 16, ties of the rounding, decimal
    strings of 5 and of 300 digits, every refusal (and w left alone by it);
  - fr_debug_reference_orbit_wide against tests/pt_wide_model.py bit for bit: the Misiurewicz centre at n = 5 and n = 9, the
    period-3 nucleus cut by the cap at 602 entries, the Julia fixed point's V and K;
  - the domain refusals, each with a message, before any device work (on a box without a device anything that touched one
    would answer FR_ERR_NO_DEVICE instead), and the no-ops that need no device;
  - the header states the definition; the Python mirror sizes n by the domain rule and refuses what it must."""
import ctypes as C
import math
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest

import pt_wide_model as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


@pytest.fixture(scope="module")
def fr():
    import __graft_entry__ as ge

    ge.build()
    import fractal_renderer_amd

    return fractal_renderer_amd


@pytest.fixture(scope="module")
def lib(fr):
    from fractal_renderer_amd import _native

    return _native.load()


def message(lib):
    return lib.fr_last_error().decode()


def from_double(lib, v, n):
    w = np.full(n, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = lib.fr_wide_from_double(v, w.ctypes.data, n)
    return rc, w


def to_double(lib, i, n):
    w = W.to_words(i, n)
    hi, lo = C.c_double(7.0), C.c_double(7.0)
    assert lib.fr_wide_to_double(w.ctypes.data, n, C.byref(hi), C.byref(lo)) == 0, message(lib)
    return hi.value, lo.value


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


# ---- helpers ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [2, 3, 16])
def test_from_double_is_the_floor(lib, n):
    f = W.frac_bits(n)
    rng = random.Random(n)
    values = [0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 0.1, -0.1, -0.8, 0.156, math.ldexp(1.0, -f), -math.ldexp(1.0, -f),
              math.ldexp(1.0, -f - 1), -math.ldexp(1.0, -f - 1), -math.ldexp(1.5, -f), math.ldexp(1.75, -f + 3), -5e-324, 5e-324,
              -1e-300, math.ldexp(-1.0 - 2.0 ** -52, -f + 20), math.nextafter(2.0, 0.0), -math.nextafter(2.0, 0.0)]
    values += [rng.uniform(-2, 2) * 2.0 ** -rng.randrange(0, f + 60) for _ in range(200)]
    for v in values:
        rc, w = from_double(lib, v, n)
        assert rc == 0, (v, message(lib))
        want = math.floor(Fraction(v) * (1 << f))
        assert W.from_words(w) == want, (v, n)
    # a negative value below the last bit floors to -1: every word all ones
    rc, w = from_double(lib, -1e-320, n)
    assert rc == 0 and all(int(x) == 0xFFFFFFFFFFFFFFFF for x in w)


@pytest.mark.parametrize("n", [2, 5, 16])
def test_add_double_carries_across_every_word_boundary(lib, n):
    f = W.frac_bits(n)
    ulp = math.ldexp(1.0, -f)
    for k in range(1, n):
        for sign in (1, -1):
            i = sign * ((1 << (64 * k)) - 1) if k < n - 1 or sign > 0 else -((1 << (64 * k)) - 1)
            if abs(i) > (2 << f):
                continue
            w = W.to_words(i, n)
            assert lib.fr_wide_add_double(w.ctypes.data, n, sign * ulp) == 0, message(lib)
            assert W.from_words(w) == i + sign, (n, k, sign)  # the carry (borrow) runs through boundary k
            assert lib.fr_wide_add_double(w.ctypes.data, n, -sign * ulp) == 0
            assert W.from_words(w) == i
    # the carry runs through all of the words below the top one at once
    i = (1 << (64 * (n - 1))) - 1
    w = W.to_words(i, n)
    assert lib.fr_wide_add_double(w.ctypes.data, n, ulp) == 0 and W.from_words(w) == i + 1
    w = W.to_words(-1, n)
    assert lib.fr_wide_add_double(w.ctypes.data, n, ulp) == 0 and W.from_words(w) == 0
    # I += floor(delta 2^F), toward -inf for a negative delta
    rng = random.Random(100 + n)
    i = 0
    w = W.to_words(0, n)
    for _ in range(300):
        d = rng.uniform(-1, 1) * 2.0 ** -rng.randrange(0, f + 10)
        step = math.floor(Fraction(d) * (1 << f))
        rc = lib.fr_wide_add_double(w.ctypes.data, n, d)
        if abs(i + step) > (2 << f):
            assert rc == INVALID
        else:
            assert rc == 0
            i += step
        assert W.from_words(w) == i
    w = W.to_words(5, n)
    assert lib.fr_wide_add_double(w.ctypes.data, n, -1.5 * ulp) == 0 and W.from_words(w) == 3


@pytest.mark.parametrize("n", [2, 4, 16])
def test_to_double_rounds_to_nearest_even_and_splits(lib, n):
    f = W.frac_bits(n)
    rng = random.Random(200 + n)
    cases = [0, 1, -1, 3, (2 << f), -(2 << f), (1 << 53) - 1, (1 << 53) + 1, -((1 << 53) + 1)]
    for s in (0, 1, 5, 63, 64, 65, f - 60):
        for m in ((1 << 52), (1 << 52) + 1, (1 << 53) - 2, (1 << 53) - 1, (1 << 52) + 12345):
            tie = ((2 * m + 1) << s)  # exactly between m and m + 1 (times 2^(s + 1))
            for i in (tie, -tie, tie + 1, tie - 1, -tie - 1, -tie + 1, (tie << 3) + 1 if s + 3 + 54 < f else tie):
                if abs(i) <= (2 << f):
                    cases.append(i)
    cases += [rng.randrange(-(2 << f), (2 << f) + 1) >> rng.randrange(0, f) for _ in range(300)]
    ties = 0
    for i in cases:
        hi, lo = to_double(lib, i, n)
        whi, wlo = W.split(i, n)
        assert same_bits([hi, lo], [whi, wlo]), (n, i)
        v = Fraction(i, 1 << f)
        down, up = math.nextafter(hi, -math.inf), math.nextafter(hi, math.inf)
        if v != Fraction(hi) and (abs(v - Fraction(hi)) == abs(v - Fraction(down)) or abs(v - Fraction(hi)) == abs(v - Fraction(up))):
            ties += 1
            assert int(np.float64(hi).view(np.uint64)) & 1 == 0, "a tie goes to the even significand"
        assert abs(Fraction(lo)) <= Fraction(math.ulp(hi)) / 2, "lo is what hi leaves, at most half an ulp of it"
    assert ties >= 40
    # lo may be NULL
    w = W.to_words(12345, n)
    hi = C.c_double(0.0)
    assert lib.fr_wide_to_double(w.ctypes.data, n, C.byref(hi), None) == 0 and hi.value == W.to_f64(12345, n)


def decimal(lib, text, n):
    w = np.full(n, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = lib.fr_wide_from_decimal(text.encode() if text is not None else None, w.ctypes.data, n)
    return rc, w


@pytest.mark.parametrize("n", [2, 9, 16])
def test_from_decimal_is_the_floor_of_the_exact_value(lib, n):
    f = W.frac_bits(n)
    m_re, m_im = W.centre("M")
    n_re, _ = W.centre("N")
    texts = ["-1.75487", "0.15600", W.decimal_text(n_re, 300), W.decimal_text(m_re, 300), W.decimal_text(m_im, 300),
             "0", "-0", "+0.0", "2", "-2", "2.000", "-2.0e0", "1e-3", "-1e-3", "+.5", "5.e-1", "-12.5e-1", "0.2E+1", "20e-1",
             "1e-400", "-1e-400", "-0." + "0" * 400 + "1", "0." + "3" * 700, "-0." + "6" * 700, "0.000e9999", "1.9999999999999999999999",
             "123456789e-9", "00001.5"]
    assert len(W.decimal_text(n_re, 300)) == 303 and len("-1.75487") - 2 == 6
    for t in texts:
        rc, w = decimal(lib, t, n)
        assert rc == 0, (t, message(lib))
        mant, _, ex = t.lower().partition("e")
        exact = Fraction(mant if mant[-1] != "." else mant + "0") * Fraction(10) ** int(ex or 0)
        assert W.from_words(w) == math.floor(exact * (1 << f)), (t, n)


def test_the_helpers_refuse_what_they_must_and_leave_w_alone(lib):
    poison = 0xA5A5A5A5A5A5A5A5
    for n in (2, 16):
        f = W.frac_bits(n)
        for v in (2.5, -2.5, math.nextafter(2.0, 3.0), 1e300, math.inf, -math.inf, math.nan):
            rc, w = from_double(lib, v, n)
            assert rc == INVALID and message(lib) and all(int(x) == poison for x in w), v
        for t in ("2.5", "-2.5", "3", "-2." + "0" * 300 + "1", "2." + "0" * 20 + "1", "1e1", "0.3e1", "128", "-128", "1e9999",
                  "99999999999999999999999999999999999999999999"):
            rc, w = decimal(lib, t, n)
            assert rc == INVALID and "[-2, 2]" in message(lib) and all(int(x) == poison for x in w), t
        for t in ("", "-", "+", ".", "-.", "abc", "1.2.3", "1e", "1e+", "1e-", " 1", "1 ", "--1", "0x10", "1,5", "1e5.0", "e5", "1e12345",
                  "nan", "inf", "1f"):
            rc, w = decimal(lib, t, n)
            assert rc == INVALID and "expected" in message(lib) and all(int(x) == poison for x in w), t
        rc, w = decimal(lib, None, n)
        assert rc == INVALID and "NULL" in message(lib)
        # the sum leaves [-2, 2]; a non-finite delta
        w = W.to_words(2 << f, n)
        assert lib.fr_wide_add_double(w.ctypes.data, n, math.ldexp(1.0, -f)) == INVALID and W.from_words(w) == 2 << f
        assert lib.fr_wide_add_double(w.ctypes.data, n, -4.0) == 0 and W.from_words(w) == -(2 << f)
        assert lib.fr_wide_add_double(w.ctypes.data, n, -math.ldexp(1.0, -f - 3)) == INVALID and W.from_words(w) == -(2 << f)
        for d in (math.nan, math.inf, 1e300):
            assert lib.fr_wide_add_double(w.ctypes.data, n, d) == INVALID and W.from_words(w) == -(2 << f)
        # a stored value outside [-2, 2] is not handed over
        w = W.to_words((2 << f) + 1, n)
        hi = C.c_double(7.0)
        assert lib.fr_wide_to_double(w.ctypes.data, n, C.byref(hi), None) == INVALID and hi.value == 7.0
        assert lib.fr_wide_to_double(W.to_words(1, n).ctypes.data, n, None, None) == INVALID
    w = np.zeros(17, dtype=np.uint64)
    hi = C.c_double(0.0)
    for n in (0, 1, 17, 1 << 20):
        assert lib.fr_wide_from_double(1.0, w.ctypes.data, n) == INVALID and "2 .." in message(lib)
        assert lib.fr_wide_add_double(w.ctypes.data, n, 1.0) == INVALID
        assert lib.fr_wide_to_double(w.ctypes.data, n, C.byref(hi), None) == INVALID
        assert lib.fr_wide_from_decimal(b"1", w.ctypes.data, n) == INVALID
    assert not w.any()
    assert lib.fr_wide_from_double(1.0, None, 4) == INVALID and "NULL" in message(lib)
    assert lib.fr_wide_add_double(None, 4, 1.0) == INVALID
    assert lib.fr_wide_to_double(None, 4, C.byref(hi), None) == INVALID
    assert lib.fr_wide_from_decimal(b"1", None, 4) == INVALID


# ---- the reference orbits against the integer model ------------------------------------------------------------------


def c_centre(cre, cim, n):
    from fractal_renderer_amd import _native

    wr, wi = W.to_words(cre, n), W.to_words(cim, n)
    p64 = C.POINTER(C.c_uint64)
    return _native.fr_wide_centre(n, wr.ctypes.data_as(p64), wi.ctypes.data_as(p64)), (wr, wi)


def lib_orbit(lib, cfg, cre, cim, n, which=0):
    c, _keep = c_centre(cre, cim, n)
    ln = C.c_uint32(0)
    out = np.full((cfg.iterations + 3, 2), np.nan)
    assert lib.fr_debug_reference_orbit_wide(C.byref(cfg), C.byref(c), which, out.ctypes.data, len(out), C.byref(ln)) == 0, message(lib)
    assert np.isnan(out[ln.value:]).all()
    return out[:ln.value]


@pytest.mark.parametrize("name,n,scale_log2,cap,which,entries,ended", [
    ("M", 5, 200, 3000, 0, 194, True),
    ("M", 9, 440, 3000, 0, 352, True),
    ("N", 5, 100, 600, 0, 602, False),  # cut by the cap: kmax + 1 entries
    ("J", 4, 150, 3000, 0, None, True),  # V
    ("J", 4, 150, 3000, 1, None, True),  # K
    ("M", 16, 440, 3000, 0, None, True),
    ("M", 5, 200, 100, 0, 102, False),
    ("M", 5, 200, 0, 0, 2, False),
])
def test_reference_orbit_is_the_models_bit_for_bit(fr, lib, name, n, scale_log2, cap, which, entries, ended):
    cfg = W.view(fr.Config.new(), name, scale_log2, 16, 12, cap)
    cre, cim = W.centre_ints(name, n)
    want, want_ended, _ = W.orbit(cre, cim, n, cfg.algo, cap, W.JULIA_SET, which)
    got = lib_orbit(lib, cfg, cre, cim, n, which)
    assert got.shape == want.shape and same_bits(got, want)
    assert want_ended == ended and (entries is None or len(want) == entries)
    assert len(want) > 100 or cap <= 100  # the view is not trivial
    # cap: only that many entries are written, *len is the whole length
    c, _keep = c_centre(cre, cim, n)
    ln = C.c_uint32(0)
    out = np.full((5, 2), np.nan)
    assert lib.fr_debug_reference_orbit_wide(C.byref(cfg), C.byref(c), which, out.ctypes.data, 2, C.byref(ln)) == 0
    assert ln.value == len(want) and same_bits(out[:2], want[:2]) and np.isnan(out[2:]).all()


def test_reference_orbit_of_random_centres(fr, lib):
    """centres off the special points: orbits that wander, escape early or stay; both algorithms; n = 2 .. 16"""
    rng = random.Random(7)
    for n in (2, 3, 7, 16):
        f = W.frac_bits(n)
        for algo in (0, 2):
            for _ in range(6):
                cfg = fr.Config.new()
                cfg.algo, cfg.iterations, cfg.limit = algo, 150, 2.0
                cfg.scale.re = cfg.scale.im = 4.0
                cfg.julia_set.re, cfg.julia_set.im = rng.uniform(-1, 1), rng.uniform(-1, 1)
                cre, cim = rng.randrange(-(2 << f), (2 << f) + 1), rng.randrange(-(1 << f), (1 << f))
                if algo == 0:
                    cre = cre * 3 // 8 - (1 << (f - 1))  # around the set
                for which in ((0, 1) if algo == 2 else (0,)):
                    want, _, _ = W.orbit(cre, cim, n, algo, 150, (cfg.julia_set.re, cfg.julia_set.im), which)
                    got = lib_orbit(lib, cfg, cre, cim, n, which)
                    assert got.shape == want.shape and same_bits(got, want), (n, algo, which, cre, cim)


# ---- the domain ----------------------------------------------------------------------------------------------------------


def calls(lib, cfg, centre, from_iterations=None):
    """every entry point that takes a wide centre, with host buffers that a refusal must not need"""
    npx = cfg.width * cfg.height
    z, dz = np.zeros(2 * npx), np.zeros(2 * npx)
    it, m = np.zeros(npx, dtype=np.uint32), np.zeros(npx, dtype=np.uint32)
    rgb = np.zeros(4 * npx, dtype=np.uint8)
    ln = C.c_uint32(0)
    c = C.byref(centre) if centre is not None else None
    frm = cfg.iterations if from_iterations is None else from_iterations
    h = cfg.height
    return {
        "fr_render_rows_pt_wide": lambda: lib.fr_render_rows_pt_wide(C.byref(cfg), c, 0, h, 3, rgb.ctypes.data, rgb.nbytes),
        "fr_render_rows_pt_wide_device": lambda: lib.fr_render_rows_pt_wide_device(C.byref(cfg), c, 0, h, 4, rgb.ctypes.data, rgb.nbytes, None),
        "fr_escape_rows_pt_wide": lambda: lib.fr_escape_rows_pt_wide(C.byref(cfg), c, 0, h, z.ctypes.data, it.ctypes.data),
        "fr_escape_rows_pt_wide_state": lambda: lib.fr_escape_rows_pt_wide_state(C.byref(cfg), c, 0, h, z.ctypes.data, it.ctypes.data,
                                                                                 dz.ctypes.data, m.ctypes.data),
        "fr_escape_rows_pt_wide_state_device": lambda: lib.fr_escape_rows_pt_wide_state_device(
            C.byref(cfg), c, 0, h, z.ctypes.data, it.ctypes.data, dz.ctypes.data, m.ctypes.data, None),
        "fr_escape_extend_pt_wide": lambda: lib.fr_escape_extend_pt_wide(C.byref(cfg), c, 0, h, frm, z.ctypes.data, it.ctypes.data,
                                                                         dz.ctypes.data, m.ctypes.data),
        "fr_escape_extend_pt_wide_device": lambda: lib.fr_escape_extend_pt_wide_device(
            C.byref(cfg), c, 0, h, frm, z.ctypes.data, it.ctypes.data, dz.ctypes.data, m.ctypes.data, None),
        "fr_debug_reference_orbit_wide": lambda: lib.fr_debug_reference_orbit_wide(C.byref(cfg), c, 0, None, 0, C.byref(ln)),
    }


def good_view(fr, n=5, scale_log2=200):
    cfg = W.view(fr.Config.new(), "M", scale_log2, 16, 12, 300)
    centre, keep = c_centre(*W.centre_ints("M", n), n)
    return cfg, centre, keep


def refused(lib, cfg, centre, word):
    for name, call in calls(lib, cfg, centre).items():
        assert call() == INVALID, name
        assert word in message(lib), (name, message(lib))


def test_domain_refusals_come_with_a_message_and_before_any_device_work(fr, lib):
    from fractal_renderer_amd import _native

    p64 = C.POINTER(C.c_uint64)
    cfg, centre, _keep = good_view(fr)
    assert calls(lib, cfg, centre)["fr_debug_reference_orbit_wide"]() == 0  # the view itself is inside the domain
    words = np.zeros(17, dtype=np.uint64)
    for n in (1, 17, 0):
        refused(lib, cfg, _native.fr_wide_centre(n, words.ctypes.data_as(p64), words.ctypes.data_as(p64)), "n_words")
    refused(lib, cfg, _native.fr_wide_centre(5, None, centre.im), "NULL")
    refused(lib, cfg, _native.fr_wide_centre(5, centre.re, None), "NULL")
    refused(lib, cfg, None, "centre is NULL")
    # the scale: 2^440 is inside (n = 9), 2^441 is not, whatever n
    deep, centre9, _k9 = good_view(fr, 9, 440)
    assert calls(lib, deep, centre9)["fr_debug_reference_orbit_wide"]() == 0
    deep.scale.re = math.ldexp(1.0, 441)
    centre16, _k16 = c_centre(*W.centre_ints("M", 16), 16)
    refused(lib, deep, centre16, "2^440")
    deep.scale.re, deep.scale.im = 1.0, -math.ldexp(1.0, 441)
    refused(lib, deep, centre16, "2^440")
    # F one word too small for the scale: 2^200 needs n = 5, 2^440 needs n = 9
    centre4, _k4 = c_centre(*W.centre_ints("M", 4), 4)
    refused(lib, cfg, centre4, "too coarse")
    deep.scale.re = deep.scale.im = math.ldexp(1.0, 440)
    centre8, _k8 = c_centre(*W.centre_ints("M", 8), 8)
    refused(lib, deep, centre8, "too coarse")
    assert W.words_for_scale(2.0 ** 200) == 5 and W.words_for_scale(2.0 ** 440) == 9 and W.words_for_scale(0.4) == 2
    # the exact edge of the rule: F = 312 serves e + 64 <= 312, i.e. scales below 2^248
    cfg.scale.re = cfg.scale.im = math.nextafter(math.ldexp(1.0, 248), 0.0)
    assert calls(lib, cfg, centre)["fr_debug_reference_orbit_wide"]() == 0
    cfg.scale.im = math.ldexp(1.0, 248)
    refused(lib, cfg, centre, "too coarse")
    # a component of 2.5
    cfg, centre, _keep = good_view(fr)
    f = W.frac_bits(5)
    for bad in (5 << (f - 1), -(5 << (f - 1)), (2 << f) + 1, -(2 << f) - 1):
        c_bad, _kb = c_centre(bad, 0, 5)
        refused(lib, cfg, c_bad, "[-2, 2]")
        c_bad, _kb = c_centre(0, bad, 5)
        refused(lib, cfg, c_bad, "[-2, 2]")
    c_edge, _ke = c_centre(2 << f, -(2 << f), 5)
    assert calls(lib, cfg, c_edge)["fr_debug_reference_orbit_wide"]() == 0
    cfg.algo = 2
    cfg.julia_set.re = 2.5
    refused(lib, cfg, centre, "julia_set")
    cfg.julia_set.re, cfg.julia_set.im = 0.0, -2.5
    refused(lib, cfg, centre, "julia_set")
    # PT's domain on the remaining fields
    for field, value, word in (("limit", 0.0, "limit"), ("limit", math.inf, "finite"), ("exposure", math.nan, "finite"),
                               ("iterations", (1 << 24) + 1, "FR_PT_MAX_ITERATIONS")):
        cfg, centre, _keep = good_view(fr)
        setattr(cfg, field, value)
        refused(lib, cfg, centre, word)
    cfg, centre, _keep = good_view(fr)
    cfg.scale.re = math.ldexp(1.0, -65)
    refused(lib, cfg, centre, "2^-64")
    # cfg->pos is not read: not even its finiteness
    cfg, centre, _keep = good_view(fr)
    cfg.pos.re, cfg.pos.im = math.nan, math.inf
    assert calls(lib, cfg, centre)["fr_debug_reference_orbit_wide"]() == 0
    # a lower cap cannot be derived
    for name in ("fr_escape_extend_pt_wide", "fr_escape_extend_pt_wide_device"):
        assert calls(lib, cfg, centre, from_iterations=cfg.iterations + 1)[name]() == INVALID and "lower cap" in message(lib)
    assert lib.fr_render_rows_pt_wide(C.byref(cfg), C.byref(centre), 0, 1, 5, None, 0) == INVALID and "channels" in message(lib)


def test_no_ops_need_no_device(fr, lib):
    cfg, centre, _keep = good_view(fr)
    for name in ("fr_escape_extend_pt_wide", "fr_escape_extend_pt_wide_device"):
        assert calls(lib, cfg, centre, from_iterations=cfg.iterations)[name]() == 0, name  # M == N
    c = C.byref(centre)
    assert lib.fr_render_rows_pt_wide(C.byref(cfg), c, 3, 3, 3, None, 0) == 0
    assert lib.fr_render_rows_pt_wide_device(C.byref(cfg), c, 3, 3, 4, None, 0, None) == 0
    assert lib.fr_escape_rows_pt_wide(C.byref(cfg), c, 3, 3, None, None) == 0
    assert lib.fr_escape_rows_pt_wide_state(C.byref(cfg), c, 3, 3, None, None, None, None) == 0
    assert lib.fr_escape_rows_pt_wide_state_device(C.byref(cfg), c, 3, 3, None, None, None, None, None) == 0
    assert lib.fr_escape_extend_pt_wide(C.byref(cfg), c, 3, 3, 10, None, None, None, None) == 0
    assert lib.fr_escape_extend_pt_wide_device(C.byref(cfg), c, 3, 3, 10, None, None, None, None, None) == 0


def test_without_a_device_the_wide_renders_fail_loudly(fr, lib):
    if fr.device_count() > 0:
        return  # tests/test_gpu_pt_wide.py covers a box with a device
    cfg, centre, _keep = good_view(fr)
    for name, call in calls(lib, cfg, centre, from_iterations=10).items():
        if name != "fr_debug_reference_orbit_wide":
            assert call() == 3, name  # FR_ERR_NO_DEVICE: no CPU fallback


# ---- the header and the Python mirror ----------------------------------------------------------------------------------


def test_the_header_states_the_definition(lib):
    text = " ".join(open(os.path.join(ROOT, "include", "fractal_hip.h")).read().replace(" * ", " ").split())
    for phrase in ("WIDE PT", "F = 64 n - 8", "mul(a, b) = floor(a b / 2^F)", "mul2(a, b) = floor(2 a b / 2^F)",
                   "next(X, A) = (mul(X.re, X.re) - mul(X.im, X.im) + A.re, mul2(X.re, X.im) + A.im)",
                   "R_0 = 0, R_1 = C, R_{k+1} = next(R_k, C)", "V_0 = C, V_{k+1} = next(V_k, J)", "K_0 = 0, K_{k+1} = next(K_k, J)",
                   "f64 nearest to I / 2^F (ties to even)", "cfg->pos is not read", "Fixed point cannot overflow", "The range is 128",
                   "2^440", "2^458", "F >= e + 64", "64 guard bits", "#define FR_WIDE_MAX_WORDS 16", "#define FR_ABI_VERSION 3",
                   "typedef struct fr_wide_centre { uint32_t n_words; const uint64_t *re; const uint64_t *im; } fr_wide_centre;"):
        assert phrase in text, phrase
    assert lib.fr_abi_version() == 3
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fractal_hip.h")).read(), flags=re.S)
    for name in ("fr_wide_from_double", "fr_wide_add_double", "fr_wide_to_double", "fr_wide_from_decimal", "fr_render_rows_pt_wide",
                 "fr_render_rows_pt_wide_device", "fr_escape_rows_pt_wide", "fr_escape_rows_pt_wide_state_device",
                 "fr_escape_extend_pt_wide_device", "fr_escape_rows_pt_wide_state", "fr_escape_extend_pt_wide",
                 "fr_debug_reference_orbit_wide"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name)


def test_python_wide_centre(fr):
    m_re, m_im = W.centre("M")
    tre, tim = W.decimal_text(m_re, 140), W.decimal_text(m_im, 140)
    c = fr.WideCentre.from_str(tre, tim, scale=2.0 ** 200)
    assert c.words == 5 and fr.WideCentre.from_str(tre, tim, scale=(1.0, 2.0 ** 440)).words == 9
    assert fr.WideCentre.from_str(" 1.5 ", "-2", words=2).words == 2
    f = W.frac_bits(5)
    assert W.from_words(c.re) == math.floor(Fraction(tre) * (1 << f)) and W.from_words(c.im) == math.floor(Fraction(tim) * (1 << f))
    # 140 digits say more than the 312 fraction bits keep: the centre is the model's, but for the floor of a truncated string
    assert abs(W.from_words(c.re) - W.centre_ints("M", 5)[0]) <= 1
    (hi_re, hi_im), (lo_re, lo_im) = c.to_dd()
    assert (hi_re, lo_re) == W.split(W.from_words(c.re), 5) and (hi_im, lo_im) == W.split(W.from_words(c.im), 5)
    assert (hi_re, lo_re) == fr.split_dd(Fraction(W.from_words(c.re), 1 << f))
    before = W.from_words(c.re), W.from_words(c.im)
    off = (-0.37 / 2.0 ** 200, 0.21 / 2.0 ** 200)
    assert c.add(*off) is c
    assert W.from_words(c.re) == before[0] + math.floor(Fraction(off[0]) * (1 << f))
    assert W.from_words(c.im) == before[1] + math.floor(Fraction(off[1]) * (1 << f))
    cfg = W.view(fr.Config.new(), "M", 200, 16, 12, 300)
    want, _, _ = W.orbit(W.from_words(c.re), W.from_words(c.im), 5, 0, 300)
    assert same_bits(fr.reference_orbit_wide(cfg, c), want)
    with pytest.raises(ValueError):
        fr.get_image(cfg, fr.Precision.PT, centre=c, supersample=2)
    with pytest.raises(ValueError):
        fr.get_image_rows(cfg, 0, 1, fr.Precision.PT, centre=c, supersample=2)
    with pytest.raises(ValueError):
        fr.get_image_rgba(cfg, fr.Precision.PT, centre=c, supersample=3)
    with pytest.raises(ValueError):
        fr.get_image(cfg, fr.Precision.PT, centre=c, pos_lo=(0.0, 0.0))
    with pytest.raises(ValueError):
        fr.get_image(cfg, fr.Precision.DD, centre=c)
    with pytest.raises(ValueError):
        fr.escape_rows(cfg, precision=fr.Precision.F64, centre=c)
    with pytest.raises(ValueError):
        fr.WideCentre(1)
    with pytest.raises(ValueError):
        fr.WideCentre.from_str("1", "1")
    with pytest.raises(fr.FractalHipError):
        fr.WideCentre.from_str("2.5", "0", words=4)
    with pytest.raises(fr.FractalHipError):
        fr.WideCentre.from_str("1..5", "0", words=4)
    with pytest.raises(fr.FractalHipError) as e:
        fr.get_image(cfg, fr.Precision.PT, centre=fr.WideCentre.from_str(tre, tim, words=4))
    assert e.value.code == INVALID and "too coarse" in str(e.value)
