"""The host models of FR_PRECISION_DD and FR_PRECISION_PT (tests/dd_model.c, tests/pt_model.c) against the header text.

The GPU tests compare each kernel with its model bit for bit; a misreading of include/fractal_hip.h shared by a model and
its kernel would pass them.  Here DD's operations, one DD iteration, the start, and PT's reference orbits and pixel step
are restated once more, in Python, straight from the header: Python floats for + - * (IEEE binary64, round to nearest,
subnormals kept) and the C library's correctly rounded fma through ctypes.  Both must agree bit for bit, zero signs
included, on pixels of every edge view of tests/deep_edge_views.py and of the existing deep views.  No device needed."""
import ctypes as C
import ctypes.util
import math
import struct

import numpy as np
import pytest

import dd_model as D
import deep_edge_views as V
import oracle_lib as O
import pt_model as P

_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.fma.restype = C.c_double
_libm.fma.argtypes = [C.c_double, C.c_double, C.c_double]
fma = _libm.fma


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def test_fma_is_fused():
    """the fma used below rounds once: 1 + 2^-52 squared minus its rounded square leaves 2^-104"""
    a = 1.0 + 2.0 ** -52
    p = a * a
    assert fma(a, a, -p) == 2.0 ** -104


# ---- DD, as include/fractal_hip.h defines it -----------------------------------------------------------------------


def two_sum(a, b):
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    return s, e


def fast_two_sum(a, b):
    s = a + b
    e = b - (s - a)
    return s, e


def add_dd(a, b):
    sh, sl = two_sum(a[0], b[0])
    th, tl = two_sum(a[1], b[1])
    sl = sl + th
    sh, sl = fast_two_sum(sh, sl)
    sl = sl + tl
    return fast_two_sum(sh, sl)


def add_d(a, d):
    sh, sl = two_sum(a[0], d)
    sl = sl + a[1]
    return fast_two_sum(sh, sl)


def sqr(x):
    p = x[0] * x[0]
    e = fma(x[0], x[0], -p)
    e = fma(x[0] + x[0], x[1], e)
    return fast_two_sum(p, e)


def twice_mul(x, y):
    p = x[0] * y[0]
    e = fma(x[0], y[0], -p)
    e = fma(x[0], y[1], e)
    e = fma(x[1], y[0], e)
    h, l = fast_two_sum(p, e)
    return h + h, l + l


def neg(x):
    return -x[0], -x[1]


def offsets(cfg, x, y):
    """off_re = ((x/h) - ((w/h)/2)) / scale.re, off_im = ((y/h) - 0.5) / scale.im, one f64 operation each"""
    w, h = float(cfg.width), float(cfg.height)
    return ((float(x) / h) - ((w / h) / 2.0)) / cfg.scale.re, ((float(y) / h) - 0.5) / cfg.scale.im


def dd_step(cfg, re, im, cre, cim):
    """one iteration; Mandelbrot: c = the start (dd), Julia: c = julia_set (f64) with add_d outside"""
    a = add_dd(sqr(re), neg(sqr(im)))
    b = twice_mul(re, im)
    if cfg.algo == 2:
        return add_d(a, cfg.julia_set.re), add_d(b, cfg.julia_set.im)
    return add_dd(a, cre), add_dd(b, cim)


def dd_pixel(cfg, x, y, lo):
    """(re.hi, re.lo, im.hi, im.lo, index) of recursive() in dd"""
    if cfg.algo not in (0, 2):
        return (0.0, 0.0, 0.0, 0.0), 0
    off_re, off_im = offsets(cfg, x, y)
    re, im = add_d((cfg.pos.re, lo[0]), off_re), add_d((cfg.pos.im, lo[1]), off_im)
    cre, cim = re, im
    squared = cfg.limit * cfg.limit
    for i in range(cfg.iterations):
        nre, nim = dd_step(cfg, re, im, cre, cim)
        if nre[0] * nre[0] + nim[0] * nim[0] > squared:
            return (nre[0], nre[1], nim[0], nim[1]), i
        re, im = nre, nim
    return (re[0], re[1], im[0], im[1]), cfg.iterations


# ---- PT, as include/fractal_hip.h defines it -----------------------------------------------------------------------


def pt_orbit(cfg, lo, which):
    """R (Mandelbrot), V (which 0, Julia) or K (which 1, Julia) as a list of stored (re.hi, im.hi)"""
    julia = cfg.algo == 2
    kmin, kmax = (1, max(cfg.iterations, 1)) if julia else (2, cfg.iterations + 1)
    cre, cim = (cfg.pos.re, lo[0]), (cfg.pos.im, lo[1])
    zr, zi = (cre, cim) if julia and which == 0 else ((0.0, 0.0), (0.0, 0.0))
    out = []
    k = 0
    while True:
        out.append((zr[0], zi[0]))
        if k >= kmin and zr[0] * zr[0] + zi[0] * zi[0] > 4.0:
            break
        if k == kmax:
            break
        if not julia and k == 0:
            zr, zi = cre, cim  # R_1 = C
        else:
            zr, zi = dd_step(cfg, zr, zi, cre, cim)
        k += 1
    return out


def pt_pixel(cfg, x, y, orbits):
    """(re, im, index) of one pixel's perturbed iteration; orbits = (X, K): R, R or V, K"""
    if cfg.algo not in (0, 2):
        return (0.0, 0.0), 0
    julia = cfg.algo == 2
    off_re, off_im = offsets(cfg, x, y)
    X = orbits[0]
    m = 0 if julia else 1
    dzr, dzi = off_re, off_im
    dcr, dci = (0.0, 0.0) if julia else (off_re, off_im)
    zr, zi = X[m][0] + dzr, X[m][1] + dzi
    squared = cfg.limit * cfg.limit
    for i in range(cfg.iterations):
        tr, ti = X[m][0] + zr, X[m][1] + zi
        ndr = fma(tr, dzr, fma(-ti, dzi, dcr))
        ndi = fma(tr, dzi, fma(ti, dzr, dci))
        m += 1
        zr, zi = X[m][0] + ndr, X[m][1] + ndi
        dzr, dzi = ndr, ndi
        dist = zr * zr + zi * zi
        if dist > squared:
            return (zr, zi), i
        if dist < dzr * dzr + dzi * dzi or m == len(X) - 1:
            dzr, dzi = zr, zi
            m = 0
            X = orbits[1]
    return (zr, zi), cfg.iterations


def pt_orbits(cfg, lo):
    x = pt_orbit(cfg, lo, 0)
    return (x, pt_orbit(cfg, lo, 1)) if cfg.algo == 2 else (x, x)


# ---- the views and their pixels ------------------------------------------------------------------------------------


def existing_views():
    """the deep views of test_gpu_dd.py / test_gpu_pt.py: (name, cfg, pos_lo)"""
    out = []
    for julia in (False, True):
        for lo in ((0.0, 0.0), (0.0, 2.0 ** -60)):
            cfg = O.config_new(0)
            D.deep_view(cfg, julia, 257, 193, 3000)
            out.append(("deep_%s%s" % ("julia" if julia else "mandelbrot", "_lo" if lo[1] else ""), cfg, lo))
    for name, make in (("seahorse", P.seahorse_view), ("early", P.early_escape_view), ("julia_rebase", P.julia_rebase_view)):
        cfg = O.config_new(0)
        lo = make(cfg)
        out.append((name, cfg, lo))
    return out


def edge_cases():
    out = []
    for flat in (False, True):
        for name, lo in V.cases(flat):
            cfg = O.config_new(V.VIEWS[name][0])
            V.make(cfg, name)
            out.append((V.case_id((name, lo)), cfg, lo))
    return out


ALL = existing_views() + edge_cases()


def pixels(cfg, n=5, seed=3):
    """corners, the centre and a few seeded others"""
    w, h = cfg.width, cfg.height
    rng = np.random.default_rng(seed)
    pts = {(0, 0), (w - 1, h - 1), (w // 2, h // 2), (w - 1, 0)}
    while len(pts) < 4 + n:
        pts.add((int(rng.integers(w)), int(rng.integers(h))))
    return sorted(pts)


def same_bits(a, b):
    return all(bits(u) == bits(v) or (math.isnan(u) and math.isnan(v)) for u, v in zip(a, b))


@pytest.mark.parametrize("name,cfg,lo", ALL, ids=[c[0] for c in ALL])
def test_dd_model_is_the_header_text(name, cfg, lo):
    for x, y in pixels(cfg):
        want_z, want_it = dd_pixel(cfg, x, y, lo)
        z, it = D.pixel(cfg, x, y, lo)
        assert it == want_it and same_bits(z, want_z), (name, x, y, it, want_it, list(z), want_z)
        zr, itr = D.escape_rows(cfg, lo, y, y + 1)  # the row form of the model gives the same pixel
        assert itr[0, x] == it and same_bits(zr[0, x], z), (name, x, y)


@pytest.mark.parametrize("name,cfg,lo", ALL, ids=[c[0] for c in ALL])
def test_pt_model_is_the_header_text(name, cfg, lo):
    orbits = pt_orbits(cfg, lo)
    assert [tuple(e) for e in P.reference_orbit(cfg, lo, 0).tolist()] == orbits[0] or cfg.algo not in (0, 2)
    for x, y in pixels(cfg):
        want_z, want_it = pt_pixel(cfg, x, y, orbits)
        z, it = P.pixel(cfg, x, y, lo)
        assert it == want_it and same_bits(z, want_z), (name, x, y, it, want_it, list(z), want_z)
        zr, itr = P.escape_rows(cfg, lo, y, y + 1)
        assert itr[0, x] == it and same_bits(zr[0, x], z), (name, x, y)


@pytest.mark.parametrize("name,cfg,lo", ALL, ids=[c[0] for c in ALL])
def test_views_are_in_the_domain(name, cfg, lo):
    """what check_deep accepts (include/fractal_hip.h): the GPU tests render these views expecting FR_OK"""
    fields = [cfg.limit, cfg.stable_limit, cfg.pos.re, cfg.pos.im, cfg.scale.re, cfg.scale.im, cfg.exposure, cfg.color_weight,
              cfg.julia_set.re, cfg.julia_set.im, lo[0], lo[1]]
    assert all(math.isfinite(v) for v in fields)
    assert 0.0 < cfg.limit <= 2.0 ** 500
    assert max(abs(cfg.pos.re), abs(cfg.pos.im), abs(cfg.julia_set.re), abs(cfg.julia_set.im)) <= 2.0 ** 64
    assert min(abs(cfg.scale.re), abs(cfg.scale.im)) >= 2.0 ** -64
    assert cfg.pos.re + lo[0] == cfg.pos.re and cfg.pos.im + lo[1] == cfg.pos.im, "pos_lo is not normalised"


def test_orbits_compare_zero_signs():
    """same_bits tells -0.0 from +0.0: the comparison above would see a zero of the wrong sign"""
    assert not same_bits((0.0,), (-0.0,)) and same_bits((float("nan"),), (float("nan"),))


def test_subnormal_views_reach_subnormals():
    """the tiny edge views do what they are there for: most of the models' final positions are subnormal"""
    tiny = 2.0 ** -1022
    for name, least in (("origin_1e308", 12000), ("julia_c_subnormal", 4000)):
        cfg = O.config_new(V.VIEWS[name][0])
        V.make(cfg, name)
        dz, _ = D.escape_rows(cfg)
        pz, _ = P.escape_rows(cfg)
        for z2 in (dz[..., 0::2], pz):
            assert int(((z2 != 0) & (np.abs(z2) < tiny)).sum()) >= least, name
