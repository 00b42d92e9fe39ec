"""FR_PRECISION_PT without a device: the host model (tests/pt_model.c) against 200-bit arithmetic on the deep views of the
DD tests, the long-orbit seahorse view (against the DD model too), a view whose reference orbit ends at once and a Julia
view that rebases onto the critical orbit; PT against the f64 oracle on the shallow default view; the library's
reference orbit against the model's bit for bit; and the PT argument checks of the C ABI answering before any device is
needed."""
import ctypes as C
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import dd_model as D
import oracle_lib as O
import pt_model as M

PT = 3
LIMIT2_MARGIN = Fraction(1, 2 ** 40)  # as tests/test_dd_model_cpu.py: a pixel whose escaping |z|^2 is this close to limit^2 is ambiguous


@pytest.fixture(scope="module")
def fr():
    import __graft_entry__ as ge

    ge.build()
    import fractal_renderer_amd

    return fractal_renderer_amd


def sample_pixels(width, height, n=64, seed=7):
    rng = np.random.default_rng(seed)
    flat = rng.choice(width * height, size=min(n, width * height), replace=False)
    return [(int(k % width), int(k // width)) for k in flat]


def exact_start(cfg, x, y, pos_lo):
    """pos + pos_lo + off with off evaluated as the definition does (one IEEE f64 operation each, in order)."""
    w, h = float(cfg.width), float(cfg.height)
    off_re = ((float(x) / h) - ((w / h) / 2.0)) / cfg.scale.re
    off_im = ((float(y) / h) - 0.5) / cfg.scale.im
    return (Fraction(cfg.pos.re) + Fraction(pos_lo[0]) + Fraction(off_re),
            Fraction(cfg.pos.im) + Fraction(pos_lo[1]) + Fraction(off_im))


def orbit_200(cfg, start):
    """recursive() at 200 bits: (escape index, |z|^2 at the escape or None)"""
    with mpmath.workprec(200):
        zr = mpmath.mpf(start[0].numerator) / start[0].denominator
        zi = mpmath.mpf(start[1].numerator) / start[1].denominator
        if cfg.algo == 2:
            cr, ci = mpmath.mpf(cfg.julia_set.re), mpmath.mpf(cfg.julia_set.im)
        else:
            cr, ci = zr, zi
        lim2 = mpmath.mpf(cfg.limit) ** 2
        for i in range(cfg.iterations):
            zr, zi = zr * zr - zi * zi + cr, 2 * zr * zi + ci
            d = zr * zr + zi * zi
            if d > lim2:
                return i, d
        return cfg.iterations, None


def ambiguous(cfg, dist):
    if dist is None:
        return False
    lim2 = mpmath.mpf(cfg.limit) ** 2
    return abs(dist - lim2) <= lim2 * mpmath.mpf(LIMIT2_MARGIN.numerator) / LIMIT2_MARGIN.denominator


def agreement(cfg, pos_lo, it, n=64):
    """(checked, agreeing, escape indices of the 200-bit orbits) over the unambiguous sampled pixels"""
    checked = agree = 0
    escapes = []
    for x, y in sample_pixels(cfg.width, cfg.height, n):
        want, dist = orbit_200(cfg, exact_start(cfg, x, y, pos_lo))
        if ambiguous(cfg, dist):
            continue
        checked += 1
        agree += int(it[y, x]) == want
        escapes.append(want)
    return checked, agree, escapes


VIEWS = [("mandelbrot", False, (0.0, 0.0)), ("julia", True, (0.0, 0.0)), ("mandelbrot_lo", False, (0.0, 2.0 ** -60)),
         ("julia_lo", True, (0.0, 2.0 ** -60))]


@pytest.mark.parametrize("name,julia,pos_lo", VIEWS, ids=[v[0] for v in VIEWS])
def test_model_follows_the_200_bit_orbit_on_the_deep_views(name, julia, pos_lo):
    cfg = D.deep_view(O.config_new(), julia)
    _, it = M.escape_rows(cfg, pos_lo)
    checked, agree, escapes = agreement(cfg, pos_lo, it)
    assert checked >= 60, checked
    assert agree == checked, "the PT model left the 200-bit orbit on %d of %d pixels" % (checked - agree, checked)
    assert max(escapes) < cfg.iterations and len(set(escapes)) >= 2, sorted(set(escapes))


def test_long_orbit_view_pt_is_no_worse_than_dd():
    """The seahorse-valley centre at scale 10^20: orbits of ~9000 to 20000 iterations.  On such chaotic orbits neither
    method is exact; PT must follow the 200-bit orbit on at least as many sampled pixels as DD does, and on nearly all."""
    cfg = O.config_new()
    lo = M.seahorse_view(cfg)
    _, it = M.escape_rows(cfg, lo)
    _, itd = D.escape_rows(cfg, lo)
    pt_checked, pt_agree, escapes = agreement(cfg, lo, it, n=48)
    dd_checked, dd_agree, _ = agreement(cfg, lo, itd, n=48)
    assert pt_checked == dd_checked >= 44
    assert pt_agree >= dd_agree, (pt_agree, dd_agree, pt_checked)
    assert pt_agree >= pt_checked - 2, (pt_agree, pt_checked)
    assert min(escapes) > 8000 and len(set(escapes)) >= 8  # long orbits, a resolved image
    # over the whole 32 x 24 view the two models differ on a handful of pixels (2 of 768 when this was written)
    assert int((it != itd).sum()) <= 8


def test_view_whose_reference_escapes_early():
    """c = 0.26: the reference orbit ends after 31 entries, and every pixel that lives longer rebases at its end."""
    cfg = O.config_new()
    lo = M.early_escape_view(cfg)
    n = len(M.reference_orbit(cfg, lo))
    assert n == 31
    _, it = M.escape_rows(cfg, lo)
    assert int((it == cfg.iterations).sum()) > it.size // 3  # many pixels far beyond the orbit's end
    checked, agree, escapes = agreement(cfg, lo, it)
    assert checked >= 60
    assert agree == checked, "the PT model left the 200-bit orbit on %d of %d pixels" % (checked - agree, checked)
    assert max(escapes) == cfg.iterations and min(escapes) < n and len(set(escapes)) >= 8


def test_julia_view_that_rebases_onto_the_critical_orbit():
    """V ends after 202 entries and every pixel outlives it: the pixels go on on K (which, c lying outside the
    Mandelbrot set, ends too, after 253 entries: the pixels rebase onto K's start again there)."""
    cfg = O.config_new()
    lo = M.julia_rebase_view(cfg)
    v, k = M.reference_orbit(cfg, lo, 0), M.reference_orbit(cfg, lo, 1)
    assert len(v) == 202 and len(k) == 253
    _, it = M.escape_rows(cfg, lo)
    assert int(it.min()) >= len(v) - 8
    checked, agree, escapes = agreement(cfg, lo, it)
    assert checked >= 60
    assert agree == checked, "the PT model left the 200-bit orbit on %d of %d pixels" % (checked - agree, checked)
    assert max(escapes) > len(v) + len(k) and len(set(escapes)) >= 20


@pytest.mark.parametrize("julia", [False, True], ids=["mandelbrot", "julia"])
def test_shallow_default_view_is_f64_but_for_a_small_fraction(oracle, julia):
    """On the shallow default views PT and the f64 oracle computed the same escape index on every pixel when this was
    written (257 x 193, 200 / 300 iterations); the threshold allows 0.5 %, as the two are different arithmetics."""
    cfg = O.config_new()
    cfg.width, cfg.height, cfg.iterations = 257, 193, 200
    if julia:
        cfg.algo, cfg.iterations = 2, 300
        cfg.julia_set.re, cfg.julia_set.im = -0.8, 0.156
        cfg.scale.re = cfg.scale.im = 0.3
    _, it = M.escape_rows(cfg)
    _, it64 = oracle.escape_rows(cfg)
    assert int((it != it64).sum()) <= it.size // 200


def test_model_count_matches_its_escape_rows():
    cfg = O.config_new()
    M.julia_rebase_view(cfg, 40, 24, 500)
    _, it = M.escape_rows(cfg)
    want = int(np.where(it < cfg.iterations, it.astype(np.uint64) + 1, cfg.iterations).sum())
    assert M.count_iterations(cfg) == want


def test_precision_enum_has_pt(fr):
    assert int(fr.Precision.PT) == 3


# ---- the library's reference orbit (no device) -----------------------------------------------------------------------


def library_orbit(fr, cfg, pos_lo, which):
    from fractal_renderer_amd import _native

    lib = _native.load()
    n = C.c_uint32()
    lo = C.byref(_native.Imaginary(*pos_lo))
    _native.check(lib.fr_debug_reference_orbit(C.byref(cfg), lo, which, None, 0, C.byref(n)))
    out = np.empty((n.value, 2), dtype=np.float64)
    _native.check(lib.fr_debug_reference_orbit(C.byref(cfg), lo, which, out.ctypes.data, n.value, C.byref(n)))
    return out


@pytest.mark.parametrize("name", ["seahorse", "early", "deep_mandelbrot", "deep_julia", "julia_rebase", "short"])
def test_library_reference_orbit_is_the_model_s(fr, name):
    cfg = fr.Config.new()
    lo = (0.0, 0.0)
    if name == "seahorse":
        lo = M.seahorse_view(cfg)
    elif name == "early":
        M.early_escape_view(cfg)
    elif name.startswith("deep"):
        D.deep_view(cfg, name == "deep_julia")
        lo = (0.0, 2.0 ** -60)
    elif name == "julia_rebase":
        M.julia_rebase_view(cfg)
    else:
        cfg.iterations = 1
    for which in ((0, 1) if cfg.algo == 2 else (0,)):
        got, want = library_orbit(fr, cfg, lo, which), M.reference_orbit(cfg, lo, which)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (which, got.shape,
                                                                                                       want.shape)


# ---- C ABI: PT argument errors need no device ------------------------------------------------------------------------


def test_pt_argument_errors_need_no_device(fr):
    from fractal_renderer_amd import _native

    lib = _native.load()
    INV = _native.FR_ERR_INVALID_ARGUMENT
    buf = np.zeros(4 * 16 * 8, dtype=np.uint8)
    z = np.zeros(4 * 16 * 8, dtype=np.float64)
    it = np.zeros(16 * 8, dtype=np.uint32)

    def cfg_with(**kw):
        c = fr.Config.new()
        c.width, c.height, c.iterations = 16, 8, 20
        for k, v in kw.items():
            if "." in k:
                a, b = k.split(".")
                setattr(getattr(c, a), b, v)
            else:
                setattr(c, k, v)
        return c

    def calls(cfg, lo=None):
        lop = C.byref(_native.Imaginary(*lo)) if lo is not None else None
        total, npx, px, n = C.c_uint64(), C.c_uint64(), _native.RGB(), C.c_uint32()
        return {
            "rows_rgb8": lambda: lib.fr_render_rows_rgb8(C.byref(cfg), PT, 0, 1, buf.ctypes.data, buf.nbytes),
            "rows_rgba8": lambda: lib.fr_render_rows_rgba8(C.byref(cfg), PT, 0, 1, buf.ctypes.data, buf.nbytes),
            "rows_rgb8_device": lambda: lib.fr_render_rows_rgb8_device(C.byref(cfg), PT, 0, 1, buf.ctypes.data, buf.nbytes, None),
            "pixel_p": lambda: lib.fr_pixel_p(C.byref(cfg), PT, 0, 0, C.byref(px)),
            "escape_rows": lambda: lib.fr_escape_rows(C.byref(cfg), PT, 0, 1, z.ctypes.data, it.ctypes.data),
            "count": lambda: lib.fr_count_iterations(C.byref(cfg), PT, 0, 1, 1, 1, C.byref(total), C.byref(npx)),
            "rows_pt": lambda: lib.fr_render_rows_pt(C.byref(cfg), lop, 0, 1, 3, buf.ctypes.data, buf.nbytes),
            "rows_pt_rgba": lambda: lib.fr_render_rows_pt(C.byref(cfg), lop, 0, 1, 4, buf.ctypes.data, buf.nbytes),
            "rows_pt_device": lambda: lib.fr_render_rows_pt_device(C.byref(cfg), lop, 0, 1, 3, buf.ctypes.data, buf.nbytes,
                                                                   None),
            "escape_rows_pt": lambda: lib.fr_escape_rows_pt(C.byref(cfg), lop, 0, 1, z.ctypes.data, it.ctypes.data),
            "reference_orbit": lambda: lib.fr_debug_reference_orbit(C.byref(cfg), lop, 0, None, 0, C.byref(n)),
        }

    bad = {
        "NaN pos": cfg_with(**{"pos.re": float("nan")}),
        "inf scale": cfg_with(**{"scale.im": float("inf")}),
        "NaN exposure": cfg_with(exposure=float("nan")),
        "limit 0": cfg_with(limit=0.0),
        "limit > 2^500": cfg_with(limit=2.0 ** 501),
        "|pos| > 2^64": cfg_with(**{"pos.im": -(2.0 ** 65)}),
        "|julia_set| > 2^64": cfg_with(**{"julia_set.re": 2.0 ** 65}),
        "|scale| < 2^-64": cfg_with(**{"scale.re": 2.0 ** -65}),
        "iterations > cap": cfg_with(iterations=(1 << 24) + 1),
    }
    for what, cfg in bad.items():
        for name, call in calls(cfg).items():
            assert call() == INV, (what, name)
            assert b"FR_PRECISION_PT" in lib.fr_last_error(), (what, name, lib.fr_last_error())
    deep = cfg_with(**{"pos.im": 1.0})
    for lo in [(0.0, 2.0 ** -52), (1.0, 0.0), (0.0, float("nan")), (float("inf"), 0.0)]:
        for name in ("rows_pt", "rows_pt_rgba", "rows_pt_device", "escape_rows_pt", "reference_orbit"):
            assert calls(deep, lo)[name]() == INV, (lo, name)
            assert b"FR_PRECISION_PT" in lib.fr_last_error()
    for ch in (0, 1, 2, 5):
        assert lib.fr_render_rows_pt(C.byref(deep), None, 0, 1, ch, buf.ctypes.data, buf.nbytes) == INV
        assert lib.fr_render_rows_pt_device(C.byref(deep), None, 0, 1, ch, buf.ctypes.data, buf.nbytes, None) == INV
    n = C.c_uint32()
    assert lib.fr_debug_reference_orbit(C.byref(deep), None, 1, None, 0, C.byref(n)) == INV  # K is Julia's
    assert lib.fr_debug_reference_orbit(C.byref(deep), None, 0, None, 0, None) == INV
    assert lib.fr_render_rows_pt(C.byref(deep), None, 5, 4, 3, buf.ctypes.data, buf.nbytes) == INV
    assert lib.fr_escape_rows_pt(None, None, 0, 1, z.ctypes.data, it.ctypes.data) == INV
    assert lib.fr_render_rows_pt(C.byref(deep), None, 0, 1, 3, buf.ctypes.data, 3) == _native.FR_ERR_BUFFER_TOO_SMALL
    # the cap itself is accepted (the orbit is computed on the host: no device needed for this call)
    assert lib.fr_debug_reference_orbit(C.byref(cfg_with(iterations=1 << 24)), None, 0, None, 0, C.byref(n)) == _native.FR_OK
    # multi-device, block-cyclic and the batch refuse PT
    blk = C.c_uint64()
    assert lib.fr_render_rgb8_multi(C.byref(deep), PT, 8, buf.ctypes.data, buf.nbytes) == INV
    assert lib.fr_render_rgb8_multi_device(C.byref(deep), PT, 8, 0, buf.ctypes.data, buf.nbytes) == INV
    assert lib.fr_render_block_cyclic_rgb8(C.byref(deep), PT, 8, 0, 1, buf.ctypes.data, buf.nbytes, C.byref(blk)) == INV
    assert lib.fr_render_block_cyclic_rgb8_device(C.byref(deep), PT, 8, 0, 1, buf.ctypes.data, buf.nbytes, None,
                                                  C.byref(blk)) == INV
    pts = (_native.Imaginary * 1)()
    outp, outi = (_native.Imaginary * 1)(), (C.c_uint32 * 1)()
    assert lib.fr_recursive_batch(10, pts, pts, 1, 2.0, PT, outp, outi) == INV
    assert b"FR_PRECISION_PT is single-device" in lib.fr_last_error()
    # empty ranges are legal no-ops
    assert lib.fr_render_rows_rgb8(C.byref(deep), PT, 3, 3, None, 0) == _native.FR_OK
    assert lib.fr_render_rows_pt(C.byref(deep), None, 3, 3, 4, None, 0) == _native.FR_OK
    assert lib.fr_escape_rows_pt(C.byref(deep), C.byref(_native.Imaginary(0.0, 2.0 ** -60)), 2, 2, None, None) == _native.FR_OK
    # Python: pos_lo takes PT as well as DD; with_lo stays DD's
    with pytest.raises(ValueError):
        fr.escape_rows(deep, precision=fr.Precision.PT, with_lo=True)
    with pytest.raises(ValueError):
        fr.get_image(deep, fr.Precision.F64, pos_lo=(0.0, 0.0))
