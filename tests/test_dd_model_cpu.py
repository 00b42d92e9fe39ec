"""FR_PRECISION_DD without a device: the host model (tests/dd_model.c) against 200-bit arithmetic on the deep reference
views, the f64 oracle failing on the same views (what DD is for), split_dd's exactness, and the DD argument checks of
the C ABI answering before any device is needed."""
import ctypes as C
from decimal import Decimal
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import dd_model as M
import oracle_lib as O

LIMIT2_MARGIN = Fraction(1, 2 ** 40)  # relative distance of the escaping |z|^2 from limit^2 below which a pixel is ambiguous


@pytest.fixture(scope="module")
def fr():
    import __graft_entry__ as ge

    ge.build()
    import fractal_renderer_amd

    return fractal_renderer_amd


def sample_pixels(width, height, n=64, seed=7):
    rng = np.random.default_rng(seed)
    flat = rng.choice(width * height, size=n, replace=False)
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


VIEWS = [("mandelbrot", False, (0.0, 0.0)), ("julia", True, (0.0, 0.0)), ("mandelbrot_lo", False, (0.0, 2.0 ** -60)),
         ("julia_lo", True, (0.0, 2.0 ** -60))]


@pytest.mark.parametrize("name,julia,pos_lo", VIEWS, ids=[v[0] for v in VIEWS])
def test_model_follows_the_200_bit_orbit_on_the_deep_views(name, julia, pos_lo):
    cfg = M.deep_view(O.config_new(), julia)
    z, it = M.escape_rows(cfg, pos_lo)
    checked = agree = 0
    escapes = set()
    for x, y in sample_pixels(cfg.width, cfg.height):
        want, dist = orbit_200(cfg, exact_start(cfg, x, y, pos_lo))
        if ambiguous(cfg, dist):
            continue
        checked += 1
        agree += int(it[y, x]) == want
        escapes.add(want)
    assert checked >= 60, checked
    assert agree == checked, "the DD model left the 200-bit orbit on %d of %d pixels" % (checked - agree, checked)
    # the views are what they claim to be: every sampled pixel escapes after a few dozen iterations, centred on c = i at
    # many different indices (a flat image would be a poor test); shifted by pos_lo (~42 pixels) the view still resolves
    # pixels f64 cannot tell apart
    assert max(escapes) < cfg.iterations and len(escapes) >= (8 if pos_lo == (0.0, 0.0) else 2), sorted(escapes)


@pytest.mark.parametrize("julia", [False, True], ids=["mandelbrot", "julia"])
def test_f64_fails_where_dd_holds(oracle, julia):
    """The f64 oracle on the same view: adjacent pixels share one f64 start, the orbits are wrong."""
    cfg = M.deep_view(O.config_new(), julia)
    _, it64 = oracle.escape_rows(cfg)
    agree = checked = 0
    for x, y in sample_pixels(cfg.width, cfg.height):
        want, dist = orbit_200(cfg, exact_start(cfg, x, y, (0.0, 0.0)))
        if ambiguous(cfg, dist):
            continue
        checked += 1
        agree += int(it64[y, x]) == want
    assert checked >= 60
    assert agree <= checked // 4, "f64 agreed with the 200-bit orbit on %d of %d pixels" % (agree, checked)


def test_model_start_hi_is_the_f64_start_when_pos_lo_is_zero(oracle):
    cfg = O.config_new()
    cfg.width, cfg.height, cfg.iterations = 97, 61, 0
    cfg.pos.re, cfg.pos.im, cfg.scale.re, cfg.scale.im = -0.743643887037158, 0.131825904205312, 3.1e14, 2.9e14
    z, it = M.escape_rows(cfg)
    z64, _ = oracle.escape_rows(cfg)
    assert np.array_equal(z[..., 0].view(np.uint64), z64[..., 0].view(np.uint64))
    assert np.array_equal(z[..., 2].view(np.uint64), z64[..., 1].view(np.uint64))
    assert (it == 0).all()
    # and the lo parts carry what f64 dropped: pos + off is exact in dd
    x, y = 13, 40
    s = M.start(cfg, x, y)
    want = exact_start(cfg, x, y, (0.0, 0.0))
    assert Fraction(s[0]) + Fraction(s[1]) == want[0] and Fraction(s[2]) + Fraction(s[3]) == want[1]


def test_model_count_matches_its_escape_rows():
    cfg = M.deep_view(O.config_new(), False, 40, 24, 500)
    _, it = M.escape_rows(cfg)
    want = int(np.where(it < cfg.iterations, it.astype(np.uint64) + 1, cfg.iterations).sum())
    assert M.count_iterations(cfg) == want


# ---- split_dd -----------------------------------------------------------------------------------------------------


def check_split(value, exact):
    import fractal_renderer_amd as fr

    hi, lo = fr.split_dd(value)
    assert isinstance(hi, float) and isinstance(lo, float)
    assert hi == float(exact)  # the nearest f64
    assert hi + lo == hi  # normalised: a valid pos / pos_lo pair
    rest = exact - Fraction(hi)
    assert lo == float(rest)  # the nearest f64 to the rest
    return hi, lo


def test_split_dd_is_exact_for_every_input_type(fr):
    text = "-0.74364388703715870475219150611477418"
    exact = Fraction(text)
    got = {check_split(v, exact) for v in (text, Decimal(text), exact)}
    assert len(got) == 1
    with mpmath.workprec(300):
        m = mpmath.mpf(text)
        man, exp = m.man_exp
        check_split(m, Fraction(int(man)) * Fraction(2) ** int(exp))
    # a value that IS a dd comes back unchanged
    assert fr.split_dd(Fraction(1) + Fraction(1, 2 ** 60)) == (1.0, 2.0 ** -60)
    assert fr.split_dd("0.1") == (0.1, float(Fraction("0.1") - Fraction(0.1)))
    assert fr.split_dd(0.1) == (0.1, 0.0) and fr.split_dd(3) == (3.0, 0.0)
    hi, lo = fr.split_dd("1e-30")
    assert Fraction(hi) + Fraction(lo) != Fraction("1e-30") and abs(Fraction(hi) + Fraction(lo) - Fraction("1e-30")) < Fraction(1, 10 ** 60)


def test_precision_enum_has_dd(fr):
    assert int(fr.Precision.DD) == 2


# ---- C ABI: DD argument errors need no device ------------------------------------------------------------------------


def test_dd_argument_errors_need_no_device(fr):
    from fractal_renderer_amd import _native

    lib = _native.load()
    INV = _native.FR_ERR_INVALID_ARGUMENT
    DD = 2
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
        opts = fr.RenderOpts()
        total, npx, px = C.c_uint64(), C.c_uint64(), _native.RGB()
        return {
            "rows_rgb8": lambda: lib.fr_render_rows_rgb8(C.byref(cfg), DD, 0, 1, buf.ctypes.data, buf.nbytes),
            "rows_rgba8": lambda: lib.fr_render_rows_rgba8(C.byref(cfg), DD, 0, 1, buf.ctypes.data, buf.nbytes),
            "rows_rgb8_opts": lambda: lib.fr_render_rows_rgb8_opts(C.byref(cfg), DD, 0, 1, buf.ctypes.data, buf.nbytes,
                                                                   C.byref(opts)),
            "rows_rgb8_device": lambda: lib.fr_render_rows_rgb8_device(C.byref(cfg), DD, 0, 1, buf.ctypes.data, buf.nbytes, None),
            "rows_rgba8_device_opts": lambda: lib.fr_render_rows_rgba8_device_opts(C.byref(cfg), DD, 0, 1, buf.ctypes.data,
                                                                                   buf.nbytes, None, C.byref(opts)),
            "pixel_p": lambda: lib.fr_pixel_p(C.byref(cfg), DD, 0, 0, C.byref(px)),
            "escape_rows": lambda: lib.fr_escape_rows(C.byref(cfg), DD, 0, 1, z.ctypes.data, it.ctypes.data),
            "count": lambda: lib.fr_count_iterations(C.byref(cfg), DD, 0, 1, 1, 1, C.byref(total), C.byref(npx)),
            "rows_dd": lambda: lib.fr_render_rows_dd(C.byref(cfg), lop, 0, 1, 3, buf.ctypes.data, buf.nbytes),
            "rows_dd_rgba": lambda: lib.fr_render_rows_dd(C.byref(cfg), lop, 0, 1, 4, buf.ctypes.data, buf.nbytes),
            "rows_dd_device": lambda: lib.fr_render_rows_dd_device(C.byref(cfg), lop, 0, 1, 3, buf.ctypes.data, buf.nbytes,
                                                                   None),
            "escape_rows_dd": lambda: lib.fr_escape_rows_dd(C.byref(cfg), lop, 0, 1, z.ctypes.data, it.ctypes.data),
        }

    bad = {
        "NaN pos": cfg_with(**{"pos.re": float("nan")}),
        "inf scale": cfg_with(**{"scale.im": float("inf")}),
        "NaN exposure": cfg_with(exposure=float("nan")),
        "inf stable_limit": cfg_with(stable_limit=float("inf")),
        "NaN julia_set": cfg_with(**{"julia_set.im": float("nan")}),
        "limit 0": cfg_with(limit=0.0),
        "limit < 0": cfg_with(limit=-2.0),
        "limit > 2^500": cfg_with(limit=2.0 ** 501),
        "|pos| > 2^64": cfg_with(**{"pos.im": -(2.0 ** 65)}),
        "|julia_set| > 2^64": cfg_with(**{"julia_set.re": 2.0 ** 65}),
        "|scale| < 2^-64": cfg_with(**{"scale.re": 2.0 ** -65}),
    }
    for what, cfg in bad.items():
        for name, call in calls(cfg).items():
            assert call() == INV, (what, name)
            assert b"FR_PRECISION_DD" in lib.fr_last_error(), (what, name, lib.fr_last_error())
    # pos_lo: not normalised / not finite
    deep = cfg_with(**{"pos.im": 1.0})
    for lo in [(0.0, 2.0 ** -52), (1.0, 0.0), (0.0, float("nan")), (float("inf"), 0.0)]:
        for name, call in calls(deep, lo).items():
            if name.endswith("dd") or name.endswith("dd_rgba") or name.endswith("dd_device"):
                assert call() == INV, (lo, name)
    # channels
    for ch in (0, 1, 2, 5):
        assert lib.fr_render_rows_dd(C.byref(deep), None, 0, 1, ch, buf.ctypes.data, buf.nbytes) == INV
        assert lib.fr_render_rows_dd_device(C.byref(deep), None, 0, 1, ch, buf.ctypes.data, buf.nbytes, None) == INV
    # the row checks come first as for every precision
    assert lib.fr_render_rows_dd(C.byref(deep), None, 5, 4, 3, buf.ctypes.data, buf.nbytes) == INV
    assert lib.fr_escape_rows_dd(None, None, 0, 1, z.ctypes.data, it.ctypes.data) == INV
    assert lib.fr_render_rows_dd(C.byref(deep), None, 0, 1, 3, buf.ctypes.data, 3) == _native.FR_ERR_BUFFER_TOO_SMALL
    # multi-device, block-cyclic and the batch keep rejecting DD
    blk = C.c_uint64()
    assert lib.fr_render_rgb8_multi(C.byref(deep), DD, 8, buf.ctypes.data, buf.nbytes) == INV
    assert lib.fr_render_rgb8_multi_device(C.byref(deep), DD, 8, 0, buf.ctypes.data, buf.nbytes) == INV
    assert lib.fr_render_block_cyclic_rgb8(C.byref(deep), DD, 8, 0, 1, buf.ctypes.data, buf.nbytes, C.byref(blk)) == INV
    assert lib.fr_render_block_cyclic_rgb8_device(C.byref(deep), DD, 8, 0, 1, buf.ctypes.data, buf.nbytes, None,
                                                  C.byref(blk)) == INV
    pts = (_native.Imaginary * 1)()
    outp, outi = (_native.Imaginary * 1)(), (C.c_uint32 * 1)()
    assert lib.fr_recursive_batch(10, pts, pts, 1, 2.0, DD, outp, outi) == INV
    assert b"single-device" in lib.fr_last_error()
    # empty ranges are legal no-ops, as for F64 (this precision used to be refused outright)
    assert lib.fr_render_rows_rgb8(C.byref(deep), DD, 3, 3, None, 0) == _native.FR_OK
    assert lib.fr_render_rows_dd(C.byref(deep), None, 3, 3, 4, None, 0) == _native.FR_OK
    assert lib.fr_escape_rows_dd(C.byref(deep), C.byref(_native.Imaginary(0.0, 2.0 ** -60)), 2, 2, None, None) == _native.FR_OK


def test_valid_dd_calls_are_accepted(fr):
    """A valid DD call is not an argument error: without a device it fails with FR_ERR_NO_DEVICE like every compute call
    (with one, tests/test_gpu_dd.py checks what it computes)."""
    from fractal_renderer_amd import _native

    if fr.device_count() > 0:
        pytest.skip("a HIP device is present: tests/test_gpu_dd.py runs these calls")
    lib = _native.load()
    cfg = M.deep_view(fr.Config.new(), False, 16, 8, 20)
    buf = np.zeros(4 * 16 * 8, dtype=np.uint8)
    z = np.zeros(4 * 16 * 8, dtype=np.float64)
    it = np.zeros(16 * 8, dtype=np.uint32)
    lo = C.byref(_native.Imaginary(0.0, 2.0 ** -60))
    total = C.c_uint64()
    rcs = [
        lib.fr_render_rows_rgb8(C.byref(cfg), 2, 0, 8, buf.ctypes.data, buf.nbytes),
        lib.fr_render_rows_rgba8(C.byref(cfg), 2, 0, 8, buf.ctypes.data, buf.nbytes),
        lib.fr_pixel_p(C.byref(cfg), 2, 3, 4, C.byref(_native.RGB())),
        lib.fr_escape_rows(C.byref(cfg), 2, 0, 8, z.ctypes.data, it.ctypes.data),
        lib.fr_count_iterations(C.byref(cfg), 2, 0, 8, 1, 1, C.byref(total), None),
        lib.fr_render_rows_dd(C.byref(cfg), lo, 0, 8, 3, buf.ctypes.data, buf.nbytes),
        lib.fr_render_rows_dd(C.byref(cfg), None, 0, 8, 4, buf.ctypes.data, buf.nbytes),
        lib.fr_escape_rows_dd(C.byref(cfg), lo, 0, 8, z.ctypes.data, it.ctypes.data),
    ]
    assert rcs == [_native.FR_ERR_NO_DEVICE] * len(rcs), rcs
