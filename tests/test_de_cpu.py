"""DE, distance estimation (include/fractal_hip.h, fr_precision: "DE"), on the CPU: the model of tests/de_model.c against the
roads it rides on, against truth, and the library's refusals (which need no device).

  - road identity: the model's z and iters are pt_model's / the oracle's, bit for bit; caps 0 and 1 give the start state;
  - one derivative, two roads: where both roads' arithmetic is exact they agree in every bit, der included.  (On the shallow
    default views the two roads do NOT produce the same z on every pixel — PT's fma rounds once where recursive() rounds
    twice: 472 of 1536 pixels of the default 48 x 32 view end on the same bits — so their derivatives differ in the last
    bits there too, and no bit-for-bit statement holds on them; the figures are in the test below.);
  - truth with a closed form (Julia, c = 0: the unit circle) and by bounds (the real axis left of -2, right of 1/4);
  - a derivative that overflows: D is 0 there, no D is NaN or negative;
  - shading: thickness 0 is the colour map, capped pixels are never shaded, both branches are populated;
  - the domain, refusal by refusal, with its messages."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import colour_model as CM
import de_model as D
import oracle_lib as O
import pt_model as PTM
import pt_wide_model as W


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- road identity -----------------------------------------------------------------------------------------------------------


def _f64_views():
    out = []
    for w, h in ((40, 24), (37, 23)):
        out.append(D.default_view(O.config_new(0), w, h, 200))
        out.append(D.julia_view(O.config_new(0), w, h, 300))
    return out


def test_f64_model_is_the_oracle_bit_for_bit():
    for cfg in _f64_views():
        z, it, der = D.f64_rows(cfg)
        wz, wit = O.escape_rows(cfg)
        assert np.array_equal(it, wit) and same_bits(z, wz)
        assert np.isfinite(der).all() and (it < cfg.iterations).any()


def _pt_views():
    out = []
    for make in (PTM.early_escape_view, PTM.julia_rebase_view):
        cfg = O.config_new(0)
        out.append((cfg, make(cfg, 40, 24)))
    cfg = O.config_new(0)
    out.append((cfg, D.seahorse_shallow(cfg)))
    cfg = O.config_new(0)
    out.append((cfg, PTM.seahorse_view(cfg, 37, 23, 3000, 1e20)))  # needs pos_lo: 1e20 is past the f64 limit
    return out


def test_pt_model_is_pt_model_bit_for_bit():
    for cfg, lo in _pt_views():
        z, it, der = D.pt_rows(cfg, lo)
        wz, wit = PTM.escape_rows(cfg, lo)
        assert np.array_equal(it, wit) and same_bits(z, wz)
    # a row piece is the slice of the whole
    cfg, lo = _pt_views()[1]
    whole, piece = D.pt_rows(cfg, lo), D.pt_rows(cfg, lo, 5, 19)
    for a, b in zip(whole, piece):
        assert same_bits(a[5:19].astype(np.float64), b.astype(np.float64))


def test_pt_model_on_a_wide_centre_is_the_wide_model():
    cfg = W.view(O.config_new(0), "M", 200, 16, 12, 3000)
    orbits = W.Orbits(cfg, *W.centre_ints("M", 5), 5)
    z, it, der = D.pt_wide_rows(cfg, orbits)
    (wz, wit, _, _), _ = W.state_rows(cfg, orbits, rule=1)
    assert np.array_equal(it, wit) and same_bits(z, wz)
    assert (it < 3000).sum() >= 100 and np.isfinite(der[it < 3000]).all()


@pytest.mark.parametrize("algo", [0, 2])
def test_caps_zero_and_one_give_the_start_state(algo):
    cfg = D.julia_view(O.config_new(0), 12, 8, 0) if algo else D.default_view(O.config_new(0), 12, 8, 0)
    for rows in (D.f64_rows, D.pt_rows):
        z, it, der = rows(cfg)
        assert not it.any() and same_bits(der, np.broadcast_to([1.0, 0.0], der.shape))
        if rows is D.f64_rows:  # (start, 0, (1, 0))
            x = np.arange(12, dtype=np.float64)
            assert same_bits(z[3, :, 0], ((x / 8.0) - ((12.0 / 8.0) / 2.0)) / cfg.scale.re + cfg.pos.re)
    cfg.iterations = 1
    z, it, der = D.f64_rows(cfg)
    z0, _, _ = D.f64_rows(D.julia_view(O.config_new(0), 12, 8, 0) if algo else D.default_view(O.config_new(0), 12, 8, 0))
    want = np.stack([z0[..., 0] + z0[..., 0] + (0.0 if algo else 1.0), z0[..., 1] + z0[..., 1]], -1)  # 2 z0 * 1 + b0, exact
    assert same_bits(der, want)
    assert set(np.unique(it)) <= {0, 1}


# ---- one derivative, two roads -----------------------------------------------------------------------------------------------


def test_where_both_roads_are_exact_they_agree_in_every_bit():
    """pos = 0, scale = 1/4, height = 16: every coordinate is a multiple of 2^-2 below 2^2 (5 bits), so through three steps
    every product and sum of both roads is exact (z3 has at most 40 bits, d3 at most 36): PT's fma and recursive()'s separate
    roundings give the same numbers, the z sequences coincide, and so must the derivatives."""
    for algo in (0, 2):
        cfg = O.config_new(0)
        cfg.algo = algo
        cfg.width, cfg.height, cfg.iterations = 24, 16, 3
        cfg.scale.re = cfg.scale.im = 0.25
        cfg.julia_set.re, cfg.julia_set.im = -0.75, 0.125
        cfg.limit = 4.0
        f, p = D.f64_rows(cfg), D.pt_rows(cfg)
        assert np.array_equal(f[1], p[1]) and same_bits(f[0], p[0]), "the premise: the same z on every pixel"
        assert same_bits(f[2], p[2])
        assert len(np.unique(f[1])) >= 3 and (f[2] != [1.0, 0.0]).any(-1).sum() > f[1].size // 2


def test_on_the_shallow_default_view_the_roads_differ_in_the_last_bits():
    """Measured, not required: the default view at 48 x 32 and 200 iterations, F64 against PT.  472 pixels ended on the same z
    bits and 738 on the same der bits when this was written.  What holds is that the roads agree on most escape indices (two
    arithmetics for one orbit) — so a bit-for-bit comparison of der across the roads is not a property of the definition."""
    cfg = D.default_view(O.config_new(0))
    f, p = D.f64_rows(cfg), D.pt_rows(cfg)
    same_z = (bits(f[0]) == bits(p[0])).all(-1)
    same_der = (bits(f[2]) == bits(p[2])).all(-1)
    print("same z: %d, same der: %d of %d" % (same_z.sum(), same_der.sum(), same_z.size))
    assert 0 < same_z.sum() < same_z.size
    assert int((f[1] != p[1]).sum()) <= f[1].size // 50


# ---- truth -------------------------------------------------------------------------------------------------------------------


def _coords(cfg):
    """the pixels' f64 coordinates, with coord_to_space's operations"""
    w, h = float(cfg.width), float(cfg.height)
    re = ((np.arange(cfg.width, dtype=np.float64) / h) - ((w / h) / 2.0)) / cfg.scale.re + cfg.pos.re
    im = ((np.arange(cfg.height, dtype=np.float64) / h) - 0.5) / cfg.scale.im + cfg.pos.im
    return re, im


def test_the_unit_circle_has_a_closed_form():
    """Julia, c = 0: z_n = z_0^(2^n) and d_n = 2^n z_0^(2^n - 1), so |z_n| ln|z_n| / |d_n| = |z_0| ln|z_0| whatever n is.
    16 squarings each at most double the relative error and add 2^-52: 2^-28 leaves 16 x room."""
    import mpmath

    cfg = D.unit_circle_view(O.config_new(0))
    z, it, der = D.f64_rows(cfg)
    dist = D.distance(cfg, z, it, der)
    re, im = _coords(cfg)
    checked = 0
    with mpmath.workprec(200):
        for y in range(cfg.height):
            for x in range(cfg.width):
                r0 = mpmath.sqrt(mpmath.mpf(re[x]) ** 2 + mpmath.mpf(im[y]) ** 2)
                if r0 < mpmath.mpf("1.001") or it[y, x] >= cfg.iterations:
                    continue
                want = r0 * mpmath.log(r0)
                got = mpmath.mpf(dist[y, x]) / (mpmath.mpf(cfg.height) * mpmath.mpf(cfg.scale.re))
                assert abs(got - want) <= want * mpmath.mpf(2) ** -28, (x, y, got, want)
                checked += 1
    assert checked >= 500


def test_the_real_axis_bounds_the_estimate():
    """Mandelbrot, row height / 2 (im = 0 exactly).  Left of -2 the nearest point of the set is -2, so the true distance is
    -2 - re, and true / D lies strictly inside (1/2, 2) (at an antenna's tip Koebe's lower bound is nearly attained: 0.50 to
    0.52 here).  Right of 1/4 the distance to the cusp, re - 1/4, is NOT the true distance: the cardioid's lobes close in on
    the axis there (near the cusp the boundary is y^2 = 4 (x - 1/4)^3, so at re = 0.26 the set is 0.002 away, not 0.01), and
    (re - 1/4) / D was measured between 1.0 and 11.  What is known in closed form is the main cardioid, a subset of the set:
    its distance d_c bounds the true one from above, so d_c / D > 1/2 is the half of the statement that can be checked."""
    cfg = O.config_new(0)
    cfg.width, cfg.height, cfg.iterations = 48, 32, 1000
    cfg.pos.re = -0.6
    z, it, der = D.f64_rows(cfg)
    dist = D.distance(cfg, z, it, der)
    re, im = _coords(cfg)
    y = cfg.height // 2
    assert im[y] == 0.0
    px = cfg.height * cfg.scale.re
    left, right = re < -2.0, re > 0.25
    assert left.sum() >= 5 and right.sum() >= 10 and (it[y][left | right] < cfg.iterations).all()
    ratio = (-2.0 - re[left]) * px / dist[y][left]
    assert ((ratio > 0.5) & (ratio < 2.0)).all(), ratio
    t = np.linspace(-np.pi, np.pi, 400001)
    cardioid = np.exp(1j * t) / 2 - np.exp(2j * t) / 4
    d_c = np.array([np.abs(cardioid - r).min() for r in re[right]])
    assert (d_c * px / dist[y][right] > 0.5).all() and (d_c <= re[right] - 0.25 + 1e-12).all()


# ---- a derivative that overflows -----------------------------------------------------------------------------------------------


def misiurewicz_i(cfg, width=40, height=24, iterations=3000):
    """Mandelbrot centred on c = i with even sides: the centre pixel IS c = i, whose orbit i, -1 + i, -i, -1 + i, ... is exact
    in f64 and never escapes, while its derivative grows by |2 (-1 + i)| |2 i| = 5.66 every two steps: past 2^1024 after some
    800 steps."""
    cfg.algo = 0
    cfg.width, cfg.height, cfg.iterations = width, height, iterations
    cfg.limit = 2.0
    cfg.pos.re, cfg.pos.im = 0.0, 1.0
    cfg.scale.re = cfg.scale.im = 1e3
    return cfg


@pytest.mark.parametrize("road", ["f64", "pt"])
def test_a_derivative_that_overflows_gives_distance_zero(road):
    """The seahorse-valley views of the PT tests do not get there: their orbits linger near a parabolic cycle and |d| reaches
    1e29 at a cap of 3000 (measured with this model at scales 1e6 to 1e20), far from 2^1024.  The view on c = i does."""
    cfg = misiurewicz_i(O.config_new(0))
    z, it, der = D.f64_rows(cfg) if road == "f64" else D.pt_rows(cfg)
    dist = D.distance(cfg, z, it, der)
    bad = ~np.isfinite(der).all(-1)
    assert bad.sum() >= 1, "the case has vanished: no derivative overflowed"
    assert (dist[bad] == 0.0).all()
    assert not np.isnan(dist).any() and not (dist < 0.0).any()
    assert (it < cfg.iterations).sum() >= 900 and np.isfinite(der[it < cfg.iterations]).all()


def test_seahorse_distances_are_never_nan_or_negative():
    cfg = O.config_new(0)
    lo = D.seahorse_shallow(cfg)
    for z, it, der in (D.pt_rows(cfg, lo), D.f64_rows(cfg)):
        dist = D.distance(cfg, z, it, der)
        assert not np.isnan(dist).any() and not (dist < 0.0).any() and (dist[it == cfg.iterations] == 0.0).all()
        assert (it == cfg.iterations).sum() >= 50 and (dist > 0.0).sum() >= 500


def test_distance_special_values():
    cfg = D.default_view(O.config_new(0))
    z = np.array([[3.0, 4.0]] * 6)
    der = np.array([[0.0, 0.0], [np.inf, 1.0], [np.nan, 1.0], [1e200, 1e200], [3.0, 4.0], [-3.0, 0.0]])
    it = np.array([1, 1, 1, 1, 200, 1], dtype=np.uint32)
    dist = D.distance(cfg, z, it, der)
    assert dist[0] == np.inf and (dist[1:5] == 0.0).all()  # d == 0: nothing near; inf, NaN, dn2 overflow, capped
    want = (5.0 * math.log(5.0) / 3.0) * (32 * 0.4)
    assert abs(dist[5] - want) <= want * 2.0 ** -50


# ---- shading -------------------------------------------------------------------------------------------------------------------


def test_shading_on_the_default_view():
    cfg = D.default_view(O.config_new(0))
    z, it, der = D.f64_rows(cfg)
    dist = D.distance(cfg, z, it, der)
    escaped = it < cfg.iterations
    below, above = escaped & (dist < 2.0), escaped & ~(dist < 2.0)
    assert below.sum() >= 100 and above.sum() >= 100 and (~escaped).sum() >= 100  # 313, 969 and 254 when this was written
    plain = D.colour(cfg, z, it, der, 0.0)
    assert np.array_equal(plain, D.base_colours(cfg, z, it))
    shaded = D.colour(cfg, z, it, der, 2.0)
    assert np.array_equal(shaded[~below], plain[~below]), "capped pixels and pixels at or beyond the thickness are unshaded"
    s = dist[below] / 2.0
    want = (plain[below].astype(np.float64) * s[:, None]).astype(np.uint8)  # 0 <= byte * s < 255: astype truncates
    assert np.array_equal(shaded[below], want) and (shaded[below] <= plain[below]).all()
    assert (shaded[below] != plain[below]).any(-1).sum() >= 100
    rgba = D.colour(cfg, z, it, der, 2.0, channels=4)
    assert np.array_equal(rgba[..., :3], shaded) and (rgba[..., 3] == 255).all()


def test_thickness_zero_is_the_colour_model():
    """where tests/colour_model.py's filter decides a pixel's bytes, they are the model's at thickness 0"""
    cfg = D.default_view(O.config_new(0))
    z, it, der = D.f64_rows(cfg)
    plain = D.colour(cfg, z, it, der, 0.0)
    c = CM.Consts(cfg.iterations, cfg.exposure, (cfg.primary_color.r, cfg.primary_color.g, cfg.primary_color.b), cfg.stable_limit)
    decided = 0
    for y in range(0, cfg.height, 3):
        for x in range(cfg.width):
            dist = z[y, x, 0] * z[y, x, 0] + z[y, x, 1] * z[y, x, 1]
            if not dist > cfg.stable_limit:
                continue
            how, b = CM.road(c, dist, int(it[y, x]))
            if b is not None:
                decided += 1
                assert tuple(plain[y, x]) == tuple(b), (x, y, how)
    assert decided >= 200


# ---- the domain: every refusal, by message, with no device ---------------------------------------------------------------------


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


INVALID, TOO_SMALL = 1, 2


def refused(lib, rc, *words):
    msg = lib.fr_last_error().decode()
    assert rc == INVALID, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_constants(fr):
    from fractal_renderer_amd import _native

    assert (_native.FR_ERR_INVALID_ARGUMENT, _native.FR_ERR_BUFFER_TOO_SMALL) == (INVALID, TOO_SMALL)


def test_escape_rows_de_refusals(fr, lib):
    cfg = fr.Config.new()
    cfg.width, cfg.height = 8, 6
    z, der = np.zeros((6, 8, 2)), np.zeros((6, 8, 2))
    it = np.zeros((6, 8), dtype=np.uint32)
    arrays = (z.ctypes.data, it.ctypes.data, der.ctypes.data)
    lo = fr.Imaginary(0.0, 0.0)
    for form, tail in ((lib.fr_escape_rows_de, ()), (lib.fr_escape_rows_de_device, (None,))):
        for precision in (1, 2, 7):  # F32, DD, nonsense
            refused(lib, form(C.byref(cfg), precision, None, 0, 6, *arrays, *tail), "FR_PRECISION_F32", "FR_PRECISION_DD", "BLA-PT",
                    "SCALED PT", "block-cyclic", "multi-device", "supersampling", "fr_pixel", "raising a DE view's cap")
        refused(lib, form(C.byref(cfg), 0, C.byref(lo), 0, 6, *arrays, *tail), "pos_lo", "F64 road takes none")
        refused(lib, form(C.byref(cfg), 0, None, 4, 2, *arrays, *tail), "y0 > y1")
        refused(lib, form(C.byref(cfg), 0, None, 0, 7, *arrays, *tail), "y1 > height")
        refused(lib, form(None, 0, None, 0, 6, *arrays, *tail), "cfg is NULL")
        for k in range(3):
            a = list(arrays)
            a[k] = None
            refused(lib, form(C.byref(cfg), 0, None, 0, 6, *a, *tail), "all three")
        refused(lib, form(C.byref(cfg), 0, None, 0, 6, arrays[0] + 4, arrays[1], arrays[2], *tail), "8-byte aligned")
        refused(lib, form(C.byref(cfg), 0, None, 0, 6, arrays[0], arrays[1] + 2, arrays[2], *tail), "4-byte aligned")
        refused(lib, form(C.byref(cfg), 0, None, 0, 6, arrays[0], arrays[1], arrays[2] + 4, *tail), "8-byte aligned")
        for precision in (0, 3):
            big = fr.Config.from_buffer_copy(bytes(cfg))
            # PT's own domain speaks first about a limit that is not finite
            for limit in (2.0 ** 20 * (1 + 2.0 ** -52), 2.0 ** 21) + ((float("inf"), float("nan")) if precision == 0 else ()):
                big.limit = limit
                refused(lib, form(C.byref(big), precision, None, 0, 6, *arrays, *tail), "limit must be <= 2^20")
            big.limit = 2.0 ** 20
            assert form(C.byref(big), precision, None, 3, 3, None, None, None, *tail) == 0  # y0 == y1: a no-op without a device
        # the road's own domain: PT's
        pt = fr.Config.from_buffer_copy(bytes(cfg))
        pt.iterations = (1 << 24) + 1
        refused(lib, form(C.byref(pt), 3, None, 0, 6, *arrays, *tail), "FR_PRECISION_PT", "FR_PT_MAX_ITERATIONS")
        pt.iterations, pt.scale.re = 50, 2.0 ** -65
        refused(lib, form(C.byref(pt), 3, None, 0, 6, *arrays, *tail), "FR_PRECISION_PT", "|scale|")
        off = fr.Imaginary(1.0, 0.0)
        pt.scale.re = 0.4
        pt.pos.re = 1.0
        refused(lib, form(C.byref(pt), 3, C.byref(off), 0, 6, *arrays, *tail), "pos_lo is not normalised")


def test_wide_centre_refusals(fr, lib):
    from fractal_renderer_amd import _native

    cfg = W.view(fr.Config.new(), "M", 200, 8, 6, 100)
    ints = W.centre_ints("M", 9)
    words = W.to_words(ints[0], 9), W.to_words(ints[1], 9)
    p64 = C.POINTER(C.c_uint64)
    centre = _native.fr_wide_centre(9, words[0].ctypes.data_as(p64), words[1].ctypes.data_as(p64))
    z, der = np.zeros((6, 8, 2)), np.zeros((6, 8, 2))
    it = np.zeros((6, 8), dtype=np.uint32)
    arrays = (z.ctypes.data, it.ctypes.data, der.ctypes.data)
    for form, tail in ((lib.fr_escape_rows_de_pt_wide, ()), (lib.fr_escape_rows_de_pt_wide_device, (None,))):
        refused(lib, form(C.byref(cfg), None, 0, 6, *arrays, *tail), "centre is NULL")
        deep = fr.Config.from_buffer_copy(bytes(cfg))
        deep.scale.re = deep.scale.im = 2.0 ** 441
        refused(lib, form(C.byref(deep), C.byref(centre), 0, 6, *arrays, *tail), "2^440")
        deep.scale.re = deep.scale.im = 2.0 ** 440
        deep.limit = 2.0 ** 21
        refused(lib, form(C.byref(deep), C.byref(centre), 0, 6, *arrays, *tail), "limit must be <= 2^20")
        deep.limit = 2.0
        refused(lib, form(C.byref(deep), C.byref(centre), 0, 6, arrays[0], None, arrays[2], *tail), "all three")
        assert form(C.byref(deep), C.byref(centre), 2, 2, None, None, None, *tail) == 0


def test_distance_and_colour_refusals(fr, lib):
    cfg = fr.Config.new()
    n = 12
    z, der, out = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n)
    it = np.zeros(n, dtype=np.uint32)
    rgb = np.zeros(4 * n + 4, dtype=np.uint8)
    zp, ip, dp = z.ctypes.data, it.ctypes.data, der.ctypes.data
    for form, tail in ((lib.fr_distance_rows, ()), (lib.fr_distance_rows_device, (None,))):
        refused(lib, form(None, zp, ip, dp, n, out.ctypes.data, *tail), "cfg is NULL")
        refused(lib, form(C.byref(cfg), zp, ip, dp, (1 << 40) + 1, out.ctypes.data, *tail), "2^40")
        refused(lib, form(C.byref(cfg), None, ip, dp, n, out.ctypes.data, *tail), "all three")
        refused(lib, form(C.byref(cfg), zp, ip, None, n, out.ctypes.data, *tail), "all three")
        refused(lib, form(C.byref(cfg), zp, ip + 2, dp, n, out.ctypes.data, *tail), "aligned")
        refused(lib, form(C.byref(cfg), zp, ip, dp, n, None, *tail), "out is NULL")
        assert form(C.byref(cfg), None, None, None, 0, None, *tail) == 0  # n == 0 needs no device
    refused(lib, lib.fr_distance_rows_device(C.byref(cfg), zp, ip, dp, n, out.ctypes.data + 4, None), "8-byte aligned")
    for t in (-1.0, -2.0 ** -1074, 2.0 ** 20 * (1 + 2.0 ** -52), float("inf"), float("nan")):
        refused(lib, lib.fr_colour_de_rows_device(C.byref(cfg), zp, ip, dp, n, t, 3, rgb.ctypes.data, None), "thickness")
        refused(lib, lib.fr_colour_de_rgb8(C.byref(cfg), zp, ip, dp, n, t, rgb.ctypes.data, rgb.nbytes), "thickness")
    refused(lib, lib.fr_colour_de_rows_device(C.byref(cfg), zp, ip, dp, n, 1.0, 5, rgb.ctypes.data, None), "channels")
    base = rgb.ctypes.data + (-rgb.ctypes.data) % 4
    refused(lib, lib.fr_colour_de_rows_device(C.byref(cfg), zp, ip, dp, n, 1.0, 4, base + 1, None), "RGBA8 output must be 4-byte aligned")
    refused(lib, lib.fr_colour_de_rows_device(C.byref(cfg), zp, ip, dp, n, 1.0, 3, None, None), "d_out is NULL")
    refused(lib, lib.fr_colour_de_rows_device(C.byref(cfg), zp, None, dp, n, 1.0, 3, rgb.ctypes.data, None), "all three")
    assert lib.fr_colour_de_rgb8(C.byref(cfg), zp, ip, dp, n, 1.0, rgb.ctypes.data, 3 * n - 1) == TOO_SMALL
    assert lib.fr_colour_de_rows_device(C.byref(cfg), None, None, None, 0, 0.0, 3, None, None) == 0
    assert lib.fr_colour_de_rgb8(C.byref(cfg), None, None, None, 0, 2.0 ** 20, None, 0) == 0


def test_python_refusals(fr):
    cfg = fr.Config.new()
    cfg.width, cfg.height = 8, 6
    for precision in (fr.Precision.F32, fr.Precision.DD):
        with pytest.raises(fr.FractalHipError) as e:
            fr.escape_rows_de(cfg, precision=precision)
        assert e.value.code == INVALID and "out of scope" in str(e.value)
    with pytest.raises(fr.FractalHipError) as e:
        fr.get_image_de(cfg, pos_lo=(0.0, 0.0))
    assert "pos_lo" in str(e.value)
    with pytest.raises(ValueError):
        fr.escape_rows_de(cfg, precision=fr.Precision.F64, centre=fr.WideCentre(2))  # centre= needs Precision.PT
    with pytest.raises(ValueError):
        fr.colour_image_de(cfg, np.zeros((6, 8, 2)), np.zeros((6, 8), dtype=np.uint32), np.zeros((6, 8, 3)), 1.0)
    z, it, der = fr.escape_rows_de(cfg, 2, 2)  # no rows: no device
    assert z.shape == (0, 8, 2) and it.shape == (0, 8) and der.shape == (0, 8, 2)


def test_cli_refusals():
    from test_cpp_host import CLI_EXE, build_cli

    build_cli()
    for args, msg in [(["--perturbation", "--bla"], "does not combine with --bla"),
                      (["--perturbation", "--scaled"], "does not combine with --scaled"),
                      (["--supersample", "2"], "does not combine with --supersample"),
                      (["--f32"], "does not combine with --f32"),
                      (["--devices", "0"], "does not combine with --devices"),
                      (["--auto-exposure"], "does not combine with --auto-exposure"),
                      (["-a", "fern"], "does not apply to -a fern")]:
        r = subprocess.run([CLI_EXE, "--distance-shade", "2"] + args + ["64", "48"], capture_output=True, text=True)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr)
    r = subprocess.run([CLI_EXE, "--distance-shade"], capture_output=True, text=True)
    assert r.returncode == 2 and "missing value" in r.stderr
    # --supersample 1 is no supersampling: accepted as far as the device
    r = subprocess.run([CLI_EXE, "--distance-shade", "-1", "--supersample", "1", "8", "6", "-o", "/dev/null"], capture_output=True, text=True)
    assert r.returncode == 1 and ("thickness" in r.stderr or "no HIP device" in r.stderr), r.stderr
