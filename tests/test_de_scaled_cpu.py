"""DE ON SCALED PT without a device (include/fractal_hip.h, "DE ON SCALED PT"): the model of tests/de_scaled_model.c against the
models it rides on and against exact derivatives, and the library's refusals (which need no device).

  - CLAIM 1 in the models: z, iters and passes are pt_scaled_model's bit for bit, for bits -1, 40 and 53, inside WIDE PT's domain
    and past it;
  - CLAIM 2 in the models: in the common domain no intermediate of the u chain is subnormal, u 2^e is de_model's PT derivative
    (bits = -1) and de_bla_model's (bits 40 and 53) bit for bit, and the distance on the scaled view is theirs on the view;
  - accuracy: D over the model's arrays against the exact distance (tests/de_scaled_truth.py, the fixture
    tests/golden/de_scaled_truth.npz), on deep_truth's PAST and WIDE_DOMAIN views, within 4 x the measured worst per bits;
  - the table form against the plain form past 2^440, by DESIGN.md 3.22's recipe;
  - caps 0 to 3; an algorithm without orbits; the range of the u chain past 2^440;
  - the domain, refusal by refusal, in host and device form; y0 == y1 with NULL arrays; fr_de_scaled_view; the Python keywords;
    the header's paragraph."""
import ctypes as C
import math

import numpy as np
import pytest

import bla_model as B
import de_bla_model as DB
import de_model as D
import de_scaled_model as M
import de_scaled_truth as U
import deep_truth as T
import oracle_lib as O
import pt_scaled_model as S
import pt_wide_model as W

INVALID = 1
BITS = (-1, 40, 53)


def new_config():
    return O.config_new(0)


_views = {}


def view(spec):
    """the model tests' own Views, on the oracle's Config type"""
    if spec not in _views:
        _views[spec] = S.View(new_config, spec)
    return _views[spec]


class TruthView:
    """one of deep_truth's views with its config and orbits from the models' own code: what de_scaled_model.model takes"""

    def __init__(self, name, cap=None):
        self.v = v = T.view(name)
        self.cfg = v.fill(new_config(), cap)
        self.orbits = W.Orbits(self.cfg, *v.ints, v.n)
        self.x = self.orbits.x[0]
        self.k = self.orbits.k[0] if v.julia else None
        self.shape = v.shape


_truth_views = {}


def truth_view(name):
    if name not in _truth_views:
        _truth_views[name] = TruthView(name)
    return _truth_views[name]


def scaled_distance(cfg, z, it, der):
    return D.distance(M.scaled_view(cfg), z, it, der)


# ---- CLAIM 1: the derivative only reads --------------------------------------------------------------------------------------

CLAIM_1 = {"M_200": S.M_200, "M_440": S.M_440, "N_300": S.N_300, "J_300": S.J_300, "M_900": S.M_900, "N_900": S.N_900,
           "J_900": S.J_900, "MINI_861": S.MINI_861}


@pytest.mark.parametrize("name", list(CLAIM_1))
def test_z_iters_and_passes_are_the_scaled_models(name):
    v = view(CLAIM_1[name])
    for bits in BITS:
        z, it, der, passes, skips, _ = M.model(v, bits)
        wz, wit, wpasses, _ = v.model(bits)
        assert np.array_equal(it, wit) and S.same_bits(z, wz) and np.array_equal(passes, wpasses), (name, bits)
        assert (skips <= passes).all() and (bits >= 0 or not skips.any())
        escaped = it < v.cfg.iterations
        assert np.isfinite(der[escaped]).all() and (der[escaped] != 0.0).any(-1).all()


# ---- CLAIM 2: the common domain ------------------------------------------------------------------------------------------------

COMMON = {"M_200": S.M_200, "M_300": S.M_300, "N_300": S.N_300, "J_300": S.J_300, "M_440": S.M_440}


def common_view(name):
    return view(COMMON[name]) if name in COMMON else truth_view(name)


@pytest.mark.parametrize("name", list(COMMON) + ["M_OFF_299", "J_OFF_300"])
def test_in_the_common_domain_u_is_the_unscaled_derivative_scaled(name):
    v = common_view(name)
    e = S.exponent(v.cfg)
    for bits in BITS:
        z, it, u, passes, skips, (lo, hi, sub) = M.model(v, bits)
        assert not sub, (name, bits, lo)
        if bits < 0:
            wz, wit, wd = D.pt_rows_on(v.cfg, v.x, v.k)
        else:
            wz, wit, wd, _, _ = DB.escape_rows(v.cfg, v.x, v.k, bits)
        assert np.array_equal(it, wit) and S.same_bits(z, wz), (name, bits)
        assert np.isfinite(wd).all(), "no overflow in the unscaled run"
        assert D.same_doubles(np.ldexp(u, e), wd), (name, bits)
        assert D.same_doubles(scaled_distance(v.cfg, z, it, u), D.distance(v.cfg, wz, wit, wd)), (name, bits)


# ---- accuracy against exact derivatives ------------------------------------------------------------------------------------------


def test_the_fixture_holds_every_view_and_is_what_the_integers_give():
    for name in U.VIEWS:
        t, tu, v = T.load(name), U.load(name), T.view(name)
        assert tu["iters"].shape == v.shape and tu["u"].shape == v.shape + (2,) and tu["u"].dtype == np.float64
        assert tuple(tu["precision"]) == (v.P, v.P + T.EXTRA)
        assert np.array_equal(tu["iters"], t["iters"])
        for x, y in T.sample_pixels(t)[:3]:
            want = (int(tu["iters"][y, x]), tuple(tu["u"][y, x]))
            for extra in (0, T.EXTRA):
                assert U.pixel(name, x, y, extra) == want, (name, x, y, extra)


_measured = {}


@pytest.mark.parametrize("name", U.VIEWS)
def test_distance_against_exact_derivatives(name):
    v = truth_view(name)
    for bits in BITS:
        z, it, u, passes, skips, _ = M.model(v, bits)
        compared, size, worst = U.compare(name, M.scaled_view(v.cfg), D.distance, z, it, u)
        _measured[name, bits] = worst
        print("%s, bits %d: %d of %d pixels compared (%.0f %%), worst relative error of D %.4g"
              % (name, bits, compared, size, 100.0 * compared / size, worst))
        assert compared >= U.MIN_COMPARED * size, "the compared pixels are less than half of the image"
        assert worst <= U.D_TOLERANCE[bits], (name, bits, worst)


def test_the_tolerances_are_four_times_the_measured_worst():
    for bits in BITS:
        assert U.D_TOLERANCE[bits] == U.tolerance_for(U.D_ERROR_MEASURED[bits]), bits
        got = [w for (n, b), w in _measured.items() if b == bits]
        if len(got) == len(U.VIEWS):  # the whole file ran: the constant is what this machine measures, within a factor of 2
            print("bits %d: measured %.4g, recorded %.4g" % (bits, max(got), U.D_ERROR_MEASURED[bits]))
            assert max(got) <= 2.0 * U.D_ERROR_MEASURED[bits] and U.D_ERROR_MEASURED[bits] <= 2.0 * max(got)


# ---- the table form against the plain form, past 2^440 (DESIGN.md 3.22's recipe) -----------------------------------------------------

# The worst |D_table - D_plain| / D_plain over the compared pixels (equal iters, D_plain >= 2^-10 pixels) that the model gave at
# the default 40 bits when this was written; the tolerance is 4 x that at 40 and at 53 bits.  bits = 24 is outside it by its own
# eps = 2^-24 and is recorded only (printed with -s; DESIGN.md 3.24 carries the table).
MEASURED_40 = {"M_900": 4.068e-10, "J_900": 6.662e-10, "MINI_861": 1.268e-10, "MINI_OFF_860": 7.739e-11}
FACTOR = 4.0


@pytest.mark.parametrize("name", list(MEASURED_40))
def test_the_table_form_against_the_plain_form(name):
    v = truth_view(name)
    pz, pit, pu, _, _, _ = M.model(v, -1)
    d_plain = scaled_distance(v.cfg, pz, pit, pu)
    for bits in (40, 53, 24):
        z, it, u, passes, skips, _ = M.model(v, bits)
        d_table = scaled_distance(v.cfg, z, it, u)
        same = it == pit
        compared = same & (d_plain >= 2.0 ** -10)
        ratio = np.abs(d_table - d_plain)[compared] / d_plain[compared]
        print("%s, %d bits: %d of %d pixels compared, worst %.4g; escaped pixels that skipped: %d"
              % (name, bits, compared.sum(), it.size, ratio.max(), ((it < v.cfg.iterations) & (skips > 0)).sum()))
        if bits == 24:
            continue
        assert ((it < v.cfg.iterations) & (skips > 0)).sum() >= 1, "a view whose escaped pixels never skip checks no skipped derivative"
        assert 2 * int(compared.sum()) >= it.size, "the compared pixels are less than half of the image"
        assert ratio.max() < FACTOR * MEASURED_40[name], (name, bits, ratio.max())


# ---- caps 0 to 3, no orbits, the range --------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["M_900", "J_900", "MINI_861", "M_440", "J_300"])
@pytest.mark.parametrize("cap", [0, 1, 2, 3])
def test_small_caps(name, cap):
    """the table has no level to skip with while the orbit has at most 3 entries — caps 0 and 1 for Mandelbrot, 0 to
    2 for Julia.  There all three arrays are the plain form's bit for bit; at the caps above that the statement is made for the
    pixels that took no skip, and claim 1 for all."""
    base = view(getattr(S, name))
    cfg = type(base.cfg).from_buffer_copy(bytes(base.cfg))
    cfg.iterations = cap
    orbits = W.Orbits(cfg, *base.ints, base.n)
    x, k = orbits.x[0], orbits.k[0] if cfg.algo == 2 else None
    pz, pit, pu, _, _, _ = M.escape_rows(cfg, x, k, -1)
    z, it, u, passes, skips, _ = M.escape_rows(cfg, x, k, 40)
    sz, sit, _, _ = S.escape_rows(cfg, x, k, 40)
    assert np.array_equal(it, sit) and S.same_bits(z, sz)
    no_levels = all(len(o) - 1 <= 2 for o in (x, k) if o is not None)
    assert no_levels == (cap <= (2 if cfg.algo == 2 else 1))
    if no_levels:
        assert not skips.any()
    plain = skips == 0
    print("%s at cap %d: %d of %d pixels skipped" % (name, cap, int((~plain).sum()), plain.size))
    assert np.array_equal(it[plain], pit[plain]) and S.same_bits(z[plain], pz[plain]) and D.same_doubles(u[plain], pu[plain])
    if cap == 0:  # (start, 0, (Sinv, 0))
        sinv = math.ldexp(1.0, -S.exponent(cfg))
        assert not it.any() and S.same_bits(u, np.broadcast_to([sinv, 0.0], u.shape))
        assert S.same_bits(z, S.escape_rows(cfg, x, k, -1)[0])


def test_an_algorithm_without_orbits_gives_zeros():
    cfg = O.config_new(1)
    cfg.width, cfg.height, cfg.iterations = 9, 5, 50
    cfg.scale.re = cfg.scale.im = 2.0 ** 900
    for bits in (-1, 40):
        for a in M.escape_rows(cfg, bits=bits)[:5]:
            assert not a.any()


@pytest.mark.parametrize("name", T.PAST)
def test_the_u_chain_stays_normal_past_2_440(name):
    """claim 3 on the test views: no intermediate of the u chain is subnormal and none is near 2^512 on an escaped pixel"""
    v = truth_view(name)
    for bits in BITS:
        z, it, u, passes, skips, (lo, hi, sub) = M.model(v, bits)
        print("%s, bits %d: the u chain lies in [2^%.1f, 2^%.1f]" % (name, bits, math.log2(lo), math.log2(hi)))
        assert not sub and lo >= 2.0 ** -1022
        escaped = it < v.cfg.iterations
        assert (np.abs(u[escaped]) < 2.0 ** 500).all()


# ---- the domain: every refusal, by message, with no device ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def fr():
    import __graft_entry__ as ge

    ge.build()
    import fractal_renderer_amd

    return fractal_renderer_amd


@pytest.fixture(scope="module")
def native(fr):
    from fractal_renderer_amd import _native

    return _native


@pytest.fixture(scope="module")
def lib(native):
    return native.load()


def refused(lib, rc, *words):
    msg = lib.fr_last_error().decode()
    assert rc == INVALID, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def domain_view(fr, native, scale_log2, n=16):
    cfg = W.view(fr.Config.new(), "M", scale_log2, 16, 12, 100)
    re, im = W.centre_ints("M", n)
    words = W.to_words(re, n), W.to_words(im, n)
    p64 = C.POINTER(C.c_uint64)
    st = native.fr_wide_centre(n, words[0].ctypes.data_as(p64), words[1].ctypes.data_as(p64))
    return cfg, st, words


def test_refusals_need_no_device(fr, native, lib):
    cfg, st, _words = domain_view(fr, native, 900)
    centre = C.byref(st)
    h, w = cfg.height, cfg.width
    z, der = np.zeros((h, w, 2)), np.zeros((h, w, 2))
    it = np.zeros((h, w), dtype=np.uint32)
    arrays = (z.ctypes.data, it.ctypes.data, der.ctypes.data)
    for form, tail in ((lib.fr_escape_rows_de_pt_scaled, ()), (lib.fr_escape_rows_de_pt_scaled_device, (None,))):
        refused(lib, form(None, centre, -1, 0, h, *arrays, *tail), "cfg is NULL")
        refused(lib, form(C.byref(cfg), None, -1, 0, h, *arrays, *tail), "SCALED PT", "centre is NULL")
        refused(lib, form(C.byref(cfg), centre, -1, 5, 4, *arrays, *tail), "y0 > y1")
        refused(lib, form(C.byref(cfg), centre, -1, 0, h + 1, *arrays, *tail), "y1 > height")
        for bits in (23, 54, -2):
            refused(lib, form(C.byref(cfg), centre, bits, 0, h, *arrays, *tail), "SCALED PT", "bits", "24 .. 53")
        for k in range(3):
            a = list(arrays)
            a[k] = None
            for bits in (-1, 0):
                refused(lib, form(C.byref(cfg), centre, bits, 0, h, *a, *tail), "all three")
        refused(lib, form(C.byref(cfg), centre, -1, 0, h, arrays[0] + 4, arrays[1], arrays[2], *tail), "8-byte aligned")
        refused(lib, form(C.byref(cfg), centre, -1, 0, h, arrays[0], arrays[1] + 2, arrays[2], *tail), "4-byte aligned")
        refused(lib, form(C.byref(cfg), centre, 0, 0, h, arrays[0], arrays[1], arrays[2] + 4, *tail), "8-byte aligned")
        big = fr.Config.from_buffer_copy(bytes(cfg))
        for limit in (2.0 ** 20 * (1 + 2.0 ** -52), 2.0 ** 21):
            big.limit = limit
            refused(lib, form(C.byref(big), centre, -1, 0, h, *arrays, *tail), "limit", "2^20")
        big.limit = 2.0 ** 20
        assert form(C.byref(big), centre, -1, 3, 3, None, None, None, *tail) == 0
        # F >= e + 64: 15 words are too coarse for 2^900, and 2^952 is too deep for any centre
        c15, st15, _w15 = domain_view(fr, native, 900, n=15)
        refused(lib, form(C.byref(c15), C.byref(st15), -1, 0, h, *arrays, *tail), "too coarse", "e + 64")
        deep = fr.Config.from_buffer_copy(bytes(cfg))
        deep.scale.re = deep.scale.im = math.ldexp(1.0, 952)
        refused(lib, form(C.byref(deep), centre, 0, 0, h, *arrays, *tail), "e + 64")
        for axis in ("re", "im"):  # the 2^-32 axis ratio
            thin = fr.Config.from_buffer_copy(bytes(cfg))
            setattr(thin.scale, axis, math.ldexp(-1.0, 900 - 33))
            refused(lib, form(C.byref(thin), centre, -1, 0, h, *arrays, *tail), "2^-32")
        many = fr.Config.from_buffer_copy(bytes(cfg))
        many.iterations = (1 << 24) + 1
        refused(lib, form(C.byref(many), centre, -1, 0, h, *arrays, *tail), "FR_PT_MAX_ITERATIONS")
        # refusals come before the no-rows shortcut; a legal call without rows needs neither arrays nor a device
        refused(lib, form(C.byref(cfg), centre, 23, 2, 2, None, None, None, *tail), "bits")
        for bits in (-1, 0, 24, 53):
            for y in (0, 5, h):
                assert form(C.byref(cfg), centre, bits, y, y, None, None, None, *tail) == 0


def test_the_scaled_view(fr, native, lib):
    v = S.view(fr.Config.new, S.M_900)
    out = fr.Config.new()
    assert lib.fr_de_scaled_view(C.byref(v.cfg), C.byref(out)) == 0
    assert (out.scale.re, out.scale.im) == (0.5, 0.5)  # 2^900 = 0.5 2^901
    want = bytearray(bytes(v.cfg))
    got = bytearray(bytes(out))
    off = type(v.cfg).scale.offset
    assert got[:off] == want[:off] and got[off + 16:] == want[off + 16:], "every other field is unchanged"
    t = T.view("MINI_OFF_860")
    cfg = t.fill(fr.Config.new())
    view = fr.de_scaled_view(cfg)
    assert (view.scale.re, view.scale.im) == (math.ldexp(1.37, -1), math.ldexp(-0.81, -1))  # e = 861
    assert (cfg.scale.re, cfg.scale.im) == t.scale, "de_scaled_view copies"
    assert (view.height, view.iterations, view.limit) == (cfg.height, cfg.iterations, cfg.limit)
    m = M.scaled_view(cfg)
    assert bytes(m) == bytes(view)
    assert lib.fr_de_scaled_view(C.byref(cfg), C.byref(cfg)) == 0 and bytes(cfg) == bytes(view), "view may alias cfg"
    # refusals: SCALED PT's rules about the scale
    refused(lib, lib.fr_de_scaled_view(None, C.byref(out)), "cfg is NULL")
    refused(lib, lib.fr_de_scaled_view(C.byref(v.cfg), None), "view is NULL")
    bad = fr.Config.from_buffer_copy(bytes(v.cfg))
    bad.scale.im = math.ldexp(1.0, 900 - 33)
    refused(lib, lib.fr_de_scaled_view(C.byref(bad), C.byref(out)), "SCALED PT", "2^-32")
    bad.scale.im = math.inf
    refused(lib, lib.fr_de_scaled_view(C.byref(bad), C.byref(out)), "SCALED PT", "finite")
    bad.scale.re = bad.scale.im = 2.0 ** -65
    refused(lib, lib.fr_de_scaled_view(C.byref(bad), C.byref(out)), "SCALED PT", "2^-64")


def test_python_refusals(fr):
    v = S.view(fr.Config.new, S.M_900)
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    PT = fr.Precision.PT
    for call in (fr.escape_rows_de, lambda c, **kw: fr.get_image_de(c, 1.0, **kw),
                 lambda c, **kw: fr.escape_rows_de_device(c, 8, 8, 8, **kw)):
        with pytest.raises(ValueError, match="scaled= needs centre="):
            call(v.cfg, precision=PT, scaled=True)
        with pytest.raises(ValueError, match="scaled= needs centre="):
            call(v.cfg, precision=PT, pos_lo=(0.0, 0.0), scaled=True)
        with pytest.raises(ValueError, match="centre= and pos_lo= exclude each other"):
            call(v.cfg, precision=PT, pos_lo=(0.0, 0.0), centre=centre, scaled=True)
        with pytest.raises(ValueError, match="Precision.PT"):
            call(v.cfg, centre=centre, scaled=True)
        with pytest.raises(ValueError, match="scaled= takes no opts"):
            call(v.cfg, precision=PT, centre=centre, scaled=True, opts=fr.RenderOpts())
        for bits in (23, 54, -1):
            with pytest.raises(ValueError, match="24 .. 53"):
                call(v.cfg, precision=PT, centre=centre, bla=bits, scaled=True)
    for kw in ({"supersample": 2}, {"y0": 1}, {"y1": 5}, {"channels": 4}):
        with pytest.raises(ValueError, match="out of scope of DE ON SCALED PT"):
            fr.get_image_de(v.cfg, 1.0, precision=PT, centre=centre, scaled=True, **kw)
    for bla in (None, 0):  # no rows: no device
        z, it, der = fr.escape_rows_de(v.cfg, 2, 2, precision=PT, centre=centre, bla=bla, scaled=True)
        assert z.shape == (0, 37, 2) and it.shape == (0, 37) and der.shape == (0, 37, 2)


def test_the_header_states_the_definition(fr, native):
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "fractal_hip.h")).read().replace(" * ", " ").split())
    for phrase in ("DE ON SCALED PT", "u0 = (Sinv, 0)", "bs0 = Sinv for Mandelbrot and 0 for Julia",
                   "nu = (fma(t.re, u.re, fma(-t.im, u.im, bs0)), fma(t.re, u.im, t.im * u.re))",
                   "b = (B.re * Sinv, B.im * Sinv) for Mandelbrot", "b = (+0, +0) for Julia",
                   "nu = (fma(A.re, u.re, fma(-A.im, u.im, b.re)), fma(A.re, u.im, fma(A.im, u.re, b.im)))",
                   "A rebase never touches u", "iterations = 0 returns (start, 0, (Sinv, 0))", "THE SCALED VIEW",
                   "CLAIM 1: z and iters are fr_escape_rows_pt_scaled's for the same bits, bit for bit",
                   "CLAIM 2: in the common domain", "u = d 2^-e exactly", "CLAIM 3, the range", "ITS REPORTED DISTANCE IS NOT ACCURATE THERE",
                   "D = (num / sqrt(u.re*u.re + u.im*u.im)) * ((double)height * min(|sre|, |sim|))",
                   # what stays: the pinned sentences of the roads that keep refusing
                   "DE on SCALED PT stays out of scope", "Out of scope: SCALED PT"):
        assert " ".join(phrase.replace(" * ", " ").split()) in text, phrase  # the comment's " * " margin is cut from both
    assert text.index("DE ON BLA-PT (fr_escape_rows_de_pt_bla") < text.index("DE ON SCALED PT (fr_escape_rows_de_pt_scaled") \
        < text.index("SUPERSAMPLED DE (fr_render_rows_ss_de")
    for name in ("fr_escape_rows_de_pt_scaled", "fr_escape_rows_de_pt_scaled_device", "fr_de_scaled_view"):
        assert re.search(r"\bint %s\(" % name, text) and name in native.PROTOTYPES
