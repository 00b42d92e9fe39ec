"""DE ON BLA-PT without a device (include/fractal_hip.h, "DE ON BLA-PT"): the model of tests/de_bla_model.c against the models
it rides on, and the library's refusals (which need no device).

  - CLAIM 1 in the models: over the views of tests/bla_model.py the model's z, iters and passes are bla_model's bit for bit;
  - CLAIM 2 in the models: on EARLY, where no pass skips, and at the caps whose table has no level to skip with, all three
    arrays are DE's on plain PT (tests/de_model.py) bit for bit; caps 0 .. 3 are all run, and where a cap's table is not empty
    the statement is made for the pixels that took no skip (test_small_caps_give_de_on_pt has the figures);
  - N_16, whose pixels all run to the cap: D = 0 everywhere;
  - accuracy: D over the model's arrays against D over plain PT's DE, both through tests/de_model.py's distance, on M_16, J_48,
    SEAHORSE and M_DEEP;
  - every view but EARLY and N_16 has escaped pixels that took a skip;
  - the domain, refusal by refusal, with its messages; y0 == y1 with NULL arrays; the Python keywords."""
import ctypes as C

import numpy as np
import pytest

import bla_model as B
import de_bla_model as M
import de_model as D
import oracle_lib as O
import pt_model as P
import pt_wide_model as W

INVALID = 1
VIEWS = {"M_16": B.M_16, "M_37": B.M_37, "M_DEEP": B.M_DEEP, "N_16": B.N_16, "J_48": B.J_48, "SEAHORSE": B.SEAHORSE,
         "EARLY": B.EARLY, "JULIA_REBASE": B.JULIA_REBASE}


def new_config():
    return O.config_new(0)


_views = {}


def view(name):
    """the model tests' own Views, on the oracle's Config type (bla_model.view's cache is shared with the tests that build theirs
    on the library's)"""
    if name not in _views:
        _views[name] = B.View(new_config, VIEWS[name][0], VIEWS[name][1:])
    return _views[name]


_pt = {}


def pt_de(name):
    """DE on plain PT over the view's own orbits (tests/de_model.c), computed once"""
    if name not in _pt:
        v = view(name)
        r = D.pt_rows_on(v.cfg, v.x, v.k)
        for a in r:
            a.setflags(write=False)
        _pt[name] = r
    return _pt[name]


# ---- the model against the models it rides on ------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(VIEWS))
def test_z_iters_and_passes_are_bla_models(name):
    v = view(name)
    for bits in (B.DEFAULT_BITS, 24, 53):
        z, it, der, passes, skips = M.model(v, bits)
        wz, wit, wpasses = v.model(bits)
        assert np.array_equal(it, wit) and B.same_bits(z, wz) and np.array_equal(passes, wpasses), (name, bits)
        assert (skips <= passes).all()
        assert (B.steps(v.cfg, it) > int(passes.sum())) == bool(skips.any())  # steps beyond the passes: what the skips saved


def test_the_pt_de_model_on_these_orbits_is_plain_pt():
    """the reference of the comparisons below: de_model's PT loop on the views' orbits gives the views' own PT results"""
    for name in VIEWS:
        z, it, _der = pt_de(name)
        v = view(name)
        assert np.array_equal(it, v.pt[1]) and B.same_bits(z, v.pt[0]), name


def test_where_no_pass_skips_all_three_arrays_are_de_on_pt():
    v = view("EARLY")
    for bits in (B.DEFAULT_BITS, 24, 53):
        z, it, der, passes, skips = M.model(v, bits)
        assert not skips.any()
        wz, wit, wder = pt_de("EARLY")
        assert np.array_equal(it, wit) and B.same_bits(z, wz) and D.same_doubles(der, wder)
    assert (it < v.cfg.iterations).sum() >= 300 and (it == v.cfg.iterations).sum() >= 300
    assert (der[it < v.cfg.iterations] != [1.0, 0.0]).any(-1).all()


def _at_cap(name, cap):
    """(cfg, x, k) of a view at another cap, orbits from the PT models"""
    v = view(name)
    cfg = type(v.cfg).from_buffer_copy(bytes(v.cfg))
    cfg.iterations = cap
    if v.kind == "wide":
        orbits = W.Orbits(cfg, *v.ints, v.n)
        return cfg, orbits.x[0], orbits.k[0] if cfg.algo == 2 else None
    return cfg, P.reference_orbit(cfg, v.pos_lo, 0), P.reference_orbit(cfg, v.pos_lo, 1) if cfg.algo == 2 else None


@pytest.mark.parametrize("name", ["M_16", "J_48", "SEAHORSE", "EARLY", "JULIA_REBASE"])
@pytest.mark.parametrize("cap", [0, 1, 2, 3])
def test_small_caps_give_de_on_pt(name, cap):
    """Where the table has no level to skip with — an orbit of at most 3 entries (last <= 2: n0 <= 1), which is caps 0 and 1 for
    Mandelbrot and 0 to 2 for these Julia views — and on EARLY at every cap, all three arrays are DE's on plain PT bit for bit.
    At the caps above that the table of a deep view is NOT empty (cap 2: one entry of level 1) and every pixel takes it: z and
    iters stay PT's on these views (the skipped dz' is absorbed in z), but der = A d + B rounds otherwise than two nested steps
    and differs from DE on PT in the last bits on every pixel that skipped (measured: relative 1.2e-16 to 3e-16; 3.7e-12 on the
    9 pixels of JULIA_REBASE that skip at cap 3).  There the bit-for-bit statement is made for the pixels that took no skip,
    and CLAIM 1 (z, iters are bla_model's) for all."""
    cfg, x, k = _at_cap(name, cap)
    z, it, der, passes, skips = M.escape_rows(cfg, x, k)
    wz, wit, wder = D.pt_rows_on(cfg, x, k)
    bz, bit, _ = B.escape_rows(cfg, x, k)
    assert np.array_equal(it, bit) and B.same_bits(z, bz)
    no_levels = all(len(o) - 1 <= 2 for o in (x, k) if o is not None)  # from the orbits alone, not from what the model did
    assert no_levels == (cap <= (2 if cfg.algo == 2 else 1))
    if no_levels or name == "EARLY":
        assert not skips.any()
    plain = skips == 0
    print("%s at cap %d: %d of %d pixels skipped" % (name, cap, int((~plain).sum()), plain.size))
    assert np.array_equal(it[plain], wit[plain]) and B.same_bits(z[plain], wz[plain]) and D.same_doubles(der[plain], wder[plain])
    if cap == 0:  # (start, 0, (1, 0))
        assert not it.any() and B.same_bits(der, np.broadcast_to([1.0, 0.0], der.shape))
        m = 0 if cfg.algo == 2 else 1
        w, h = float(cfg.width), float(cfg.height)
        off = ((np.arange(cfg.width, dtype=np.float64) / h) - ((w / h) / 2.0)) / cfg.scale.re
        assert B.same_bits(z[3, :, 0], x[m, 0] + off)


def test_an_algorithm_without_orbits_gives_zeros():
    cfg = O.config_new(1)
    cfg.width, cfg.height, cfg.iterations = 9, 5, 50
    for a in M.escape_rows(cfg):
        assert not a.any()


def test_capped_pixels_have_distance_zero():
    v = view("N_16")
    z, it, der, passes, skips = M.model(v)
    assert (it == v.cfg.iterations).all() and skips.sum() > it.size  # every pixel capped, and through many skips
    assert (D.distance(v.cfg, z, it, der) == 0.0).all()


# ---- accuracy against DE on plain PT ---------------------------------------------------------------------------------------

# The worst |D_bla - D_pt| / D_pt over the compared pixels (equal iters, D_pt >= 2^-10 pixels) that the two exact models gave
# at the default 40 bits when this was written, and the tolerance: 4 x that (the issue's factor: slack that does not depend on
# the compiler, and the tighter setting bits = 53, measured at 9.3e-13, 3.7e-11, 1.3e-10 and 2.6e-12).  bits = 24 is outside it
# by its own eps = 2^-24 (measured 6.7e-6, 1.1e-3, 4.9e-3 and 5.2e-6) and is not asserted.  DESIGN.md 3.22 carries the table.
MEASURED_40 = {"M_16": 5.84e-11, "J_48": 9.38e-9, "SEAHORSE": 3.32e-7, "M_DEEP": 7.75e-11}
FACTOR = 4.0


@pytest.mark.parametrize("name", list(MEASURED_40))
def test_distance_against_de_on_plain_pt(name):
    v = view(name)
    pz, pit, pder = pt_de(name)
    d_pt = D.distance(v.cfg, pz, pit, pder)
    for bits in (B.DEFAULT_BITS, 53):
        z, it, der, passes, skips = M.model(v, bits)
        d_bla = D.distance(v.cfg, z, it, der)
        same = it == pit
        compared = same & (d_pt >= 2.0 ** -10)
        below = same & (d_pt > 0.0) & (d_pt < 2.0 ** -10)
        ratio = np.abs(d_bla - d_pt)[compared] / d_pt[compared]
        low = np.abs(d_bla - d_pt)[below] / d_pt[below]
        print("%s, %d bits: %d of %d pixels compared, worst %.4g (median D %.3g); below 2^-10 pixels: %d, worst %.3g (recorded only)"
              % (name, bits, compared.sum(), it.size, ratio.max(), np.median(d_pt), below.sum(), low.max() if low.size else 0.0))
        assert 2 * int(compared.sum()) >= it.size, "the compared pixels are less than half of the image"
        assert ratio.max() < FACTOR * MEASURED_40[name], (name, bits, ratio.max())
        assert np.isfinite(der[compared]).all()


@pytest.mark.parametrize("name", [n for n in VIEWS if n not in ("EARLY", "N_16")])
def test_escaped_pixels_took_skips(name):
    v = view(name)
    z, it, der, passes, skips = M.model(v)
    assert ((it < v.cfg.iterations) & (skips > 0)).sum() >= 1, "a view whose escaped pixels never skip checks no skipped derivative"


# ---- the domain: every refusal, by message, with no device ------------------------------------------------------------------


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


def test_refusals_need_no_device(fr, native, lib):
    v = B.view(fr.Config.new, *B.M_16)
    _, centre, _keep = v.args(native)
    s = B.view(fr.Config.new, *B.SEAHORSE)
    lo, _, _keep2 = s.args(native)
    h, w = v.shape
    z, der = np.zeros((h, w, 2)), np.zeros((h, w, 2))
    it = np.zeros((h, w), dtype=np.uint32)
    arrays = (z.ctypes.data, it.ctypes.data, der.ctypes.data)
    for form, tail in ((lib.fr_escape_rows_de_pt_bla, ()), (lib.fr_escape_rows_de_pt_bla_device, (None,))):
        refused(lib, form(None, None, centre, 0, 0, h, *arrays, *tail), "cfg is NULL")
        refused(lib, form(C.byref(v.cfg), None, centre, 0, 5, 4, *arrays, *tail), "y0 > y1")
        refused(lib, form(C.byref(v.cfg), None, centre, 0, 0, h + 1, *arrays, *tail), "y1 > height")
        for k in range(3):
            a = list(arrays)
            a[k] = None
            refused(lib, form(C.byref(v.cfg), None, centre, 0, 0, h, *a, *tail), "all three")
        refused(lib, form(C.byref(v.cfg), None, centre, 0, 0, h, arrays[0] + 4, arrays[1], arrays[2], *tail), "8-byte aligned")
        refused(lib, form(C.byref(v.cfg), None, centre, 0, 0, h, arrays[0], arrays[1] + 2, arrays[2], *tail), "4-byte aligned")
        refused(lib, form(C.byref(v.cfg), None, centre, 0, 0, h, arrays[0], arrays[1], arrays[2] + 4, *tail), "8-byte aligned")
        for bits in (23, 54, -1):
            refused(lib, form(C.byref(v.cfg), None, centre, bits, 0, h, *arrays, *tail), "BLA-PT", "bits", "24 .. 53")
            refused(lib, form(C.byref(s.cfg), lo, None, bits, 0, s.shape[0], *arrays, *tail), "bits")
        big = fr.Config.from_buffer_copy(bytes(v.cfg))
        for limit in (2.0 ** 20 * (1 + 2.0 ** -52), 2.0 ** 21):
            big.limit = limit
            refused(lib, form(C.byref(big), None, centre, 0, 0, h, *arrays, *tail), "limit must be <= 2^20")
        big.limit = 2.0 ** 20
        assert form(C.byref(big), None, centre, 0, 3, 3, None, None, None, *tail) == 0
        deep = fr.Config.from_buffer_copy(bytes(v.cfg))
        deep.scale.re = deep.scale.im = 2.0 ** 441  # a wide centre past WIDE PT's domain
        refused(lib, form(C.byref(deep), None, centre, 0, 0, h, *arrays, *tail), "2^440")
        refused(lib, form(C.byref(v.cfg), lo, centre, 0, 0, h, *arrays, *tail), "pos_lo must be NULL")  # both centres
        # the road's own domain on the dd side: PT's
        pt = fr.Config.from_buffer_copy(bytes(s.cfg))
        pt.iterations = (1 << 24) + 1
        refused(lib, form(C.byref(pt), lo, None, 0, 0, s.shape[0], *arrays, *tail), "FR_PT_MAX_ITERATIONS")
        # refusals come before the no-rows shortcut; a legal call without rows needs neither arrays nor a device
        refused(lib, form(C.byref(v.cfg), None, centre, 23, 2, 2, None, None, None, *tail), "bits")
        for y in (0, 5, h):
            assert form(C.byref(v.cfg), None, centre, 0, y, y, None, None, None, *tail) == 0
        assert form(C.byref(s.cfg), lo, None, 53, 1, 1, None, None, None, *tail) == 0


def test_python_refusals(fr):
    v = B.view(fr.Config.new, *B.M_16)
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    for call in (fr.escape_rows_de, lambda c, **kw: fr.get_image_de(c, 1.0, **kw),
                 lambda c, **kw: fr.escape_rows_de_device(c, 8, 8, 8, **kw)):
        with pytest.raises(ValueError, match="Precision.PT"):  # the F64 road has no such call
            call(v.cfg, precision=fr.Precision.F64, bla=0)
        with pytest.raises(ValueError, match="Precision.PT"):
            call(v.cfg, bla=40)
        with pytest.raises(ValueError, match="opts"):
            call(v.cfg, precision=fr.Precision.PT, centre=centre, bla=0, opts=fr.RenderOpts())
        for bits in (23, 54, -1):
            with pytest.raises(ValueError, match="24 .. 53"):
                call(v.cfg, precision=fr.Precision.PT, centre=centre, bla=bits)
        with pytest.raises(ValueError):
            call(v.cfg, precision=fr.Precision.PT, centre=centre, pos_lo=(0.0, 0.0), bla=0)
    z, it, der = fr.escape_rows_de(v.cfg, 2, 2, precision=fr.Precision.PT, centre=centre, bla=0)  # no rows: no device
    assert z.shape == (0, 16, 2) and it.shape == (0, 16) and der.shape == (0, 16, 2)


def test_the_header_states_the_definition(fr, native):
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "fractal_hip.h")).read().replace(" * ", " ").split())
    for phrase in ("DE ON BLA-PT", "nd.re = fma(A.re, d.re, fma(-A.im, d.im, b.re))", "nd.im = fma(A.re, d.im, fma( A.im, d.re, b.im))",
                   "b = (+0, +0) for Julia", "A rebase never touches d", "CLAIM 1: z and iters are fr_escape_rows_pt_bla's, bit for bit",
                   "CLAIM 2: on a view where no pass skips", "Out of scope: SCALED PT"):
        assert phrase in text, phrase
    for name in ("fr_escape_rows_de_pt_bla", "fr_escape_rows_de_pt_bla_device"):
        assert re.search(r"\bint %s\(" % name, text) and name in native.PROTOTYPES
