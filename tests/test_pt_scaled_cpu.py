"""SCALED PT without a device (include/fractal_hip.h, fr_precision: "SCALED PT"):
  - the MODEL (tests/pt_scaled_model.py) inside WIDE PT's domain: bits = -1 gives pt_wide_model's rule-1 run, which is plain
    WIDE PT, and bits = 40 gives bla_model's z and iters, bit for bit — the claim of the definition, on the model;
  - the model past the 2^440 edge: the counts of the issue that introduced SCALED PT (its prototype's), on the Misiurewicz
    point, the period-3 nucleus and the Julia fixed point at 2^900 and on a period-267 minibrot at 2^861;
  - skips past the edge: every escape index of the plain scaled loop kept at under a third of the passes;
  - fr_debug_bla_table_scaled against the model's table bit for bit at every level;
  - the domain: each refusal with its code and a message that names the rule, before any device work (on a box without a
    device anything that touched one would answer FR_ERR_NO_DEVICE instead), and the Python scaled= misuse cases."""
import ctypes as C
import math

import numpy as np
import pytest

import bla_model as B
import pt_scaled_model as S
import pt_wide_model as W

INVALID = 1


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


def message(lib):
    return lib.fr_last_error().decode()


# ---- 1. inside WIDE PT's domain the scaled model is the existing models ----------------------------------------------------


@pytest.mark.parametrize("spec,limit", [(S.M_200, 2.0), (S.M_440, 2.0), (S.N_300, 2.0), (S.J_300, 2.0), (S.M_440, 65536.0)],
                         ids=["M-2^200", "M-2^440", "N-2^300", "J-2^300", "M-2^440-limit-65536"])
def test_without_a_table_the_model_is_wide_pt(fr, spec, limit):
    v = S.View(fr.Config.new, spec) if limit != 2.0 else S.view(fr.Config.new, spec)
    v.cfg.limit = limit
    (z, it, _, _), reb = W.state_rows(v.cfg, v.orbits, rule=1)
    sz, sit, passes, sreb = S.escape_rows(v.cfg, v.x, v.k, S.NO_TABLE)
    assert np.array_equal(sit, it)
    assert S.same_bits(sz, z)
    assert np.array_equal(sreb, reb)  # the two-sided test rebases where PT's does
    assert int(passes.astype(np.uint64).sum()) == S.steps(v.cfg, it)  # one pass per step
    assert len(np.unique(it)) > 1 or (it == v.cfg.iterations).all()


@pytest.mark.parametrize("name", ["M_16", "M_37", "M_DEEP", "N_16", "J_48"])
def test_with_a_table_the_model_is_bla_pt(fr, name):
    b = B.view(fr.Config.new, *getattr(B, name))
    z, it, passes = b.model(40)
    sz, sit, spasses, _ = S.escape_rows(b.cfg, b.x, b.k, 40)
    assert np.array_equal(sit, it)
    assert S.same_bits(sz, z)
    assert B.steps(b.cfg, it) > int(passes.astype(np.uint64).sum())  # the view does skip
    # the passes may differ only at a pixel with |w| < 2^-53: here that is the pixel at the view's very centre, woff = 0
    differ = np.argwhere(spasses != passes)
    h, w = b.shape
    assert all((y, x) == (h // 2, w // 2) for y, x in differ), differ
    if name == "N_16":  # while its offset is 0, BLA-PT skips that pixel along and the scaled loop applies no entry to it
        assert len(differ) == 1 and spasses[h // 2, w // 2] > passes[h // 2, w // 2]


# ---- 2. past the edge: the counts of the issue's prototype ------------------------------------------------------------------


def test_misiurewicz_at_2_900(fr):
    v = S.view(fr.Config.new, S.M_900)
    assert v.cfg.limit == 2.0 and v.n == 16 and v.shape == (21, 37) and v.cfg.iterations == 6000
    z, it, passes, reb = v.model()
    assert len(v.x) == 628
    assert (int(it.min()), int(it.max()), len(np.unique(it))) == (553, 570, 15)
    assert not (it == v.cfg.iterations).any()
    assert int(reb.max()) == 5
    assert np.isfinite(z).all()


def test_minibrot_at_2_861(fr):
    v = S.view(fr.Config.new, S.MINI_861)
    assert v.shape == (16, 24) and v.cfg.iterations == 3204
    z, it, passes, reb = v.model()
    assert len(v.x) == 3206  # the nucleus never escapes: the orbit is cut by the cap
    assert int((it == v.cfg.iterations).sum()) == 69 and len(np.unique(it)) == 243


def test_nucleus_at_2_900(fr):
    v = S.view(fr.Config.new, S.N_900)
    z, it, passes, reb = v.model()
    assert v.shape == (12, 16) and (it == 1000).all()


def test_julia_at_2_900(fr):
    v = S.view(fr.Config.new, S.J_900)
    z, it, passes, reb = v.model()
    assert v.shape == (12, 16) and (int(it.min()), int(it.max())) == (557, 1139)
    assert len(np.unique(it)) == 42


# ---- 3. skips past the edge ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("spec", [S.M_900, S.MINI_861], ids=["M-2^900", "minibrot"])
def test_skips_keep_every_escape_index_at_under_a_third_of_the_passes(fr, spec):
    v = S.view(fr.Config.new, spec)
    z, it, passes, _ = v.model(40)
    assert np.array_equal(it, v.model()[1])
    total = int(passes.astype(np.uint64).sum())
    assert total < S.steps(v.cfg, it) / 3, (total, S.steps(v.cfg, it))


def test_the_top_level_at_2_900_holds_a_radius_the_unscaled_table_has_lost(fr):
    v = S.view(fr.Config.new, S.M_900)
    top = S.table(v.cfg, v.x, 40)[-1]
    assert top.shape == (1, 5) and top[0, 4] > 0
    assert (B.table(v.cfg, v.x, 40)[-1][:, 4] == 0).all()  # r2 = r*r of a radius near 2^-870 is 0


# ---- 4. the library's table -----------------------------------------------------------------------------------------------------


def lib_level(lib, native, v, which, level, bits=0):
    st = v.centre(native)
    n = C.c_uint32(12345)
    assert lib.fr_debug_bla_table_scaled(C.byref(v.cfg), C.byref(st), bits, which, level, None, 0, C.byref(n)) == 0, message(lib)
    out = np.full((n.value + 1, 5), np.nan)
    assert lib.fr_debug_bla_table_scaled(C.byref(v.cfg), C.byref(st), bits, which, level, out.ctypes.data, n.value, C.byref(n)) == 0
    assert np.isnan(out[n.value:]).all(), "a write past len entries"
    return out[:n.value]


@pytest.mark.parametrize("spec,which", [(S.M_300, 0), (S.M_900, 0), (S.J_300, 0), (S.J_300, 1), (S.MINI_861, 0)],
                         ids=["M-2^300", "M-2^900", "J-V", "J-K", "minibrot"])
def test_the_librarys_table_is_the_models(fr, native, lib, spec, which):
    v = S.view(fr.Config.new, spec)
    orbit = v.k if which else v.x
    want = S.table(v.cfg, orbit, 40)
    n0 = len(orbit) - 2
    assert n0 >= 100 and len(want) == n0.bit_length()
    applied = 0
    for k, w in enumerate(want):
        got = lib_level(lib, native, v, which, k)
        assert len(got) == len(w) == n0 >> k, "level %d" % k
        assert S.same_bits(got[:, 4], w[:, 4]), "R of level %d" % k
        live = w[:, 4] > 0
        applied += int(live.sum()) if k else 0
        assert S.same_bits(got[live, :4], w[live, :4]), "A, B of level %d" % k
        assert np.isfinite(w[live, :4]).all()  # the finiteness argument of the definition
        assert (w[live, 4] >= 2.0 ** -53).all()
    assert applied > 0, "a table nobody could apply"
    assert len(lib_level(lib, native, v, which, len(want))) == 0
    assert S.same_bits(fr.bla_table(v.cfg, 1, which, centre=fr.WideCentre(v.n, re=v.words[0], im=v.words[1]), scaled=True), want[1])


# ---- 5. the domain --------------------------------------------------------------------------------------------------------------


def domain_view(fr, native, scale_log2, n=16):
    cfg = W.view(fr.Config.new(), "M", scale_log2, 16, 12, 100)
    re, im = W.centre_ints("M", n)
    words = W.to_words(re, n), W.to_words(im, n)
    p64 = C.POINTER(C.c_uint64)
    st = native.fr_wide_centre(n, words[0].ctypes.data_as(p64), words[1].ctypes.data_as(p64))
    return cfg, st, words


def refused(lib, cfg, centre, bits=-1, y=(0, 0)):
    """the code and message of an argument-only call (y0 == y1: a legal call of it needs no device)"""
    rc = lib.fr_escape_rows_pt_scaled(C.byref(cfg), centre, bits, y[0], y[1], None, None)
    return rc, message(lib) if rc else ""


def test_2_951_is_inside_and_2_952_is_not(fr, native, lib):
    cfg, st, _w = domain_view(fr, native, 951)
    assert refused(lib, cfg, C.byref(st)) == (0, "")
    assert lib.fr_render_rows_pt_scaled(C.byref(cfg), C.byref(st), 0, 5, 5, 3, None, 0) == 0
    cfg.scale.re = cfg.scale.im = math.ldexp(1.0, 952)
    rc, msg = refused(lib, cfg, C.byref(st))
    assert rc == INVALID and "SCALED PT" in msg and "e + 64" in msg


def test_a_centre_too_coarse_for_its_scale(fr, native, lib):
    cfg, st, _w = domain_view(fr, native, 900, n=15)
    rc, msg = refused(lib, cfg, C.byref(st))
    assert rc == INVALID and "too coarse" in msg and "e + 64" in msg
    cfg, st, _w = domain_view(fr, native, 900, n=16)
    assert refused(lib, cfg, C.byref(st)) == (0, "")


def test_the_limit_rule(fr, native, lib):
    cfg, st, _w = domain_view(fr, native, 900)
    cfg.limit = 2.0 ** 20
    assert refused(lib, cfg, C.byref(st)) == (0, "")
    cfg.limit = 2.0 ** 21
    rc, msg = refused(lib, cfg, C.byref(st))
    assert rc == INVALID and "limit" in msg and "2^20" in msg


def test_the_axis_ratio_rule(fr, native, lib):
    cfg, st, _w = domain_view(fr, native, 900)
    cfg.scale.im = math.ldexp(1.0, 900 - 32)
    assert refused(lib, cfg, C.byref(st)) == (0, "")
    for axis in ("re", "im"):
        cfg, st, _w = domain_view(fr, native, 900)
        setattr(cfg.scale, axis, math.ldexp(-1.0, 900 - 33))  # the rule is on magnitudes
        rc, msg = refused(lib, cfg, C.byref(st))
        assert rc == INVALID and "2^-32" in msg, axis


def test_a_centre_is_required(fr, native, lib):
    cfg, st, _w = domain_view(fr, native, 900)
    rc, msg = refused(lib, cfg, None)
    assert rc == INVALID and "centre is NULL" in msg
    n = C.c_uint32(0)
    assert lib.fr_debug_bla_table_scaled(C.byref(cfg), None, 0, 0, 1, None, 0, C.byref(n)) == INVALID


@pytest.mark.parametrize("bits", [23, 54, -2, 1])
def test_bits_out_of_range(fr, native, lib, bits):
    cfg, st, _w = domain_view(fr, native, 900)
    rc, msg = refused(lib, cfg, C.byref(st), bits)
    assert rc == INVALID and "bits" in msg and "24 .. 53" in msg
    a, b = C.c_uint64(0), C.c_uint64(0)
    assert lib.fr_debug_pt_scaled_count(C.byref(cfg), C.byref(st), bits, 0, 0, C.byref(a), C.byref(b)) == INVALID


def test_bits_in_range_and_a_table_needs_bits(fr, native, lib):
    cfg, st, _w = domain_view(fr, native, 900)
    for bits in (-1, 0, 24, 53):
        assert refused(lib, cfg, C.byref(st), bits) == (0, "")
    n = C.c_uint32(0)
    assert lib.fr_debug_bla_table_scaled(C.byref(cfg), C.byref(st), -1, 0, 1, None, 0, C.byref(n)) == INVALID
    assert "bits" in message(lib)


def test_rows_and_the_rest_of_wide_pts_domain_still_hold(fr, native, lib):
    cfg, st, _w = domain_view(fr, native, 900)
    assert refused(lib, cfg, C.byref(st), y=(3, 2))[0] == INVALID
    assert refused(lib, cfg, C.byref(st), y=(0, 13))[0] == INVALID
    cfg.iterations = (1 << 24) + 1
    rc, msg = refused(lib, cfg, C.byref(st))
    assert rc == INVALID and "FR_PT_MAX_ITERATIONS" in msg
    assert lib.fr_escape_rows_pt_scaled(None, C.byref(st), -1, 0, 0, None, None) == INVALID


def test_the_wide_road_still_stops_at_2_440(fr, native, lib):
    cfg, st, _w = domain_view(fr, native, 441)
    assert lib.fr_escape_rows_pt_wide(C.byref(cfg), C.byref(st), 0, 0, None, None) == INVALID
    assert "|scale| must be <= 2^440 on both axes (deeper views need a scaled pixel loop)" in message(lib)
    assert lib.fr_escape_rows_pt_bla(C.byref(cfg), None, C.byref(st), 0, 0, 0, None, None) == INVALID
    assert refused(lib, cfg, C.byref(st)) == (0, "")  # the scaled road takes the same view
    cfg.scale.re = cfg.scale.im = math.ldexp(1.0, 440)
    assert lib.fr_escape_rows_pt_wide(C.byref(cfg), C.byref(st), 0, 0, None, None) == 0


def test_python_scaled_misuse(fr):
    v = S.view(fr.Config.new, S.M_900)
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    PT = fr.Precision.PT
    with pytest.raises(ValueError, match="scaled= needs centre="):
        fr.escape_rows(v.cfg, precision=PT, scaled=True)
    with pytest.raises(ValueError, match="scaled= needs centre="):
        fr.get_image(v.cfg, PT, pos_lo=(0.0, 0.0), scaled=True)
    with pytest.raises(ValueError, match="scaled= needs centre="):
        fr.get_image_rgba(v.cfg, PT, supersample=2, scaled=True)
    # the existing refusals keep their text and come first
    with pytest.raises(ValueError, match="centre= and pos_lo= exclude each other"):
        fr.get_image(v.cfg, PT, pos_lo=(0.0, 0.0), centre=centre, scaled=True)
    with pytest.raises(ValueError, match="supersample does not take centre= yet"):
        fr.get_image(v.cfg, PT, supersample=2, centre=centre, scaled=True)
    with pytest.raises(ValueError, match="centre= needs precision=Precision.PT"):
        fr.get_image(v.cfg, fr.Precision.F64, centre=centre, scaled=True)
    with pytest.raises(ValueError, match="bla= is None"):
        fr.escape_rows(v.cfg, precision=PT, centre=centre, bla=23, scaled=True)
    with pytest.raises(ValueError, match="scaled= takes no opts"):
        fr.get_image_rows(v.cfg, 0, 1, PT, opts=fr.RenderOpts(), centre=centre, scaled=True)
    # a legal call with no rows needs no device
    assert fr.get_image_rows(v.cfg, 4, 4, PT, centre=centre, scaled=True).shape == (0, 37, 3)
    assert fr.get_image_rows(v.cfg, 4, 4, PT, centre=centre, bla=0, scaled=True).shape == (0, 37, 3)
