"""ADAPTIVE SUPERSAMPLED SCALED DE (include/fractal_hip.h) without a device, in three parts: the numpy model of the definition —
tests/ss_adaptive_de_model.py run on the scaled view (tests/de_scaled_model.py: scaled_view) over the arrays of
de_scaled_model.escape_rows on cfg_s — obeys every consequence the header lists, on tests/pt_scaled_model.py's views at their own
sizes; the domain checks of all four spellings, which come before any device work and name their argument (fake pointers: nothing
is dereferenced before the checks have passed); the no-op forms, the Python wrapper's keyword checks, and a valid call that
answers FR_ERR_NO_DEVICE where there is no device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import de_bla_model as DB
import de_model as DE
import de_scaled_model as DSM
import pt_scaled_model as S
import ss_adaptive_de_model as M
import ss_adaptive_de_views as AV
import ss_adaptive_model as A
import ss_de_model as SD

INVALID, TOO_SMALL, NO_DEVICE = 1, 2, 3
T, TAU, REACH = 1.0, 8, 2.0
PAST = {"M_900": S.M_900, "J_900": S.J_900, "MINI_861": S.MINI_861, "N_900": S.N_900}
INSIDE = {"M_440": S.M_440, "J_300": S.J_300}
# (union, near-only, union pixels with F != P) at T = 1, t = 8, R = 2, for s = 2 and 3; the same at bits -1 and 40
FIGURES = {"M_900": ((85, 1, 46), (83, 2, 48)), "J_900": ((76, 6, 48), (74, 12, 50)), "MINI_861": ((346, 167, 262), (347, 180, 275)),
           "N_900": ((0, 0, 0), (0, 0, 0))}


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


def spec_s(spec, s):
    name, n, log2, w, h, cap = spec
    return (name, n, log2, w * s, h * s, cap)


def modelled(fr, spec, s, bits):
    """(view of the OUTPUT size, view of cfg_s, the scaled view of the output's config, z, iters, u, skips) by the host model"""
    v, vs = S.view(fr.Config.new, spec), S.view(fr.Config.new, spec_s(spec, s))
    assert bytes(vs.cfg) == bytes(SD.config_s(v.cfg, s))
    z, it, u, _passes, skips, _range = DSM.model(vs, bits)
    return v, vs, DSM.scaled_view(v.cfg), z, it, u, skips


# ---- 1. the model on the scaled view ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("bits", [-1, 40])
@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("name", list(PAST))
def test_model_obeys_every_consequence_of_the_definition(fr, name, s, bits):
    v, vs, cfg_v, z, it, u, _ = modelled(fr, PAST[name], s, bits)
    w, h, p = v.cfg.width, v.cfg.height, s // 2
    assert bytes(SD.config_s(cfg_v, s)) == bytes(DSM.scaled_view(vs.cfg))  # cfg_sv either way
    H = SD.shaded(cfg_v, z, it, u, s, T)
    full = SD.colour(cfg_v, z, it, u, s, T)  # SUPERSAMPLED SCALED DE's bytes
    # t = -1: the bytes of fr_render_rows_ss_de_pt_scaled, for every R
    for reach in (0.0, REACH):
        out, n = M.adaptive_de(cfg_v, z, it, u, s, T, -1, reach)
        assert np.array_equal(out, full) and n == w * h
    # t = 255 with R = 0: the probe image
    out, n = M.adaptive_de(cfg_v, z, it, u, s, T, 255, 0.0)
    assert np.array_equal(out, H[p::s, p::s]) and n == 0
    # R = 0: the colour rule on the shaded bytes
    out, n = M.adaptive_de(cfg_v, z, it, u, s, T, TAU, 0.0)
    want, wn = A.adaptive(H, s, TAU)
    assert np.array_equal(out, want) and n == wn
    assert not M.near_only(cfg_v, z, it, u, s, T, TAU, 0.0).any()
    # T = 0 with R = 0: ADAPTIVE SUPERSAMPLING on SCALED PT's own bytes (claim 1: z and iters are pt_scaled_model's)
    zs, its = vs.model(bits)[:2]
    assert np.array_equal(its, it) and S.same_bits(zs, z)
    plain = DE.base_colours(vs.cfg, np.ascontiguousarray(zs), its)
    out, n = M.adaptive_de(cfg_v, z, it, u, s, 0.0, TAU, 0.0)
    want, wn = A.adaptive(plain, s, TAU)
    assert np.array_equal(out, want) and n == wn
    # s = 1: the scaled DE render coloured on cfg_v with T, for every t and R
    if s == 1:
        want = DE.colour(cfg_v, z, it, u, T, 3)
        for tau, reach in ((-1, 0.0), (0, 1.0), (TAU, REACH), (255, 0.0), (255, 3.0)):
            assert np.array_equal(M.adaptive_de(cfg_v, z, it, u, 1, T, tau, reach)[0], want)
    # row pieces sum to the whole; RGBA
    for reach in (0.0, REACH):
        whole, total = M.adaptive_de(cfg_v, z, it, u, s, T, TAU, reach)
        for y0 in (0, 1, 7):
            cuts = sorted({0, y0, y0 + 1, h})
            parts = [M.adaptive_de(cfg_v, z, it, u, s, T, TAU, reach, a, b) for a, b in zip(cuts, cuts[1:])]
            assert np.array_equal(np.concatenate([q[0] for q in parts]), whole), (reach, y0)
            assert sum(q[1] for q in parts) == total
        rgba, n4 = M.adaptive_de(cfg_v, z, it, u, s, T, TAU, reach, channels=4)
        assert np.array_equal(rgba[..., :3], whole) and (rgba[..., 3] == 255).all() and n4 == total
    # the sRGB filter replaces F and nothing else
    lin, n = M.adaptive_de(cfg_v, z, it, u, s, T, TAU, REACH, filter=AV.srgb_filter)
    e, nr = M.edge_sets(cfg_v, z, it, u, s, T, TAU, REACH)
    assert n == int((e | nr).sum()) and np.array_equal(lin[~(e | nr)], H[p::s, p::s][~(e | nr)])


@pytest.mark.parametrize("bits", [-1, 40])
@pytest.mark.parametrize("name", list(PAST))
def test_the_views_have_the_teeth_the_gpu_tests_rest_on(fr, name, bits):
    """the figures of the GPU file's cases, from the model alone: the union, the near-only pixels, the union pixels with F != P, and
    no pixel outside the union with F != P — a missed refinement shows in the bytes, an excess one in `refined`"""
    for s, (union, lonely, differ) in zip((2, 3), FIGURES[name]):
        v, vs, cfg_v, z, it, u, skips = modelled(fr, PAST[name], s, bits)
        e, n = M.edge_sets(cfg_v, z, it, u, s, T, TAU, REACH)
        H = SD.shaded(cfg_v, z, it, u, s, T)
        d = (SD.box(H, s) != A.probe(H, s)).any(axis=-1)
        got = (int((e | n).sum()), int((n & ~e).sum()), int(((e | n) & d).sum()))
        print("%s s=%d bits=%d: union %d of %d, near-only %d, union with F != P %d" % ((name, s, bits, got[0], e.size) + got[1:]))
        assert got == (union, lonely, differ), (name, s, bits, got)
        assert not (~(e | n) & d).any()
        assert M.adaptive_de(cfg_v, z, it, u, s, T, TAU, REACH)[1] == union
        if name == "N_900":
            assert (it == v.cfg.iterations).all()  # every sample is capped: a capped probe is never near
            assert not M.near(cfg_v, z, it, u, s, 2.0 ** 19).any()
        elif bits >= 0:  # the table form is another loop on the refined samples
            per_pixel = skips.reshape(v.cfg.height, s, v.cfg.width, s).sum(axis=(1, 3))
            assert (per_pixel[e | n] > 0).any()
        if name != "N_900":  # the sRGB filter is seen at a refined pixel
            assert (((AV.srgb_filter(H, s) != SD.box(H, s)).any(axis=-1)) & (e | n)).any()


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", list(INSIDE))
def test_inside_wide_pt_the_model_is_adaptive_de_on_the_wide_roads(fr, name, s):
    """DE ON SCALED PT's claim 2 carried through: with bits = -1 the bytes and the count are ADAPTIVE SUPERSAMPLED DE's on WIDE PT's
    arrays and the view's own scale; with a table they are BLA-PT's (the two table models agree on z and iters on these views)"""
    v, vs, cfg_v, z, it, u, _ = modelled(fr, INSIDE[name], s, -1)
    zw, itw, dw = DE.pt_wide_rows(vs.cfg, vs.orbits)[:3]
    assert np.array_equal(itw, it) and S.same_bits(zw, z)
    want, count = M.adaptive_de(v.cfg, zw, itw, dw, s, T, TAU, REACH)
    got, n = M.adaptive_de(cfg_v, z, it, u, s, T, TAU, REACH)
    assert np.array_equal(got, want) and n == count and 0 < n < it.size // (s * s)
    assert M.near_only(cfg_v, z, it, u, s, T, TAU, REACH).any()
    v, vs, cfg_v, z, it, u, _ = modelled(fr, INSIDE[name], s, 40)
    zb, itb, db = DB.escape_rows(vs.cfg, vs.x, vs.k, 40)[:3]
    assert np.array_equal(itb, it) and S.same_bits(zb, z)  # SCALED PT's caveat about |w| < 2^-53 touches no sample of these views
    want, count = M.adaptive_de(v.cfg, zb, itb, db, s, T, TAU, REACH)
    got, n = M.adaptive_de(cfg_v, z, it, u, s, T, TAU, REACH)
    assert np.array_equal(got, want) and n == count and 0 < n < it.size // (s * s)


# ---- 2. the domain ----------------------------------------------------------------------------------------------------------------


def spellings(lib):
    """the four spellings as call(cfg, centre, **kw) -> rc; fake device pointers, a real host buffer"""

    def host(tf):
        def call(cfg, centre, bits=-1, thickness=T, s=2, transfer=0, tau=TAU, reach=REACH, y0=0, y1=None, channels=3, out_len=None,
                 has_out=True, **_):
            y1 = cfg.height if y1 is None else y1
            out = np.zeros(max(channels * cfg.width * max(y1 - y0, 0), 1), dtype=np.uint8)
            n = C.c_uint64(7)
            tail = (tau, reach, y0, y1, channels, out.ctypes.data if has_out else None, out.nbytes if out_len is None else out_len, C.byref(n))
            if tf:
                return lib.fr_render_rows_ss_adaptive_de_pt_scaled_tf(C.byref(cfg), centre, bits, thickness, s, transfer, *tail)
            return lib.fr_render_rows_ss_adaptive_de_pt_scaled(C.byref(cfg), centre, bits, thickness, s, *tail)

        return call

    def device(tf):
        def call(cfg, centre, bits=-1, thickness=T, s=2, transfer=0, tau=TAU, reach=REACH, y0=0, y1=None, channels=3, d_out=0x1000,
                 out_len=1 << 40, d_work=0x2000, work_len=1 << 40, d_refined=0x3000, has_out=True, **_):
            y1 = cfg.height if y1 is None else y1
            tail = (tau, reach, y0, y1, channels, d_out if has_out else None, out_len, d_work, work_len, d_refined, None)
            if tf:
                return lib.fr_render_rows_ss_adaptive_de_pt_scaled_tf_device(C.byref(cfg), centre, bits, thickness, s, transfer, *tail)
            return lib.fr_render_rows_ss_adaptive_de_pt_scaled_device(C.byref(cfg), centre, bits, thickness, s, *tail)

        return call

    return {"host": host(False), "host_tf": host(True), "device": device(False), "device_tf": device(True)}


@pytest.mark.parametrize("form", ["host", "host_tf", "device", "device_tf"])
def test_domain_errors_need_no_device_and_name_the_argument(fr, native, lib, form):
    call = spellings(lib)[form]
    v = S.view(fr.Config.new, S.M_900)
    cfg, st = v.cfg, v.centre(native)
    centre = C.byref(st)

    def err(rc, code, *words):
        msg = lib.fr_last_error().decode()
        assert rc == code, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    err(call(cfg, None), INVALID, "SCALED PT", "centre is NULL")
    for bits in (-2, 23, 54):
        err(call(cfg, centre, bits=bits), INVALID, "SCALED PT", "bits", "24 .. 53")
    for bad in (-1.0, -0.0625, float("nan"), float("inf"), -float("inf")):
        err(call(cfg, centre, reach=bad), INVALID, "reach")
    err(call(cfg, centre, s=2, reach=2.0 ** 19 + 1.0), INVALID, "reach", "2^20")
    err(call(cfg, centre, s=8, reach=2.0 ** 17 + 0.125), INVALID, "reach")
    for bad in (-1.0, float("nan"), float("inf")):
        err(call(cfg, centre, thickness=bad), INVALID, "thickness")
    err(call(cfg, centre, s=2, thickness=2.0 ** 19 + 1.0), INVALID, "thickness", "2^20")
    err(call(cfg, centre, s=8, thickness=2.0 ** 17 + 0.125), INVALID, "thickness")
    err(call(cfg, centre, tau=-2), INVALID, "threshold")
    err(call(cfg, centre, tau=256), INVALID, "threshold")
    err(call(cfg, centre, s=0), INVALID, "supersample")
    err(call(cfg, centre, s=9), INVALID, "supersample")
    err(call(cfg, centre, channels=2), INVALID, "channels")
    err(call(cfg, centre, y0=5, y1=4), INVALID, "y0 > y1")
    err(call(cfg, centre, y1=cfg.height + 1), INVALID, "y1 > height")
    many = fr.Config.from_buffer_copy(bytes(cfg))
    many.width, many.height = 0x10000, 0x10000
    err(call(many, centre, s=1, has_out=False), INVALID, "width * (y1 - y0)")
    # SCALED PT's own domain, on cfg_s: the axis ratio, the limit, the depth, the cap
    for axis in ("re", "im"):
        thin = fr.Config.from_buffer_copy(bytes(cfg))
        setattr(thin.scale, axis, math.ldexp(-1.0, 900 - 33))
        err(call(thin, centre), INVALID, "2^-32")
    far = fr.Config.from_buffer_copy(bytes(cfg))
    for limit in (2.0 ** 20 * (1 + 2.0 ** -52), 2.0 ** 21):
        far.limit = limit
        err(call(far, centre), INVALID, "limit", "2^20")
    deep = fr.Config.from_buffer_copy(bytes(cfg))
    deep.scale.re = deep.scale.im = math.ldexp(1.0, 952)
    err(call(deep, centre, bits=0), INVALID, "e + 64")
    big = fr.Config.from_buffer_copy(bytes(cfg))
    big.iterations = (1 << 24) + 1
    err(call(big, centre), INVALID, "FR_PT_MAX_ITERATIONS")
    # an unknown transfer is reported first, whatever else is wrong
    if form.endswith("_tf"):
        for bad in (-1, 2, 7):
            err(call(cfg, None, transfer=bad, s=0, tau=300, reach=-1.0), INVALID, "transfer")
    # the buffers, after the domain
    need = 3 * cfg.width * cfg.height
    err(call(cfg, centre, out_len=need - 1), TOO_SMALL, "out_len")
    err(call(cfg, centre, has_out=False), INVALID, "out")
    if form.startswith("device"):
        n = C.c_size_t()
        assert lib.fr_ss_adaptive_de_workspace_bytes(C.byref(cfg), 2, 0, cfg.height, C.byref(n)) == 0 and n.value > 0
        assert n.value == M.workspace_bytes(cfg.width, cfg.height, 0, cfg.height)
        err(call(cfg, centre, work_len=n.value - 1), TOO_SMALL, "work_len", "fr_ss_adaptive_de_workspace_bytes")
        err(call(cfg, centre, d_work=None), INVALID, "d_work")
        err(call(cfg, centre, d_work=0x2004), INVALID, "d_work", "aligned")
        err(call(cfg, centre, d_refined=0x3004), INVALID, "d_refined")
        err(call(cfg, centre, channels=4, d_out=0x1002), INVALID, "d_out", "aligned")
    # a refusal comes before the no-rows shortcut; the valid extremes pass the domain
    err(call(cfg, centre, bits=23, y0=2, y1=2), INVALID, "bits")
    rc = call(cfg, centre, reach=2.0 ** 19, thickness=2.0 ** 19, has_out=False)
    assert rc == INVALID and b"reach" not in lib.fr_last_error() and b"thickness" not in lib.fr_last_error()


def test_null_config_is_refused_by_all_four(lib):
    for rc in (lib.fr_render_rows_ss_adaptive_de_pt_scaled(None, None, -1, 1.0, 2, 8, 2.0, 0, 0, 3, None, 0, None),
               lib.fr_render_rows_ss_adaptive_de_pt_scaled_tf(None, None, -1, 1.0, 2, 0, 8, 2.0, 0, 0, 3, None, 0, None),
               lib.fr_render_rows_ss_adaptive_de_pt_scaled_device(None, None, -1, 1.0, 2, 8, 2.0, 0, 0, 3, None, 0, None, 0, None, None),
               lib.fr_render_rows_ss_adaptive_de_pt_scaled_tf_device(None, None, -1, 1.0, 2, 0, 8, 2.0, 0, 0, 3, None, 0, None, 0, None, None)):
        assert rc == INVALID and b"cfg" in lib.fr_last_error()


def test_empty_row_range_is_a_no_op_without_a_device_or_a_buffer(fr, native, lib):
    v = S.view(fr.Config.new, S.M_900)
    st = v.centre(native)
    for s in (1, 2, 8):
        for bits in (-1, 0, 24, 53):
            for y in (0, 3, v.cfg.height):
                n = C.c_uint64(7)
                assert lib.fr_render_rows_ss_adaptive_de_pt_scaled(C.byref(v.cfg), C.byref(st), bits, 1.0, s, 8, 2.0, y, y, 3, None, 0, C.byref(n)) == 0
                assert n.value == 0
                n = C.c_uint64(7)
                assert lib.fr_render_rows_ss_adaptive_de_pt_scaled_tf(C.byref(v.cfg), C.byref(st), bits, 1.0, s, 1, 8, 2.0, y, y, 4, None, 0,
                                                                      C.byref(n)) == 0
                assert n.value == 0
                assert lib.fr_render_rows_ss_adaptive_de_pt_scaled_device(C.byref(v.cfg), C.byref(st), bits, 1.0, s, 8, 2.0, y, y, 4, None, 0, None,
                                                                          0, None, None) == 0
                assert lib.fr_render_rows_ss_adaptive_de_pt_scaled_tf_device(C.byref(v.cfg), C.byref(st), bits, 1.0, s, 1, 8, 2.0, y, y, 3, None, 0,
                                                                             None, 0, None, None) == 0
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    img, n = fr.get_image_de_adaptive_scaled(v.cfg, 1.0, centre, supersample=3, y0=4, y1=4)
    assert img.shape == (0, v.cfg.width, 3) and n == 0


def test_python_wrapper_checks_its_keywords_and_does_not_fall_back(fr):
    v = S.view(fr.Config.new, S.M_900)
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    for kw in (dict(supersample=0), dict(supersample=9), dict(threshold=-2), dict(threshold=256), dict(channels=2), dict(bla=23),
               dict(bla=54), dict(bla=-1)):
        with pytest.raises(ValueError):
            fr.get_image_de_adaptive_scaled(v.cfg, 1.0, centre, **kw)
    with pytest.raises(ValueError, match="needs centre="):  # a missing centre is refused
        fr.get_image_de_adaptive_scaled(v.cfg, 1.0, None)
    with pytest.raises(TypeError):  # the road takes no dd centre and no precision
        fr.get_image_de_adaptive_scaled(v.cfg, 1.0, centre, pos_lo=(0.0, 0.0))
    for kw in (dict(reach=-1.0), dict(reach=float("nan")), dict(transfer=2)):  # the library's own refusal comes through
        with pytest.raises(fr.FractalHipError) as e:
            fr.get_image_de_adaptive_scaled(v.cfg, 1.0, centre, **kw)
        assert e.value.code == INVALID
    with pytest.raises(fr.FractalHipError) as e:
        fr.get_image_de_adaptive_scaled(v.cfg, -1.0, centre)
    assert e.value.code == INVALID and "thickness" in str(e.value)
    assert "get_image_de_adaptive_scaled" in fr.__all__


def test_a_valid_call_needs_a_device(fr, native, lib):
    """every refusal above came before the device; without one a valid call of each spelling answers FR_ERR_NO_DEVICE.  With
    one, the no-device answer cannot be had: the four symbols are looked up and tests/test_gpu_ss_adaptive_de_scaled.py runs them"""
    calls = spellings(lib)
    for name in ("fr_render_rows_ss_adaptive_de_pt_scaled", "fr_render_rows_ss_adaptive_de_pt_scaled_tf",
                 "fr_render_rows_ss_adaptive_de_pt_scaled_device", "fr_render_rows_ss_adaptive_de_pt_scaled_tf_device"):
        assert getattr(lib, name).argtypes == native.PROTOTYPES[name][1]
    if fr.device_count() > 0:
        return
    v = S.view(fr.Config.new, S.M_900)
    st = v.centre(native)
    fern = fr.Config.from_buffer_copy(bytes(v.cfg))
    fern.algo = int(fr.Algo.BarnsleyFern)
    for name, call in calls.items():
        for cfg in (v.cfg, fern):  # the fern renders black ON THE DEVICE: no shortcut on the host either
            for bits in (-1, 0, 40):
                for s in (1, 2):
                    assert call(cfg, C.byref(st), bits=bits, s=s, transfer=1) == NO_DEVICE, (name, bits, s, lib.fr_last_error())
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    with pytest.raises(fr.FractalHipError) as e:
        fr.get_image_de_adaptive_scaled(v.cfg, 1.0, centre, bla=0)
    assert e.value.code == NO_DEVICE


# ---- 3. the header and the bindings -----------------------------------------------------------------------------------------------


def test_the_header_states_the_definition_and_the_bindings_hold_the_calls(native):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "fractal_hip.h")).read().replace(" * ", " ").split())
    for phrase in ("ADAPTIVE SUPERSAMPLED SCALED DE (fr_render_rows_ss_adaptive_de_pt_scaled(_device) below)",
                   "(z, iters, u) = fr_escape_rows_de_pt_scaled(cfg_s, centre, bits, ...), bit for bit",
                   "cfg_sv = fr_de_scaled_view(cfg_s)", "(double)(s * height) * min(|sre|, |sim|)",
                   "t = -1 gives the bytes of fr_render_rows_ss_de_pt_scaled for every R",
                   "fr_ss_adaptive_de_workspace_bytes serves these calls unchanged", "ss_refine_de_scaled_kernel",
                   # the refusing sections point at the new one, in the file's idiom
                   "FR_PT_ROAD_SCALED is out of scope of THESE calls; ADAPTIVE SUPERSAMPLED SCALED DE below has calls of its own",
                   # and what they said stays
                   "FR_PT_ROAD_SCALED is refused by name, as are FR_PRECISION_F32 and FR_PRECISION_DD"):
        assert " ".join(phrase.replace(" * ", " ").split()) in text, phrase
    assert text.index("ADAPTIVE SUPERSAMPLED DE (fr_render_rows_ss_adaptive_de(_device) below)") \
        < text.index("ADAPTIVE SUPERSAMPLED SCALED DE (fr_render_rows_ss_adaptive_de_pt_scaled") < text.index("LINEAR-LIGHT SUPERSAMPLING (the _tf calls")
    for name in ("fr_render_rows_ss_adaptive_de_pt_scaled", "fr_render_rows_ss_adaptive_de_pt_scaled_device",
                 "fr_render_rows_ss_adaptive_de_pt_scaled_tf", "fr_render_rows_ss_adaptive_de_pt_scaled_tf_device"):
        assert re.search(r"\bint %s\(" % name, text) and name in native.PROTOTYPES
        assert hasattr(native.load(), name)
