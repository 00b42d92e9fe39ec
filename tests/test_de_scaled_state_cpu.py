"""RESUMABLE SCALED DE and SUPERSAMPLED SCALED DE without a device (include/fractal_hip.h, the two sections of those names).
  - claim 1 on MODELS: z, iters and der of tests/de_scaled_state_model.py's state run are tests/de_scaled_model.py's (bits = -1)
    and w and m are tests/pt_scaled_state_model.py's, at every cap of every chain;
  - claim 2: the state continued link by link, and in one jump, is the state run at the higher cap in all five arrays;
  - claim 3: inside WIDE PT's domain z, iters and m are tests/de_state_model.py's wide state, w is ldexp(dz, e) and ldexp(der, e) is
    its der, as bits;
  - through the library, no device: the domain of the six new calls, each refusal with its status and a message, and the legal
    no-ops; the phrases of the two header sections; the Python refusals.  On the commit before the calls existed these fail for
    lack of the symbols.

The chains are pt_scaled_state_model.CHAINS, unchanged: the derivative changes nothing about (z, iters, w, m), so the conditions
(a) .. (e) that tests/test_pt_scaled_state_cpu.py asserts on them hold here as they hold there."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import de_model as D
import de_scaled_model as DSM
import de_scaled_state_model as U
import de_state_model as DS
import pt_scaled_model as S
import pt_scaled_state_model as T
import pt_wide_model as W

INVALID, TOO_SMALL = 1, 2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fractal_hip.h")


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


def err(lib, rc, status, *words):
    assert rc == status, (rc, message(lib))
    for w in words:
        assert w in message(lib), (w, message(lib))


# ---- claims 1 and 2 on every chain ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(U.CHAINS))
def test_claim_1_z_iters_der_are_scaled_des_and_w_m_are_the_scaled_states(fr, name):
    c = T.chain(fr.Config.new, name)
    sinv = math.ldexp(1.0, -S.exponent(c.cfg(0)))
    for cap in c.caps:
        z, it, w, m, der = U.state(c, cap)
        o = c.orbits(cap)
        dz, dit, dder = DSM.escape_rows(c.cfg(cap), o.x[0], o.k[0] if o.julia else None, DSM.NO_TABLE)[:3]
        assert np.array_equal(it, dit), (name, cap)
        assert S.same_bits(z, dz) and D.same_doubles(der, dder), (name, cap)
        sz, sit, sw, sm = c.state(cap)[0]
        assert np.array_equal(it, sit) and np.array_equal(m, sm) and S.same_bits(z, sz) and S.same_bits(w, sw), (name, cap)
        escaped = it < cap
        assert (w[escaped] == 0).all() and (m[escaped] == 0).all(), "an escaped pixel stores w = (0, 0), m = 0"
    z, it, w, m, der = U.state(c, 0)  # N = 0: RESUMABLE SCALED PT's initial state with der = (Sinv, 0)
    assert (it == 0).all() and (der[..., 0] == sinv).all() and (der[..., 1] == 0).all()
    assert not (U.state(c, c.caps[-1])[4][..., 0] == sinv).any()  # the derivative moves in every pixel


@pytest.mark.parametrize("name", list(U.CHAINS))
def test_claim_2_link_by_link_and_in_one_jump(fr, name):
    c = T.chain(fr.Config.new, name)
    state = U.state(c, c.caps[0])
    for a, b in c.links():
        state = U.continue_rows(c.cfg(b), c.orbits(b), state, a)
        assert U.same_state(state, U.state(c, b)), "%s: %d -> %d" % (name, a, b)
    first, last = c.caps[0], c.caps[-1]
    jump = U.continue_rows(c.cfg(last), c.orbits(last), U.state(c, first), first)
    assert U.same_state(jump, U.state(c, last)), "%s: %d -> %d in one jump" % (name, first, last)


def test_rows_of_the_model_are_slices_of_the_whole_and_no_orbits_is_zeros(fr):
    c = T.chain(fr.Config.new, "M_900")
    piece = U.state_rows(c.cfg(560), c.orbits(560), 5, 12)
    assert U.same_state(piece, tuple(a[5:12] for a in U.state(c, 560)))
    cont = U.continue_rows(c.cfg(600), c.orbits(600), piece, 560, 5, 12)
    assert U.same_state(cont, tuple(a[5:12] for a in U.state(c, 600)))
    assert all(not a.any() for a in U.state_rows(c.cfg(300), None))


# ---- claim 3: inside WIDE PT's domain ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("spec", [S.M_200, S.M_440, S.N_300, S.J_300], ids=["M_200", "M_440", "N_300", "J_300"])
def test_claim_3_inside_wide_pts_domain_the_state_is_the_wide_de_state(fr, spec):
    v = S.view(fr.Config.new, spec)
    e = S.exponent(v.cfg)
    z, it, dz, m, der = DS.pt_wide_state_rows(v.cfg, v.orbits)
    sz, sit, sw, sm, su = U.state_rows(v.cfg, v.orbits)
    assert np.array_equal(sit, it) and np.array_equal(sm, m)
    assert S.same_bits(sz, z)
    assert S.same_bits(sw, np.ldexp(dz, e))  # w = dz 2^e exactly
    assert np.isfinite(der).all() and S.same_bits(np.ldexp(su, e), der)  # der 2^e is its der, exactly
    assert (it == v.cfg.iterations).any() or len(np.unique(it)) > 1


# ---- the library's domain, no device: the state calls ---------------------------------------------------------------------------


def domain_view(fr, native, scale_log2=900, n=16, cap=100):
    cfg = W.view(fr.Config.new(), "M", scale_log2, 16, 12, cap)
    re_, im = W.centre_ints("M", n)
    words = W.to_words(re_, n), W.to_words(im, n)
    p64 = C.POINTER(C.c_uint64)
    st = native.fr_wide_centre(n, words[0].ctypes.data_as(p64), words[1].ctypes.data_as(p64))
    return cfg, st, words


class Arrays:
    NAMES = ("z", "it", "w", "m", "der")

    def __init__(self, cfg, rows):
        npx = rows * cfg.width
        self.a = {"z": np.zeros(2 * npx + 1), "w": np.zeros(2 * npx + 1), "der": np.zeros(2 * npx + 1),
                  "it": np.zeros(npx + 1, dtype=np.uint32), "m": np.zeros(npx + 1, dtype=np.uint32)}

    def ptrs(self, null=None, skew=None):
        p = {k: v.ctypes.data for k, v in self.a.items()}
        if null:
            p[null] = None
        if skew:
            p[skew[0]] += skew[1]
        return tuple(p[k] for k in self.NAMES)

    def untouched(self):
        return all(not v.any() for v in self.a.values())


def calls(lib):
    """the four state calls as f(cfg, centre, y0, y1, from, z, it, w, m, der) -> status; the state renders ignore `from`"""
    ref = lambda cfg: None if cfg is None else C.byref(cfg)  # noqa: E731
    return {
        "state": lambda cfg, st, y0, y1, frm, *a: lib.fr_escape_rows_de_pt_scaled_state(ref(cfg), st, y0, y1, *a),
        "state_device": lambda cfg, st, y0, y1, frm, *a: lib.fr_escape_rows_de_pt_scaled_state_device(ref(cfg), st, y0, y1, *a, None),
        "extend": lambda cfg, st, y0, y1, frm, *a: lib.fr_escape_extend_de_pt_scaled(ref(cfg), st, y0, y1, frm, *a),
        "extend_device": lambda cfg, st, y0, y1, frm, *a: lib.fr_escape_extend_de_pt_scaled_device(ref(cfg), st, y0, y1, frm, *a, None),
    }


CALLS = ["state", "state_device", "extend", "extend_device"]


@pytest.mark.parametrize("call", CALLS)
def test_a_null_array_is_refused(fr, native, lib, call):
    cfg, st, _w = domain_view(fr, native)
    a = Arrays(cfg, 12)
    for null in Arrays.NAMES:
        err(lib, calls(lib)[call](cfg, C.byref(st), 0, 12, 50, *a.ptrs(null=null)), INVALID, "NULL array", "SCALED PT", "w, m and der", "all five")


@pytest.mark.parametrize("call", CALLS)
def test_a_misaligned_array_is_refused(fr, native, lib, call):
    cfg, st, _w = domain_view(fr, native)
    a = Arrays(cfg, 12)
    for skew in (("z", 4), ("w", 4), ("der", 4), ("it", 2), ("m", 2)):
        err(lib, calls(lib)[call](cfg, C.byref(st), 0, 12, 50, *a.ptrs(skew=skew)), INVALID, "z, w and der must be 8-byte aligned")


@pytest.mark.parametrize("call", ["extend", "extend_device"])
def test_a_lower_cap_is_refused(fr, native, lib, call):
    cfg, st, _w = domain_view(fr, native, cap=100)
    a = Arrays(cfg, 12)
    err(lib, calls(lib)[call](cfg, C.byref(st), 0, 12, 101, *a.ptrs()), INVALID, "from_iterations")
    assert calls(lib)[call](cfg, C.byref(st), 0, 0, 101, None, None, None, None, None) == INVALID  # before the rows are looked at


@pytest.mark.parametrize("call", CALLS)
def test_a_scale_of_2_952_and_a_null_centre_are_refused(fr, native, lib, call):
    cfg, st, _w = domain_view(fr, native, 951)
    a = Arrays(cfg, 12)
    assert calls(lib)[call](cfg, C.byref(st), 0, 0, 100, *a.ptrs()) == 0  # 2^951 is inside
    cfg.scale.re = cfg.scale.im = math.ldexp(1.0, 952)
    err(lib, calls(lib)[call](cfg, C.byref(st), 0, 12, 50, *a.ptrs()), INVALID, "SCALED PT", "e + 64")
    cfg, st, _w = domain_view(fr, native)
    err(lib, calls(lib)[call](cfg, None, 0, 12, 50, *a.ptrs()), INVALID, "SCALED PT", "centre is NULL")
    cfg.limit = 2.0 ** 21  # SCALED PT's limit, which is DE's
    err(lib, calls(lib)[call](cfg, C.byref(st), 0, 12, 50, *a.ptrs()), INVALID, "2^20")
    assert calls(lib)[call](None, C.byref(st), 0, 0, 50, *a.ptrs()) == INVALID


@pytest.mark.parametrize("call", CALLS)
def test_the_legal_no_ops_need_no_device(fr, native, lib, call):
    cfg, st, _w = domain_view(fr, native, cap=100)
    a = Arrays(cfg, 12)
    assert calls(lib)[call](cfg, C.byref(st), 5, 5, 100, None, None, None, None, None) == 0  # y0 == y1 needs no arrays either
    assert calls(lib)[call](cfg, C.byref(st), 12, 12, 40, *a.ptrs()) == 0
    assert calls(lib)[call](cfg, C.byref(st), 3, 2, 100, *a.ptrs()) == INVALID
    assert calls(lib)[call](cfg, C.byref(st), 0, 13, 100, *a.ptrs()) == INVALID
    if call.startswith("extend"):
        assert calls(lib)[call](cfg, C.byref(st), 0, 12, 100, *a.ptrs()) == 0  # M == N
        cfg.algo = int(fr.Algo.BarnsleyFern)  # no orbits: the extension does nothing
        assert calls(lib)[call](cfg, C.byref(st), 0, 12, 50, *a.ptrs()) == 0
        assert a.untouched()


# ---- the library's domain, no device: the supersampled calls --------------------------------------------------------------------


def ss_host(lib, cfg, centre, s, bits=-1, thickness=1.0, y0=0, y1=None, channels=3, out_len=None, **_):
    y1 = cfg.height if y1 is None else y1
    out = np.zeros(max(channels * cfg.width * max(y1 - y0, 0), 1), dtype=np.uint8)
    return lib.fr_render_rows_ss_de_pt_scaled(C.byref(cfg), centre, bits, thickness, s, y0, y1, channels, out.ctypes.data,
                                              out.nbytes if out_len is None else out_len)


def ss_device(lib, cfg, centre, s, bits=-1, thickness=1.0, y0=0, y1=None, channels=3, out_len=1 << 40, d_out=0x1000, d_work=0x2000,
              work_len=1 << 40):
    """argument checks only: the pointers are never dereferenced before the checks have passed"""
    y1 = cfg.height if y1 is None else y1
    return lib.fr_render_rows_ss_de_pt_scaled_device(C.byref(cfg), centre, bits, thickness, s, y0, y1, channels, d_out, out_len, d_work,
                                                     work_len, None)


@pytest.mark.parametrize("call", [ss_host, ss_device], ids=["host", "device"])
def test_supersampled_refusals_need_no_device_and_name_the_argument(fr, native, lib, call):
    cfg, st, _w = domain_view(fr, native)
    c = C.byref(st)
    err(lib, call(lib, cfg, c, 0), INVALID, "supersample")
    err(lib, call(lib, cfg, c, 9), INVALID, "supersample")
    err(lib, call(lib, cfg, c, 2, channels=5), INVALID, "channels")
    err(lib, call(lib, cfg, c, 2, y0=5, y1=4), INVALID, "y0 > y1")
    err(lib, call(lib, cfg, c, 2, y1=cfg.height + 1), INVALID, "y1 > height")
    wide = cfg.clone()
    wide.width = 0x40000000
    err(lib, call(lib, wide, c, 4, y1=0), INVALID, "width")
    tall = cfg.clone()
    tall.height = 0x80000000
    err(lib, call(lib, tall, c, 2, y1=0), INVALID, "height")
    # the thickness: T * s within [0, 2^20], finite
    err(lib, call(lib, cfg, c, 2, thickness=-1.0), INVALID, "thickness")
    err(lib, call(lib, cfg, c, 2, thickness=float("nan")), INVALID, "thickness")
    err(lib, call(lib, cfg, c, 2, thickness=float("inf")), INVALID, "thickness")
    err(lib, call(lib, cfg, c, 2, thickness=2.0 ** 19 + 1.0), INVALID, "thickness", "2^20")
    assert call(lib, cfg, c, 2, thickness=2.0 ** 19, y0=3, y1=3) == 0  # T * s == 2^20 is inside
    assert call(lib, cfg, c, 1, thickness=2.0 ** 19 + 1.0, y0=3, y1=3) == 0
    # bits: -1, 0 or 24 .. 53
    for bits in (-2, 1, 23, 54):
        err(lib, call(lib, cfg, c, 2, bits=bits), INVALID, "SCALED PT", "bits")
    for bits in (-1, 0, 24, 40, 53):
        assert call(lib, cfg, c, 2, bits=bits, y0=3, y1=3) == 0
    # DE ON SCALED PT's domain on cfg_s: the centre, the scale, the limit
    err(lib, call(lib, cfg, None, 2), INVALID, "SCALED PT", "centre is NULL")
    far = cfg.clone()
    far.scale.re = far.scale.im = math.ldexp(1.0, 952)
    err(lib, call(lib, far, c, 2), INVALID, "SCALED PT", "e + 64")
    bad = cfg.clone()
    bad.limit = 2.0 ** 21
    err(lib, call(lib, bad, c, 2), INVALID, "2^20")
    assert lib.fr_render_rows_ss_de_pt_scaled(None, c, -1, 1.0, 2, 0, 0, 3, None, 0) == INVALID and b"cfg" in lib.fr_last_error()


def test_supersampled_buffer_refusals_and_no_ops_need_no_device(fr, native, lib):
    cfg, st, _w = domain_view(fr, native)
    c = C.byref(st)
    need = 3 * cfg.width * cfg.height
    for s in (1, 2):  # s = 1 needs its workspace too
        mn = fr.ss_de_workspace_bytes(cfg, s)[0]
        assert mn == 36 * s * cfg.width * min(8 * s, s * cfg.height)
        err(lib, ss_host(lib, cfg, c, s, out_len=need - 1), TOO_SMALL, "out_len")
        err(lib, ss_device(lib, cfg, c, s, out_len=need - 1), TOO_SMALL, "out_len")
        err(lib, ss_device(lib, cfg, c, s, work_len=mn - 1), TOO_SMALL, "work_len", "fr_ss_de_workspace_bytes")
        err(lib, ss_device(lib, cfg, c, s, d_work=None), INVALID, "d_work")
        err(lib, ss_device(lib, cfg, c, s, d_work=0x2004), INVALID, "d_work", "8-byte aligned")
        err(lib, ss_device(lib, cfg, c, s, d_out=None), INVALID, "d_out")
        err(lib, ss_device(lib, cfg, c, s, channels=4, d_out=0x1002), INVALID, "4-byte aligned")
        assert lib.fr_render_rows_ss_de_pt_scaled(C.byref(cfg), c, -1, 1.0, s, 0, cfg.height, 3, None, need) == INVALID
        assert b"out" in lib.fr_last_error()
        # no rows: nothing to do, no device, no buffer
        assert ss_host(lib, cfg, c, s, y0=3, y1=3, out_len=0) == 0
        assert ss_device(lib, cfg, c, s, y0=3, y1=3, out_len=0, d_out=None, d_work=None, work_len=0) == 0
        empty = cfg.clone()
        empty.width = 0
        assert ss_device(lib, empty, c, s, out_len=0, d_out=None, d_work=None, work_len=0) == 0


def test_the_unscaled_supersampled_call_keeps_refusing_the_scaled_road(fr, native, lib):
    cfg, st, _w = domain_view(fr, native)
    out = np.zeros(3 * cfg.width * cfg.height, dtype=np.uint8)
    rc = lib.fr_render_rows_ss_de(C.byref(cfg), 3, None, C.byref(st), 2, -1, 1.0, 2, 0, cfg.height, 3, out.ctypes.data, out.nbytes)
    err(lib, rc, INVALID, "FR_PT_ROAD_SCALED", "SCALED PT", "out of scope")


# ---- the header -----------------------------------------------------------------------------------------------------------------


def section(title):
    text = open(HEADER).read()
    start = text.index(" * " + title + " (")
    return re.sub(r"\s+", " ", re.sub(r"\n \*", " ", text[start:text.index("*/", start)]))  # one paragraph, single spaces


def test_the_header_defines_resumable_scaled_de():
    s = section("RESUMABLE SCALED DE")
    for phrase in ("(z, w, m, onK, u)", "RESUMABLE SCALED PT's state run, word for word", "bits = -1", "ENDED BY ESCAPE", "BIG and not BIG",
                   "u0 = (Sinv, 0)", "bs0 = Sinv for Mandelbrot and 0 for Julia", "t = (z.re + z.re, z.im + z.im)",
                   "nu = (fma(t.re, u.re, fma(-t.im, u.im, bs0)), fma(t.re, u.im, t.im * u.re))", "A rebase never touches u",
                   "56 bytes per pixel", "(z, iters, w, m, der)", "(next, i, w = (0, 0), m = 0, nu)", "(z, N, w, m | onK << 31, u)",
                   "der = (Sinv, 0)", "zeros into all five arrays", "CLAIM 1", "CLAIM 2", "CLAIM 3", "a NaN in der is any NaN",
                   "fr_escape_rows_de_pt_scaled's with bits = -1", "fr_escape_rows_pt_scaled_state's", "fr_escape_rows_de_pt_state's",
                   "w = dz 2^e", "der 2^e is its der", "u reads only z", "does not depend on where a run was interrupted",
                   "the centre REQUIRED", "no bits argument", "M >= N", "M == N is a legal no-op", "all five arrays non-NULL",
                   "z, w and der 8-byte aligned", "iters and m 4-byte aligned", "The table form (bits >= 0) has no state",
                   "i + 2^k <= iterations"):
        assert phrase in s, phrase


def test_the_header_defines_supersampled_scaled_de():
    s = section("SUPERSAMPLED SCALED DE")
    for phrase in ("fr_render_rows_ss_de keeps refusing FR_PT_ROAD_SCALED", "cfg_s = cfg with width * s and height * s",
                   "fr_escape_rows_de_pt_scaled(cfg_s, centre, bits, ...), bit for bit", "bits is -1, 0 or 24 .. 53",
                   "over the whole image of cfg_s", "cfg_sv = fr_de_scaled_view(cfg_s)", "Ts = T * (double)s, one f64 product",
                   "fr_colour_de_rows_device(cfg_sv, z, iters, u, n, Ts, 3)", "(double)(s * height) * min(|sre|, |sim|)",
                   "integer box filter of H", "floor(s*s / 2)", "s = 1 is fr_escape_rows_de_pt_scaled followed by",
                   "fr_colour_de_rows_device(cfg_v, ..., T, channels), byte for byte",
                   "T = 0 gives the bytes of fr_render_rows_ss_pt(..., FR_PT_ROAD_SCALED, bits, s)", "An algorithm without orbits gives black",
                   "s in 1 .. FR_SS_MAX", "fit in 32 bits", "0 <= T * s <= 2^20", "channels 3 or 4", "fr_ss_de_workspace_bytes",
                   "36 bytes per sample", "No colour or filter kernel is added or changed"):
        assert phrase in s, phrase
    text = open(HEADER).read()
    for name in ("fr_escape_rows_de_pt_scaled_state", "fr_escape_rows_de_pt_scaled_state_device", "fr_escape_extend_de_pt_scaled",
                 "fr_escape_extend_de_pt_scaled_device", "fr_render_rows_ss_de_pt_scaled", "fr_render_rows_ss_de_pt_scaled_device"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
    assert "#define FR_ABI_VERSION 3" in text


# ---- Python ---------------------------------------------------------------------------------------------------------------------


def test_python_refusals_and_no_ops(fr):
    c = T.chain(fr.Config.new, "N_900")
    cfg = c.cfg(7)
    centre = fr.WideCentre(c.n, re=c.words[0], im=c.words[1])
    with pytest.raises(ValueError, match="centre="):
        fr.escape_rows_de_pt_scaled_state(cfg, None)
    z, it, w, m, der = fr.escape_rows_de_pt_scaled_state(cfg, centre, y0=4, y1=4)  # no rows: no device
    assert z.shape == (0, 16, 2) and m.shape == (0, 16) and der.shape == (0, 16, 2)
    with pytest.raises(ValueError, match="centre="):
        fr.extend_rows_de_pt_scaled(cfg, z, it, w, m, der, 7, None, y0=4, y1=4)
    with pytest.raises(ValueError, match="rows"):
        fr.extend_rows_de_pt_scaled(cfg, np.zeros((3, 16, 2)), it, w, m, der, 7, centre, y0=4, y1=4)
    same = fr.extend_rows_de_pt_scaled(cfg, z, it, w, m, der, 7, centre, y0=4, y1=4)
    assert len(same) == 5 and same[4].shape == (0, 16, 2)
    with pytest.raises(fr.FractalHipError, match="from_iterations"):
        fr.extend_rows_de_pt_scaled(cfg, z, it, w, m, der, 8, centre, y0=4, y1=4)
    with pytest.raises(ValueError, match="supersample"):
        fr.get_image_de_scaled_ss(cfg, 1.0, centre, 9)
    with pytest.raises(ValueError, match="channels"):
        fr.get_image_de_scaled_ss(cfg, 1.0, centre, 2, channels=5)
    with pytest.raises(ValueError, match="centre="):
        fr.get_image_de_scaled_ss(cfg, 1.0, None, 2)
    with pytest.raises(ValueError, match="bla="):
        fr.get_image_de_scaled_ss(cfg, 1.0, centre, 2, bla=23)
    with pytest.raises(fr.FractalHipError, match="thickness"):
        fr.get_image_de_scaled_ss(cfg, 2.0 ** 20, centre, 2, y0=4, y1=4)
    assert fr.get_image_de_scaled_ss(cfg, 1.0, centre, 2, y0=4, y1=4, channels=4).shape == (0, 16, 4)
    with pytest.raises(ValueError, match="get_image_de_scaled_ss"):  # the unscaled front keeps refusing, and says where to go
        fr.get_image_de(cfg, precision=fr.Precision.PT, centre=centre, scaled=True, supersample=2)
