"""ADAPTIVE SUPERSAMPLED DE (include/fractal_hip.h) without a device, in three parts: the numpy model of the definition
(tests/ss_adaptive_de_model.py) on the DE arrays of the CPU model (tests/de_model.py) — every consequence the header lists holds;
the domain checks of both forms, which come before any device work and name their argument (fake pointers: nothing is
dereferenced before the checks have passed); and fr_ss_adaptive_de_workspace_bytes against the rule restated in the model."""
import ctypes as C

import numpy as np
import pytest

import de_model as DE
import ss_adaptive_de_model as M
import ss_adaptive_model as A
import ss_de_model as SD

INVALID, TOO_SMALL, NO_DEVICE = 1, 2, 3
F64, F32, DD, PT = 0, 1, 2, 3
PLAIN, BLA, SCALED = 0, 1, 2
T, TAU = 1.0, 8


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


def small(fr, w=16, h=8):
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = w, h, 50
    return cfg


# ---- 1. the model on the CPU model's DE arrays ----------------------------------------------------------------------------------

VIEWS = {"default": DE.default_view, "julia": DE.julia_view}  # 48 x 32 at cap 200, 40 x 24 at cap 300
_arrays = {}


def arrays(fr, view, s):
    key = (view, s)
    if key not in _arrays:
        cfg = VIEWS[view](fr.Config.new())
        z, it, der = DE.f64_rows(SD.config_s(cfg, s))
        for a in (z, it, der):
            a.setflags(write=False)
        _arrays[key] = cfg, z, it, der
    return _arrays[key]


@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("view", list(VIEWS))
def test_model_obeys_every_consequence_of_the_definition(fr, view, s):
    cfg, z, it, der = arrays(fr, view, s)
    w, h, p = cfg.width, cfg.height, s // 2
    H = SD.shaded(cfg, z, it, der, s, T)
    full = SD.colour(cfg, z, it, der, s, T)
    # t = -1: the bytes of SUPERSAMPLED DE, for every R
    for reach in (0.0, 2.0):
        out, n = M.adaptive_de(cfg, z, it, der, s, T, -1, reach)
        assert np.array_equal(out, full) and n == w * h
    # t = 255 with R = 0: the probe image
    out, n = M.adaptive_de(cfg, z, it, der, s, T, 255, 0.0)
    assert np.array_equal(out, H[p::s, p::s]) and n == 0
    # R = 0: the colour rule on the shaded bytes
    out, n = M.adaptive_de(cfg, z, it, der, s, T, TAU, 0.0)
    want, wn = A.adaptive(H, s, TAU)
    assert np.array_equal(out, want) and n == wn
    assert not M.near_only(cfg, z, it, der, s, T, TAU, 0.0).any()
    # T = 0 with R = 0: ADAPTIVE SUPERSAMPLING on the unshaded bytes
    plain = DE.colour(SD.config_s(cfg, s), z, it, der, 0.0, 3)
    assert np.array_equal(plain, DE.base_colours(SD.config_s(cfg, s), z, it))
    out, n = M.adaptive_de(cfg, z, it, der, s, 0.0, TAU, 0.0)
    want, wn = A.adaptive(plain, s, TAU)
    assert np.array_equal(out, want) and n == wn
    # s = 1: the DE render coloured with T, for every t and R
    if s == 1:
        want = DE.colour(cfg, z, it, der, T, 3)
        for tau, reach in ((-1, 0.0), (0, 1.0), (8, 2.0), (255, 0.0), (255, 3.0)):
            assert np.array_equal(M.adaptive_de(cfg, z, it, der, 1, T, tau, reach)[0], want)
    # row pieces sum to the whole
    for reach in (0.0, 2.0):
        whole, total = M.adaptive_de(cfg, z, it, der, s, T, TAU, reach)
        for y0 in (0, 1, 7):
            cuts = [c for c in (0, y0, y0 + 1, h) if c <= h]
            cuts = sorted(set(cuts))
            parts = [M.adaptive_de(cfg, z, it, der, s, T, TAU, reach, a, b) for a, b in zip(cuts, cuts[1:])]
            assert np.array_equal(np.concatenate([q[0] for q in parts]), whole), (reach, y0)
            assert sum(q[1] for q in parts) == total
        rgba, n4 = M.adaptive_de(cfg, z, it, der, s, T, TAU, reach, channels=4)
        assert np.array_equal(rgba[..., :3], whole) and (rgba[..., 3] == 255).all() and n4 == total


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("view", list(VIEWS))
def test_distance_rule_finds_what_the_colour_rule_leaves(fr, view, s):
    """the figures the feature rests on: the colour rule alone leaves pixels further than t from the full supersampled DE image,
    the distance rule marks pixels the colour rule had not, fewer are left, and there is still work to save"""
    cfg, z, it, der = arrays(fr, view, s)
    full = SD.colour(cfg, z, it, der, s, T).astype(np.int32)

    def left(out):
        return int((np.abs(out.astype(np.int32) - full) > TAU).any(axis=-1).sum())

    alone = left(M.adaptive_de(cfg, z, it, der, s, T, TAU, 0.0)[0])
    assert 1 <= alone <= 25
    for reach in (1.0, 2.0, 3.0):
        e, n = M.edge_sets(cfg, z, it, der, s, T, TAU, reach)
        out, refined = M.adaptive_de(cfg, z, it, der, s, T, TAU, reach)
        assert refined == int((e | n).sum())
        assert left(out) <= 2 and left(out) < alone
        assert 69 <= int((n & ~e).sum()) <= 242
        assert 0.17 <= round(float((e | n).mean()), 2) <= 0.42
    # a capped probe is never near, whatever the reach
    p = s // 2
    capped = it[p::s, p::s] == cfg.iterations
    assert capped.any() and not (M.near(cfg, z, it, der, s, 2.0 ** 20 / s) & capped).any()


def test_model_near_rule_on_hand_made_arrays(fr):
    """a flat exterior with one probe close to the set, one with an overflowed derivative and one capped"""
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = 5, 4, 100
    s = 2
    z = np.empty((8, 10, 2))
    z[...] = (300.0, 40.0)
    it = np.full((8, 10), 37, dtype=np.uint32)
    der = np.empty((8, 10, 2))
    der[...] = (1.0e-3, 0.0)  # far from the set
    der[3, 3] = (3600.0, 0.0)  # the probe of (1, 1): D = 1.54 sample pixels
    der[5, 7] = (np.inf, 1.0)  # the probe of (3, 2): D = 0
    it[7, 1], der[7, 1] = 100, (np.inf, 0.0)  # the probe of (0, 3): capped
    D = DE.distance(SD.config_s(cfg, s), z, it, der)
    assert 1.5 < D[3, 3] < 1.6 and D[5, 7] == 0.0 and D[7, 1] == 0.0
    n = M.near(cfg, z, it, der, s, 1.0)  # Rs = 2
    want = np.zeros((4, 5), dtype=bool)
    want[1, 1] = want[2, 3] = True
    assert np.array_equal(n, want)
    assert M.near(cfg, z, it, der, s, 0.75)[2, 3] and not M.near(cfg, z, it, der, s, 0.75)[1, 1]  # Rs = 1.5 < D
    assert not M.near(cfg, z, it, der, s, 0.0).any()
    # unshaded, the three probes' colours equal their neighbours' except the capped one: near is what refines (1, 1) and (3, 2)
    out, refined = M.adaptive_de(cfg, z, it, der, s, 0.0, 255, 1.0)
    assert refined == 2
    fern = cfg.clone()
    fern.algo = int(fr.Algo.BarnsleyFern)
    black, refined = M.adaptive_de(fern, z, it, der, s, T, -1, 1.0, channels=4)
    assert refined == 0 and not black[..., :3].any() and (black[..., 3] == 255).all()


# ---- 2. the domain ----------------------------------------------------------------------------------------------------------------


def ad_host(lib, cfg, s=2, tau=8, thickness=1.0, reach=2.0, y0=0, y1=None, precision=F64, pos_lo=None, centre=None, road=PLAIN, bits=0,
            channels=3, out=None, out_len=None, **_):
    y1 = cfg.height if y1 is None else y1
    if out is None:
        out = np.zeros(max(channels * cfg.width * max(y1 - y0, 0), 1), dtype=np.uint8)
    n = C.c_uint64(7)
    return lib.fr_render_rows_ss_adaptive_de(C.byref(cfg), precision, pos_lo, centre, road, bits, thickness, s, tau, reach, y0, y1, channels,
                                             out.ctypes.data, out.nbytes if out_len is None else out_len, C.byref(n))


def ad_device(lib, cfg, s=2, tau=8, thickness=1.0, reach=2.0, y0=0, y1=None, precision=F64, pos_lo=None, centre=None, road=PLAIN, bits=0,
              channels=3, d_out=0x1000, out_len=1 << 40, d_work=0x2000, work_len=1 << 40, d_refined=0x3000):
    y1 = cfg.height if y1 is None else y1
    return lib.fr_render_rows_ss_adaptive_de_device(C.byref(cfg), precision, pos_lo, centre, road, bits, thickness, s, tau, reach, y0, y1,
                                                    channels, d_out, out_len, d_work, work_len, d_refined, None)


@pytest.mark.parametrize("call", [ad_host, ad_device], ids=["host", "device"])
def test_domain_errors_need_no_device_and_name_the_argument(fr, lib, call):
    from fractal_renderer_amd import _native

    cfg = small(fr)

    def err(rc, code, *words):
        assert rc == code, (rc, lib.fr_last_error())
        msg = lib.fr_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)

    err(call(lib, cfg, s=0), INVALID, "supersample")
    err(call(lib, cfg, s=9), INVALID, "supersample")
    err(call(lib, cfg, y0=5, y1=4), INVALID, "y0 > y1")
    err(call(lib, cfg, y1=cfg.height + 1), INVALID, "y1 > height")
    err(call(lib, cfg, channels=2), INVALID, "channels")
    # the reach and the thickness
    for bad in (-1.0, -0.0625, float("nan"), float("inf"), -float("inf")):
        err(call(lib, cfg, reach=bad), INVALID, "reach")
    err(call(lib, cfg, s=2, reach=2.0 ** 19 + 1.0), INVALID, "reach", "2^20")
    err(call(lib, cfg, s=8, reach=2.0 ** 17 + 0.125), INVALID, "reach")
    for bad in (-1.0, float("nan"), float("inf")):
        err(call(lib, cfg, thickness=bad), INVALID, "thickness")
    err(call(lib, cfg, s=2, thickness=2.0 ** 19 + 1.0), INVALID, "thickness", "2^20")
    err(call(lib, cfg, tau=-2), INVALID, "threshold")
    err(call(lib, cfg, tau=256), INVALID, "threshold")
    many = small(fr)
    many.width, many.height = 0x10000, 0x10000
    err(call(lib, many, s=1), INVALID, "width * (y1 - y0)")
    # the precisions and the roads' argument rule
    st = fr.WideCentre.from_str("-0.75", "0.1", scale=2.0 ** 100).c_struct()
    lo = _native.Imaginary(0.0, 0.0)
    err(call(lib, cfg, precision=PT, road=SCALED, centre=C.byref(st)), INVALID, "FR_PT_ROAD_SCALED")
    err(call(lib, cfg, road=SCALED), INVALID, "FR_PT_ROAD_SCALED")
    err(call(lib, cfg, precision=F32), INVALID, "FR_PRECISION_F32")
    err(call(lib, cfg, precision=DD), INVALID, "FR_PRECISION_DD")
    err(call(lib, cfg, precision=7), INVALID, "precision")
    err(call(lib, cfg, road=3, precision=PT), INVALID, "road")
    err(call(lib, cfg, road=BLA), INVALID, "road", "FR_PRECISION_PT")
    err(call(lib, cfg, bits=40), INVALID, "bits")
    err(call(lib, cfg, pos_lo=C.byref(lo)), INVALID, "pos_lo")
    err(call(lib, cfg, centre=C.byref(st)), INVALID, "centre")
    err(call(lib, cfg, precision=PT, bits=40), INVALID, "bits")
    err(call(lib, cfg, precision=PT, centre=C.byref(st), pos_lo=C.byref(lo)), INVALID, "pos_lo")
    err(call(lib, cfg, precision=PT, road=BLA, centre=C.byref(st), pos_lo=C.byref(lo)), INVALID, "pos_lo")
    err(call(lib, cfg, precision=PT, road=BLA, bits=23), INVALID, "bits")
    err(call(lib, cfg, precision=PT, road=BLA, bits=-1), INVALID, "bits")
    err(call(lib, cfg, precision=PT, road=BLA, bits=54), INVALID, "bits")
    # the road's own DE domain, on cfg_s
    big = small(fr)
    big.iterations = (1 << 24) + 1
    err(call(lib, big, precision=PT), INVALID, "iterations")
    far = small(fr)
    far.limit = 2.0 ** 21
    for kw in (dict(), dict(precision=PT), dict(precision=PT, road=BLA)):
        err(call(lib, far, **kw), INVALID, "limit")
    # the valid extremes pass the domain: what stops the call then is the missing buffer or device, never the argument
    rc = call(lib, cfg, reach=2.0 ** 19, thickness=2.0 ** 19, d_out=None)
    assert rc != INVALID or (b"reach" not in lib.fr_last_error() and b"thickness" not in lib.fr_last_error())
    assert lib.fr_render_rows_ss_adaptive_de(None, F64, None, None, PLAIN, 0, 1.0, 2, 8, 2.0, 0, 0, 3, None, 0, None) == INVALID
    assert b"cfg" in lib.fr_last_error()
    assert lib.fr_render_rows_ss_adaptive_de_device(None, F64, None, None, PLAIN, 0, 1.0, 2, 8, 2.0, 0, 0, 3, None, 0, None, 0, None,
                                                    None) == INVALID
    assert b"cfg" in lib.fr_last_error()


def test_buffer_errors_need_no_device(fr, lib):
    cfg = small(fr)
    need = 3 * cfg.width * cfg.height
    assert ad_host(lib, cfg, out_len=need - 1) == TOO_SMALL and b"out_len" in lib.fr_last_error()
    assert lib.fr_render_rows_ss_adaptive_de(C.byref(cfg), F64, None, None, PLAIN, 0, 1.0, 2, 8, 2.0, 0, cfg.height, 3, None, need,
                                             None) == INVALID
    assert b"out" in lib.fr_last_error()
    assert ad_device(lib, cfg, out_len=need - 1) == TOO_SMALL and b"out_len" in lib.fr_last_error()
    assert ad_device(lib, cfg, d_out=None) == INVALID and b"d_out" in lib.fr_last_error()
    assert ad_device(lib, cfg, channels=4, d_out=0x1002) == INVALID and b"d_out" in lib.fr_last_error() and b"aligned" in lib.fr_last_error()
    n = C.c_size_t()
    assert lib.fr_ss_adaptive_de_workspace_bytes(C.byref(cfg), 2, 0, cfg.height, C.byref(n)) == 0 and n.value > 0
    assert ad_device(lib, cfg, work_len=n.value - 1) == TOO_SMALL and b"work_len" in lib.fr_last_error()
    assert ad_device(lib, cfg, d_work=None) == INVALID and b"d_work" in lib.fr_last_error()
    assert ad_device(lib, cfg, d_work=0x2004) == INVALID and b"d_work" in lib.fr_last_error() and b"aligned" in lib.fr_last_error()
    assert ad_device(lib, cfg, d_refined=0x3004) == INVALID and b"d_refined" in lib.fr_last_error()


def test_empty_row_range_is_a_no_op_without_a_device_or_a_buffer(fr, lib):
    cfg = small(fr)
    st = fr.WideCentre.from_str("-0.75", "0.1", scale=2.0 ** 100).c_struct()
    for s in (1, 2, 8):
        for prec, centre, road in ((F64, None, PLAIN), (PT, None, PLAIN), (PT, None, BLA), (PT, C.byref(st), PLAIN), (PT, C.byref(st), BLA)):
            n = C.c_uint64(7)
            assert lib.fr_render_rows_ss_adaptive_de(C.byref(cfg), prec, None, centre, road, 0, 1.0, s, 8, 2.0, 3, 3, 3, None, 0,
                                                     C.byref(n)) == 0
            assert n.value == 0
            assert lib.fr_render_rows_ss_adaptive_de_device(C.byref(cfg), prec, None, centre, road, 0, 1.0, s, 8, 2.0, 3, 3, 4, None, 0, None,
                                                            0, None, None) == 0
    img, n = fr.get_image_de_adaptive(cfg, supersample=3, y0=4, y1=4)
    assert img.shape == (0, cfg.width, 3) and n == 0


def test_python_wrapper_checks_its_keywords_and_does_not_fall_back(fr):
    cfg = small(fr)
    centre = fr.WideCentre.from_str("-0.75", "0.1", scale=2.0 ** 100)
    for kw in (dict(supersample=0), dict(supersample=9), dict(threshold=-2), dict(threshold=256), dict(channels=2),
               dict(precision=fr.Precision.F32), dict(precision=fr.Precision.DD), dict(bla=0), dict(centre=centre), dict(pos_lo=(0.0, 0.0)),
               dict(precision=fr.Precision.PT, centre=centre, pos_lo=(0.0, 0.0))):
        with pytest.raises(ValueError):
            fr.get_image_de_adaptive(cfg, **kw)
    with pytest.raises(TypeError):  # the scaled road is not offered
        fr.get_image_de_adaptive(cfg, precision=fr.Precision.PT, centre=centre, scaled=True)
    for kw in (dict(reach=-1.0), dict(reach=float("nan")), dict(thickness=-1.0)):  # the library's own refusal comes through
        with pytest.raises(fr.FractalHipError) as e:
            fr.get_image_de_adaptive(cfg, **kw)
        assert e.value.code == INVALID
    if fr.device_count() == 0:
        fern = small(fr)
        fern.algo = int(fr.Algo.BarnsleyFern)
        for c in (cfg, fern):  # the fern renders black ON THE DEVICE: no shortcut on the host either
            for kw in (dict(), dict(precision=fr.Precision.PT), dict(precision=fr.Precision.PT, bla=0)):
                with pytest.raises(fr.FractalHipError) as e:
                    fr.get_image_de_adaptive(c, **kw)
                assert e.value.code == NO_DEVICE


# ---- 3. the workspace -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("s", [1, 2, 8])
@pytest.mark.parametrize("width", [0, 1, 7, 257, 16384])
def test_workspace_bytes_follow_the_rule(fr, lib, s, width):
    cfg = fr.Config.new()
    cfg.width, cfg.height = width, 16384
    for y0, y1 in [(0, 16384), (0, 1), (5, 37), (16383, 16384), (3, 3), (0, 7), (1, 9), (100, 16001)]:
        n = C.c_size_t(123)
        assert lib.fr_ss_adaptive_de_workspace_bytes(C.byref(cfg), s, y0, y1, C.byref(n)) == 0
        assert n.value == M.workspace_bytes(width, 16384, y0, y1), (s, width, y0, y1)
        assert fr.ss_adaptive_de_workspace_bytes(cfg, s, y0, y1) == n.value
        assert n.value % 8 == 0
        if width and y1 > y0:  # the unshaded sibling's workspace plus the probe's 36 bytes per pixel, rounded
            assert n.value > A.workspace_bytes(width, 16384, y0, y1) + 36 * width * (y1 - y0) - 8
        else:
            assert n.value == 0


def test_workspace_bytes_domain(fr, lib):
    cfg = small(fr)
    n = C.c_size_t()
    f = lib.fr_ss_adaptive_de_workspace_bytes
    assert f(C.byref(cfg), 0, 0, 1, C.byref(n)) == INVALID and b"supersample" in lib.fr_last_error()
    assert f(C.byref(cfg), 9, 0, 1, C.byref(n)) == INVALID
    assert f(C.byref(cfg), 2, 2, 1, C.byref(n)) == INVALID
    assert f(C.byref(cfg), 2, 0, cfg.height + 1, C.byref(n)) == INVALID
    assert f(None, 2, 0, 1, C.byref(n)) == INVALID and b"cfg" in lib.fr_last_error()
    assert f(C.byref(cfg), 2, 0, 1, None) == INVALID and b"bytes" in lib.fr_last_error()
