"""SUPERSAMPLED DE (include/fractal_hip.h: fr_render_rows_ss_de(_device), fr_ss_de_workspace_bytes, fr_colour_de_rows_ss_device,
fr_colour_de_ss_rgb8) without a device: every refusal comes before any device work — it is checked on a box that has none —
and names the argument; the legal no-ops need no device; the workspace rule is the band rule at 36 bytes per sample; and the
numpy model of the definition (tests/ss_de_model.py) gives the bytes worked out by hand for 2 x 2 samples."""
import ctypes as C
import math

import numpy as np
import pytest

import ss_de_model as M

INVALID, TOO_SMALL = 1, 2
F64, F32, DD, PT = 0, 1, 2, 3
PLAIN, BLA, SCALED = 0, 1, 2


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


def err(lib, rc, code, *words):
    assert rc == code, (rc, lib.fr_last_error())
    msg = lib.fr_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def shallow(fr, w=16, h=8):
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = w, h, 50
    return cfg


def deep(fr, log2scale=300, w=16, h=8):
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations, cfg.limit = w, h, 50, 2.0
    cfg.scale.re = cfg.scale.im = math.ldexp(1.0, log2scale)
    return cfg, fr.WideCentre.from_str("-0.75", "0.1", scale=cfg.scale.re)


def ss_host(lib, cfg, s, precision=F64, road=PLAIN, bits=0, pos_lo=None, centre=None, thickness=1.0, y0=0, y1=None, channels=3,
            out_len=None, **_):
    y1 = cfg.height if y1 is None else y1
    out = np.zeros(max(channels * cfg.width * max(y1 - y0, 0), 1), dtype=np.uint8)
    return lib.fr_render_rows_ss_de(C.byref(cfg), precision, pos_lo, centre, road, bits, thickness, s, y0, y1, channels, out.ctypes.data,
                                    out.nbytes if out_len is None else out_len)


def ss_device(lib, cfg, s, precision=F64, road=PLAIN, bits=0, pos_lo=None, centre=None, thickness=1.0, y0=0, y1=None, channels=3,
              out_len=1 << 40, d_out=0x1000, d_work=0x2000, work_len=1 << 40):
    """argument checks only: the pointers are never dereferenced before the checks have passed"""
    y1 = cfg.height if y1 is None else y1
    return lib.fr_render_rows_ss_de_device(C.byref(cfg), precision, pos_lo, centre, road, bits, thickness, s, y0, y1, channels, d_out,
                                           out_len, d_work, work_len, None)


@pytest.mark.parametrize("call", [ss_host, ss_device], ids=["host", "device"])
def test_render_refusals_need_no_device_and_name_the_argument(fr, native, lib, call):
    cfg = shallow(fr)
    dcfg, wc = deep(fr)
    st = wc.c_struct()
    c = C.byref(st)
    lo = C.byref(native.Imaginary(0.0, 0.0))
    for view, kw in ((cfg, dict()), (cfg, dict(precision=PT)), (dcfg, dict(precision=PT, centre=c)),
                     (dcfg, dict(precision=PT, centre=c, road=BLA))):
        err(lib, call(lib, view, 0, **kw), INVALID, "supersample")
        err(lib, call(lib, view, 9, **kw), INVALID, "supersample")
        err(lib, call(lib, view, 2, channels=2, **kw), INVALID, "channels")
        err(lib, call(lib, view, 2, y0=5, y1=4, **kw), INVALID, "y0 > y1")
        err(lib, call(lib, view, 2, y1=view.height + 1, **kw), INVALID, "y1 > height")
        wide = view.clone()
        wide.width = 0x40000000
        err(lib, call(lib, wide, 4, y1=0, **kw), INVALID, "width")
        tall = view.clone()
        tall.height = 0x80000000
        err(lib, call(lib, tall, 2, y1=0, **kw), INVALID, "height")
        # the thickness: T * s within [0, 2^20], finite
        err(lib, call(lib, view, 2, thickness=-1.0, **kw), INVALID, "thickness")
        err(lib, call(lib, view, 2, thickness=float("nan"), **kw), INVALID, "thickness")
        err(lib, call(lib, view, 2, thickness=float("inf"), **kw), INVALID, "thickness")
        err(lib, call(lib, view, 2, thickness=2.0 ** 19 + 1.0, **kw), INVALID, "thickness", "2^20")
        assert call(lib, view, 2, thickness=2.0 ** 19, y0=3, y1=3, **kw) == 0  # T * s == 2^20 is inside
        assert call(lib, view, 1, thickness=2.0 ** 19 + 1.0, y0=3, y1=3, **kw) == 0
    # refused by name
    err(lib, call(lib, cfg, 2, precision=F32), INVALID, "FR_PRECISION_F32", "FR_PRECISION_DD", "out of scope")
    err(lib, call(lib, cfg, 2, precision=DD), INVALID, "FR_PRECISION_F32", "FR_PRECISION_DD", "out of scope")
    err(lib, call(lib, dcfg, 2, precision=PT, road=SCALED, bits=-1, centre=c), INVALID, "FR_PT_ROAD_SCALED", "SCALED PT", "out of scope")
    err(lib, call(lib, cfg, 2, precision=PT, road=3), INVALID, "road")
    err(lib, call(lib, cfg, 2, precision=PT, road=-1), INVALID, "road")
    # the centre: never both; the F64 road takes neither, no table and no bits
    err(lib, call(lib, dcfg, 2, precision=PT, centre=c, pos_lo=lo), INVALID, "pos_lo")
    err(lib, call(lib, dcfg, 2, precision=PT, road=BLA, centre=c, pos_lo=lo), INVALID, "pos_lo")
    err(lib, call(lib, cfg, 2, precision=F64, pos_lo=lo), INVALID, "pos_lo")
    err(lib, call(lib, cfg, 2, precision=F64, centre=c), INVALID, "centre")
    err(lib, call(lib, cfg, 2, precision=F64, road=BLA), INVALID, "FR_PT_ROAD_BLA")
    err(lib, call(lib, cfg, 2, precision=F64, bits=40), INVALID, "bits")
    # bits per road, fr_render_rows_ss_pt's rules
    err(lib, call(lib, cfg, 2, precision=PT, bits=40), INVALID, "bits")
    err(lib, call(lib, dcfg, 2, precision=PT, bits=-1, centre=c), INVALID, "bits")
    for bits in (23, -1, 54):
        err(lib, call(lib, dcfg, 2, precision=PT, road=BLA, bits=bits, centre=c), INVALID, "bits")
    # the road's own DE domain is checked on cfg_s
    bad = cfg.clone()
    bad.limit = 2.0 ** 21
    err(lib, call(lib, bad, 2), INVALID, "limit", "2^20")
    err(lib, call(lib, bad, 2, precision=PT, road=BLA), INVALID, "limit")
    far, fc = deep(fr, 900)
    fst = fc.c_struct()
    err(lib, call(lib, far, 2, precision=PT, centre=C.byref(fst)), INVALID, "2^440")
    err(lib, call(lib, far, 2, precision=PT, road=BLA, centre=C.byref(fst)), INVALID, "2^440")
    coarse = fr.WideCentre(2).c_struct()
    err(lib, call(lib, dcfg, 2, precision=PT, centre=C.byref(coarse)), INVALID, "too coarse")
    big = dcfg.clone()
    big.iterations = (1 << 24) + 1
    err(lib, call(lib, big, 2, precision=PT, road=BLA, centre=c), INVALID, "iterations")
    assert lib.fr_render_rows_ss_de(None, F64, None, None, PLAIN, 0, 1.0, 2, 0, 0, 3, None, 0) == INVALID and b"cfg" in lib.fr_last_error()


def test_render_buffer_refusals_and_no_ops_need_no_device(fr, native, lib):
    cfg = shallow(fr)
    dcfg, wc = deep(fr)
    st = wc.c_struct()
    c = C.byref(st)
    need = 3 * cfg.width * cfg.height
    for view, kw in ((cfg, dict()), (dcfg, dict(precision=PT, centre=c)), (dcfg, dict(precision=PT, road=BLA, centre=c))):
        for s in (1, 2):  # s = 1 needs its workspace too
            mn = fr.ss_de_workspace_bytes(view, s)[0]
            assert mn > 0
            err(lib, ss_host(lib, view, s, out_len=need - 1, **kw), TOO_SMALL, "out_len")
            err(lib, ss_device(lib, view, s, out_len=need - 1, **kw), TOO_SMALL, "out_len")
            err(lib, ss_device(lib, view, s, work_len=mn - 1, **kw), TOO_SMALL, "work_len", "fr_ss_de_workspace_bytes")
            err(lib, ss_device(lib, view, s, d_work=None, **kw), INVALID, "d_work")
            err(lib, ss_device(lib, view, s, d_work=0x2004, **kw), INVALID, "d_work", "8-byte aligned")
            err(lib, ss_device(lib, view, s, d_out=None, **kw), INVALID, "d_out")
            err(lib, ss_device(lib, view, s, channels=4, d_out=0x1002, **kw), INVALID, "4-byte aligned")
            assert lib.fr_render_rows_ss_de(C.byref(view), kw.get("precision", F64), None, kw.get("centre"), kw.get("road", PLAIN), 0, 1.0, s,
                                            0, view.height, 3, None, need) == INVALID and b"out" in lib.fr_last_error()
            # no rows: nothing to do, no device, no buffer
            assert ss_host(lib, view, s, y0=3, y1=3, out_len=0, **kw) == 0
            assert ss_device(lib, view, s, y0=3, y1=3, out_len=0, d_out=None, d_work=None, work_len=0, **kw) == 0
            empty = view.clone()
            empty.width = 0
            assert ss_device(lib, empty, s, out_len=0, d_out=None, d_work=None, work_len=0, **kw) == 0


def colour_device(lib, cfg, s, width=16, rows=8, thickness=1.0, channels=3, d_z=0x1000, d_iters=0x2000, d_der=0x3000, d_out=0x4000,
                  out_len=1 << 40):
    return lib.fr_colour_de_rows_ss_device(C.byref(cfg), d_z, d_iters, d_der, width, rows, s, thickness, channels, d_out, out_len, None)


def colour_host(lib, cfg, s, width=16, rows=8, thickness=1.0, channels=3, out_len=None, **_):
    n = max(s, 1) ** 2 * width * rows
    z, der, it = np.zeros(max(2 * n, 1)), np.zeros(max(2 * n, 1)), np.zeros(max(n, 1), dtype=np.uint32)
    out = np.zeros(max(channels * width * rows, 1), dtype=np.uint8)
    return lib.fr_colour_de_ss_rgb8(C.byref(cfg), z.ctypes.data, it.ctypes.data, der.ctypes.data, width, rows, s, thickness, channels,
                                    out.ctypes.data, out.nbytes if out_len is None else out_len)


@pytest.mark.parametrize("call", [colour_host, colour_device], ids=["host", "device"])
def test_recolour_refusals_need_no_device(fr, lib, call):
    cfg = shallow(fr)
    err(lib, call(lib, cfg, 0), INVALID, "supersample")
    err(lib, call(lib, cfg, 9), INVALID, "supersample")
    err(lib, call(lib, cfg, 4, width=0x40000000, rows=0), INVALID, "32 bits")
    err(lib, call(lib, cfg, 4, width=0, rows=0x40000000), INVALID, "32 bits")
    tall = cfg.clone()
    tall.height = 0x80000000
    err(lib, call(lib, tall, 2), INVALID, "32 bits")
    err(lib, call(lib, cfg, 2, channels=2), INVALID, "channels")
    err(lib, call(lib, cfg, 2, thickness=-0.5), INVALID, "thickness")
    err(lib, call(lib, cfg, 2, thickness=float("nan")), INVALID, "thickness")
    err(lib, call(lib, cfg, 4, thickness=2.0 ** 18 + 1.0), INVALID, "thickness")
    err(lib, call(lib, cfg, 2, out_len=3 * 16 * 8 - 1), TOO_SMALL, "out_len")
    assert call(lib, cfg, 2, width=0, out_len=0) == 0 and call(lib, cfg, 2, rows=0, out_len=0) == 0  # empty: a no-op
    if call is colour_device:
        assert call(lib, cfg, 2, rows=0, d_z=None, d_iters=None, d_der=None, d_out=None, out_len=0) == 0
        for name in ("d_z", "d_iters", "d_der", "d_out"):
            err(lib, call(lib, cfg, 2, **{name: None}), INVALID, "NULL")
        err(lib, call(lib, cfg, 2, d_der=0x3004), INVALID, "d_der", "8-byte aligned")
        err(lib, call(lib, cfg, 2, d_z=0x1004), INVALID, "8-byte aligned")
        err(lib, call(lib, cfg, 2, d_iters=0x2002), INVALID, "4-byte aligned")
        err(lib, call(lib, cfg, 2, channels=4, d_out=0x4001), INVALID, "RGBA8", "4-byte aligned")
    assert lib.fr_colour_de_rows_ss_device(None, 8, 8, 8, 1, 1, 2, 1.0, 3, 8, 3, None) == INVALID and b"cfg" in lib.fr_last_error()


def test_python_front_end_refuses_before_any_c_call(fr):
    cfg = shallow(fr)
    z, it = np.zeros((4, 4, 2)), np.zeros((4, 4), dtype=np.uint32)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            fr.get_image_de(cfg, supersample=bad)
        with pytest.raises(ValueError):
            fr.colour_image_de_ss(cfg, z, it, z, bad, 1.0)
        with pytest.raises(ValueError):
            fr.colour_de_rows_ss_device(cfg, 8, 8, 8, 2, 2, bad, 1.0, 8)
    with pytest.raises(ValueError):
        fr.get_image_de(cfg, supersample=2, channels=5)
    with pytest.raises(ValueError):
        fr.get_image_de(cfg, supersample=2, bla=0)  # bla= needs Precision.PT
    with pytest.raises(ValueError):
        fr.colour_image_de_ss(cfg, z, it, z, 3, 1.0)  # 4 x 4 samples are no whole 3 x 3 blocks
    with pytest.raises(fr.FractalHipError) as e:
        fr.get_image_de(cfg, supersample=2, precision=fr.Precision.DD)
    assert e.value.code == INVALID and "out of scope" in str(e.value)
    assert fr.get_image_de(cfg, supersample=2, y0=3, y1=3).shape == (0, 16, 3)


# ---- the workspace: ss_band_rows' rule at 36 bytes per sample ------------------------------------------------------------------


def band_rule(width, rows_out, s):
    """(min_bytes, best_bytes) of include/fractal_hip.h, restated: a source row is 36 * s * width bytes"""
    row_bytes, rows = 36 * s * width, s * rows_out
    mn = min(8 * s, rows) * row_bytes
    return mn, max(mn, min(rows * row_bytes, 1 << 30))


@pytest.mark.parametrize("s", range(1, 9))
def test_workspace_is_the_band_rule_at_36_bytes_per_sample(fr, lib, s):
    for width in (1, 65, 1000):
        for height, y0, y1 in ((40, 0, 3), (40, 5, 13), (40, 0, 8), (40, 3, 40), (700, 0, 700)):
            cfg = shallow(fr, width, height)
            got = fr.ss_de_workspace_bytes(cfg, s, y0, y1)
            assert got == band_rule(width, y1 - y0, s), (s, width, y0, y1)
            assert got[0] > 0 and got[0] % 36 == 0  # s = 1 needs its workspace too: the arrays must live somewhere
    cfg = shallow(fr, 1000, 700)
    if s == 8:
        assert fr.ss_de_workspace_bytes(cfg, s)[1] == 1 << 30  # 36 * 64 * 700000 bytes: the cap holds
    assert fr.ss_de_workspace_bytes(cfg, s, 4, 4) == (0, 0)
    mn = C.c_size_t()
    assert lib.fr_ss_de_workspace_bytes(C.byref(cfg), s, 0, 700, C.byref(mn), None) == 0 and mn.value == 8 * s * 36 * s * 1000
    assert lib.fr_ss_de_workspace_bytes(C.byref(cfg), s, 0, 700, None, None) == 0


def test_workspace_refusals(fr, lib):
    cfg = shallow(fr)
    for s in (0, 9):
        err(lib, lib.fr_ss_de_workspace_bytes(C.byref(cfg), s, 0, 8, None, None), INVALID, "supersample")
    err(lib, lib.fr_ss_de_workspace_bytes(C.byref(cfg), 2, 5, 4, None, None), INVALID, "y0 > y1")
    err(lib, lib.fr_ss_de_workspace_bytes(None, 2, 0, 0, None, None), INVALID, "cfg")


# ---- the model of the definition against bytes worked out by hand ---------------------------------------------------------------


def hand_config(fr, height=1):
    """One output pixel of 2 x 2 samples.  The flat colour map with iters / iterations * exposure = 128 / 256 * 2 = 1 gives an
    escaped sample the stored colour itself, (r, b, g) = (201, 50, 100); a sample at z = 0 is inside and, with inside off, black.
    scale 0.5: the distance's last factor is (s * height) * 0.5 = height sample pixels per unit."""
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = 1, height, 256
    cfg.scale.re = cfg.scale.im = 0.5
    cfg.smooth, cfg.inside, cfg.exposure = 0, 0, 2.0
    cfg.primary_color.r, cfg.primary_color.g, cfg.primary_color.b = 201, 100, 50
    return cfg


def hand_samples():
    """z = (1024, 0): |z| ln|z| = 1024 * 20 * (ln 2 / 2) = 7097.827...; with |d| = 4725 the distance is 1.50218 units.
       [0, 0] |d| = 4725    D = 1.50218 * pixels
       [0, 1] |d| = 1       D = 7097.8 * pixels: far
       [1, 0] capped, z = 0 D = 0 by definition, never shaded, black
       [1, 1] d = 0         D = +inf: nothing is near"""
    z = np.array([[[1024.0, 0.0], [1024.0, 0.0]], [[0.0, 0.0], [1024.0, 0.0]]])
    it = np.array([[128, 128], [256, 128]], dtype=np.uint32)
    der = np.array([[[4725.0, 0.0], [1.0, 0.0]], [[1.0, 0.0], [0.0, 0.0]]])
    return z, it, der


def test_model_gives_the_hand_computed_bytes(fr):
    z, it, der = hand_samples()
    cfg = hand_config(fr)
    # T = 1.5, s = 2: Ts = 3 sample pixels, pixels = 1: sample [0, 0] has s = 1.50218 / 3 = 0.500727 and its bytes are
    # 201 * s = 100.65 -> 100, 50 * s = 25.04 -> 25, 100 * s = 50.07 -> 50; the other three keep theirs
    H = M.shaded(cfg, z, it, der, 2, 1.5)
    assert H.tolist() == [[[100, 25, 50], [201, 50, 100]], [[0, 0, 0], [201, 50, 100]]]
    # (100 + 201 + 0 + 201 + 2) // 4 = 126, (25 + 50 + 0 + 50 + 2) // 4 = 31, (50 + 100 + 0 + 100 + 2) // 4 = 63
    assert M.colour(cfg, z, it, der, 2, 1.5).tolist() == [[[126, 31, 63]]]
    assert M.colour(cfg, z, it, der, 2, 1.5, channels=4).tolist() == [[[126, 31, 63, 255]]]
    # T = 0: no shading: (3 * 201 + 2) // 4 = 151, (3 * 50 + 2) // 4 = 38, (3 * 100 + 2) // 4 = 75
    assert M.colour(cfg, z, it, der, 2, 0.0).tolist() == [[[151, 38, 75]]]
    # the WHOLE image's height enters the distance, not the rows at hand: at height 2 the same arrays are one row of two, pixels
    # = 2, D = 3.004 > Ts and nothing is shaded
    assert M.colour(hand_config(fr, 2), z, it, der, 2, 1.5).tolist() == [[[151, 38, 75]]]
    # a thicker line reaches it again: T = 3.5, Ts = 7, s = 3.00436 / 7 = 0.42919: 86, 21, 42
    assert M.shaded(hand_config(fr, 2), z, it, der, 2, 3.5)[0, 0].tolist() == [86, 21, 42]
    # s = 1 over the same four samples as a 2 x 2 image: Ts = T, pixels = height * 0.5 = 1, no filter
    one = hand_config(fr, 2)
    one.width = 2
    assert M.colour(one, z, it, der, 1, 3.0).tolist() == [[[100, 25, 50], [201, 50, 100]], [[0, 0, 0], [201, 50, 100]]]


def test_box_filter_of_the_model_truncates_and_rounds_half_up():
    big = np.zeros((3, 6, 3), dtype=np.uint8)
    big[..., 0] = [[1, 0, 0, 255, 255, 255], [0, 0, 0, 255, 255, 255], [0, 0, 3, 255, 255, 254]]
    big[..., 1] = 9
    out = M.box(big, 3)
    # (4 + 4) // 9 = 0, (9 * 255 - 1 + 4) // 9 = 255; nine nines are nine
    assert out.tolist() == [[[0, 9, 0], [255, 9, 0]]]
    big[0, 1, 0] = 1  # (5 + 4) // 9 = 1
    assert M.box(big, 3)[0, 0, 0] == 1
