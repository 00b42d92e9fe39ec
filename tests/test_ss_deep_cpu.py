"""Anti-aliased deep views (include/fractal_hip.h, "supersampled rendering on the deep roads": fr_render_rows_ss_pt(_device),
fr_colour_rows_ss_device, fr_colour_ss_rgb8) without a device: every refusal comes before any device work — it is checked on
a box that has none — and names the argument; the legal no-ops need no device; a well-formed call answers FR_ERR_NO_DEVICE
and the Python wrappers raise ValueError for their own rules before any C call."""
import ctypes as C
import math

import numpy as np
import pytest

INVALID, TOO_SMALL, NO_DEVICE = 1, 2, 3
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


def deep(fr, log2scale=300, w=16, h=8):
    """(a view at 2^log2scale, a wide centre with the words that scale asks for)"""
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations, cfg.limit = w, h, 50, 2.0
    cfg.scale.re = cfg.scale.im = math.ldexp(1.0, log2scale)
    centre = fr.WideCentre.from_str("-0.75", "0.1", scale=cfg.scale.re)
    return cfg, centre


def err(lib, rc, code, *words):
    assert rc == code, (rc, lib.fr_last_error())
    msg = lib.fr_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def ss_host(lib, cfg, s, road, bits=0, pos_lo=None, centre=None, y0=0, y1=None, channels=3, out_len=None, **_):
    y1 = cfg.height if y1 is None else y1
    out = np.zeros(max(channels * cfg.width * max(y1 - y0, 0), 1), dtype=np.uint8)
    return lib.fr_render_rows_ss_pt(C.byref(cfg), pos_lo, centre, road, bits, s, y0, y1, channels, out.ctypes.data,
                                    out.nbytes if out_len is None else out_len)


def ss_device(lib, cfg, s, road, bits=0, pos_lo=None, centre=None, y0=0, y1=None, channels=3, out_len=1 << 40, d_out=0x1000,
              d_work=0x2000, work_len=1 << 40):
    """argument checks only: the pointers are never dereferenced before the checks have passed"""
    y1 = cfg.height if y1 is None else y1
    return lib.fr_render_rows_ss_pt_device(C.byref(cfg), pos_lo, centre, road, bits, s, y0, y1, channels, d_out, out_len, d_work,
                                           work_len, None)


@pytest.mark.parametrize("call", [ss_host, ss_device], ids=["host", "device"])
def test_render_refusals_need_no_device_and_name_the_argument(fr, native, lib, call):
    cfg, wc = deep(fr)
    st = wc.c_struct()
    c = C.byref(st)
    lo = C.byref(native.Imaginary(0.0, 0.0))
    shallow = fr.Config.new()
    shallow.width, shallow.height, shallow.iterations = 16, 8, 50
    for road, kw in ((PLAIN, dict(centre=c)), (BLA, dict(centre=c)), (SCALED, dict(centre=c, bits=-1)), (PLAIN, dict())):
        view = cfg if kw else shallow
        err(lib, call(lib, view, 0, road, **kw), INVALID, "supersample")
        err(lib, call(lib, view, 9, road, **kw), INVALID, "supersample")
        err(lib, call(lib, view, 2, road, channels=5, **kw), INVALID, "channels")
        err(lib, call(lib, view, 2, road, y0=5, y1=4, **kw), INVALID, "y0 > y1")
        err(lib, call(lib, view, 2, road, y1=view.height + 1, **kw), INVALID, "y1 > height")
        wide = view.clone()
        wide.width = 0x40000000
        err(lib, call(lib, wide, 4, road, y1=0, **kw), INVALID, "width")
        tall = view.clone()
        tall.height = 0x80000000
        err(lib, call(lib, tall, 2, road, y1=0, **kw), INVALID, "height")
    err(lib, call(lib, cfg, 2, 3, centre=c), INVALID, "road")
    err(lib, call(lib, cfg, 2, -1, centre=c), INVALID, "road")
    # bits per road
    err(lib, call(lib, cfg, 2, PLAIN, bits=40, centre=c), INVALID, "bits")
    err(lib, call(lib, shallow, 2, PLAIN, bits=-1), INVALID, "bits")
    err(lib, call(lib, cfg, 2, BLA, bits=23, centre=c), INVALID, "bits")
    err(lib, call(lib, cfg, 2, BLA, bits=-1, centre=c), INVALID, "bits")
    err(lib, call(lib, cfg, 2, BLA, bits=54, centre=c), INVALID, "bits")
    err(lib, call(lib, cfg, 2, SCALED, bits=23, centre=c), INVALID, "bits")
    err(lib, call(lib, cfg, 2, SCALED, bits=-2, centre=c), INVALID, "bits")
    # the centre per road
    err(lib, call(lib, cfg, 2, SCALED, bits=-1), INVALID, "centre is NULL")
    for road, bits in ((PLAIN, 0), (BLA, 0), (SCALED, -1)):
        err(lib, call(lib, cfg, 2, road, bits=bits, centre=c, pos_lo=lo), INVALID, "pos_lo")
    err(lib, call(lib, cfg, 2, SCALED, bits=-1, pos_lo=lo), INVALID, "pos_lo")
    # a centre too coarse for its scale: 2^300 needs six words, this one has two
    coarse = fr.WideCentre(2).c_struct()
    for road, bits in ((PLAIN, 0), (BLA, 0), (SCALED, -1)):
        err(lib, call(lib, cfg, 2, road, bits=bits, centre=C.byref(coarse)), INVALID, "too coarse")
    # past 2^440 the plain and the BLA road refuse; SCALED PT takes the view (the empty range passes every check)
    far, fc = deep(fr, 900)
    fst = fc.c_struct()
    err(lib, call(lib, far, 2, PLAIN, centre=C.byref(fst)), INVALID, "2^440")
    err(lib, call(lib, far, 2, BLA, centre=C.byref(fst)), INVALID, "2^440")
    assert call(lib, far, 2, SCALED, bits=-1, centre=C.byref(fst), y0=3, y1=3) == 0
    assert call(lib, far, 2, SCALED, bits=40, centre=C.byref(fst), y0=3, y1=3) == 0
    # the road's own domain is checked on cfg_s
    bad = cfg.clone()
    bad.limit = float("inf")
    err(lib, call(lib, bad, 2, PLAIN, centre=c), INVALID, "wide centre")
    err(lib, call(lib, bad, 2, SCALED, bits=-1, centre=c), INVALID, "SCALED PT")
    err(lib, call(lib, bad, 2, PLAIN), INVALID, "FR_PRECISION_PT")
    big = cfg.clone()
    big.iterations = (1 << 24) + 1
    err(lib, call(lib, big, 2, BLA, centre=c), INVALID, "iterations")
    assert lib.fr_render_rows_ss_pt(None, None, c, PLAIN, 0, 2, 0, 0, 3, None, 0) == INVALID and b"cfg" in lib.fr_last_error()


def test_render_buffer_refusals_need_no_device(fr, native, lib):
    cfg, wc = deep(fr)
    st = wc.c_struct()
    c = C.byref(st)
    need = 3 * cfg.width * cfg.height
    mn = C.c_size_t()
    assert lib.fr_ss_workspace_bytes(C.byref(cfg), 2, 0, cfg.height, C.byref(mn), None) == 0 and mn.value > 0
    for road, bits in ((PLAIN, 0), (BLA, 0), (SCALED, -1), (SCALED, 40)):
        kw = dict(bits=bits, centre=c)
        err(lib, ss_host(lib, cfg, 2, road, out_len=need - 1, **kw), TOO_SMALL, "out_len")
        assert lib.fr_render_rows_ss_pt(C.byref(cfg), None, c, road, bits, 2, 0, cfg.height, 3, None, need) == INVALID
        assert b"out" in lib.fr_last_error()
        err(lib, ss_device(lib, cfg, 2, road, out_len=need - 1, **kw), TOO_SMALL, "out_len")
        err(lib, ss_device(lib, cfg, 2, road, d_out=None, **kw), INVALID, "d_out")
        err(lib, ss_device(lib, cfg, 2, road, channels=4, d_out=0x1002, **kw), INVALID, "aligned")
        err(lib, ss_device(lib, cfg, 2, road, work_len=mn.value - 1, **kw), TOO_SMALL, "work_len")
        err(lib, ss_device(lib, cfg, 2, road, d_work=None, **kw), INVALID, "d_work")


def test_colour_refusals_need_no_device(fr, lib):
    cfg = fr.Config.new()
    dev, host = lib.fr_colour_rows_ss_device, lib.fr_colour_ss_rgb8
    z, it, out = np.zeros(64 * 4), np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint8)

    def d(z_width=2, width=2, rows=2, s=2, channels=3, d_z=0x1000, d_iters=0x2000, d_out=0x3000, out_len=1 << 40):
        return dev(C.byref(cfg), d_z, z_width, d_iters, width, rows, s, channels, d_out, out_len, None)

    def h(z_width=2, width=2, rows=2, s=2, channels=3, out_len=64, zp=z.ctypes.data, ip=it.ctypes.data, op=out.ctypes.data, **_):
        return host(C.byref(cfg), zp, z_width, ip, width, rows, s, channels, op, out_len)

    for call in (d, h):
        err(lib, call(z_width=3), INVALID, "z_width")
        err(lib, call(z_width=0), INVALID, "z_width")
        err(lib, call(s=0), INVALID, "supersample")
        err(lib, call(s=9), INVALID, "supersample")
        err(lib, call(channels=5), INVALID, "channels")
        err(lib, call(channels=2), INVALID, "channels")
        err(lib, call(width=0x40000000, rows=0, s=4), INVALID, "width")
        err(lib, call(width=0, rows=0x80000000, s=2), INVALID, "rows")
        err(lib, call(out_len=3 * 2 * 2 - 1), TOO_SMALL, "out_len")
        err(lib, call(channels=4, out_len=4 * 2 * 2 - 1), TOO_SMALL, "out_len")
    err(lib, d(d_z=0x1004), INVALID, "d_z", "aligned")
    err(lib, d(d_iters=0x2002), INVALID, "d_iters", "aligned")
    err(lib, d(channels=4, d_out=0x3002), INVALID, "aligned")
    err(lib, d(d_z=None), INVALID, "NULL")
    err(lib, d(d_iters=None), INVALID, "NULL")
    err(lib, d(d_out=None), INVALID, "NULL")
    err(lib, h(zp=None), INVALID, "NULL")
    assert dev(None, 0x1000, 2, 0x2000, 2, 2, 2, 3, 0x3000, 64, None) == INVALID and b"cfg" in lib.fr_last_error()
    assert host(None, z.ctypes.data, 2, it.ctypes.data, 2, 2, 2, 3, out.ctypes.data, 64) == INVALID and b"cfg" in lib.fr_last_error()


def test_empty_calls_are_legal_without_a_device(fr, native, lib):
    cfg, wc = deep(fr)
    st = wc.c_struct()
    c = C.byref(st)
    for s in (1, 2, 8):
        for road, bits in ((PLAIN, 0), (BLA, 0), (BLA, 30), (SCALED, -1), (SCALED, 0)):
            assert lib.fr_render_rows_ss_pt(C.byref(cfg), None, c, road, bits, s, 3, 3, 3, None, 0) == 0
            assert lib.fr_render_rows_ss_pt_device(C.byref(cfg), None, c, road, bits, s, 3, 3, 4, None, 0, None, 0, None) == 0
        assert lib.fr_render_rows_ss_pt(C.byref(cfg), None, None, PLAIN, 0, s, 0, 0, 3, None, 0) == 0  # the dd centre (cfg.pos)
    empty = cfg.clone()
    empty.width = 0
    assert lib.fr_render_rows_ss_pt(C.byref(empty), None, c, SCALED, -1, 2, 0, empty.height, 3, None, 0) == 0
    assert fr.get_image_ss_pt(cfg, 3, centre=wc, y0=4, y1=4).shape == (0, cfg.width, 3)
    for width, rows in ((0, 5), (5, 0), (0, 0)):
        for s in (1, 3):
            assert lib.fr_colour_rows_ss_device(C.byref(cfg), None, 2, None, width, rows, s, 3, None, 0, None) == 0
            assert lib.fr_colour_ss_rgb8(C.byref(cfg), None, 4, None, width, rows, s, 4, None, 0) == 0
    assert fr.colour_image_ss(cfg, np.zeros((0, 6, 2)), np.zeros((0, 6), dtype=np.uint32), 2).shape == (0, 3, 3)


def test_well_formed_calls_do_not_fall_back_without_a_device(fr, native, lib):
    if fr.device_count() > 0:
        pytest.skip("a HIP device is present")
    cfg, wc = deep(fr)
    far, fc = deep(fr, 900)
    fern = cfg.clone()
    fern.algo = int(fr.Algo.BarnsleyFern)  # black ON THE DEVICE: no shortcut on the host either
    shallow = fr.Config.new()
    shallow.width, shallow.height, shallow.iterations = 16, 8, 50
    calls = [lambda: fr.get_image_ss_pt(cfg, 2, centre=wc), lambda: fr.get_image_ss_pt(cfg, 1, centre=wc),
             lambda: fr.get_image_ss_pt(cfg, 3, centre=wc, bla=0), lambda: fr.get_image_ss_pt(cfg, 3, centre=wc, bla=30, channels=4),
             lambda: fr.get_image_ss_pt(far, 2, centre=fc, scaled=True), lambda: fr.get_image_ss_pt(far, 8, centre=fc, scaled=True, bla=0),
             lambda: fr.get_image_ss_pt(fern, 2, centre=wc), lambda: fr.get_image_ss_pt(shallow, 2),
             lambda: fr.get_image_ss_pt(shallow, 2, pos_lo=(0.0, 0.0), bla=0, y0=2, y1=5),
             lambda: fr.colour_image_ss(cfg, np.zeros((4, 6, 2)), np.zeros((4, 6), dtype=np.uint32), 2),
             lambda: fr.colour_image_ss(fern, np.zeros((4, 6, 4)), np.zeros((4, 6), dtype=np.uint32), 1, channels=4)]
    for call in calls:
        with pytest.raises(fr.FractalHipError) as e:
            call()
        assert e.value.code == NO_DEVICE
    # the device forms: every check passes (the pointers are not read before a device exists)
    st = wc.c_struct()
    assert ss_device(lib, cfg, 2, BLA, centre=C.byref(st)) == NO_DEVICE
    assert lib.fr_colour_rows_ss_device(C.byref(cfg), 0x1000, 2, 0x2000, 2, 2, 2, 3, 0x3000, 12, None) == NO_DEVICE


def test_python_wrappers_check_their_own_rules(fr):
    cfg, wc = deep(fr)
    for kw in (dict(scaled=True), dict(scaled=True, pos_lo=(0.0, 0.0)), dict(centre=wc, pos_lo=(0.0, 0.0)), dict(bla=23),
               dict(bla=54), dict(bla=-1), dict(centre=wc, bla=7), dict(centre=wc, scaled=True, bla=60), dict(channels=5),
               dict(channels=1, centre=wc)):
        with pytest.raises(ValueError):
            fr.get_image_ss_pt(cfg, 2, **kw)
    for s in (0, 9, -1):
        with pytest.raises(ValueError, match="supersample"):
            fr.get_image_ss_pt(cfg, s, centre=wc)
        with pytest.raises(ValueError, match="supersample"):
            fr.colour_image_ss(cfg, np.zeros((4, 4, 2)), np.zeros((4, 4), dtype=np.uint32), s)
        with pytest.raises(ValueError, match="supersample"):
            fr.colour_rows_ss_device(cfg, 0x1000, 0x2000, 2, 2, s, 0x3000)
    z, it = np.zeros((4, 6, 2)), np.zeros((4, 6), dtype=np.uint32)
    for bad_z, bad_it, s in ((z, it, 4), (z, it[:, :4], 2), (np.zeros((4, 6, 3)), it, 2), (np.zeros((4, 6)), it, 2), (z, it, 3)):
        with pytest.raises(ValueError):
            fr.colour_image_ss(cfg, bad_z, bad_it, s)
    with pytest.raises(ValueError):
        fr.colour_image_ss(cfg, z, it, 2, channels=5)
    with pytest.raises(ValueError):
        fr.colour_rows_ss_device(cfg, 0x1000, 0x2000, 2, 2, 2, 0x3000, z_width=3)
    with pytest.raises(ValueError):
        fr.colour_rows_ss_device(cfg, 0x1000, 0x2000, 2, 2, 2, 0x3000, channels=2)
    # the road and bits the keywords select
    from fractal_renderer_amd import _ss_pt_road

    assert _ss_pt_road(None, None, None, False) == (PLAIN, 0) and _ss_pt_road((0, 0), None, None, False) == (PLAIN, 0)
    assert _ss_pt_road(None, wc, None, False) == (PLAIN, 0)
    assert _ss_pt_road(None, wc, 0, False) == (BLA, 0) and _ss_pt_road((0, 0), None, 30, False) == (BLA, 30)
    assert _ss_pt_road(None, wc, None, True) == (SCALED, -1) and _ss_pt_road(None, wc, 0, True) == (SCALED, 0)
    assert _ss_pt_road(None, wc, 53, True) == (SCALED, 53)
