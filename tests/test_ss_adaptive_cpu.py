"""ADAPTIVE SUPERSAMPLING (include/fractal_hip.h) without a device, in three parts: the numpy model of the definition
(tests/ss_adaptive_model.py) on images of the CPU oracle — its consequences hold; the domain checks of both forms, which come
before any device work and name their argument (fake pointers: nothing is dereferenced before the checks have passed); and
fr_ss_adaptive_workspace_bytes against the rule restated in the model."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import ss_adaptive_model as A

INVALID, TOO_SMALL, NO_DEVICE = 1, 2, 3
F64, F32, DD, PT = 0, 1, 2, 3
PLAIN, BLA, SCALED = 0, 1, 2


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


# ---- 1. the model on oracle images ------------------------------------------------------------------------------------------


def oracle_big(fr, s, w, h, julia=False):
    cfg = fr.Config.new(fr.Algo.Julia) if julia else fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = s * w, s * h, 200
    return O.get_image(O.Config.from_buffer_copy(bytes(cfg)))


@pytest.mark.parametrize("julia", [False, True], ids=["mandelbrot", "julia"])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_model_consequences_on_oracle_images(fr, s, julia):
    w, h = 37, 29
    big = oracle_big(fr, s, w, h, julia)
    assert big.shape == (s * h, s * w, 3)
    p = s // 2
    out, n = A.adaptive(big, s, -1)
    assert np.array_equal(out, A.np_filter(big, s)) and n == w * h
    out, n = A.adaptive(big, s, 255)
    assert np.array_equal(out, big[p::s, p::s]) and n == 0
    if s == 1:  # F = P = H
        for tau in (-1, 0, 8, 255):
            assert np.array_equal(A.adaptive(big, 1, tau)[0], big)
    # the edge set shrinks as tau grows, and it is not trivial on these views
    prev = A.edges(big, s, -1)
    for tau in (0, 8, 40, 255):
        e = A.edges(big, s, tau)
        assert not (e & ~prev).any(), tau
        prev = e
    assert 0.05 <= A.edge_share(big, s, 8) <= 0.95
    # row pieces are the whole image's rows, and the counts add up
    for tau in (0, 8):
        whole, total = A.adaptive(big, s, tau)
        parts = [A.adaptive(big, s, tau, a, b) for a, b in ((0, 7), (7, 8), (8, h))]
        assert np.array_equal(np.concatenate([q[0] for q in parts]), whole)
        assert sum(q[1] for q in parts) == total
        rgba, _ = A.adaptive(big, s, tau, channels=4)
        assert np.array_equal(rgba[..., :3], whole) and (rgba[..., 3] == 255).all()


def test_model_edge_rule_on_a_hand_made_image():
    """one bright probe in a flat field: it and its 8 neighbours are edges, clipped at the image's border"""
    s = 2
    big = np.zeros((8, 10, 3), dtype=np.uint8)
    big[1, 1] = (0, 9, 0)  # the probe of output pixel (0, 0): p = 1
    e = A.edges(big, s, 8)
    want = np.zeros((4, 5), dtype=bool)
    want[:2, :2] = True
    assert np.array_equal(e, want)
    assert not A.edges(big, s, 9).any()
    out, n = A.adaptive(big, s, 8)
    assert n == 4 and out[0, 0, 1] == (9 + 2) // 4 and not out[1:, :, :].any()
    black, n = A.adaptive(big, s, 8, channels=4, escape_algo=False)
    assert n == 0 and not black[..., :3].any() and (black[..., 3] == 255).all()


# ---- 2. the domain ----------------------------------------------------------------------------------------------------------


def ad_host(lib, cfg, s=2, tau=8, y0=0, y1=None, precision=F64, pos_lo=None, centre=None, road=PLAIN, bits=0, channels=3, out=None,
            out_len=None, **_):
    y1 = cfg.height if y1 is None else y1
    if out is None:
        out = np.zeros(max(channels * cfg.width * max(y1 - y0, 0), 1), dtype=np.uint8)
    n = C.c_uint64(7)
    return lib.fr_render_rows_ss_adaptive(C.byref(cfg), precision, pos_lo, centre, road, bits, s, tau, y0, y1, channels, out.ctypes.data,
                                          out.nbytes if out_len is None else out_len, C.byref(n))


def ad_device(lib, cfg, s=2, tau=8, y0=0, y1=None, precision=F64, pos_lo=None, centre=None, road=PLAIN, bits=0, channels=3, d_out=0x1000,
              out_len=1 << 40, d_work=0x2000, work_len=1 << 40, d_refined=0x3000):
    y1 = cfg.height if y1 is None else y1
    return lib.fr_render_rows_ss_adaptive_device(C.byref(cfg), precision, pos_lo, centre, road, bits, s, tau, y0, y1, channels, d_out,
                                                 out_len, d_work, work_len, d_refined, None)


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
    wide = small(fr)
    wide.width = 0x40000000
    err(call(lib, wide, s=4, y1=0), INVALID, "width")
    tall = small(fr)
    tall.height = 0x80000000
    err(call(lib, tall, s=2, y1=0), INVALID, "height")
    err(call(lib, cfg, y0=5, y1=4), INVALID, "y0 > y1")
    err(call(lib, cfg, y1=cfg.height + 1), INVALID, "y1 > height")
    err(call(lib, cfg, channels=2), INVALID, "channels")
    err(call(lib, cfg, tau=-2), INVALID, "threshold")
    err(call(lib, cfg, tau=256), INVALID, "threshold")
    many = small(fr)
    many.width, many.height = 0x10000, 0x10000
    err(call(lib, many, s=1), INVALID, "width * (y1 - y0)")
    # the precisions and the roads' argument rules
    err(call(lib, cfg, precision=F32), INVALID, "FR_PRECISION_F32")
    err(call(lib, cfg, precision=DD), INVALID, "FR_PRECISION_DD")
    err(call(lib, cfg, precision=7), INVALID, "precision")
    err(call(lib, cfg, road=3, precision=PT), INVALID, "road")
    err(call(lib, cfg, road=BLA), INVALID, "road", "FR_PRECISION_PT")
    err(call(lib, cfg, road=SCALED), INVALID, "road", "FR_PRECISION_PT")
    err(call(lib, cfg, bits=40), INVALID, "bits")
    lo = _native.Imaginary(0.0, 0.0)
    err(call(lib, cfg, pos_lo=C.byref(lo)), INVALID, "pos_lo")
    st = fr.WideCentre.from_str("-0.75", "0.1", scale=2.0 ** 100).c_struct()
    err(call(lib, cfg, centre=C.byref(st)), INVALID, "centre")
    err(call(lib, cfg, precision=PT, bits=40), INVALID, "bits")
    err(call(lib, cfg, precision=PT, centre=C.byref(st), pos_lo=C.byref(lo)), INVALID, "pos_lo")
    err(call(lib, cfg, precision=PT, road=BLA, bits=23), INVALID, "bits")
    err(call(lib, cfg, precision=PT, road=BLA, bits=-1), INVALID, "bits")
    err(call(lib, cfg, precision=PT, road=SCALED), INVALID, "centre")
    err(call(lib, cfg, precision=PT, road=SCALED, centre=C.byref(st), pos_lo=C.byref(lo)), INVALID, "pos_lo")
    err(call(lib, cfg, precision=PT, road=SCALED, centre=C.byref(st), bits=54), INVALID, "bits")
    # the road's own domain, on cfg_s
    big = small(fr)
    big.iterations = (1 << 24) + 1
    err(call(lib, big, precision=PT), INVALID, "iterations")
    bad = small(fr)
    bad.limit = float("inf")
    err(call(lib, bad, precision=PT), INVALID, "FR_PRECISION_PT")
    err(call(lib, bad, precision=PT, road=BLA), INVALID, "FR_PRECISION_PT")
    assert lib.fr_render_rows_ss_adaptive(None, F64, None, None, PLAIN, 0, 2, 8, 0, 0, 3, None, 0, None) == INVALID
    assert b"cfg" in lib.fr_last_error()
    assert lib.fr_render_rows_ss_adaptive_device(None, F64, None, None, PLAIN, 0, 2, 8, 0, 0, 3, None, 0, None, 0, None, None) == INVALID
    assert b"cfg" in lib.fr_last_error()


def test_buffer_errors_need_no_device(fr, lib):
    cfg = small(fr)
    need = 3 * cfg.width * cfg.height
    assert ad_host(lib, cfg, out_len=need - 1) == TOO_SMALL and b"out_len" in lib.fr_last_error()
    assert lib.fr_render_rows_ss_adaptive(C.byref(cfg), F64, None, None, PLAIN, 0, 2, 8, 0, cfg.height, 3, None, need, None) == INVALID
    assert b"out" in lib.fr_last_error()
    assert ad_device(lib, cfg, out_len=need - 1) == TOO_SMALL and b"out_len" in lib.fr_last_error()
    assert ad_device(lib, cfg, d_out=None) == INVALID and b"d_out" in lib.fr_last_error()
    assert ad_device(lib, cfg, channels=4, d_out=0x1002) == INVALID and b"aligned" in lib.fr_last_error()
    n = C.c_size_t()
    assert lib.fr_ss_adaptive_workspace_bytes(C.byref(cfg), 2, 0, cfg.height, C.byref(n)) == 0 and n.value > 0
    assert ad_device(lib, cfg, work_len=n.value - 1) == TOO_SMALL and b"work_len" in lib.fr_last_error()
    assert ad_device(lib, cfg, d_work=None) == INVALID and b"d_work" in lib.fr_last_error()
    assert ad_device(lib, cfg, d_work=0x2004) == INVALID and b"d_work" in lib.fr_last_error() and b"aligned" in lib.fr_last_error()
    assert ad_device(lib, cfg, d_refined=0x3004) == INVALID and b"d_refined" in lib.fr_last_error()


def test_empty_row_range_is_a_no_op_without_a_device_or_a_buffer(fr, lib):
    cfg = small(fr)
    st = fr.WideCentre.from_str("-0.75", "0.1", scale=2.0 ** 100).c_struct()
    for s in (1, 2, 8):
        for args in ((F64, None, PLAIN, 0), (PT, None, PLAIN, 0), (PT, None, BLA, 0), (PT, C.byref(st), SCALED, -1)):
            prec, centre, road, bits = args
            n = C.c_uint64(7)
            assert lib.fr_render_rows_ss_adaptive(C.byref(cfg), prec, None, centre, road, bits, s, 8, 3, 3, 3, None, 0, C.byref(n)) == 0
            assert n.value == 0
            assert lib.fr_render_rows_ss_adaptive_device(C.byref(cfg), prec, None, centre, road, bits, s, 8, 3, 3, 4, None, 0, None, 0, None,
                                                         None) == 0
    img, n = fr.get_image_ss_adaptive(cfg, 3, y0=4, y1=4)
    assert img.shape == (0, cfg.width, 3) and n == 0


def test_python_wrapper_checks_its_keywords_and_does_not_fall_back(fr):
    cfg = small(fr)
    centre = fr.WideCentre.from_str("-0.75", "0.1", scale=2.0 ** 100)
    for kw in (dict(supersample=0), dict(supersample=9), dict(supersample=2, threshold=-2), dict(supersample=2, threshold=256),
               dict(supersample=2, channels=2), dict(supersample=2, precision=fr.Precision.F32), dict(supersample=2, precision=fr.Precision.DD),
               dict(supersample=2, bla=0), dict(supersample=2, centre=centre), dict(supersample=2, pos_lo=(0.0, 0.0)),
               dict(supersample=2, precision=fr.Precision.PT, scaled=True),
               dict(supersample=2, precision=fr.Precision.PT, centre=centre, pos_lo=(0.0, 0.0))):
        with pytest.raises(ValueError):
            fr.get_image_ss_adaptive(cfg, **kw)
    if fr.device_count() == 0:
        fern = small(fr)
        fern.algo = int(fr.Algo.BarnsleyFern)
        for c in (cfg, fern):  # the fern renders black ON THE DEVICE: no shortcut on the host either
            for kw in (dict(), dict(precision=fr.Precision.PT), dict(precision=fr.Precision.PT, bla=0),
                       dict(precision=fr.Precision.PT, centre=centre, scaled=True)):
                with pytest.raises(fr.FractalHipError) as e:
                    fr.get_image_ss_adaptive(c, 2, **kw)
                assert e.value.code == NO_DEVICE


# ---- 3. the workspace -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("s", [1, 2, 8])
@pytest.mark.parametrize("width", [0, 1, 7, 257, 16384])
def test_workspace_bytes_follow_the_rule(fr, lib, s, width):
    cfg = fr.Config.new()
    cfg.width, cfg.height = width, 16384
    for y0, y1 in [(0, 16384), (0, 1), (5, 37), (16383, 16384), (3, 3), (0, 7), (1, 9), (100, 16001)]:
        n = C.c_size_t(123)
        assert lib.fr_ss_adaptive_workspace_bytes(C.byref(cfg), s, y0, y1, C.byref(n)) == 0
        assert n.value == A.workspace_bytes(width, 16384, y0, y1), (s, width, y0, y1)
        assert fr.ss_adaptive_workspace_bytes(cfg, s, y0, y1) == n.value
        assert n.value % 8 == 0


def test_workspace_bytes_domain(fr, lib):
    cfg = small(fr)
    n = C.c_size_t()
    f = lib.fr_ss_adaptive_workspace_bytes
    assert f(C.byref(cfg), 0, 0, 1, C.byref(n)) == INVALID and b"supersample" in lib.fr_last_error()
    assert f(C.byref(cfg), 9, 0, 1, C.byref(n)) == INVALID
    assert f(C.byref(cfg), 2, 2, 1, C.byref(n)) == INVALID
    assert f(C.byref(cfg), 2, 0, cfg.height + 1, C.byref(n)) == INVALID
    assert f(None, 2, 0, 1, C.byref(n)) == INVALID and b"cfg" in lib.fr_last_error()
    assert f(C.byref(cfg), 2, 0, 1, None) == INVALID and b"bytes" in lib.fr_last_error()
