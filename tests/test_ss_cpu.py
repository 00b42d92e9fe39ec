"""Supersampled rendering (include/fractal_hip.h, "supersampled rendering") without a device: the domain checks come
before any device work and name the argument, fr_ss_workspace_bytes follows the band rule restated here, the Python
wrappers raise FR_ERR_NO_DEVICE instead of falling back, and the empty row range is legal."""
import ctypes as C

import numpy as np
import pytest

INVALID, TOO_SMALL, NO_DEVICE = 1, 2, 3
F64, F32, DD, PT = 0, 1, 2, 3
GIB = 1 << 30


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


def ss_host(lib, cfg, s, y0=0, y1=None, precision=F64, pos_lo=None, channels=3, out=None, out_len=None):
    y1 = cfg.height if y1 is None else y1
    if out is None:
        out = np.zeros(max(channels * cfg.width * max(y1 - y0, 0), 1), dtype=np.uint8)
    return lib.fr_render_rows_ss(C.byref(cfg), precision, pos_lo, s, y0, y1, channels, out.ctypes.data,
                                 out.nbytes if out_len is None else out_len, None)


def ss_device(lib, cfg, s, y0=0, y1=None, precision=F64, pos_lo=None, channels=3, d_out=0x1000, out_len=1 << 40,
              d_work=0x2000, work_len=1 << 40):
    """argument checks only: the pointers are never dereferenced before the checks have passed"""
    y1 = cfg.height if y1 is None else y1
    return lib.fr_render_rows_ss_device(C.byref(cfg), precision, pos_lo, s, y0, y1, channels, d_out, out_len, d_work,
                                        work_len, None, None)


@pytest.mark.parametrize("call", [ss_host, ss_device], ids=["host", "device"])
def test_domain_errors_need_no_device_and_name_the_argument(fr, lib, call):
    from fractal_renderer_amd import _native

    cfg = small(fr)

    def err(rc, code, *words):
        assert rc == code, (rc, lib.fr_last_error())
        msg = lib.fr_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)

    err(call(lib, cfg, 0), INVALID, "supersample")
    err(call(lib, cfg, 9), INVALID, "supersample")
    wide = small(fr)
    wide.width = 0x40000000
    err(call(lib, wide, 4, y1=0), INVALID, "width")
    tall = small(fr)
    tall.height = 0x80000000
    err(call(lib, tall, 2, y1=0), INVALID, "height")
    err(call(lib, cfg, 2, y0=5, y1=4), INVALID, "y0 > y1")
    err(call(lib, cfg, 2, y1=cfg.height + 1), INVALID, "y1 > height")
    err(call(lib, cfg, 2, channels=2), INVALID, "channels")
    err(call(lib, cfg, 2, channels=5), INVALID, "channels")
    err(call(lib, cfg, 2, precision=7), INVALID, "precision")
    lo = _native.Imaginary(0.0, 0.0)
    err(call(lib, cfg, 2, precision=F64, pos_lo=C.byref(lo)), INVALID, "pos_lo")
    err(call(lib, cfg, 2, precision=F32, pos_lo=C.byref(lo)), INVALID, "pos_lo")
    # the precision's own domain, on cfg_s
    bad = small(fr)
    bad.limit = float("inf")
    err(call(lib, bad, 2, precision=DD), INVALID, "FR_PRECISION_DD")
    err(call(lib, bad, 2, precision=PT), INVALID, "FR_PRECISION_PT")
    big = small(fr)
    big.iterations = (1 << 24) + 1
    err(call(lib, big, 2, precision=PT), INVALID, "iterations")
    unnorm = _native.Imaginary(1.0, 0.0)  # pos + pos_lo does not round to pos
    err(call(lib, cfg, 3, precision=DD, pos_lo=C.byref(unnorm)), INVALID, "pos_lo")
    assert lib.fr_render_rows_ss(None, F64, None, 2, 0, 0, 3, None, 0, None) == INVALID
    assert b"cfg" in lib.fr_last_error()


def test_buffer_errors_need_no_device(fr, lib):
    cfg = small(fr)
    need = 3 * cfg.width * cfg.height
    assert ss_host(lib, cfg, 2, out_len=need - 1) == TOO_SMALL and b"out_len" in lib.fr_last_error()
    assert lib.fr_render_rows_ss(C.byref(cfg), F64, None, 2, 0, cfg.height, 3, None, need, None) == INVALID
    assert b"out" in lib.fr_last_error()
    assert ss_device(lib, cfg, 2, out_len=need - 1) == TOO_SMALL and b"out_len" in lib.fr_last_error()
    assert ss_device(lib, cfg, 2, d_out=None) == INVALID and b"d_out" in lib.fr_last_error()
    assert ss_device(lib, cfg, 2, channels=4, d_out=0x1002) == INVALID and b"aligned" in lib.fr_last_error()
    mn, best = C.c_size_t(), C.c_size_t()
    assert lib.fr_ss_workspace_bytes(C.byref(cfg), 2, 0, cfg.height, C.byref(mn), C.byref(best)) == 0
    assert ss_device(lib, cfg, 2, work_len=mn.value - 1) == TOO_SMALL and b"work_len" in lib.fr_last_error()
    assert ss_device(lib, cfg, 2, d_work=None) == INVALID and b"d_work" in lib.fr_last_error()
    # the filter alone
    buf = np.zeros(64, dtype=np.uint8)
    f = lib.fr_box_filter_rgb8
    assert f(buf.ctypes.data, 2, 2, 0, 3, buf.ctypes.data, 64) == INVALID and b"supersample" in lib.fr_last_error()
    assert f(buf.ctypes.data, 2, 2, 9, 3, buf.ctypes.data, 64) == INVALID
    assert f(buf.ctypes.data, 2, 2, 2, 5, buf.ctypes.data, 64) == INVALID and b"channels" in lib.fr_last_error()
    assert f(buf.ctypes.data, 0x40000000, 1, 4, 3, buf.ctypes.data, 64) == INVALID and b"width" in lib.fr_last_error()
    assert f(buf.ctypes.data, 2, 2, 2, 3, buf.ctypes.data, 11) == TOO_SMALL and b"out_len" in lib.fr_last_error()
    assert f(None, 2, 2, 2, 3, buf.ctypes.data, 64) == INVALID
    assert f(None, 0, 2, 2, 3, None, 0) == 0  # nothing to do
    g = lib.fr_box_filter_rgb8_device
    assert g(0x1000, 2, 2, 2, 4, 0x2001, 64, None) == INVALID and b"aligned" in lib.fr_last_error()
    assert g(0x1000, 2, 2, 2, 3, 0x2001, 11, None) == TOO_SMALL
    assert g(None, 2, 2, 2, 3, 0x2000, 64, None) == INVALID


def band_rule(width, rows_out, s, work_len=None):
    """The band rule of include/fractal_hip.h restated: (min_bytes, best_bytes) and, for a workspace length, the source
    rows per band."""
    if s == 1:
        return 0, 0, None
    row_bytes = 3 * s * width
    rows = s * rows_out
    mn = min(8 * s, rows) * row_bytes
    best = max(mn, min(rows * row_bytes, GIB))
    if work_len is None or rows == 0:
        return mn, best, None
    bmax = work_len // row_bytes
    if bmax >= rows:
        return mn, best, rows
    bmax -= bmax % (8 * s)
    nb = -(-rows // bmax)
    b = -(-rows // nb)
    b = -(-b // (8 * s)) * (8 * s)
    return mn, best, b


@pytest.mark.parametrize("s", range(1, 9))
@pytest.mark.parametrize("width", [1, 7, 257, 16384])
def test_workspace_bytes_follow_the_band_rule(fr, lib, s, width):
    cfg = fr.Config.new()
    cfg.width, cfg.height = width, 16384
    for y0, y1 in [(0, 16384), (0, 1), (5, 37), (16383, 16384), (3, 3), (0, 7), (0, 8), (0, 9), (100, 16001)]:
        mn, best = C.c_size_t(123), C.c_size_t(456)
        assert lib.fr_ss_workspace_bytes(C.byref(cfg), s, y0, y1, C.byref(mn), C.byref(best)) == 0
        wmn, wbest, _ = band_rule(width, y1 - y0, s)
        assert (mn.value, best.value) == (wmn, wbest), (s, width, y0, y1)
        assert fr.ss_workspace_bytes(cfg, s, y0, y1) == (wmn, wbest)
        assert best.value <= max(GIB, mn.value) and mn.value <= best.value
    assert lib.fr_ss_workspace_bytes(C.byref(cfg), s, 0, 8, None, None) == 0  # either pointer may be NULL


def test_the_band_rule_leaves_no_sliver():
    """properties of the rule itself: bands are whole tile rows and whole output rows, fit the workspace, and the last
    band is never a sliver beside the others"""
    for s in (2, 3, 5, 8):
        for width, rows_out in [(257, 193), (16384, 16384), (96, 64), (7, 1000)]:
            mn, best, _ = band_rule(width, rows_out, s)
            for work_len in {mn, mn + 1, (mn + best) // 2 | 1, best, best + 5}:
                _, _, b = band_rule(width, rows_out, s, work_len)
                rows = s * rows_out
                assert b * 3 * s * width <= max(work_len, mn)
                if b < rows:
                    assert b % (8 * s) == 0
                    nb = -(-rows // b)
                    last = rows - (nb - 1) * b
                    assert last > 0 and b - last < 8 * s * nb  # the bands differ by the rounding only


def test_workspace_bytes_domain(fr, lib):
    cfg = small(fr)
    mn, best = C.c_size_t(), C.c_size_t()
    assert lib.fr_ss_workspace_bytes(C.byref(cfg), 0, 0, 1, C.byref(mn), C.byref(best)) == INVALID
    assert lib.fr_ss_workspace_bytes(C.byref(cfg), 9, 0, 1, C.byref(mn), C.byref(best)) == INVALID
    assert lib.fr_ss_workspace_bytes(C.byref(cfg), 2, 2, 1, C.byref(mn), C.byref(best)) == INVALID
    assert lib.fr_ss_workspace_bytes(C.byref(cfg), 2, 0, cfg.height + 1, C.byref(mn), C.byref(best)) == INVALID
    assert lib.fr_ss_workspace_bytes(None, 2, 0, 1, C.byref(mn), C.byref(best)) == INVALID


def test_empty_row_range_is_legal_without_a_device(fr, lib):
    cfg = small(fr)
    for s in (1, 2, 8):
        for prec in (F64, F32, DD, PT):
            assert lib.fr_render_rows_ss(C.byref(cfg), prec, None, s, 3, 3, 3, None, 0, None) == 0
            assert lib.fr_render_rows_ss_device(C.byref(cfg), prec, None, s, 3, 3, 4, None, 0, None, 0, None, None) == 0
    assert fr.get_image_rows(cfg, 4, 4, supersample=3).shape == (0, cfg.width, 3)
    empty = small(fr, w=0)
    assert lib.fr_render_rows_ss(C.byref(empty), F64, None, 2, 0, empty.height, 3, None, 0, None) == 0


def test_python_wrappers_do_not_fall_back_without_a_device(fr):
    if fr.device_count() > 0:
        pytest.skip("a HIP device is present")
    cfg = small(fr)
    fern = small(fr)
    fern.algo = int(fr.Algo.BarnsleyFern)
    for c in (cfg, fern):  # the fern renders black ON THE DEVICE: no shortcut on the host either
        for call in (lambda: fr.get_image(c, supersample=2), lambda: fr.get_image_rows(c, 0, 4, supersample=3),
                     lambda: fr.get_image_rgba(c, supersample=2), lambda: fr.get_image(c, fr.Precision.F32, supersample=8),
                     lambda: fr.get_image(c, fr.Precision.DD, pos_lo=(0.0, 0.0), supersample=2),
                     lambda: fr.get_image(c, fr.Precision.PT, supersample=2)):
            with pytest.raises(fr.FractalHipError) as e:
                call()
            assert e.value.code == NO_DEVICE
    with pytest.raises(fr.FractalHipError) as e:
        fr.box_filter(np.zeros((4, 4, 3), dtype=np.uint8), 2)
    assert e.value.code == NO_DEVICE
    with pytest.raises(fr.FractalHipError) as e:
        fr.get_image(cfg, supersample=9)
    assert e.value.code == INVALID


def test_box_filter_wrapper_checks_its_shape(fr):
    with pytest.raises(ValueError):
        fr.box_filter(np.zeros((5, 4, 3), dtype=np.uint8), 2)
    with pytest.raises(ValueError):
        fr.box_filter(np.zeros((4, 4, 4), dtype=np.uint8), 2)
