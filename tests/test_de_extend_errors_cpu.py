"""The domain of the RESUMABLE DE calls (include/fractal_hip.h: fr_escape_extend_de, fr_escape_rows_de_pt_state,
fr_escape_extend_de_pt, each with its _device form): every refusal by message, before any device work, and the no-ops that need
no device.  The tests run without a GPU: there a call that got as far as the device fails with FR_ERR_NO_DEVICE, not with the
message asserted here, and a no-op that touched the device would not return 0."""
import ctypes as C

import numpy as np
import pytest

import pt_wide_model as W

INVALID = 1


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


def refused(lib, rc, *words):
    msg = lib.fr_last_error().decode()
    assert rc == INVALID, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def small(fr):
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = 8, 6, 100
    return cfg


def host_arrays():
    """z, iters, dz, m, der of 6 x 8 pixels; kept alive by the caller"""
    z, dz, der = np.zeros((6, 8, 2)), np.zeros((6, 8, 2)), np.zeros((6, 8, 2))
    it, m = np.zeros((6, 8), dtype=np.uint32), np.zeros((6, 8), dtype=np.uint32)
    return z, it, dz, m, der


def wide_centre(words=9):
    from fractal_renderer_amd import _native

    ints = W.centre_ints("M", words)
    w = W.to_words(ints[0], words), W.to_words(ints[1], words)
    p64 = C.POINTER(C.c_uint64)
    return _native.fr_wide_centre(words, w[0].ctypes.data_as(p64), w[1].ctypes.data_as(p64)), w


def test_extend_de_refusals(fr, lib):
    cfg = small(fr)
    keep = host_arrays()
    arrays = (keep[0].ctypes.data, keep[1].ctypes.data, keep[4].ctypes.data)
    for form, tail in ((lib.fr_escape_extend_de, ()), (lib.fr_escape_extend_de_device, (None,))):
        refused(lib, form(C.byref(cfg), 3, 0, 6, 50, *arrays, *tail), "FR_PRECISION_PT", "fr_escape_extend_de_pt", "fr_escape_rows_de_pt_state")
        for precision in (1, 2, 7):  # F32, DD, nonsense: DE's scope message
            refused(lib, form(C.byref(cfg), precision, 0, 6, 50, *arrays, *tail), "FR_PRECISION_F32", "FR_PRECISION_DD", "BLA-PT",
                    "SCALED PT", "out of scope", "fr_escape_extend_de")
        refused(lib, form(C.byref(cfg), 0, 0, 6, 101, *arrays, *tail), "cfg->iterations < from_iterations")
        refused(lib, form(C.byref(cfg), 0, 4, 2, 50, *arrays, *tail), "y0 > y1")
        refused(lib, form(C.byref(cfg), 0, 0, 7, 50, *arrays, *tail), "y1 > height")
        refused(lib, form(None, 0, 0, 6, 50, *arrays, *tail), "cfg is NULL")
        for k in range(3):
            a = list(arrays)
            a[k] = None
            refused(lib, form(C.byref(cfg), 0, 0, 6, 50, *a, *tail), "NULL array", "z, iters and der", "all three")
        for k, (off, words) in enumerate(((4, "8-byte aligned"), (2, "4-byte aligned"), (4, "8-byte aligned"))):
            a = list(arrays)
            a[k] += off
            refused(lib, form(C.byref(cfg), 0, 0, 6, 50, *a, *tail), "z and der must be", words)
        big = fr.Config.from_buffer_copy(bytes(cfg))
        for limit in (2.0 ** 20 * (1 + 2.0 ** -52), 2.0 ** 21, float("inf"), float("nan")):
            big.limit = limit
            refused(lib, form(C.byref(big), 0, 0, 6, 50, *arrays, *tail), "limit must be <= 2^20")
        # the no-ops need no device and no arrays (y0 == y1) / valid arrays that are not touched (M == N)
        assert form(C.byref(cfg), 0, 3, 3, 50, None, None, None, *tail) == 0
        assert form(C.byref(cfg), 0, 0, 6, 100, *arrays, *tail) == 0
        fern = fr.Config.from_buffer_copy(bytes(cfg))
        fern.algo = 1
        assert form(C.byref(fern), 0, 0, 6, 50, *arrays, *tail) == 0  # an algorithm without orbits: nothing is done
        # M < N is refused even where there is nothing to do
        refused(lib, form(C.byref(cfg), 0, 3, 3, 101, None, None, None, *tail), "cfg->iterations < from_iterations")
    assert not any(a.any() for a in keep)


def pt_forms(lib):
    """(call(cfg, lo, centre, y0, y1, from, arrays), is an extension) of the four PT calls"""
    def bind(fn, extend, tail):
        return (lambda cfg, lo, centre, y0, y1, n, a: fn(cfg, lo, centre, y0, y1, *((n,) if extend else ()), *a, *tail)), extend

    return [bind(lib.fr_escape_rows_de_pt_state, False, ()), bind(lib.fr_escape_rows_de_pt_state_device, False, (None,)),
            bind(lib.fr_escape_extend_de_pt, True, ()), bind(lib.fr_escape_extend_de_pt_device, True, (None,))]


def test_pt_state_refusals_with_a_dd_centre(fr, lib):
    cfg = small(fr)
    keep = host_arrays()
    arrays = tuple(a.ctypes.data for a in keep)
    none = (None,) * 5
    for call, extend in pt_forms(lib):
        if extend:
            refused(lib, call(C.byref(cfg), None, None, 0, 6, 101, arrays), "cfg->iterations < from_iterations")
            refused(lib, call(C.byref(cfg), None, None, 3, 3, 101, none), "cfg->iterations < from_iterations")
            assert call(C.byref(cfg), None, None, 0, 6, 100, arrays) == 0  # M == N: no device
            fern = fr.Config.from_buffer_copy(bytes(cfg))
            fern.algo = 1
            assert call(C.byref(fern), None, None, 0, 6, 50, arrays) == 0
        assert call(C.byref(cfg), None, None, 3, 3, 50, none) == 0  # y0 == y1: no device, no arrays
        refused(lib, call(C.byref(cfg), None, None, 4, 2, 50, arrays), "y0 > y1")
        refused(lib, call(C.byref(cfg), None, None, 0, 7, 50, arrays), "y1 > height")
        refused(lib, call(None, None, None, 0, 6, 50, arrays), "cfg is NULL")
        for k in range(5):
            a = list(arrays)
            a[k] = None
            refused(lib, call(C.byref(cfg), None, None, 0, 6, 50, a), "NULL array", "z, iters, dz, m and der", "all five")
        for k, off in enumerate((4, 2, 4, 2, 4)):
            a = list(arrays)
            a[k] += off
            refused(lib, call(C.byref(cfg), None, None, 0, 6, 50, a), "z, dz and der must be 8-byte aligned", "iters and m 4-byte aligned")
        big = fr.Config.from_buffer_copy(bytes(cfg))
        for limit in (2.0 ** 20 * (1 + 2.0 ** -52), 2.0 ** 21):
            big.limit = limit
            refused(lib, call(C.byref(big), None, None, 0, 6, 50, arrays), "limit must be <= 2^20")
        # without a centre the domain is PT's with its dd centre
        pt = fr.Config.from_buffer_copy(bytes(cfg))
        pt.iterations = (1 << 24) + 1
        refused(lib, call(C.byref(pt), None, None, 0, 6, 50, arrays), "FR_PRECISION_PT", "FR_PT_MAX_ITERATIONS")
        pt.iterations, pt.scale.re = 100, 2.0 ** -65
        refused(lib, call(C.byref(pt), None, None, 0, 6, 50, arrays), "FR_PRECISION_PT", "|scale|")
        pt.scale.re, pt.limit = 0.4, float("inf")
        refused(lib, call(C.byref(pt), None, None, 0, 6, 50, arrays), "FR_PRECISION_PT", "finite")
        pt.limit, pt.pos.re = 2.0, 1.0
        off = fr.Imaginary(1.0, 0.0)
        refused(lib, call(C.byref(pt), C.byref(off), None, 0, 6, 50, arrays), "pos_lo is not normalised")
    assert not any(a.any() for a in keep)


def test_pt_state_refusals_with_a_wide_centre(fr, lib):
    cfg = W.view(fr.Config.new(), "M", 200, 8, 6, 100)
    centre, _words = wide_centre()
    keep = host_arrays()
    arrays = tuple(a.ctypes.data for a in keep)
    lo = fr.Imaginary(0.0, 0.0)
    for call, extend in pt_forms(lib):
        refused(lib, call(C.byref(cfg), C.byref(lo), C.byref(centre), 0, 6, 50, arrays), "pos_lo must be NULL when a wide centre is given")
        deep = fr.Config.from_buffer_copy(bytes(cfg))
        deep.scale.re = deep.scale.im = 2.0 ** 441
        refused(lib, call(C.byref(deep), None, C.byref(centre), 0, 6, 50, arrays), "2^440")
        deep.scale.re = deep.scale.im = 2.0 ** 440
        deep.limit = 2.0 ** 21
        refused(lib, call(C.byref(deep), None, C.byref(centre), 0, 6, 50, arrays), "limit must be <= 2^20")
        deep.limit = 2.0
        a = list(arrays)
        a[4] = None
        refused(lib, call(C.byref(deep), None, C.byref(centre), 0, 6, 50, a), "all five")
        assert call(C.byref(deep), None, C.byref(centre), 2, 2, 50, (None,) * 5) == 0
        if extend:
            refused(lib, call(C.byref(deep), None, C.byref(centre), 0, 6, 101, arrays), "cfg->iterations < from_iterations")
            assert call(C.byref(deep), None, C.byref(centre), 0, 6, 100, arrays) == 0
        short = fr.Config.from_buffer_copy(bytes(cfg))  # WIDE PT's own rule: the words must cover the scale
        two, _w2 = wide_centre(2)
        assert call(C.byref(short), None, C.byref(two), 0, 6, 50, arrays) == INVALID


def test_python_refusals(fr):
    cfg = small(fr)
    z, it, dz, m, der = host_arrays()
    centre = fr.WideCentre(2)
    with pytest.raises(ValueError):
        fr.escape_rows_de_pt_state(cfg, pos_lo=(0.0, 0.0), centre=centre)
    with pytest.raises(ValueError):
        fr.extend_rows_de_pt(cfg, z, it, dz, m, der, 50, pos_lo=(0.0, 0.0), centre=centre)
    with pytest.raises(ValueError):
        fr.escape_rows_de_pt_state_device(cfg, 8, 8, 8, 8, 8, pos_lo=(0.0, 0.0), centre=centre)
    with pytest.raises(ValueError):
        fr.extend_rows_de_pt_device(cfg, 8, 8, 8, 8, 8, 50, pos_lo=(0.0, 0.0), centre=centre)
    with pytest.raises(ValueError):
        fr.extend_rows_de_pt(cfg, z, it, dz, m, np.zeros((6, 8, 3)), 50)  # a wrong shape
    with pytest.raises(ValueError):
        fr.extend_rows_de(cfg, z, it[:5], der, 50)
    for call in (lambda: fr.extend_rows_de(cfg, z, it, der, 101), lambda: fr.extend_rows_de_pt(cfg, z, it, dz, m, der, 101),
                 lambda: fr.extend_rows_de_device(cfg, 8, 8, 8, 101), lambda: fr.extend_rows_de_pt_device(cfg, 8, 8, 8, 8, 8, 101)):
        with pytest.raises(fr.FractalHipError) as e:
            call()
        assert e.value.code == INVALID and "from_iterations" in str(e.value)
    with pytest.raises(fr.FractalHipError) as e:
        fr.extend_rows_de(cfg, z, it, der, 50, precision=fr.Precision.PT)
    assert "fr_escape_extend_de_pt" in str(e.value)
    with pytest.raises(fr.FractalHipError) as e:
        fr.extend_rows_de(cfg, z, it, der, 50, precision=fr.Precision.DD)
    assert "out of scope" in str(e.value)
    # the no-ops reach no device
    st = fr.escape_rows_de_pt_state(cfg, y0=2, y1=2)
    assert [a.shape for a in st] == [(0, 8, 2), (0, 8), (0, 8, 2), (0, 8), (0, 8, 2)]
    out = fr.extend_rows_de_pt(cfg, z, it, dz, m, der, 100)
    assert all(np.array_equal(a, b) for a, b in zip(out, (z, it, dz, m, der)))
    out = fr.extend_rows_de(cfg, z, it, der, 100)
    assert all(np.array_equal(a, b) for a, b in zip(out, (z, it, der)))
