"""Keeping a view on the device (include/fractal_hip.h: fr_escape_rows_device, fr_escape_extend_device, fr_escape_extend,
fr_colour_rows_device), the part that needs no device:
  - the domain of the four calls — every refusal comes back with its code before any device work, and the legal no-ops
    return FR_OK without a device;
  - the definition of the extension itself on the CPU oracle: a stored (z, iters == N) continued for M - N steps IS the
    render at cap M, and the views the GPU tests use exercise every class of pixel (the table of extend_cases.py,
    recomputed here, so that the GPU cases are known to be non-trivial before they run)."""
import ctypes as C

import numpy as np
import pytest

import extend_cases as X
import oracle_lib as O

FAKE = 0x10000  # a non-NULL, aligned "device pointer" for calls that must be refused before they touch it


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


def small(fr, iterations=37):
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = X.W, X.H, iterations
    return cfg


def extend_dev(lib, cfg, precision, n, zw=2, z=FAKE, it=FAKE, y0=0, y1=None, lo=None, opts=None):
    y1 = cfg.height if y1 is None else y1
    return lib.fr_escape_extend_device(C.byref(cfg) if cfg is not None else None, precision, lo, y0, y1, n, zw, z, it, None, opts)


def extend_host(lib, cfg, precision, n, zw=2, z=FAKE, it=FAKE, y0=0, y1=None, lo=None):
    y1 = cfg.height if y1 is None else y1
    return lib.fr_escape_extend(C.byref(cfg) if cfg is not None else None, precision, lo, y0, y1, n, zw, z, it)


@pytest.mark.parametrize("call", [extend_dev, extend_host], ids=["device", "host"])
def test_extend_domain_is_checked_without_a_device(fr, lib, call):
    from fractal_renderer_amd import _native

    INVALID, OK = _native.FR_ERR_INVALID_ARGUMENT, _native.FR_OK
    cfg = small(fr)
    # a lower cap
    assert call(lib, cfg, X.F64, 38) == INVALID
    assert b"lower cap cannot be derived" in lib.fr_last_error()
    # perturbation
    assert call(lib, cfg, X.PT, 5) == INVALID
    assert b"FR_PRECISION_PT" in lib.fr_last_error()
    assert call(lib, cfg, X.PT, 5, lo=C.byref(_native.Imaginary(0.0, 0.0))) == INVALID
    assert b"FR_PRECISION_PT" in lib.fr_last_error()
    # z_width: DD keeps its low parts, the others have none
    assert call(lib, cfg, X.DD, 5, zw=2) == INVALID and b"z_width" in lib.fr_last_error()
    assert call(lib, cfg, X.F64, 5, zw=4) == INVALID and b"z_width" in lib.fr_last_error()
    assert call(lib, cfg, X.F32, 5, zw=4) == INVALID
    for prec in (X.F64, X.F32, X.DD):
        assert call(lib, cfg, prec, 5, zw=3) == INVALID
    # pos_lo belongs to the deep precisions; rows; cfg; the precision itself
    assert call(lib, cfg, X.F64, 5, lo=C.byref(_native.Imaginary(0.0, 0.0))) == INVALID and b"pos_lo" in lib.fr_last_error()
    assert call(lib, cfg, X.F64, 5, y0=9, y1=8) == INVALID and b"y0 > y1" in lib.fr_last_error()
    assert call(lib, cfg, X.F64, 5, y1=cfg.height + 1) == INVALID and b"y1 > height" in lib.fr_last_error()
    assert call(lib, None, X.F64, 5, y1=1) == INVALID and b"cfg is NULL" in lib.fr_last_error()
    assert call(lib, cfg, 7, 5) == INVALID
    # DD's own domain is check_dd's, on cfg and pos_lo
    bad = small(fr)
    bad.limit = float("inf")
    assert call(lib, bad, X.DD, 5, zw=4) == INVALID and b"FR_PRECISION_DD" in lib.fr_last_error()
    assert call(lib, cfg, X.DD, 5, zw=4, lo=C.byref(_native.Imaginary(1.0, 0.0))) == INVALID and b"normalised" in lib.fr_last_error()
    # both arrays are required
    assert call(lib, cfg, X.F64, 5, z=None) == INVALID and b"NULL" in lib.fr_last_error()
    assert call(lib, cfg, X.F64, 5, it=None) == INVALID
    assert call(lib, cfg, X.F64, 37, z=None, it=None) == INVALID  # ... whatever the caps
    # the legal no-ops need no device: M == N, no rows
    assert call(lib, cfg, X.F64, 37) == OK
    assert call(lib, cfg, X.F32, 37) == OK
    assert call(lib, cfg, X.DD, 37, zw=4) == OK
    assert call(lib, cfg, X.F64, 5, y0=7, y1=7) == OK
    assert call(lib, cfg, X.F64, 5, y0=7, y1=7, z=None, it=None) == OK
    zero = small(fr, 0)
    assert call(lib, zero, X.F64, 0) == OK


def test_extend_device_checks_its_opts(fr, lib):
    from fractal_renderer_amd import _native

    cfg = small(fr)
    opts = fr.RenderOpts()
    opts.loop_mode = 3
    assert extend_dev(lib, cfg, X.F64, 5, opts=C.byref(opts)) == _native.FR_ERR_INVALID_ARGUMENT
    assert b"loop_mode" in lib.fr_last_error()
    opts = fr.RenderOpts(loop_mode=5)
    assert extend_dev(lib, cfg, X.F64, 37, opts=C.byref(opts)) == _native.FR_OK


def test_escape_rows_device_domain(fr, lib):
    from fractal_renderer_amd import _native

    INVALID, OK = _native.FR_ERR_INVALID_ARGUMENT, _native.FR_OK
    cfg = small(fr)

    def call(precision, zw=2, z=FAKE, it=FAKE, y0=0, y1=cfg.height, lo=None, c=cfg):
        return lib.fr_escape_rows_device(C.byref(c) if c is not None else None, precision, lo, y0, y1, zw, z, it, None, None)

    assert call(X.F64, zw=4) == INVALID and b"z_width" in lib.fr_last_error()
    assert call(X.PT, zw=4) == INVALID
    assert call(X.DD, zw=3) == INVALID
    assert call(X.F64, lo=C.byref(_native.Imaginary(0.0, 0.0))) == INVALID and b"pos_lo" in lib.fr_last_error()
    assert call(X.F64, y0=3, y1=2) == INVALID
    assert call(X.F64, y1=cfg.height + 1) == INVALID
    assert call(X.F64, c=None) == INVALID
    assert call(9) == INVALID
    assert call(X.F64, z=FAKE + 4) == INVALID and b"aligned" in lib.fr_last_error()
    # nothing to write: no rows, or no array asked for
    assert call(X.F64, y0=4, y1=4) == OK
    assert call(X.DD, zw=4, y0=4, y1=4) == OK
    assert call(X.F64, z=None, it=None) == OK


def test_colour_rows_device_domain(fr, lib):
    from fractal_renderer_amd import _native

    INVALID, SMALL, OK = _native.FR_ERR_INVALID_ARGUMENT, _native.FR_ERR_BUFFER_TOO_SMALL, _native.FR_OK
    cfg = small(fr)

    def call(n=100, channels=3, zw=2, out_len=None, z=FAKE, it=FAKE, out=FAKE, c=cfg):
        out_len = channels * n if out_len is None else out_len
        return lib.fr_colour_rows_device(C.byref(c) if c is not None else None, z, zw, it, n, channels, out, out_len, None)

    assert call(channels=5) == INVALID and b"channels" in lib.fr_last_error()
    assert call(channels=2) == INVALID
    assert call(zw=3) == INVALID and b"z_width" in lib.fr_last_error()
    assert call(out_len=299) == SMALL and b"out_len" in lib.fr_last_error()
    assert call(channels=4, out_len=399) == SMALL
    assert call(z=None) == INVALID and call(it=None) == INVALID and call(out=None) == INVALID
    assert call(channels=4, out=FAKE + 2) == INVALID and b"4-byte aligned" in lib.fr_last_error()
    assert call(c=None) == INVALID
    assert call(n=0, z=None, it=None, out=None) == OK


def test_python_extend_rows_checks_shapes_and_is_a_no_op_at_the_same_cap(fr):
    cfg = small(fr)
    z = np.zeros((X.H, X.W, 2))
    it = np.full((X.H, X.W), 37, dtype=np.uint32)
    z2, it2 = fr.extend_rows(cfg, z, it, 37)
    assert z2 is not z and np.array_equal(z2, z) and np.array_equal(it2, it)
    with pytest.raises(ValueError):
        fr.extend_rows(cfg, z[:-1], it, 37)
    with pytest.raises(ValueError):
        fr.extend_rows(cfg, z, it, 37, precision=fr.Precision.DD)  # DD state is four doubles
    with pytest.raises(fr.FractalHipError) as e:
        fr.extend_rows(cfg, z, it, 38)
    assert e.value.code == 1 and "lower cap" in str(e.value)
    with pytest.raises(fr.FractalHipError):
        fr.extend_rows(cfg, z, it, 5, precision=fr.Precision.PT)


# ---- the definition, on the oracle alone ------------------------------------------------------------------


@pytest.mark.parametrize("precision", [X.F64, X.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["mandelbrot", "julia"])
def test_class_table_of_the_gpu_views(name, precision):
    """The views and links of tests/test_gpu_extend.py hold every class of pixel in the numbers stated with the feature."""
    for (view, n, m), want in X.table(precision).items():
        if view != name:
            continue
        got = X.classes(X.reference(name, precision, n)[1], X.reference(name, precision, m)[1], n, m)
        assert sum(got[:3]) == X.W * X.H
        assert got == want, (view, n, m, got)
    # the 0 -> 1 link has no escapes at the CLI's limit; with limit = 2 on the Mandelbrot view 1 019 pixels escape at step 0
    it1 = X.reference("mandelbrot", precision, 1)[1]
    assert (it1 == 1).all()
    assert int((X.reference("mandelbrot", precision, 1, limit=2.0)[1] == 0).sum()) == 1019


@pytest.mark.parametrize("precision", [X.F64, X.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,count", [("mandelbrot", 1921), ("julia", 1936)])
def test_continuing_a_stored_orbit_is_the_render_at_the_higher_cap(name, count, precision):
    """recursive() from the position stored at cap 5 for 32 more steps gives position and index of the cap-37 render, bit
    for bit, for every orbit still running at cap 5."""
    n, m = 5, 37
    z_n, it_n = X.reference(name, precision, n)
    z_m, it_m = X.reference(name, precision, m)
    cfg = X.view_cfg(name, m)
    ys, xs = np.nonzero(it_n == n)
    assert len(ys) == count
    for y, x in zip(ys.tolist(), xs.tolist()):
        c = O.lib().fro_xy_to_imaginary(C.byref(cfg), x, y)
        c = (cfg.julia_set.re, cfg.julia_set.im) if name == "julia" else (c.re, c.im)
        pos, it = O.recursive(m - n, tuple(z_n[y, x]), c, cfg.limit, f32=precision == X.F32)
        assert n + it == it_m[y, x], (x, y)
        assert X.same_f64(np.array(pos), z_m[y, x]), (x, y)
    # and a finished pixel's stored result does not depend on the cap
    done = it_n != n
    assert np.array_equal(it_n[done], it_m[done]) and X.same_f64(z_n[done], z_m[done])
