"""The host plumbing around the deep kernels, road by road (what each kernel computes is the business of test_gpu_dd.py,
test_gpu_pt.py, test_gpu_pt_state.py, test_gpu_pt_wide.py and test_gpu_bla.py, which compare with the models):
  - the host-buffer form and the device-pointer form of a call give identical bytes and arrays;
  - rows [5, 12) alone are rows 5 .. 11 of the whole call (the row grid of a launch);
  - with fr_set_profiling(1) every road reports a time and its own kernel, in both forms.
Roads: DD and PT renders (RGB and RGBA), the PT state, the PT extension 150 -> 300, BLA-PT renders and escape rows; PT and
BLA-PT with the centre as pos_lo and as the WideCentre of exactly the same value.  SCALED PT on the wide views: renders and
escape rows with bits = -1 (the plain loop, scaled-pt-*) and bits = 0 (the table, scaled-bla-*), its state and its extension.
Views: 33 x 17 at 300 iterations — ragged against the 16 x 16 pixels of a workgroup on both axes, more than one workgroup per
axis — Mandelbrot on the Misiurewicz point and Julia on the repelling fixed point of tests/pt_wide_model.py (the centres of
test_gpu_bla.py), at 2^84 with the centre split into pos + pos_lo, and Mandelbrot at 2^300 on the 6-word centre (wide only).
By tests/pt_model.py the Julia view has 85 distinct escape indices, 60 pixels still running at 150 and 23 at 300; the
Mandelbrot view at 2^84 has 14 and every pixel out by 69 (its extension has nothing to do and must do nothing); at 2^300
every pixel runs past 150.
The wide and the double-double road of one centre are NOT compared with each other: their reference orbits come from
different arithmetic (fixed point, double-double), and no test of the project asserts that they agree."""
import ctypes as C
import functools

import numpy as np
import pytest

import pt_wide_model as W

pytestmark = pytest.mark.gpu

W_, H_, CAP, LOW_CAP = 33, 17, 300, 150
SUB = (5, 12)


@pytest.fixture(scope="module")
def fr():
    import fractal_renderer_amd

    assert fractal_renderer_amd.device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    fractal_renderer_amd.init(0)
    assert fractal_renderer_amd.device_name().startswith("gfx950")
    return fractal_renderer_amd


@pytest.fixture(scope="module")
def lib(fr):
    from fractal_renderer_amd import _native

    return _native.load()


def check(rc):
    from fractal_renderer_amd import _native

    _native.check(rc)


# ---- the views ------------------------------------------------------------------------------------------------------------

VIEWS = ("M-lo", "M-wide", "J-lo", "J-wide", "M-2^300")


class View:
    """cfg at 300 and at 150 iterations, and the centre as the C calls take it: (pos_lo, None) or (None, wide centre)"""

    def __init__(self, fr, name):
        from fractal_renderer_amd import _native

        point, kind = name.split("-")
        deep = kind == "2^300"
        self.name, self.wide = name, kind != "lo"
        self.cfg = W.view(fr.Config.new(), point, 300 if deep else 84, W_, H_, CAP)
        if deep:
            n = 6
            self.words = [np.array(W.to_words(i, n), dtype=np.uint64) for i in W.centre_ints(point, n)]
        else:  # the centre to ~106 bits as pos + pos_lo, and the wide centre of exactly that value
            n = 3
            (hi_re, lo_re), (hi_im, lo_im) = (W.split(i, 16) for i in W.centre_ints(point, 16))
            self.cfg.pos.re, self.cfg.pos.im = hi_re, hi_im
            centre = fr.WideCentre(n).add(hi_re, hi_im).add(lo_re, lo_im)
            assert centre.to_dd() == ((hi_re, hi_im), (lo_re, lo_im)), "the two centres are not the same point"
            self.words = [centre.re, centre.im]
            self.lo = _native.Imaginary(lo_re, lo_im)
        p64 = C.POINTER(C.c_uint64)
        self.centre = _native.fr_wide_centre(n, self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64))
        self.low = fr.Config.from_buffer_copy(bytes(self.cfg))
        self.low.iterations = LOW_CAP

    def where(self):
        """the centre argument of the calls that take one"""
        return C.byref(self.centre) if self.wide else C.byref(self.lo)

    def both(self):
        """(pos_lo, centre) of the BLA-PT calls"""
        return (None, C.byref(self.centre)) if self.wide else (C.byref(self.lo), None)


@functools.lru_cache(maxsize=None)
def _view(fr, name):
    return View(fr, name)


# ---- the roads: run(lib, v, road, form, y0, y1) -> the arrays the call wrote ----------------------------------------------------

KERNEL = {"dd-rgb": "escape_dd_kernel", "dd-rgba": "escape_dd_kernel", "pt-rgb": "escape_pt_kernel", "pt-rgba": "escape_pt_kernel",
          "pt-state": "escape_pt_state_kernel", "pt-extend": "escape_extend_pt_kernel", "bla-rgb": "escape_bla_kernel",
          "bla-rgba": "escape_bla_kernel", "bla-escape": "escape_bla_kernel",
          "scaled-pt-rgb": "escape_pt_scaled_kernel", "scaled-pt-rgba": "escape_pt_scaled_kernel",
          "scaled-pt-escape": "escape_pt_scaled_kernel", "scaled-bla-rgb": "escape_bla_scaled_kernel",
          "scaled-bla-rgba": "escape_bla_scaled_kernel", "scaled-bla-escape": "escape_bla_scaled_kernel",
          "scaled-state": "escape_pt_scaled_state_kernel", "scaled-extend": "escape_extend_pt_scaled_kernel"}
ROADS = tuple(KERNEL)
DTYPES = (np.float64, np.uint32, np.float64, np.uint32)  # z, iters, dz (SCALED PT: w), m


def scaled(road):
    return road.startswith("scaled")


def applies(v, road):
    """DD takes no wide centre, SCALED PT nothing else; v: a view's name"""
    return not (road.startswith("dd") and not v.endswith("-lo")) and not (scaled(road) and v.endswith("-lo"))


def state_road(road):
    """the state road whose result an extension continues and must reproduce"""
    return "scaled-state" if scaled(road) else "pt-state"


def cases():
    return [(v, r) for v in VIEWS for r in ROADS if applies(v, r)]


def raw_shapes(rows, n):
    return [(rows, W_, 2) if k % 2 == 0 else (rows, W_) for k in range(n)]


def run(lib, torch, v, road, form, y0, y1, start=None):
    """`start`: the state at 150 of rows [y0, y1) that pt-extend / scaled-extend continues"""
    rows, device = y1 - y0, form == "device"
    w = "_wide" if v.wide else ""
    if road.endswith(("rgb", "rgba")):
        ch = 4 if road.endswith("rgba") else 3
        n = ch * W_ * rows
        buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0") if device else np.zeros(n, dtype=np.uint8)
        tail = (y0, y1, ch, buf.data_ptr() if device else buf.ctypes.data, n) + ((None,) if device else ())
        suffix = "_device" if device else ""
        if road.startswith("dd"):
            check(getattr(lib, "fr_render_rows_dd" + suffix)(C.byref(v.cfg), v.where(), *tail))
        elif road.startswith("pt"):
            check(getattr(lib, "fr_render_rows_pt" + w + suffix)(C.byref(v.cfg), v.where(), *tail))
        elif scaled(road):
            check(getattr(lib, "fr_render_rows_pt_scaled" + suffix)(C.byref(v.cfg), C.byref(v.centre), -1 if "-pt-" in road else 0, *tail))
        else:
            check(getattr(lib, "fr_render_rows_pt_bla" + suffix)(C.byref(v.cfg), *v.both(), 0, *tail))
        if device:
            torch.cuda.synchronize()
            buf = buf.cpu().numpy()
        return (buf.reshape(rows, W_, ch),)
    n_arrays = 2 if road.endswith("escape") else 4
    shapes = raw_shapes(rows, n_arrays)
    host = [np.zeros(s, dtype=d) if start is None else np.array(start[k], dtype=d, order="C") for k, (s, d) in enumerate(zip(shapes, DTYPES))]
    if device:
        dev = [torch.from_numpy(a.view(np.uint8).reshape(-1)).to("cuda:0") for a in host]
        ptrs = [t.data_ptr() for t in dev] + [None]
    else:
        ptrs = [a.ctypes.data for a in host]
    suffix = "_device" if device else ""
    if road == "bla-escape":
        check(getattr(lib, "fr_escape_rows_pt_bla" + suffix)(C.byref(v.cfg), *v.both(), 0, y0, y1, *ptrs))
    elif road.endswith("escape"):
        check(getattr(lib, "fr_escape_rows_pt_scaled" + suffix)(C.byref(v.cfg), C.byref(v.centre), -1 if "-pt-" in road else 0, y0, y1, *ptrs))
    elif road == "pt-state":
        check(getattr(lib, "fr_escape_rows_pt%s_state%s" % (w, suffix))(C.byref(v.cfg), v.where(), y0, y1, *ptrs))
    elif road == "pt-extend":
        check(getattr(lib, "fr_escape_extend_pt%s%s" % (w, suffix))(C.byref(v.cfg), v.where(), y0, y1, LOW_CAP, *ptrs))
    elif road == "scaled-state":
        check(getattr(lib, "fr_escape_rows_pt_scaled_state" + suffix)(C.byref(v.cfg), C.byref(v.centre), y0, y1, *ptrs))
    else:
        check(getattr(lib, "fr_escape_extend_pt_scaled" + suffix)(C.byref(v.cfg), C.byref(v.centre), y0, y1, LOW_CAP, *ptrs))
    if device:
        torch.cuda.synchronize()
        host = [t.cpu().numpy().view(d).reshape(s) for t, s, d in zip(dev, shapes, DTYPES)]
    return tuple(host)


@functools.lru_cache(maxsize=None)
def _state_at_150(lib, v, road):
    """the host form's state at the low cap, whole image: what the extension `road` starts from"""
    host = [np.zeros(s, dtype=d) for s, d in zip(raw_shapes(H_, 4), DTYPES)]
    if scaled(road):
        check(lib.fr_escape_rows_pt_scaled_state(C.byref(v.low), C.byref(v.centre), 0, H_, *(a.ctypes.data for a in host)))
    else:
        name = "fr_escape_rows_pt%s_state" % ("_wide" if v.wide else "")
        check(getattr(lib, name)(C.byref(v.low), v.where(), 0, H_, *(a.ctypes.data for a in host)))
    for a in host:
        a.setflags(write=False)
    return tuple(host)


@functools.lru_cache(maxsize=None)
def _whole(lib, torch, v, road, form):
    """the whole image by one call, computed once per (view, road, form) and never written to"""
    out = run(lib, torch, v, road, form, 0, H_, _state_at_150(lib, v, road) if road.endswith("extend") else None)
    for a in out:
        a.setflags(write=False)
    return out


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ---- the tests ------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.mark.parametrize("name,road", cases())
def test_host_form_and_device_form_write_the_same(fr, lib, torch, name, road):
    v = _view(fr, name)
    host, device = _whole(lib, torch, v, road, "host"), _whole(lib, torch, v, road, "device")
    assert same(host, device), "%s, %s: the two forms differ" % (name, road)
    if road.endswith(("rgb", "rgba")):  # not a flat image, and rows that differ (the raw roads below count the view's indices)
        assert len(np.unique(host[0].reshape(-1, host[0].shape[2]), axis=0)) > 1
        assert len({row.tobytes() for row in host[0][SUB[0]:SUB[1]]}) > 1
        assert road.endswith("rgb") or (host[0][..., 3] == 255).all()
    else:
        assert len(np.unique(host[1])) > 5 and host[1].max() <= CAP
    if road.endswith("extend"):  # it moved the pixels still running at 150 and nothing else; what it gives is the state at 300
        low = _state_at_150(lib, v, road)
        running = low[1] == LOW_CAP
        assert running.any() == (not name.startswith("M-") or name == "M-2^300")
        assert same(tuple(a[~running] for a in host), tuple(a[~running] for a in low))
        assert not running.any() or not np.array_equal(host[2][running], low[2][running])
        assert same(host, _whole(lib, torch, v, state_road(road), "host"))


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name,road", cases())
def test_rows_5_to_12_alone_are_those_rows_of_the_whole(fr, lib, torch, name, road, form):
    v = _view(fr, name)
    y0, y1 = SUB
    start = tuple(a[y0:y1] for a in _state_at_150(lib, v, road)) if road.endswith("extend") else None
    piece = run(lib, torch, v, road, form, y0, y1, start)
    assert same(piece, tuple(a[y0:y1] for a in _whole(lib, torch, v, road, form))), "%s, %s, %s form" % (name, road, form)


@pytest.mark.parametrize("name", ["M-lo", "M-wide", "J-wide"])
def test_profiling_reports_each_roads_kernel_in_both_forms(fr, lib, torch, name):
    v = _view(fr, name)

    def last():
        buf, ms = C.create_string_buffer(256), C.c_float(-1.0)
        check(lib.fr_last_kernel_name(buf, len(buf)))
        check(lib.fr_last_kernel_ms(C.byref(ms)))
        return buf.value.decode(), ms.value

    try:
        for road in ROADS:
            if not applies(name, road):
                continue
            for form in ("host", "device"):
                check(lib.fr_set_profiling(0))  # forgets the last kernel: a road that records nothing has nothing to report
                check(lib.fr_set_profiling(1))
                got = run(lib, torch, v, road, form, 0, H_, _state_at_150(lib, v, road) if road.endswith("extend") else None)
                kname, ms = last()
                assert kname == KERNEL[road] and ms > 0.0, "%s, %s form: %r, %r ms" % (road, form, kname, ms)
                assert same(got, _whole(lib, torch, v, road, form)), "%s, %s form: profiling changed the result" % (road, form)
    finally:
        check(lib.fr_set_profiling(0))
