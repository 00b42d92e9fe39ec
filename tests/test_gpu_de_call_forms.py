"""The two forms of every plain DE row, state and extension call against each other, by one table: the host form (context
scratch, one synchronisation) and the device form (the caller's arrays and stream) of
  fr_escape_rows_de (F64 and PT), fr_escape_rows_de_pt_wide, fr_escape_rows_de_pt_bla, fr_escape_rows_de_pt_scaled,
  fr_escape_rows_de_pt_state, fr_escape_rows_de_pt_scaled_state,
  fr_escape_extend_de, fr_escape_extend_de_pt, fr_escape_extend_de_pt_scaled
give the same bytes on rows [2, 19) of a 37 x 21 view: 3 x 2 deep workgroups with ragged right and bottom edges, a range that
starts and ends inside a workgroup.  Each on a Mandelbrot view, a Julia view and an algorithm without orbits (every array zero).
An extension starts from the state the device rendered at the cap N, goes to M through either form from that one stored state,
and both must agree with each other and with a direct render at M.  With profiling on, every call that launches leaves the
kernel name the road's own tests assert, and fr_last_kernel_ms succeeds.

The views are those of the roads' own tests at this size: tests/de_extend_cases.py's F64 / PT views (de_model.default_view,
julia_view) and wide views (pt_wide_model.view on M at 2^200 with 5 words and on J at 2^100 with 3) with their caps, and for
the scaled pairs pt_scaled_model's M and J at a scale of 2^900 with 16 words and caps of tests/pt_scaled_state_model.py's chains.
What the arrays must hold is the business of tests/test_gpu_de*.py; this file holds the forms together."""
import ctypes as C

import numpy as np
import pytest

import de_model as D
import pt_scaled_model as S
import pt_wide_model as W

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT, Y0, Y1 = 37, 21, 2, 19
NPX = WIDTH * (Y1 - Y0)
F64, PT = 0, 3
FERN = 1
FILL = 0xA5
# bytes per pixel and type of z, iters, d (dz / w), m, der
SIZES = {"z": 16, "it": 4, "d": 16, "m": 4, "der": 16}
THREE, FIVE = ("z", "it", "der"), ("z", "it", "d", "m", "der")


@pytest.fixture(scope="module")
def fr():
    import fractal_renderer_amd

    assert fractal_renderer_amd.device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    fractal_renderer_amd.init(0)
    assert fractal_renderer_amd.device_name().startswith("gfx950")
    return fractal_renderer_amd


@pytest.fixture(scope="module")
def native(fr):
    from fractal_renderer_amd import _native

    return _native


@pytest.fixture(scope="module")
def lib(native):
    lib = native.load()
    native.check(lib.fr_set_profiling(1))
    yield lib
    native.check(lib.fr_set_profiling(0))


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


class View:
    """a 37 x 21 view at its cap M, the lower cap N of its extension, and its wide centre where it has one"""

    def __init__(self, cfg, n, ints=None, words=0, fern=False):
        assert (cfg.width, cfg.height) == (WIDTH, HEIGHT) and n < cfg.iterations
        if fern:
            cfg.algo = FERN
        self.cfg, self.n, self.orbits = cfg, n, not fern
        self.words = (W.to_words(ints[0], words), W.to_words(ints[1], words)) if ints else None

    def at(self, cap):
        cfg = type(self.cfg).from_buffer_copy(bytes(self.cfg))
        cfg.iterations = cap
        return cfg

    def centre(self, native):
        if not self.words:
            return None
        p64 = C.POINTER(C.c_uint64)
        return C.byref(native.fr_wide_centre(len(self.words[0]), self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64)))


def views(fr, family):
    """{name: View} of a family: "shallow" (the F64 road and PT with a dd centre), "wide", "scaled" (past 2^440)"""
    new = fr.Config.new
    if family == "shallow":
        return {"mandelbrot": View(D.default_view(new(), WIDTH, HEIGHT, 200), 10), "julia": View(D.julia_view(new(), WIDTH, HEIGHT, 300), 20),
                "fern": View(D.default_view(new(), WIDTH, HEIGHT, 200), 10, fern=True)}
    if family == "wide":
        m, j = W.centre_ints("M", 5), W.centre_ints("J", 3)
        return {"mandelbrot": View(W.view(new(), "M", 200, WIDTH, HEIGHT, 3000), 120, m, 5),
                "julia": View(W.view(new(), "J", 100, WIDTH, HEIGHT, 400), 100, j, 3),
                "fern": View(W.view(new(), "M", 200, WIDTH, HEIGHT, 3000), 120, m, 5, fern=True)}
    m, j = S.centre_ints("M", 16), S.centre_ints("J", 16)
    return {"mandelbrot": View(W.view(new(), "M", 900, WIDTH, HEIGHT, 600), 560, m, 16),
            "julia": View(W.view(new(), "J", 900, WIDTH, HEIGHT, 632), 400, j, 16),
            "fern": View(W.view(new(), "M", 900, WIDTH, HEIGHT, 600), 560, m, 16, fern=True)}


# name -> (host function, view family, arrays, the arguments between cfg and y0 given the centre, kernel, the pair it extends)
PAIRS = {
    "de[f64]": ("fr_escape_rows_de", "shallow", THREE, lambda c: (F64, None), "escape_de_kernel", None),
    "de[pt]": ("fr_escape_rows_de", "shallow", THREE, lambda c: (PT, None), "escape_pt_de_kernel", None),
    "de_pt_wide": ("fr_escape_rows_de_pt_wide", "wide", THREE, lambda c: (c,), "escape_pt_de_kernel", None),
    "de_pt_bla[dd]": ("fr_escape_rows_de_pt_bla", "shallow", THREE, lambda c: (None, None, 0), "escape_bla_de_kernel", None),
    "de_pt_bla[wide]": ("fr_escape_rows_de_pt_bla", "wide", THREE, lambda c: (None, c, 30), "escape_bla_de_kernel", None),
    "de_pt_scaled[plain]": ("fr_escape_rows_de_pt_scaled", "scaled", THREE, lambda c: (c, -1), "escape_pt_scaled_de_kernel", None),
    "de_pt_scaled[table]": ("fr_escape_rows_de_pt_scaled", "scaled", THREE, lambda c: (c, 0), "escape_bla_scaled_de_kernel", None),
    "de_pt_state[dd]": ("fr_escape_rows_de_pt_state", "shallow", FIVE, lambda c: (None, None), "escape_pt_de_state_kernel", None),
    "de_pt_state[wide]": ("fr_escape_rows_de_pt_state", "wide", FIVE, lambda c: (None, c), "escape_pt_de_state_kernel", None),
    "de_pt_scaled_state": ("fr_escape_rows_de_pt_scaled_state", "scaled", FIVE, lambda c: (c,), "escape_pt_scaled_de_state_kernel", None),
    "extend_de": ("fr_escape_extend_de", "shallow", THREE, lambda c: (F64,), "escape_extend_de_kernel", "de[f64]"),
    "extend_de_pt[dd]": ("fr_escape_extend_de_pt", "shallow", FIVE, lambda c: (None, None), "escape_extend_pt_de_kernel", "de_pt_state[dd]"),
    "extend_de_pt[wide]": ("fr_escape_extend_de_pt", "wide", FIVE, lambda c: (None, c), "escape_extend_pt_de_kernel", "de_pt_state[wide]"),
    "extend_de_pt_scaled": ("fr_escape_extend_de_pt_scaled", "scaled", FIVE, lambda c: (c,), "escape_extend_pt_scaled_de_kernel",
                            "de_pt_scaled_state"),
}
CASES = [(pair, view) for pair in PAIRS for view in ("mandelbrot", "julia", "fern")]


def test_the_table_holds_the_nine_pairs_of_the_c_abi(native):
    functions = {p[0] for p in PAIRS.values()}
    assert len(functions) == 9 and all(f in native.PROTOTYPES and f + "_device" in native.PROTOTYPES for f in functions)


def last_kernel(native, lib):
    buf, ms = C.create_string_buffer(128), C.c_float(-1.0)
    native.check(lib.fr_last_kernel_name(buf, len(buf)))
    native.check(lib.fr_last_kernel_ms(C.byref(ms)))
    assert ms.value >= 0.0
    return buf.value.decode()


def call(native, lib, pair, view, cap, pointers, device, n=None, expect_launch=True):
    """one call of the pair in its host or device form on rows [Y0, Y1) at the cap; n: the extension's lower cap"""
    fn, _family, _arrays, head, kernel, _base = PAIRS[pair]
    cfg = view.at(cap)
    args = [C.byref(cfg), *head(view.centre(native)), Y0, Y1, *(() if n is None else (n,)), *pointers, *((None,) if device else ())]
    native.check(getattr(lib, fn + ("_device" if device else ""))(*args))
    if expect_launch:
        assert last_kernel(native, lib) == kernel, (pair, "device" if device else "host")


def device_arrays(torch, names):
    return [torch.full((NPX * SIZES[k],), FILL, dtype=torch.uint8, device="cuda:0") for k in names]


def host_arrays(names):
    return [np.full(NPX * SIZES[k], FILL, dtype=np.uint8) for k in names]


def to_host(torch, tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def same_but_for_a_nan(a, b, name):
    """the bytes equal; a double that is a NaN in both counts as equal, as the roads' own tests compare z and der"""
    if name in ("it", "m"):
        return np.array_equal(a, b)
    x, y = a.view(np.float64), b.view(np.float64)
    return np.array_equal(x.view(np.uint64)[~np.isnan(x)], y.view(np.uint64)[~np.isnan(y)]) and np.array_equal(np.isnan(x), np.isnan(y))


@pytest.mark.parametrize("pair,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_the_host_form_gives_the_device_form_s_bytes(fr, native, lib, torch, pair, name):
    _fn, family, names, _head, _kernel, base = PAIRS[pair]
    view = views(fr, family)[name]
    m = view.cfg.iterations
    if base is None:  # a render: the two forms at the cap
        dev, host = device_arrays(torch, names), host_arrays(names)
        call(native, lib, pair, view, m, [t.data_ptr() for t in dev], True)
        call(native, lib, pair, view, m, [a.ctypes.data for a in host], False)
        got = to_host(torch, dev)
        for k, a, b in zip(names, got, host):
            assert np.array_equal(a, b), "%s of %s on the %s view: the forms differ at %d bytes" % (k, pair, name, int((a != b).sum()))
            assert view.orbits or not a.any(), "%s of %s: an algorithm without orbits leaves zeros" % (k, pair)
        assert view.orbits is False or any((a != FILL).any() for a in got)
        return
    # an extension: the state at N on the device, continued to M through either form from that one stored state
    stored = device_arrays(torch, names)
    call(native, lib, base, view, view.n, [t.data_ptr() for t in stored], True)
    host = [a.copy() for a in to_host(torch, stored)]
    dev = [t.clone() for t in stored]
    call(native, lib, pair, view, m, [t.data_ptr() for t in dev], True, n=view.n, expect_launch=view.orbits)
    call(native, lib, pair, view, m, [a.ctypes.data for a in host], False, n=view.n, expect_launch=view.orbits)
    direct = device_arrays(torch, names)
    call(native, lib, base, view, m, [t.data_ptr() for t in direct], True)
    got, want = to_host(torch, dev), to_host(torch, direct)
    for k, a, b, c in zip(names, got, host, want):
        assert np.array_equal(a, b), "%s of %s on the %s view: the forms differ at %d bytes" % (k, pair, name, int((a != b).sum()))
        assert same_but_for_a_nan(a, c, k), "%s of %s on the %s view: the extension is not the render at M" % (k, pair, name)
        assert view.orbits or not a.any()
