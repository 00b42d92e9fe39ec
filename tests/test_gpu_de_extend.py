"""RESUMABLE DE on the device (include/fractal_hip.h, fr_precision: "RESUMABLE DE"; csrc/fr_de.hip: escape_extend_de_kernel,
escape_pt_de_state_kernel, escape_extend_pt_de_kernel), bit for bit against tests/de_state_model.py.  A NaN compares as a NaN;
every other double by its bits.

Per case (tests/de_extend_cases.py: a view, its road, a cap change N -> M): the state render at M against the model and against
the device's own fr_escape_rows_de and fr_escape_rows_pt_state; the render at N extended to M, with the finished pixels' arrays
poisoned first; a row piece and an empty one; the shaded bytes over the extended arrays.  Then the host forms and the Python
surface, the orbit cache across an extension, and the kernels' names.  Guard bytes lie on both sides of every device array."""
import ctypes as C

import numpy as np
import pytest

import de_extend_cases as X
import de_model as D
from test_gpu_de import Buf, _lo, check

pytestmark = pytest.mark.gpu

POISON_D = -1234.5
POISON_U = 0x25A5A5A5  # bit 31 clear: a foreign m, not an on-K flag


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


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


# ---- a case on the device ------------------------------------------------------------------------------------------------------


class Dev:
    """a case with the library's Config and, for a wide centre, its fr_wide_centre"""

    def __init__(self, name):
        import fractal_renderer_amd as fr
        from fractal_renderer_amd import _native

        self.c = c = X.case(name)
        self.name, self.pt = name, c.road == "pt"
        self.centre = self.words = None
        if c.wide:
            n = c.wide[1]
            self.words = X.W.to_words(c.ints[0], n), X.W.to_words(c.ints[1], n)
            p64 = C.POINTER(C.c_uint64)
            self.centre = _native.fr_wide_centre(n, self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64))
        self.lo = None if c.pos_lo is None else _lo(c.pos_lo)
        self.Config = fr.Config

    def cfg(self, cap):
        cfg = self.Config.from_buffer_copy(bytes(self.c.cfg))
        cfg.iterations = cap
        return cfg

    def where(self):
        """the (pos_lo, centre) arguments of the PT calls"""
        return (None if self.lo is None else C.byref(self.lo)), (None if self.centre is None else C.byref(self.centre))

    def py_kw(self, fr):
        if self.centre is not None:
            return dict(centre=fr.WideCentre(len(self.words[0]), self.words[0], self.words[1]))
        return dict(pos_lo=self.c.pos_lo) if self.c.pos_lo is not None else {}


_devs = {}


def dev(name):
    if name not in _devs:
        _devs[name] = Dev(name)
    return _devs[name]


class Arrays:
    """the state of rows x width pixels in device memory, in the model's order: F64 (z, iters, der), PT (z, iters, dz, m, der)"""

    def __init__(self, torch, pt, rows, width):
        self.shape, self.n, self.pt = (rows, width), rows * width, pt
        kinds = "dudud" if pt else "dud"
        self.kinds = kinds
        self.bufs = [Buf(torch, (16 if k == "d" else 4) * self.n) for k in kinds]

    def ptrs(self):
        return [b.ptr for b in self.bufs]

    def get(self):
        return tuple(b.get(np.float64, self.shape + (2,)) if k == "d" else b.get(np.uint32, self.shape) for b, k in zip(self.bufs, self.kinds))

    def put(self, state):
        for b, a in zip(self.bufs, state):
            b.put(a)
        return self

    def untouched(self):
        return all(b.untouched() for b in self.bufs)

    def der(self):
        return self.bufs[-1]


def render(lib, torch, d, cap, y0=0, y1=None):
    """the resumable render of the road at the cap: fr_escape_rows_de (F64) or fr_escape_rows_de_pt_state"""
    cfg = d.cfg(cap)
    y1 = cfg.height if y1 is None else y1
    a = Arrays(torch, d.pt, y1 - y0, cfg.width)
    if d.pt:
        check(lib.fr_escape_rows_de_pt_state_device(C.byref(cfg), *d.where(), y0, y1, *a.ptrs(), None))
    else:
        check(lib.fr_escape_rows_de_device(C.byref(cfg), 0, None, y0, y1, *a.ptrs(), None))
    return a


def extend(lib, d, a, n, cap, y0=0, y1=None):
    cfg = d.cfg(cap)
    y1 = cfg.height if y1 is None else y1
    if d.pt:
        check(lib.fr_escape_extend_de_pt_device(C.byref(cfg), *d.where(), y0, y1, n, *a.ptrs(), None))
    else:
        check(lib.fr_escape_extend_de_device(C.byref(cfg), 0, y0, y1, n, *a.ptrs(), None))


def assert_state(got, want, what):
    assert len(got) == len(want)
    labels = ("z", "iters", "dz", "m", "der") if len(got) == 5 else ("z", "iters", "der")
    for g, w, label in zip(got, want, labels):
        if g.dtype == np.float64:
            assert D.same_doubles(g, w), "%s: %s differs" % (what, label)
        else:
            assert np.array_equal(g, w), "%s: %s differs at %d pixels" % (what, label, int((g != w).sum()))


# ---- 1: the state render -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", X.PT)
def test_the_state_render_is_the_model_de_and_resumable_pt(lib, torch, name):
    d = dev(name)
    c, cfg = d.c, d.cfg(d.c.m)
    a = render(lib, torch, d, c.m)
    z, it, dz, m, der = got = a.get()
    assert_state(got, c.state(c.m), name)
    # fr_escape_rows_de's (z, iters, der) and fr_escape_rows_pt_state's (dz, m), on the device
    de = Arrays(torch, False, *a.shape)
    pts = Arrays(torch, True, *a.shape)  # its fifth array stays unused
    if d.centre is not None:
        check(lib.fr_escape_rows_de_pt_wide_device(C.byref(cfg), C.byref(d.centre), 0, cfg.height, *de.ptrs(), None))
        check(lib.fr_escape_rows_pt_wide_state_device(C.byref(cfg), C.byref(d.centre), 0, cfg.height, *pts.ptrs()[:4], None))
    else:
        lo = d.where()[0]
        check(lib.fr_escape_rows_de_device(C.byref(cfg), 3, lo, 0, cfg.height, *de.ptrs(), None))
        check(lib.fr_escape_rows_pt_state_device(C.byref(cfg), lo, 0, cfg.height, *pts.ptrs()[:4], None))
    assert_state((z, it, der), de.get(), name + ": against fr_escape_rows_de")
    pz, pit, pdz, pm = (b.get(np.float64, a.shape + (2,)) if k == "d" else b.get(np.uint32, a.shape)
                        for b, k in list(zip(pts.bufs, pts.kinds))[:4])
    assert_state((z, it, dz, m, der), (pz, pit, pdz, pm, der), name + ": against fr_escape_rows_pt_state")
    assert pts.der().untouched()


@pytest.mark.parametrize("name", ["pt-mandelbrot-37x23", "pt-julia-rebase", "wide-2^200-37x21"])
def test_the_state_render_at_caps_zero_and_one(lib, torch, name):
    d = dev(name)
    for cap in (0, 1):
        got = render(lib, torch, d, cap).get()
        assert_state(got, d.c.state(cap), "%s at cap %d" % (name, cap))
        if cap == 0:
            assert (got[4] == [1.0, 0.0]).all() and not got[1].any()


# ---- 2, 3, 6: render at N, poison what is finished, extend to M, colour ----------------------------------------------------------


def poisoned(state, n):
    """the finished pixels' arrays other than iters overwritten: (the poisoned copies, the finished mask)"""
    finished = state[1] != n
    out = []
    for k, a in enumerate(state):
        a = np.array(a)
        if k != 1:
            a[finished] = POISON_U if a.dtype == np.uint32 else POISON_D
        out.append(a)
    return tuple(out), finished


@pytest.mark.parametrize("name", X.ALL)
def test_render_at_n_extend_to_m(lib, torch, name):
    d = dev(name)
    c = d.c
    want = c.state(c.m)
    assert X.classes(want[1], c.n, c.m)[1:] != (0, 0), "nothing would be continued"
    a = render(lib, torch, d, c.n)
    assert_state(a.get(), c.state(c.n), name + " at N")
    extend(lib, d, a, c.n, c.m)
    assert_state(a.get(), want, "%s %d -> %d" % (name, c.n, c.m))
    if not d.pt:  # (z, iters) are fr_escape_rows_device's at M as well
        cfg = d.cfg(c.m)
        plain = Arrays(torch, False, *a.shape)
        check(lib.fr_escape_rows_device(C.byref(cfg), 0, None, 0, cfg.height, 2, plain.bufs[0].ptr, plain.bufs[1].ptr, None, None))
        got = a.get()
        assert np.array_equal(got[1], plain.bufs[1].get(np.uint32, a.shape))
        assert D.same_doubles(got[0], plain.bufs[0].get(np.float64, a.shape + (2,)))
    # the end-to-end bytes: the shaded colour map over the extended arrays is the model's image at M
    cfg = d.cfg(c.m)
    for channels in (3, 4):
        out = Buf(torch, channels * a.n)
        check(lib.fr_colour_de_rows_device(C.byref(cfg), a.bufs[0].ptr, a.bufs[1].ptr, a.der().ptr, a.n, 1.5, channels, out.ptr, None))
        assert np.array_equal(out.get(np.uint8, a.shape + (channels,)), c.image(1.5, channels)), "%s: %d channels" % (name, channels)
    # finished pixels are known by their iters word alone: poison in their other arrays survives the extension
    start, finished = poisoned(c.state(c.n), c.n)
    b = Arrays(torch, d.pt, *a.shape).put(start)
    extend(lib, d, b, c.n, c.m)
    got = b.get()
    assert np.array_equal(got[1], want[1])
    for k, (g, w) in enumerate(zip(got, want)):
        if k == 1:
            continue
        assert np.array_equal(g[finished], start[k][finished]), "%s: array %d of a finished pixel was written" % (name, k)
        running = ~finished
        assert D.same_doubles(g[running], w[running]) if g.dtype == np.float64 else np.array_equal(g[running], w[running]), (name, k)


def test_values_above_n_are_foreign_and_left_alone(lib, torch):
    d = dev("pt-seahorse-pos-lo")
    c = d.c
    start = tuple(np.array(a) for a in c.state(c.n))
    start[1][3, :] = c.n + 1  # a row of foreign escape indices, running pixels among them
    start[1][4, 0] = 0xFFFFFFFF
    b = Arrays(torch, True, *start[1].shape).put(start)
    extend(lib, d, b, c.n, c.m)
    got = b.get()
    for k in range(5):
        assert np.array_equal(got[k][3], start[k][3]) and np.array_equal(got[k][4, 0], start[k][4, 0])
    keep = np.ones(start[1].shape, dtype=bool)
    keep[3, :] = keep[4, 0] = False
    assert np.array_equal(got[1][keep], c.state(c.m)[1][keep])


def test_the_chain_150_300_3000(lib, torch):
    d = dev("pt-julia-rebase")
    c = d.c
    a = render(lib, torch, d, 150)
    assert (a.get()[1] == 150).all()  # every pixel is running
    for n, m in zip(c.chain, c.chain[1:]):
        extend(lib, d, a, n, m)
        got = a.get()
        assert_state(got, c.state(m), "chain %d -> %d" % (n, m))
    on_k = c.state(300)[3][c.state(300)[1] == 300] & 0x80000000
    assert on_k.all()  # the link 300 -> 3000 continued pixels that follow K


# ---- 4: row pieces -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["f64-mandelbrot-37x23", "pt-seahorse-pos-lo", "pt-orbit-escapes", "wide-2^200-37x21", "wide-julia"])
def test_a_row_piece_and_an_empty_one(lib, torch, name):
    d = dev(name)
    c = d.c
    y0, y1 = (5, 17) if c.cfg.height > 17 else (5, 13)
    a = render(lib, torch, d, c.n, y0, y1)
    assert_state(a.get(), tuple(x[y0:y1] for x in c.state(c.n)), name + ": the piece at N")
    extend(lib, d, a, c.n, c.m, y0, y1)
    assert_state(a.get(), tuple(x[y0:y1] for x in c.state(c.m)), name + ": the piece extended")
    e = Arrays(torch, d.pt, 2, c.cfg.width)
    extend(lib, d, e, c.n, c.m, 7, 7)  # no rows
    extend(lib, d, e, c.m, c.m, 0, 2)  # M == N
    cfg = d.cfg(c.m)
    if d.pt:
        check(lib.fr_escape_rows_de_pt_state_device(C.byref(cfg), *d.where(), 7, 7, *e.ptrs(), None))
    assert e.untouched()


def test_a_workgroup_with_nothing_running_writes_nothing(lib, torch):
    """all pixels finished: every workgroup takes the early exit; the arrays hold poison throughout"""
    for name in ("f64-julia-40x24", "pt-julia-40x24"):
        d = dev(name)
        c = d.c
        start = [np.array(a) for a in c.state(c.n)]
        start[1][:] = 3  # below N everywhere
        start, finished = poisoned(tuple(start), c.n)
        assert finished.all()
        b = Arrays(torch, d.pt, *start[1].shape).put(start)
        extend(lib, d, b, c.n, c.m)
        assert_state(b.get(), start, name)


# ---- 5: the host forms and the Python surface --------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["f64-julia-40x24", "pt-seahorse-pos-lo", "pt-overflow", "wide-julia"])
def test_host_forms_and_python(fr, lib, name):
    d = dev(name)
    c = d.c
    cfg_n, cfg_m = d.cfg(c.n), d.cfg(c.m)
    h = cfg_m.height
    if d.pt:
        st = tuple(np.empty_like(a) for a in c.state(c.n))
        check(lib.fr_escape_rows_de_pt_state(C.byref(cfg_n), *d.where(), 0, h, *(a.ctypes.data for a in st)))
        assert_state(st, c.state(c.n), name + ": host state render")
        check(lib.fr_escape_extend_de_pt(C.byref(cfg_m), *d.where(), 0, h, c.n, *(a.ctypes.data for a in st)))
        assert_state(st, c.state(c.m), name + ": host extension")
        kw = d.py_kw(fr)
        py = fr.escape_rows_de_pt_state(cfg_n, **kw)
        assert_state(py, c.state(c.n), name + ": python state render")
        assert_state(fr.extend_rows_de_pt(cfg_m, *py, c.n, **kw), c.state(c.m), name + ": python extension")
        assert_state(py, c.state(c.n), name + ": the arguments are left alone")
        piece = fr.extend_rows_de_pt(cfg_m, *(a[3:11] for a in py), c.n, y0=3, y1=11, **kw)
        assert_state(piece, tuple(a[3:11] for a in c.state(c.m)), name + ": python piece")
    else:
        st = tuple(np.array(a) for a in c.state(c.n))
        check(lib.fr_escape_extend_de(C.byref(cfg_m), 0, 0, h, c.n, *(a.ctypes.data for a in st)))
        assert_state(st, c.state(c.m), name + ": host extension")
        py = fr.escape_rows_de(cfg_n)
        assert_state(fr.extend_rows_de(cfg_m, *py, c.n), c.state(c.m), name + ": python extension")
        piece = fr.extend_rows_de(cfg_m, *(a[3:11] for a in py), c.n, y0=3, y1=11)
        assert_state(piece, tuple(a[3:11] for a in c.state(c.m)), name + ": python piece")
    assert np.array_equal(fr.colour_image_de(cfg_m, st[0], st[1], st[-1], 1.5), c.image(1.5, 3))


def test_python_device_forms(fr, lib, torch):
    for name in ("f64-mandelbrot-37x23", "pt-mandelbrot-37x23", "wide-julia"):
        d = dev(name)
        c = d.c
        a = Arrays(torch, d.pt, c.cfg.height, c.cfg.width)
        if d.pt:
            kw = d.py_kw(fr)
            fr.escape_rows_de_pt_state_device(d.cfg(c.n), *a.ptrs(), **kw)
            fr.extend_rows_de_pt_device(d.cfg(c.m), *a.ptrs(), c.n, **kw)
        else:
            fr.escape_rows_de_device(d.cfg(c.n), *a.ptrs())
            fr.extend_rows_de_device(d.cfg(c.m), *a.ptrs(), c.n)
        assert_state(a.get(), c.state(c.m), name)


# ---- 7: the orbit cache ------------------------------------------------------------------------------------------------------


def cache(lib):
    out = (C.c_uint32 * 4)()
    check(lib.fr_debug_pt_orbit_cache(out))
    return tuple(out)


def test_the_extension_continues_the_orbit_and_the_roads_share_it(fr, lib, torch):
    cfg = fr.Config.new()  # another view through the context: the cache then holds that one
    cfg.width = cfg.height = 8
    cfg.iterations = 3
    cfg.pos.re = 0.125
    fr.escape_rows(cfg, precision=fr.Precision.PT)
    d = dev("pt-seahorse-pos-lo")
    c = d.c
    a = render(lib, torch, d, c.n)
    assert cache(lib) == (c.n, c.n + 2, 0, c.n + 2)  # R_0 .. R_{N+1}, all computed
    z, it, der = fr.escape_rows_de(d.cfg(c.n), precision=fr.Precision.PT, pos_lo=c.pos_lo)  # the DE render: the same orbit
    assert cache(lib) == (c.n, c.n + 2, 0, 0)
    fr.escape_rows(d.cfg(c.n), precision=fr.Precision.PT, pos_lo=c.pos_lo)  # and the PT render
    assert cache(lib) == (c.n, c.n + 2, 0, 0)
    extend(lib, d, a, c.n, c.m)
    assert cache(lib) == (c.m, c.m + 2, 0, c.m - c.n)  # only the missing entries
    assert_state(a.get(), c.state(c.m), "after the continued orbit")
    again = render(lib, torch, d, c.m)  # the state render on the continued orbit
    assert cache(lib)[3] == 0
    assert_state(again.get(), c.state(c.m), "the state render on the continued orbit")


# ---- 8: the kernels' names ---------------------------------------------------------------------------------------------------


def test_profiling_names_the_kernels(lib, torch):
    def last():
        torch.cuda.synchronize()
        buf = C.create_string_buffer(128)
        check(lib.fr_last_kernel_name(buf, 128))
        return buf.value

    check(lib.fr_set_profiling(1))
    try:
        d = dev("f64-julia-40x24")
        a = render(lib, torch, d, d.c.n)
        extend(lib, d, a, d.c.n, d.c.m)
        assert last() == b"escape_extend_de_kernel"
        for name in ("pt-mandelbrot-37x23", "wide-julia"):
            d = dev(name)
            a = render(lib, torch, d, d.c.n)
            assert last() == b"escape_pt_de_state_kernel"
            extend(lib, d, a, d.c.n, d.c.m)
            assert last() == b"escape_extend_pt_de_kernel"
            ms = C.c_float(-1.0)
            check(lib.fr_last_kernel_ms(C.byref(ms)))
            assert ms.value > 0.0
    finally:
        check(lib.fr_set_profiling(0))
