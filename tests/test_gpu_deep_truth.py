"""The deep kernels against exact per-pixel orbits (tests/deep_truth.py, the fixture tests/golden/deep_truth.npz), with no host
model in between: on every settled pixel the exact escape index, and z within move + floor max(|z|, 1) of the exact z.  The
views are off their special points, with negative, unequal and non-power-of-two scales and the default limit beside the
Misiurewicz, Julia and minibrot views of the scaled tests; device arrays lie between guard bytes.
  - WIDE PT: fr_escape_rows_pt_wide inside its domain; fr_escape_rows_pt_wide_state_device followed by
    fr_escape_extend_pt_wide_device, split at cap / 3 and at the median exact index;
  - BLA-PT: fr_escape_rows_pt_bla(_device) with a centre for bits 0, 40 and 53, and with pos_lo on the dd-centre view;
  - PT and DD (hi parts) on the dd-centre view;
  - SCALED PT: fr_escape_rows_pt_scaled(_device) on every wide-centre view for bits -1, 0 and 53;
    fr_escape_rows_pt_scaled_state_device followed by fr_escape_extend_pt_scaled_device past the 2^440 edge;
  - the header's CLAIM on scales whose mantissa is not 1: inside the common domain the scaled calls give the wide and BLA calls'
    z and iters bit for bit;
  - one view rendered as three ragged row pieces against the slices of the whole."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_truth as T

pytestmark = pytest.mark.gpu

GUARD = 64
WIDE_KIND = [n for n, s in T.VIEWS.items() if s.kind == "wide"]  # (a) to (g)


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
    return native.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def check(rc):
    from fractal_renderer_amd import _native

    _native.check(rc)


@functools.lru_cache(maxsize=None)
def truth(name):
    return T.load(name)


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(got, want, what):
    assert np.array_equal(got[1], want[1]), "%s: escape indices differ at %d pixels" % (what, int((got[1] != want[1]).sum()))
    assert np.array_equal(bits_of(got[0]), bits_of(want[0])), "%s: z differs at %d doubles" % (
        what, int((bits_of(got[0]) != bits_of(want[0])).sum()))


class Road:
    """the calls of one view: its config, and its centre (wide) or pos_lo (dd) kept alive beside it.  `name` is one of
    deep_truth.VIEWS, or a Spec, a record of tests/deep_random_views.py or a deep_truth.View in its place."""

    def __init__(self, fr, native, lib, name, cap=None):
        self.lib, self.v = lib, T.view(name)
        v = self.v
        self.cfg = v.fill(fr.Config.new(), cap)
        self.shape = v.shape
        if v.kind == "wide":
            p64 = C.POINTER(C.c_uint64)
            self._centre = native.fr_wide_centre(v.n, v.words[0].ctypes.data_as(p64), v.words[1].ctypes.data_as(p64))
            self.centre, self.lo = C.byref(self._centre), None
        else:
            self._lo = native.Imaginary(*v.pos_lo)
            self.centre, self.lo = None, C.byref(self._lo)

    def call(self, mode, bits, device, y0, y1):
        """-> f(z pointer, iters pointer) -> the return code of the road's call over rows [y0, y1)"""
        lib, cfg = self.lib, C.byref(self.cfg)
        if mode == "wide":
            assert not device
            return lambda z, it: lib.fr_escape_rows_pt_wide(cfg, self.centre, y0, y1, z, it)
        if mode == "bla":
            if device:
                return lambda z, it: lib.fr_escape_rows_pt_bla_device(cfg, self.lo, self.centre, bits, y0, y1, z, it, None)
            return lambda z, it: lib.fr_escape_rows_pt_bla(cfg, self.lo, self.centre, bits, y0, y1, z, it)
        if mode == "scaled":
            if device:
                return lambda z, it: lib.fr_escape_rows_pt_scaled_device(cfg, self.centre, bits, y0, y1, z, it, None)
            return lambda z, it: lib.fr_escape_rows_pt_scaled(cfg, self.centre, bits, y0, y1, z, it)
        assert not device
        if mode == "pt":
            return lambda z, it: lib.fr_escape_rows_pt(cfg, self.lo, y0, y1, z, it)
        if mode == "dd":
            return lambda z, it: lib.fr_escape_rows_dd(cfg, self.lo, y0, y1, z, it)
        raise KeyError(mode)

    def rows(self, mode, bits=-1, device=False, torch=None, y0=0, y1=None):
        """(z float64 [rows, width, 2], iters uint32 [rows, width]) of a call; the device form into guarded buffers"""
        y1 = self.shape[0] if y1 is None else y1
        h, w = y1 - y0, self.shape[1]
        per = 4 if mode == "dd" else 2
        f = self.call(mode, bits, device, y0, y1)
        if not device:
            z = np.full((h, w, per), np.nan)
            it = np.full((h, w), 0xFFFFFFFF, dtype=np.uint32)
            check(f(z.ctypes.data, it.ctypes.data))
            return (np.ascontiguousarray(z[..., 0::2]) if mode == "dd" else z), it
        npx = h * w
        zb = torch.full((GUARD + 16 * npx + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        ib = torch.full((GUARD + 4 * npx + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        check(f(zb.data_ptr() + GUARD, ib.data_ptr() + GUARD))
        torch.cuda.synchronize()
        zh, ih = zb.cpu().numpy(), ib.cpu().numpy()
        for a, n in ((zh, 16 * npx), (ih, 4 * npx)):
            assert (a[:GUARD] == 0xA5).all() and (a[GUARD + n:] == 0xA5).all(), "a write outside the array"
        return (zh[GUARD:GUARD + 16 * npx].copy().view(np.float64).reshape(h, w, 2),
                ih[GUARD:GUARD + 4 * npx].copy().view(np.uint32).reshape(h, w))


_roads = {}


def road(fr, native, lib, name, cap=None):
    if (name, cap) not in _roads:
        _roads[name, cap] = Road(fr, native, lib, name, cap)
    return _roads[name, cap]


def against_truth(name, mode, bits, got, what):
    t = truth(name)
    differ, ratio, excess = T.compare(t, got[0], got[1])
    print("%s, %s: settled %d of %d, off the exact index %d, |error| / move <= %.3g, excess %.3g" % (
        name, what, int(t["settled"].sum()), t["settled"].size, differ, ratio, excess))  # DESIGN.md's table, with -s
    T.assert_rows(t, got[0], got[1], "%s, %s" % (name, what), allowed=T.allowed(name, mode, bits), **T.bounds(name))


class State:
    """(z, iters, dz or w, m) of `npx` pixels in device memory, guard bytes on both sides of each array"""

    SIZES = (16, 4, 16, 4)
    TYPES = (np.float64, np.uint32, np.float64, np.uint32)

    def __init__(self, torch, npx):
        self.torch = torch
        self.bytes = [npx * s for s in self.SIZES]
        self.bufs = [torch.full((GUARD + b + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0") for b in self.bytes]
        assert all(t.data_ptr() % 16 == 0 for t in self.bufs)
        self.ptrs = [t.data_ptr() + GUARD for t in self.bufs]

    def read(self, shape):
        self.torch.cuda.synchronize()
        out = []
        for buf, b, ty in zip(self.bufs, self.bytes, self.TYPES):
            h = buf.cpu().numpy()
            assert (h[:GUARD] == 0xA5).all() and (h[GUARD + b:] == 0xA5).all(), "a write outside the array"
            out.append(h[GUARD:GUARD + b].copy().view(ty).reshape(tuple(shape) + ((2,) if ty is np.float64 else ())))
        return tuple(out)


def two_links(fr, native, lib, torch, name, mode, render, extend):
    """the state render at N, then the extension to the view's cap, for each N of T.splits: min(exact, N) on the settled
    pixels at N, the full comparison at the cap"""
    t, v = truth(name), T.view(name)
    h, w = v.shape
    for n in T.splits(name):
        low, high = road(fr, native, lib, name, n), road(fr, native, lib, name)
        st = State(torch, h * w)
        check(render(C.byref(low.cfg), low.centre, 0, h, *st.ptrs, None))
        z, it, _, _ = st.read(v.shape)
        T.assert_rows(t, z, it, "%s, the state at %d" % (name, n), cap=n)
        check(extend(C.byref(high.cfg), high.centre, 0, h, n, *st.ptrs, None))
        z, it, _, _ = st.read(v.shape)
        against_truth(name, mode, -1, (z, it), "the state extended %d -> %d" % (n, v.cap))


# ---- WIDE PT ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", T.WIDE_DOMAIN)
def test_wide_pt_follows_the_exact_orbit(fr, native, lib, name):
    against_truth(name, "wide", -1, road(fr, native, lib, name).rows("wide"), "fr_escape_rows_pt_wide")


@pytest.mark.parametrize("name", ["M_440", "J_OFF_300"])
def test_wide_pt_state_and_extension_follow_the_exact_orbit(fr, native, lib, torch, name):
    two_links(fr, native, lib, torch, name, "wide", lib.fr_escape_rows_pt_wide_state_device, lib.fr_escape_extend_pt_wide_device)


# ---- BLA-PT -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("bits", [0, 40, 53])
@pytest.mark.parametrize("name", T.WIDE_DOMAIN + T.DD)
def test_bla_pt_follows_the_exact_orbit(fr, native, lib, torch, name, bits):
    r = road(fr, native, lib, name)
    dev = r.rows("bla", bits, True, torch)
    against_truth(name, "bla", bits, dev, "fr_escape_rows_pt_bla_device, bits %d" % bits)
    assert_same(r.rows("bla", bits), dev, "%s: fr_escape_rows_pt_bla against its device form, bits %d" % (name, bits))


# ---- PT and DD on a dd centre --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", ["pt", "dd"])
@pytest.mark.parametrize("name", T.DD)
def test_pt_and_dd_follow_the_exact_orbit(fr, native, lib, name, mode):
    against_truth(name, mode, -1, road(fr, native, lib, name).rows(mode), "fr_escape_rows_%s" % mode)


# ---- SCALED PT ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("bits", [-1, 0, 53])
@pytest.mark.parametrize("name", WIDE_KIND)
def test_scaled_pt_follows_the_exact_orbit(fr, native, lib, torch, name, bits):
    r = road(fr, native, lib, name)
    dev = r.rows("scaled", bits, True, torch)
    against_truth(name, "scaled", bits, dev, "fr_escape_rows_pt_scaled_device, bits %d" % bits)
    assert_same(r.rows("scaled", bits), dev, "%s: fr_escape_rows_pt_scaled against its device form, bits %d" % (name, bits))


@pytest.mark.parametrize("name", ["M_900", "J_900", "MINI_OFF_860"])
def test_scaled_pt_state_and_extension_follow_the_exact_orbit(fr, native, lib, torch, name):
    two_links(fr, native, lib, torch, name, "scaled", lib.fr_escape_rows_pt_scaled_state_device,
              lib.fr_escape_extend_pt_scaled_device)


@pytest.mark.parametrize("name", T.WIDE_DOMAIN)
def test_inside_the_common_domain_the_scaled_calls_are_the_wide_and_bla_calls(fr, native, lib, torch, name):
    """the header's CLAIM ("SCALED PT"), on scales whose mantissa is not 1 and on the default limit"""
    r = road(fr, native, lib, name)
    assert_same(r.rows("scaled", -1, True, torch), r.rows("wide"), name + ": bits = -1 against fr_escape_rows_pt_wide")
    for bits in (0, 53):
        assert_same(r.rows("scaled", bits, True, torch), r.rows("bla", bits, True, torch),
                    "%s: bits = %d against fr_escape_rows_pt_bla_device" % (name, bits))


# ---- row pieces ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode,bits", [("scaled", -1), ("scaled", 0), ("bla", 0)])
def test_row_pieces_equal_the_slices_of_the_whole(fr, native, lib, torch, mode, bits):
    name = "M_OFF_299"  # 37 x 21: ragged edges, more than one workgroup on both axes, unequal scales of either sign
    r = road(fr, native, lib, name)
    whole = r.rows(mode, bits, True, torch)
    against_truth(name, mode, bits, whole, "the whole, %s bits %d" % (mode, bits))
    for y0, y1 in ((0, 5), (5, 12), (12, 21)):
        assert_same(r.rows(mode, bits, True, torch, y0, y1), (whole[0][y0:y1], whole[1][y0:y1]),
                    "%s: rows [%d, %d), %s bits %d" % (name, y0, y1, mode, bits))
