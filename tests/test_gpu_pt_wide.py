"""WIDE PT on the device (include/fractal_hip.h, fr_precision: "WIDE PT"; the fr_*_pt_wide calls), bit for bit against
tests/pt_wide_model.py — reference orbits on Python integers, the pixel loop restated in tests/pt_wide_model.c.  The counts
asserted here were computed on the CPU with that model and limit = 2, so that a view cannot go trivial unnoticed:
  - the Misiurewicz centre at n = 5, scale 2^200 (16 x 12 and 37 x 21 with row pieces) and at n = 9, scale 2^440, the edge
    of the domain; the period-3 nucleus, whose orbit the cap cuts; a Julia view on the repelling fixed point;
  - RGB and RGBA renders, host and device forms, against fr_colour_rgb8 over the escape rows;
  - the cap raised in place on orbits continued from their integer tail, finished and foreign pixels untouched;
  - one orbit slot, two roads; the Python centre= road, the C++ overload and the CLI against the C call."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pt_state_model as SM
import pt_wide_model as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
NAN_BITS = 0x7FF8DEADBEEF1234


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


def check(rc):
    from fractal_renderer_amd import _native

    _native.check(rc)


class View:
    """a view of the tests with the model's results at its cap, computed once and never written to"""

    def __init__(self, name, n, scale_log2, width, height, cap):
        import fractal_renderer_amd as fr
        from fractal_renderer_amd import _native

        self.name, self.n = name, n
        self.cfg = W.view(fr.Config.new(), name, scale_log2, width, height, cap)
        self.ints = W.centre_ints(name, n)
        self.words = W.to_words(self.ints[0], n), W.to_words(self.ints[1], n)
        p64 = C.POINTER(C.c_uint64)
        self.centre = _native.fr_wide_centre(n, self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64))
        self.orbits = W.Orbits(self.cfg, *self.ints, n)
        self.state, self.rebases = W.state_rows(self.cfg, self.orbits)  # the state rule
        self.pt, _ = W.state_rows(self.cfg, self.orbits, rule=1)  # PT's rule: z and iters of plain WIDE PT
        for a in self.state + self.pt + (self.rebases,):
            a.setflags(write=False)
        self.shape = (height, width)

    @property
    def c(self):
        return C.byref(self.centre)


@functools.lru_cache(maxsize=None)
def view(name, n, scale_log2, width, height, cap):
    return View(name, n, scale_log2, width, height, cap)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_state(got, want, what):
    assert np.array_equal(got[1], want[1]), "%s: escape indices differ at %d pixels" % (what, int((got[1] != want[1]).sum()))
    assert np.array_equal(got[3], want[3]), "%s: m differs at %d pixels" % (what, int((got[3] != want[3]).sum()))
    for k, label in ((0, "z"), (2, "dz")):
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s: %s differs at %d doubles" % (
            what, label, int((bits(got[k]) != bits(want[k])).sum()))


def escape_rows(lib, v, y0=0, y1=None, cfg=None):
    cfg = v.cfg if cfg is None else cfg
    y1 = cfg.height if y1 is None else y1
    z = np.empty((y1 - y0, cfg.width, 2), dtype=np.float64)
    it = np.empty((y1 - y0, cfg.width), dtype=np.uint32)
    check(lib.fr_escape_rows_pt_wide(C.byref(cfg), v.c, y0, y1, z.ctypes.data, it.ctypes.data))
    return z, it


def state_rows(lib, v, y0=0, y1=None, cfg=None):
    cfg = v.cfg if cfg is None else cfg
    y1 = cfg.height if y1 is None else y1
    shape = (y1 - y0, cfg.width)
    z, dz = np.empty(shape + (2,), dtype=np.float64), np.empty(shape + (2,), dtype=np.float64)
    it, m = np.empty(shape, dtype=np.uint32), np.empty(shape, dtype=np.uint32)
    check(lib.fr_escape_rows_pt_wide_state(C.byref(cfg), v.c, y0, y1, z.ctypes.data, it.ctypes.data, dz.ctypes.data, m.ctypes.data))
    return z, it, dz, m


def with_cap(fr, v, cap):
    cfg = fr.Config.from_buffer_copy(bytes(v.cfg))
    cfg.iterations = cap
    return cfg


def cache(lib):
    out = (C.c_uint32 * 4)()
    check(lib.fr_debug_pt_orbit_cache(out))
    return tuple(out)


class State:
    """(z, iters, dz, m) of `npx` pixels in device memory, guard bytes on both sides of each array"""

    SIZES = (16, 4, 16, 4)
    TYPES = (np.float64, np.uint32, np.float64, np.uint32)

    def __init__(self, torch, npx):
        dev = torch.device("cuda", 0)
        self.torch, self.npx = torch, npx
        self.bytes = [npx * s for s in self.SIZES]
        self.bufs = [torch.full((GUARD + b + GUARD,), 0xA5, dtype=torch.uint8, device=dev) for b in self.bytes]
        assert all(t.data_ptr() % 16 == 0 for t in self.bufs)
        self.ptrs = [t.data_ptr() + GUARD for t in self.bufs]

    def upload(self, state):
        t = self.torch
        for buf, b, a, ty in zip(self.bufs, self.bytes, state, self.TYPES):
            a = np.ascontiguousarray(a, dtype=ty)
            assert a.nbytes == b
            buf[GUARD:GUARD + b] = t.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(buf.device)
        t.cuda.synchronize()
        return self

    def read(self, shape):
        self.torch.cuda.synchronize()
        out = []
        for buf, b, ty in zip(self.bufs, self.bytes, self.TYPES):
            h = buf.cpu().numpy()
            assert (h[:GUARD] == 0xA5).all() and (h[GUARD + b:] == 0xA5).all(), "a write outside the array"
            a = h[GUARD:GUARD + b].copy().view(ty)
            out.append(a.reshape(tuple(shape) + ((2,) if ty is np.float64 else ())))
        return tuple(out)


# ---- escape rows and state against the model ---------------------------------------------------------------------------

MIS_16 = ("M", 5, 200, 16, 12, 3000)
MIS_37 = ("M", 5, 200, 37, 21, 3000)
MIS_DEEP = ("M", 9, 440, 16, 12, 3000)
NUCLEUS = ("N", 5, 100, 16, 12, 600)
JULIA = ("J", 4, 150, 16, 12, 3000)


@pytest.mark.parametrize("spec,entries,lo,hi,distinct,rebasing", [
    (MIS_16, 194, 122, 191, 15, 76),
    (MIS_37, 194, 122, 140, 15, 317),  # ragged edges, more than one workgroup on both axes
    (MIS_DEEP, 352, 270, 349, 13, 62),  # scale 2^440: the edge of the domain
])
def test_misiurewicz_views_match_the_model(fr, lib, spec, entries, lo, hi, distinct, rebasing):
    v = view(*spec)
    orbit, ended, _ = v.orbits.x
    assert len(orbit) == entries and ended
    it = v.state[1]
    assert (int(it.min()), int(it.max()), len(np.unique(it))) == (lo, hi, distinct)
    assert int((v.rebases > 0).sum()) == rebasing and it.size == spec[3] * spec[4]
    z, got_it = escape_rows(lib, v)
    assert np.array_equal(got_it, v.pt[1]) and np.array_equal(bits(z), bits(v.pt[0]))
    assert_state(state_rows(lib, v), v.state, "state")
    assert cache(lib)[:3] == (3000, entries, 0)


def test_row_pieces_equal_the_slices_of_the_whole(fr, lib):
    v = view(*MIS_37)
    for y0, y1 in ((0, 8), (8, 13), (13, 21)):
        z, it = escape_rows(lib, v, y0, y1)
        assert np.array_equal(it, v.pt[1][y0:y1]) and np.array_equal(bits(z), bits(v.pt[0][y0:y1])), (y0, y1)
        assert_state(state_rows(lib, v, y0, y1), tuple(a[y0:y1] for a in v.state), "rows [%d, %d)" % (y0, y1))


def test_an_orbit_cut_by_the_cap(fr, lib):
    """The period-3 nucleus: every pixel reaches the cap, the orbit is cut by it, and plain WIDE PT and the state run differ
    exactly in the final-step rebase (RESUMABLE PT's claim): same z and iters, and (dz, m) = (z, 0) against the offset and
    m = last, at the pixels that never rebased."""
    v = view(*NUCLEUS)
    orbit, ended, _ = v.orbits.x
    assert len(orbit) == 602 and not ended
    assert (v.state[1] == 600).all() and (v.pt[1] == 600).all()
    z, it = escape_rows(lib, v)
    got = state_rows(lib, v)
    assert np.array_equal(it, v.pt[1]) and np.array_equal(bits(z), bits(v.pt[0]))
    assert_state(got, v.state, "state")
    assert np.array_equal(bits(got[0]), bits(z)) and np.array_equal(got[1], it)
    at_end = v.state[3] == 601  # still on R, never rebased: m == last at the final step
    assert at_end.any()
    assert np.array_equal(bits(v.pt[2])[at_end], bits(v.pt[0])[at_end]) and (v.pt[3][at_end] == 0).all()  # PT rebased there
    assert np.array_equal(bits(v.pt[2])[~at_end], bits(v.state[2])[~at_end]) and np.array_equal(v.pt[3][~at_end], v.state[3][~at_end])
    assert not np.array_equal(bits(v.pt[2])[at_end], bits(v.state[2])[at_end])


def test_a_julia_view_on_the_repelling_fixed_point(fr, lib):
    """julia_set = -0.8 + 0.156i, centre (1 + sqrt(1 - 4J)) / 2 floored to n = 4 words, scale 2^150, 16 x 12, cap 3000.
    What the model gave when this test was written: V has 158 entries and K 253, both ended by escape; the escape indices
    run from 92 to 426 with 24 distinct values; 71 of the 192 pixels rebase (onto K)."""
    v = view(*JULIA)
    assert v.orbits.x[1] and v.orbits.k[1] and len(v.orbits.x[0]) > 100 and len(v.orbits.k[0]) > 100
    assert len(np.unique(v.state[1])) > 1
    assert (v.rebases > 0).any() and not (v.rebases > 0).all()
    z, it = escape_rows(lib, v)
    assert np.array_equal(it, v.pt[1]) and np.array_equal(bits(z), bits(v.pt[0]))
    assert_state(state_rows(lib, v), v.state, "state")
    assert cache(lib)[:3] == (3000, len(v.orbits.x[0]), len(v.orbits.k[0]))


# ---- colours ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("spec", [MIS_37, JULIA])
@pytest.mark.parametrize("smooth", [1, 0])
def test_renders_are_the_colour_map_over_the_escape_rows(fr, lib, torch, spec, smooth):
    v = view(*spec)
    cfg = with_cap(fr, v, v.cfg.iterations)
    cfg.smooth, cfg.exposure = smooth, 3.0
    h, w = v.shape
    want = fr.colour_image(cfg, v.pt[0], v.pt[1])
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 4
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    check(lib.fr_render_rows_pt_wide(C.byref(cfg), v.c, 0, h, 3, rgb.ctypes.data, rgb.nbytes))
    assert np.array_equal(rgb, want)
    rgba = np.zeros((h, w, 4), dtype=np.uint8)
    check(lib.fr_render_rows_pt_wide(C.byref(cfg), v.c, 0, h, 4, rgba.ctypes.data, rgba.nbytes))
    assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all()
    for channels in (3, 4):
        n = channels * w * h
        buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        check(lib.fr_render_rows_pt_wide_device(C.byref(cfg), v.c, 0, h, channels, buf.data_ptr() + GUARD, n, None))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:GUARD] == 0xA5).all() and (got[GUARD + n:] == 0xA5).all()
        img = got[GUARD:GUARD + n].reshape(h, w, channels)
        assert np.array_equal(img[..., :3], want) and (channels == 3 or (img[..., 3] == 255).all())
    # rows [3, 11) into the device form
    n = 3 * w * 8
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    check(lib.fr_render_rows_pt_wide_device(C.byref(cfg), v.c, 3, 11, 3, buf.data_ptr(), n, None))
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().reshape(8, w, 3), want[3:11])


# ---- the cap raised in place ---------------------------------------------------------------------------------------------


def test_raise_the_cap(fr, lib, torch):
    low, high = view("M", 5, 200, 16, 12, 100), view(*MIS_16)
    assert (low.state[1] == 100).all() and len(low.orbits.x[0]) == 102 and not low.orbits.x[1]
    h, w = low.shape
    st = State(torch, w * h)
    check(lib.fr_escape_rows_pt_wide_state_device(C.byref(low.cfg), low.c, 0, h, *st.ptrs, None))
    assert_state(st.read(low.shape), low.state, "the state at 100")
    assert cache(lib) == (100, 102, 0, 102)
    check(lib.fr_escape_extend_pt_wide_device(C.byref(high.cfg), low.c, 0, h, 100, *st.ptrs, None))
    assert_state(st.read(low.shape), high.state, "100 -> 3000")
    assert cache(lib) == (3000, 194, 0, 92)  # only the missing entries, from the integer tail
    cfg4 = with_cap(fr, high, 4000)
    check(lib.fr_escape_extend_pt_wide_device(C.byref(cfg4), low.c, 0, h, 3000, *st.ptrs, None))
    assert_state(st.read(low.shape), high.state, "3000 -> 4000: every pixel had escaped")
    assert cache(lib) == (4000, 194, 0, 0)  # ended by escape: served as it is
    # the host-array form, and the state render at 3000 after the continued orbit
    got = tuple(np.array(a) for a in low.state)
    check(lib.fr_escape_extend_pt_wide(C.byref(high.cfg), low.c, 0, h, 100, got[0].ctypes.data, got[1].ctypes.data,
                                       got[2].ctypes.data, got[3].ctypes.data))
    assert_state(got, high.state, "host arrays 100 -> 3000")
    # in steps, through a cap at which some pixels have escaped
    mid = view("M", 5, 200, 16, 12, 124)
    check(lib.fr_escape_rows_pt_wide_state_device(C.byref(low.cfg), low.c, 0, h, *st.ptrs, None))
    check(lib.fr_escape_extend_pt_wide_device(C.byref(mid.cfg), low.c, 0, h, 100, *st.ptrs, None))
    assert_state(st.read(low.shape), mid.state, "100 -> 124")
    assert cache(lib) == (124, 126, 0, 24)
    check(lib.fr_escape_extend_pt_wide_device(C.byref(high.cfg), low.c, 0, h, 124, *st.ptrs, None))
    assert_state(st.read(low.shape), high.state, "124 -> 3000")
    assert cache(lib) == (3000, 194, 0, 68)
    # rows [4, 9) alone
    check(lib.fr_escape_rows_pt_wide_state_device(C.byref(low.cfg), low.c, 0, h, *st.ptrs, None))
    p = [st.ptrs[0] + 16 * 4 * w, st.ptrs[1] + 4 * 4 * w, st.ptrs[2] + 16 * 4 * w, st.ptrs[3] + 4 * 4 * w]
    check(lib.fr_escape_extend_pt_wide_device(C.byref(high.cfg), low.c, 4, 9, 100, *p, None))
    got = st.read(low.shape)
    assert_state(tuple(a[4:9] for a in got), tuple(a[4:9] for a in high.state), "rows [4, 9)")
    assert_state(tuple(np.concatenate((a[:4], a[9:])) for a in got), tuple(np.concatenate((a[:4], a[9:])) for a in low.state),
                 "the other rows")


def test_finished_and_foreign_pixels_are_untouched(fr, lib, torch):
    mid, high = view("M", 5, 200, 16, 12, 124), view(*MIS_16)
    z, it, dz, m = (np.array(a) for a in mid.state)
    finished = it != 124
    running = np.argwhere(~finished)
    assert finished.sum() >= 10 and len(running) >= 10
    foreign = np.zeros(it.shape, dtype=bool)
    for k, value in zip((0, 3, 7), (125, 5000, 0xFFFFFFFF)):  # above N: left alone like finished pixels
        y, x = running[k]
        it[y, x] = value
        foreign[y, x] = True
    skip = finished | foreign
    z.view(np.uint64)[skip] = NAN_BITS
    dz.view(np.uint64)[skip] = NAN_BITS
    m[skip] = 0xFFFFFFFF
    st = State(torch, it.size).upload((z, it, dz, m))
    check(lib.fr_escape_extend_pt_wide_device(C.byref(high.cfg), mid.c, 0, mid.shape[0], 124, *st.ptrs, None))
    got = st.read(mid.shape)
    for k, label in ((0, "z"), (2, "dz")):
        assert (bits(got[k])[skip] == NAN_BITS).all(), label + " of a finished or foreign pixel was written"
        assert np.array_equal(bits(got[k])[~skip], bits(high.state[k])[~skip]), label
    assert np.array_equal(got[1][skip], it[skip]) and np.array_equal(got[1][~skip], high.state[1][~skip])
    assert (got[3][skip] == 0xFFFFFFFF).all() and np.array_equal(got[3][~skip], high.state[3][~skip])
    # a launch with nothing running writes nothing
    done = tuple(np.array(a) for a in high.state)
    st.upload(done)
    check(lib.fr_escape_extend_pt_wide_device(C.byref(with_cap(fr, high, 5000)), mid.c, 0, mid.shape[0], 3000, *st.ptrs, None))
    assert_state(st.read(mid.shape), done, "nothing at the old cap")


# ---- one slot, two roads ---------------------------------------------------------------------------------------------------


def test_one_orbit_slot_serves_both_roads(fr, lib):
    v = view(*MIS_16)
    cfg, lo = SM.view("early_escape", O.config_new, 2000)
    plain = SM.state_rows(cfg, lo)
    pcfg = fr.Config.from_buffer_copy(bytes(cfg))
    wider = view("M", 9, 200, 16, 12, 3000)  # the same point, other words and another n
    deep = view(*MIS_DEEP)
    for _ in range(2):
        z, it = escape_rows(lib, v)
        assert np.array_equal(it, v.pt[1]) and np.array_equal(bits(z), bits(v.pt[0]))
        z, it = fr.escape_rows(pcfg, precision=fr.Precision.PT, pos_lo=lo)
        assert np.array_equal(it, plain[1]) and np.array_equal(bits(z), bits(plain[0]))
        assert cache(lib)[0] == 2000
        z, it = escape_rows(lib, wider)
        assert np.array_equal(it, wider.pt[1]) and np.array_equal(bits(z), bits(wider.pt[0]))
        z, it = escape_rows(lib, deep, cfg=deep.cfg)
        assert np.array_equal(it, deep.pt[1]) and np.array_equal(bits(z), bits(deep.pt[0]))
    # a wide view whose cfg->pos changes is the same view: pos is not read
    z, it = escape_rows(lib, v)
    cfg2 = with_cap(fr, v, 3000)
    cfg2.pos.re, cfg2.pos.im = math.nan, 5.0
    z2, it2 = escape_rows(lib, v, cfg=cfg2)
    assert cache(lib) == (3000, 194, 0, 0) and np.array_equal(it2, it) and np.array_equal(bits(z2), bits(z))


# ---- the mirrors ---------------------------------------------------------------------------------------------------------


def test_python_centre_road_gives_the_c_calls_bytes(fr, lib):
    v = view(*MIS_37)
    h, w = v.shape
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    want = np.zeros((h, w, 3), dtype=np.uint8)
    check(lib.fr_render_rows_pt_wide(C.byref(v.cfg), v.c, 0, h, 3, want.ctypes.data, want.nbytes))
    assert np.array_equal(want, fr.colour_image(v.cfg, v.pt[0], v.pt[1]))
    assert np.array_equal(fr.get_image(v.cfg, fr.Precision.PT, centre=centre), want)
    assert np.array_equal(fr.get_image_rows(v.cfg, 3, 17, fr.Precision.PT, centre=centre), want[3:17])
    rgba = fr.get_image_rgba(v.cfg, fr.Precision.PT, centre=centre)
    assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all()
    z, it = fr.escape_rows(v.cfg, precision=fr.Precision.PT, centre=centre)
    assert np.array_equal(it, v.pt[1]) and np.array_equal(bits(z), bits(v.pt[0]))
    assert_state(fr.escape_rows_pt_state(v.cfg, centre=centre), v.state, "escape_rows_pt_state")
    low = view("M", 5, 200, 37, 21, 100)
    assert_state(fr.extend_rows_pt(v.cfg, *low.state, 100, centre=centre), v.state, "extend_rows_pt")
    assert same_orbit(fr.reference_orbit_wide(v.cfg, centre), v.orbits.x[0])


def same_orbit(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def decimal_centre(fr, name, digits, scale):
    re, im = W.centre(name)
    tre, tim = W.decimal_text(re, digits), W.decimal_text(im, digits)
    return tre, tim, fr.WideCentre.from_str(tre, tim, scale=scale)


def test_cpp_overload_gives_the_librarys_image(fr, lib, tmp_path):
    import __graft_entry__ as ge

    ge.build()
    pkg = os.path.join(ROOT, "fractal-renderer_amd")
    exe = os.path.join(ROOT, "tests", "cpp", "test_wide_centre")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(pkg, "host"), os.path.join(ROOT, "tests", "cpp", "test_wide_centre.cpp"),
                    "-L" + pkg, "-lfractal_hip", "-Wl,-rpath," + pkg, "-o", exe], check=True)
    tre, tim, centre = decimal_centre(fr, "M", 140, 2.0 ** 200)
    assert centre.words == 5
    cfg = W.view(fr.Config.new(), "M", 200, 37, 21, 3000)
    out = str(tmp_path / "image.rgb")
    r = subprocess.run([exe, tre, tim, "200", "37", "21", "3000", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.uint8).reshape(21, 37, 3)
    want = fr.get_image(cfg, fr.Precision.PT, centre=centre)
    assert np.array_equal(got, want) and len(np.unique(want.reshape(-1, 3), axis=0)) > 1


def test_cli_perturbation_gives_the_librarys_image(fr, lib, tmp_path):
    import __graft_entry__ as ge

    ge.build()
    pkg = os.path.join(ROOT, "fractal-renderer_amd")
    exe = os.path.join(ROOT, "tests", "cpp", "fractal_cli")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(pkg, "host"), os.path.join(pkg, "cli", "fractal_cli.cpp"), "-L" + pkg, "-lfractal_hip",
                    "-Wl,-rpath," + pkg, "-o", exe], check=True)
    scale = 2.0 ** 200
    tre, tim, centre = decimal_centre(fr, "M", 140, scale)
    assert len(tre) == 143 and len(tim) == 142
    out = str(tmp_path / "deep")
    r = subprocess.run([exe, "--perturbation", "-x", tre, "-y", tim, "-s", repr(scale), "-i", "3000", "-l", "2", "48", "32", "-o", out,
                        "--quiet"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    data = open(out + ".ppm", "rb").read().split(b"\n", 3)
    assert data[0] == b"P6" and data[1] == b"48 32"
    got = np.frombuffer(data[3], dtype=np.uint8).reshape(32, 48, 3)
    ocfg = O.cli_config(48, 32, scale=(scale, scale), iterations=3000, limit=2.0, pos=(float(tre), float(tim)))
    want = fr.get_image(fr.Config.from_buffer_copy(bytes(ocfg)), fr.Precision.PT, centre=centre)
    assert np.array_equal(got, want) and len(np.unique(want.reshape(-1, 3), axis=0)) > 1
    # what --perturbation does not combine with is refused
    r = subprocess.run([exe, "--perturbation", "--f32", "4", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "--perturbation" in r.stderr
