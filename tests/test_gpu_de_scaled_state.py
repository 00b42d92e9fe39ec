"""RESUMABLE SCALED DE on the device (include/fractal_hip.h, "RESUMABLE SCALED DE"; fr_escape_rows_de_pt_scaled_state,
fr_escape_extend_de_pt_scaled and their _device forms; kernels escape_pt_scaled_de_state_kernel, escape_extend_pt_scaled_de_kernel),
bit for bit against tests/de_scaled_state_model.py on the chains of caps of tests/pt_scaled_state_model.py (tiny views):
  - the state render at every cap of every chain (caps 0 and 1 among them): device arrays between guard bytes, the host form, and —
    from the library's own calls — its (z, iters, der) against fr_escape_rows_de_pt_scaled with bits = -1 and its (w, m) against
    fr_escape_rows_pt_scaled_state;
  - every chain extended link by link on the device and in one jump; before each link the finished pixels' z, w, m and der are
    poisoned and a few of their iters set above N, all of it found unchanged afterwards; the link that begins with nothing
    running leaves every byte as it was;
  - row pieces of M_900 against slices of the whole, for render and extension, and an empty piece;
  - claim 3 on the device: the views inside WIDE PT's domain against fr_escape_rows_de_pt_state with the wide centre;
  - the orbit cache: the entries a raised cap computes, and the orbit shared with the other scaled calls;
  - the Python road, an algorithm without orbits, the kernels' names."""
import ctypes as C

import numpy as np
import pytest

import pt_scaled_model as S
import pt_scaled_state_model as T
import de_scaled_state_model as U

pytestmark = pytest.mark.gpu

GUARD = 64
NAN_BITS = 0x7FF8DEADBEEF0001


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


class State:
    """(z, iters, w, m, der) of `npx` pixels in device memory, guard bytes on both sides of each array"""

    SIZES = (16, 4, 16, 4, 16)
    TYPES = U.TYPES

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
            if b:
                buf[GUARD:GUARD + b] = t.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(buf.device)
        t.cuda.synchronize()
        return self

    def read(self, shape):
        """-> (z, iters, w, m, der) as the model shapes them; the guards are checked"""
        self.torch.cuda.synchronize()
        out = []
        for buf, b, ty in zip(self.bufs, self.bytes, self.TYPES):
            h = buf.cpu().numpy()
            assert (h[:GUARD] == 0xA5).all() and (h[GUARD + b:] == 0xA5).all(), "a write outside the array"
            a = h[GUARD:GUARD + b].copy().view(ty)
            out.append(a.reshape(tuple(shape) + ((2,) if ty is np.float64 else ())))
        return tuple(out)


def render(lib, native, c, cfg, st, y0=0, y1=None):
    y1 = cfg.height if y1 is None else y1
    centre = c.centre(native)
    check(lib.fr_escape_rows_de_pt_scaled_state_device(C.byref(cfg), C.byref(centre), y0, y1, *st.ptrs, None))


def extend(lib, native, c, cfg, st, n, y0=0, y1=None):
    y1 = cfg.height if y1 is None else y1
    centre = c.centre(native)
    check(lib.fr_escape_extend_de_pt_scaled_device(C.byref(cfg), C.byref(centre), y0, y1, n, *st.ptrs, None))


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


LABELS = ("z", "iters", "w", "m", "der")


def assert_state(got, want, what):
    """the integers equal, z and w as bits, der as bits but for a NaN, which is any NaN"""
    for k in (1, 3):
        assert np.array_equal(got[k], want[k]), "%s: %s differs at %d pixels" % (what, LABELS[k], int((got[k] != want[k]).sum()))
    for k in (0, 2):
        a, b = bits_of(got[k]), bits_of(want[k])
        assert np.array_equal(a, b), "%s: %s differs at %d doubles" % (what, LABELS[k], int((a != b).sum()))
    na, nb = np.isnan(got[4]), np.isnan(want[4])
    assert np.array_equal(na, nb), "%s: der has its NaNs elsewhere" % what
    a, b = bits_of(got[4])[~na], bits_of(want[4])[~nb]
    assert np.array_equal(a, b), "%s: der differs at %d doubles" % (what, int((a != b).sum()))


def kernel_name(lib):
    buf = C.create_string_buffer(128)
    check(lib.fr_last_kernel_name(buf, len(buf)))
    return buf.value.decode()


CHAINS = list(U.CHAINS)

# ---- the state render ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", CHAINS)
def test_state_render_is_the_model_at_every_cap(fr, native, lib, torch, name):
    c = T.chain(fr.Config.new, name)
    h, w = c.shape
    centre = c.centre(native)
    for cap in c.caps:  # cap 0 in every chain, cap 1 in M_900, N_900 and J2_900
        cfg, want = c.cfg(cap), U.state(c, cap)
        st = State(torch, h * w)
        render(lib, native, c, cfg, st)
        got = st.read(c.shape)
        assert_state(got, want, "%s at cap %d, device arrays" % (name, cap))
        host = tuple(np.full((h, w, 2), np.nan) if ty is np.float64 else np.full((h, w), 0xFFFFFFFF, dtype=np.uint32) for ty in U.TYPES)
        check(lib.fr_escape_rows_de_pt_scaled_state(C.byref(cfg), C.byref(centre), 0, h, *(a.ctypes.data for a in host)))
        assert_state(host, want, "%s at cap %d, host arrays" % (name, cap))
        # claim 1 from the library's own calls
        z, der = np.full((h, w, 2), np.nan), np.full((h, w, 2), np.nan)
        it = np.full((h, w), 0xFFFFFFFF, dtype=np.uint32)
        check(lib.fr_escape_rows_de_pt_scaled(C.byref(cfg), C.byref(centre), -1, 0, h, z.ctypes.data, it.ctypes.data, der.ctypes.data))
        four = (np.full((h, w, 2), np.nan), np.full((h, w), 0xFFFFFFFF, dtype=np.uint32), np.full((h, w, 2), np.nan),
                np.full((h, w), 0xFFFFFFFF, dtype=np.uint32))
        check(lib.fr_escape_rows_pt_scaled_state(C.byref(cfg), C.byref(centre), 0, h, *(a.ctypes.data for a in four)))
        assert_state(got, (z, it, four[2], four[3], der), "%s at cap %d, against the library's own calls" % (name, cap))
        assert np.array_equal(bits_of(four[0]), bits_of(z)) and np.array_equal(four[1], it)


# ---- the chains ---------------------------------------------------------------------------------------------------------------


def poison(state, n, m):
    """finished pixels' z, w, m, der made unreadable and a few of their iters moved above N -> (the planted arrays, the mask)"""
    z, it, w, mm, der = (np.array(a) for a in state)
    done = it != n
    z.view(np.uint64)[done] = NAN_BITS  # never loaded: a NaN that reached the arithmetic would come back changed
    w.view(np.uint64)[done] = NAN_BITS + 1
    der.view(np.uint64)[done] = NAN_BITS + 2
    mm[done] = 0x7FFFFFFF
    ys, xs = np.nonzero(done)
    if len(ys):
        it[ys[0], xs[0]] = n + 1  # foreign indices above N
        it[ys[-1], xs[-1]] = 0xFFFFFFF0
        it[ys[len(ys) // 2], xs[len(ys) // 2]] = m
    return (z, it, w, mm, der), done


@pytest.mark.parametrize("name", CHAINS)
def test_cap_chain_is_the_model_after_every_link(fr, native, lib, torch, name):
    c = T.chain(fr.Config.new, name)
    st = State(torch, c.shape[0] * c.shape[1])
    render(lib, native, c, c.cfg(c.caps[0]), st)
    assert_state(st.read(c.shape), U.state(c, c.caps[0]), "cap %d" % c.caps[0])
    nothing_running = 0
    for n, m in c.links():
        planted, done = poison(U.state(c, n), n, m)  # what the device holds, bit for bit, but for the finished pixels
        st.upload(planted)
        extend(lib, native, c, c.cfg(m), st, n)
        got, want = st.read(c.shape), U.state(c, m)
        for k in range(5):
            a, p = bits_of(got[k]), bits_of(planted[k])
            assert np.array_equal(a[done], p[done]), "%s %d -> %d, %s: a finished pixel was written" % (name, n, m, LABELS[k])
        run = ~done
        assert_state(tuple(a[run] for a in got), tuple(a[run] for a in want), "%s %d -> %d, the running pixels" % (name, n, m))
        if not run.any():  # the nothing-running link: every byte as it was, foreign values in all five arrays included
            assert all(np.array_equal(bits_of(got[k]), bits_of(planted[k])) for k in range(5))
            nothing_running += 1
    if name == "M_900":
        assert nothing_running == 1 and not (U.state(c, 600)[1] == 600).any()  # that link is in this chain


@pytest.mark.parametrize("name", CHAINS)
def test_the_chain_unpoisoned_and_one_jump(fr, native, lib, torch, name):
    c = T.chain(fr.Config.new, name)
    st = State(torch, c.shape[0] * c.shape[1])
    render(lib, native, c, c.cfg(c.caps[0]), st)
    for n, m in c.links():  # the device's own arrays carried from link to link
        extend(lib, native, c, c.cfg(m), st, n)
    assert_state(st.read(c.shape), U.state(c, c.caps[-1]), "%s link by link" % name)
    first, last = c.caps[0], c.caps[-1]
    st = State(torch, c.shape[0] * c.shape[1]).upload(U.state(c, first))
    extend(lib, native, c, c.cfg(last), st, first)
    assert_state(st.read(c.shape), U.state(c, last), "%s %d -> %d in one jump" % (name, first, last))
    # the host form of the extension, on the link that mixes finished and running pixels (N_900: all running)
    n, m = c.links()[-2]
    host = tuple(np.array(a) for a in U.state(c, n))
    centre = c.centre(native)
    check(lib.fr_escape_extend_de_pt_scaled(C.byref(c.cfg(m)), C.byref(centre), 0, c.shape[0], n, *(a.ctypes.data for a in host)))
    assert_state(host, U.state(c, m), "%s %d -> %d, host arrays" % (name, n, m))


def test_row_pieces_and_an_empty_one(fr, native, lib, torch):
    c = T.chain(fr.Config.new, "M_900")  # ragged edges, more than one workgroup on both axes
    w = c.shape[1]
    for y0, y1 in ((5, 12), (0, 5), (5, 21)):
        st = State(torch, w * (y1 - y0))
        render(lib, native, c, c.cfg(300), st, y0, y1)
        assert_state(st.read((y1 - y0, w)), tuple(a[y0:y1] for a in U.state(c, 300)), "rows [%d, %d) at 300" % (y0, y1))
        for n, m in ((300, 560), (560, 600)):
            extend(lib, native, c, c.cfg(m), st, n, y0, y1)
            assert_state(st.read((y1 - y0, w)), tuple(a[y0:y1] for a in U.state(c, m)), "rows [%d, %d), %d -> %d" % (y0, y1, n, m))
    st = State(torch, 0)  # no rows: nothing is written, not even beside the arrays
    render(lib, native, c, c.cfg(300), st, 7, 7)
    extend(lib, native, c, c.cfg(560), st, 300, 7, 7)
    st.read((0, w))


# ---- claim 3 ---------------------------------------------------------------------------------------------------------------------

INSIDE = {"M-2^200": S.M_200, "M-2^440-37x21": S.M_440, "N": S.N_300, "J": S.J_300}


@pytest.mark.parametrize("name", list(INSIDE))
def test_inside_wide_pts_domain_the_state_is_the_wide_de_state(fr, native, lib, torch, name):
    v = S.view(fr.Config.new, INSIDE[name])
    h, w = v.shape
    e = S.exponent(v.cfg)
    centre = v.centre(native)
    st, wide = State(torch, h * w), State(torch, h * w)
    check(lib.fr_escape_rows_de_pt_scaled_state_device(C.byref(v.cfg), C.byref(centre), 0, h, *st.ptrs, None))
    check(lib.fr_escape_rows_de_pt_state_device(C.byref(v.cfg), None, C.byref(centre), 0, h, *wide.ptrs, None))
    got, ref = st.read(v.shape), wide.read(v.shape)
    assert np.isfinite(ref[4]).all()
    # w = dz 2^e and der 2^e is its der, both exactly
    assert_state((got[0], got[1], got[2], got[3], np.ldexp(got[4], e)), (ref[0], ref[1], np.ldexp(ref[2], e), ref[3], ref[4]), name)
    assert (ref[1] == v.cfg.iterations).any() or len(np.unique(ref[1])) > 1


# ---- the orbit cache ---------------------------------------------------------------------------------------------------------------


def forget_orbit(fr):
    """another view through the context: the cache then holds that one"""
    cfg = fr.Config.new()
    cfg.width = cfg.height = 8
    cfg.iterations = 3
    cfg.pos.re = 0.125
    fr.escape_rows(cfg, precision=fr.Precision.PT)


def test_raising_the_cap_computes_only_the_missing_entries(fr, native, lib, torch):
    c = T.chain(fr.Config.new, "N_900")
    forget_orbit(fr)
    st = State(torch, c.shape[0] * c.shape[1])
    render(lib, native, c, c.cfg(1), st)
    short, long_ = len(c.orbits(1).x[0]), len(c.orbits(1000).x[0])
    assert fr.pt_orbit_cache() == (1, short, 0, short)
    extend(lib, native, c, c.cfg(1000), st, 1)
    assert fr.pt_orbit_cache() == (1000, long_, 0, long_ - short)  # continued from the integer tail, not recomputed
    continued = st.read(c.shape)
    assert_state(continued, U.state(c, 1000), "after a continued orbit")
    # the orbit is the other scaled calls': a plain scaled render, a scaled DE render and a scaled state render are served by it
    centre = c.centre(native)
    h, w = c.shape
    z, der, it = np.zeros((h, w, 2)), np.zeros((h, w, 2)), np.zeros((h, w), dtype=np.uint32)
    check(lib.fr_escape_rows_pt_scaled(C.byref(c.cfg(1000)), C.byref(centre), -1, 0, h, z.ctypes.data, it.ctypes.data))
    assert fr.pt_orbit_cache() == (1000, long_, 0, 0)
    check(lib.fr_escape_rows_de_pt_scaled(C.byref(c.cfg(1000)), C.byref(centre), -1, 0, h, z.ctypes.data, it.ctypes.data, der.ctypes.data))
    assert fr.pt_orbit_cache() == (1000, long_, 0, 0)
    render(lib, native, c, c.cfg(1000), State(torch, h * w))
    assert fr.pt_orbit_cache() == (1000, long_, 0, 0)
    forget_orbit(fr)
    fresh = State(torch, h * w).upload(U.state(c, 1))
    extend(lib, native, c, c.cfg(1000), fresh, 1)
    assert fr.pt_orbit_cache() == (1000, long_, 0, long_)  # a fresh context's orbit: all of it
    assert_state(fresh.read(c.shape), continued, "a fresh orbit against a continued one")


# ---- the Python road, no orbits, the names -------------------------------------------------------------------------------------


def test_the_python_road(fr, native, lib, torch):
    c = T.chain(fr.Config.new, "MINI_861")
    centre = fr.WideCentre(c.n, re=c.words[0], im=c.words[1])
    state = fr.escape_rows_de_pt_scaled_state(c.cfg(1000), centre)
    assert_state(state, U.state(c, 1000), "escape_rows_de_pt_scaled_state")
    piece = fr.escape_rows_de_pt_scaled_state(c.cfg(1000), centre, y0=3, y1=9)
    assert_state(piece, tuple(a[3:9] for a in U.state(c, 1000)), "rows [3, 9)")
    before = tuple(a.copy() for a in state)
    assert_state(fr.extend_rows_de_pt_scaled(c.cfg(3204), *state, 1000, centre), U.state(c, 3204), "extend_rows_de_pt_scaled")
    assert_state(state, before, "the arguments are left alone")


def test_an_algorithm_without_orbits(fr, native, lib, torch):
    c = T.chain(fr.Config.new, "M_900")
    cfg = c.cfg(300)
    cfg.algo = int(fr.Algo.BarnsleyFern)
    st = State(torch, c.shape[0] * c.shape[1])
    render(lib, native, c, cfg, st)
    assert all(not a.any() for a in st.read(c.shape))  # zeros in all five arrays
    planted = tuple(np.array(a) for a in U.state(c, 300))
    st.upload(planted)
    cfg.iterations = 560
    extend(lib, native, c, cfg, st, 300)
    assert_state(st.read(c.shape), planted, "the extension does nothing")


def test_kernel_names(fr, native, lib, torch):
    c = T.chain(fr.Config.new, "J_900")
    centre = c.centre(native)
    h, w = c.shape
    check(lib.fr_set_profiling(1))
    try:
        st = State(torch, h * w)
        render(lib, native, c, c.cfg(400), st)
        assert kernel_name(lib) == "escape_pt_scaled_de_state_kernel"
        ms = C.c_float(-1.0)
        check(lib.fr_last_kernel_ms(C.byref(ms)))
        assert ms.value > 0.0
        extend(lib, native, c, c.cfg(631), st, 400)
        assert kernel_name(lib) == "escape_extend_pt_scaled_de_kernel"
        z = torch.zeros(2 * h * w, dtype=torch.float64, device="cuda:0")
        der = torch.zeros(2 * h * w, dtype=torch.float64, device="cuda:0")
        it = torch.zeros(h * w, dtype=torch.int32, device="cuda:0")
        check(lib.fr_escape_rows_de_pt_scaled_device(C.byref(c.cfg(400)), C.byref(centre), -1, 0, h, z.data_ptr(), it.data_ptr(),
                                                     der.data_ptr(), None))
        torch.cuda.synchronize()
        assert kernel_name(lib) == "escape_pt_scaled_de_kernel"  # the plain DE render keeps its kernel
    finally:
        check(lib.fr_set_profiling(0))
