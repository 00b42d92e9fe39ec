"""Resumable perturbation on the device (include/fractal_hip.h: fr_escape_rows_pt_state(_device), fr_escape_extend_pt(_device),
fr_debug_pt_orbit_cache; kernels escape_pt_state_kernel, escape_extend_pt_kernel), bit for bit against tests/pt_state_model.c:
  - the state render at every cap of the chain 0 .. 4000 on five views (67 x 45 for edge tiles), its (z, iters) against
    fr_escape_rows_pt as well;
  - the chain extended link by link, with and without pos_lo, row pieces, one jump, the seahorse view 4000 -> 20 000;
  - untouched means untouched: finished pixels' z, dz, m poisoned, foreign indices planted, guard bytes around every array,
    a launch with nothing running;
  - the host forms, the colour pass over the extended z against fr_render_rows_pt at the new cap;
  - the orbit cache: entries computed on the host when a cap is raised, and the results after a continued orbit against
    those after a fresh one;
  - fr_escape_extend_device still refuses PT; profiling names; BarnsleyFern; offsets past 4 GiB."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import pt_model as PM
import pt_state_model as SM

pytestmark = pytest.mark.gpu

PT = 3
GUARD = 64  # bytes, a multiple of 8: the arrays behind it keep their alignment
NAN_BITS = 0x7FF8DEADBEEF1234
NAMES = list(SM.VIEWS)


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


def lo_ptr(pos_lo):
    from fractal_renderer_amd import _native

    return C.byref(_native.Imaginary(*pos_lo)) if pos_lo is not None else None


@functools.lru_cache(maxsize=None)
def model(name, n, zero_lo=False):
    """(cfg, pos_lo, the model's state at cap n), computed once and never written to; zero_lo: the view with pos_lo = 0"""
    cfg, lo = SM.view(name, O.config_new, n)
    if zero_lo:
        lo = (0.0, 0.0)
    st = SM.state_rows(cfg, lo)
    for a in st:
        a.setflags(write=False)
    return cfg, lo, st


def fr_cfg(fr, cfg, iterations=None):
    out = fr.Config.from_buffer_copy(bytes(cfg))
    if iterations is not None:
        out.iterations = iterations
    return out


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
        """-> (z, iters, dz, m) as the model shapes them; the guards are checked"""
        self.torch.cuda.synchronize()
        out = []
        for buf, b, ty in zip(self.bufs, self.bytes, self.TYPES):
            h = buf.cpu().numpy()
            assert (h[:GUARD] == 0xA5).all() and (h[GUARD + b:] == 0xA5).all(), "a write outside the array"
            a = h[GUARD:GUARD + b].copy().view(ty)
            out.append(a.reshape(tuple(shape) + ((2,) if ty is np.float64 else ())))
        return tuple(out)


def render(lib, cfg, st, pos_lo=None, y0=0, y1=None, stream=None):
    y1 = cfg.height if y1 is None else y1
    check(lib.fr_escape_rows_pt_state_device(C.byref(cfg), lo_ptr(pos_lo), y0, y1, *st.ptrs, stream))


def extend(lib, cfg, st, n, pos_lo=None, y0=0, y1=None, stream=None):
    y1 = cfg.height if y1 is None else y1
    check(lib.fr_escape_extend_pt_device(C.byref(cfg), lo_ptr(pos_lo), y0, y1, n, *st.ptrs, stream))


def assert_state(got, want, what):
    assert np.array_equal(got[1], want[1]), "%s: escape indices differ at %d pixels" % (what, int((got[1] != want[1]).sum()))
    assert np.array_equal(got[3], want[3]), "%s: m differs at %d pixels" % (what, int((got[3] != want[3]).sum()))
    for k, label in ((0, "z"), (2, "dz")):
        a, b = np.ascontiguousarray(got[k]).view(np.uint64), np.ascontiguousarray(want[k]).view(np.uint64)
        assert np.array_equal(a, b), "%s: %s differs at %d doubles" % (what, label, int((a != b).sum()))


def cache(lib):
    out = (C.c_uint32 * 4)()
    check(lib.fr_debug_pt_orbit_cache(out))
    return tuple(out)


def forget_orbit(fr):
    """another view through the context: the cache then holds that one"""
    cfg = fr.Config.new()
    cfg.width = cfg.height = 8
    cfg.iterations = 3
    cfg.pos.re = 0.125
    fr.escape_rows(cfg, precision=fr.Precision.PT)


# ---- the state render --------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", NAMES)
def test_state_render_is_the_model_at_every_cap(fr, lib, torch, name):
    for n in SM.CHAIN:
        mcfg, lo, want = model(name, n)
        cfg = fr_cfg(fr, mcfg)
        st = State(torch, cfg.width * cfg.height)
        render(lib, cfg, st, lo)
        got = st.read((cfg.height, cfg.width))
        assert_state(got, want, "%s at cap %d" % (name, n))
        z, it = fr.escape_rows(cfg, precision=fr.Precision.PT, pos_lo=lo)  # fr_escape_rows_pt
        assert np.array_equal(it, got[1]) and np.array_equal(z.view(np.uint64), got[0].view(np.uint64)), (name, n)


# ---- the chain --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("with_lo", [True, False], ids=["pos_lo", "null_lo"])
@pytest.mark.parametrize("name", NAMES)
def test_cap_chain_is_the_model_after_every_link(fr, lib, torch, name, with_lo):
    """with_lo: the view's pos_lo through the pointer ((0, 0) for the views that have none); else NULL, which for the
    seahorse view is another view, centred on the f64 grid point"""
    zero = not with_lo
    mcfg, lo, want = model(name, SM.CHAIN[0], zero)
    arg = lo if with_lo else None
    cfg = fr_cfg(fr, mcfg)
    st = State(torch, cfg.width * cfg.height)
    render(lib, cfg, st, arg)
    assert_state(st.read((cfg.height, cfg.width)), want, "cap 0")
    for n, m in zip(SM.CHAIN, SM.CHAIN[1:]):
        want = model(name, m, zero)[2]
        cfg.iterations = m
        extend(lib, cfg, st, n, arg)
        assert_state(st.read((cfg.height, cfg.width)), want, "%s %d -> %d" % (name, n, m))


@pytest.mark.parametrize("name", NAMES)
def test_one_jump_equals_the_chain(fr, lib, torch, name):
    mcfg, lo, start = model(name, 5)
    cfg = fr_cfg(fr, mcfg, SM.CHAIN[-1])
    st = State(torch, cfg.width * cfg.height).upload(start)
    extend(lib, cfg, st, 5, lo)
    assert_state(st.read((cfg.height, cfg.width)), model(name, SM.CHAIN[-1])[2], "%s 5 -> 4000" % name)


def test_seahorse_4000_to_20000(fr, lib, torch):
    mcfg, lo, start = model("seahorse", 4000)
    cfg = fr_cfg(fr, mcfg)
    st = State(torch, 32 * 24)
    render(lib, cfg, st, lo)
    assert_state(st.read((24, 32)), start, "seahorse at 4000")
    cfg.iterations = 20000
    extend(lib, cfg, st, 4000, lo)
    want = model("seahorse", 20000)[2]
    assert (start[1] == 4000).all() and 0 < int((want[1] < 20000).sum()) < 768  # escapes within the link, and orbits that run on
    assert_state(st.read((24, 32)), want, "seahorse 4000 -> 20000")


@pytest.mark.parametrize("name", ["shallow_mandelbrot", "shallow_julia"])
def test_row_pieces(fr, lib, torch, name):
    y0, y1 = 13, 30
    mcfg, lo, at_n = model(name, 37)
    cfg = fr_cfg(fr, mcfg)
    st = State(torch, cfg.width * (y1 - y0))
    render(lib, cfg, st, lo, y0, y1)
    assert_state(st.read((y1 - y0, cfg.width)), tuple(a[y0:y1] for a in at_n), "rows [13, 30) at 37")
    cfg.iterations = 200
    extend(lib, cfg, st, 37, lo, y0, y1)
    assert_state(st.read((y1 - y0, cfg.width)), tuple(a[y0:y1] for a in model(name, 200)[2]), "rows [13, 30), 37 -> 200")


# ---- untouched means untouched ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["shallow_mandelbrot", "shallow_julia", "julia_rebase"])
def test_finished_pixels_are_not_touched(fr, lib, torch, name):
    n, m = (37, 200) if name != "julia_rebase" else (200, 333)
    mcfg, lo, at_n = model(name, n)
    z, it, dz, mm = (np.array(a) for a in at_n)
    done = it != n
    assert done.any() and (~done).any()
    z.view(np.uint64)[done] = NAN_BITS  # never loaded: a NaN that reached the arithmetic would come back changed
    dz.view(np.uint64)[done] = NAN_BITS + 1
    mm[done] = 0x7FFFFFFF
    ys, xs = np.nonzero(done)
    it[ys[0], xs[0]] = n + 1  # foreign indices above N
    it[ys[-1], xs[-1]] = 0xFFFFFFF0
    it[ys[len(ys) // 2], xs[len(ys) // 2]] = m
    planted = (z.copy(), it.copy(), dz.copy(), mm.copy())
    cfg = fr_cfg(fr, mcfg, m)
    st = State(torch, it.size).upload((z, it, dz, mm))
    extend(lib, cfg, st, n, lo)
    got = st.read(it.shape)
    want = model(name, m)[2]
    for k in range(4):
        a, b, p = (np.ascontiguousarray(v) for v in (got[k], want[k], planted[k]))
        if a.dtype == np.float64:
            a, b, p = a.view(np.uint64), b.view(np.uint64), p.view(np.uint64)
        assert np.array_equal(a[done], p[done]), "array %d: a finished pixel was written" % k
        assert np.array_equal(a[~done], b[~done]), "array %d: a running pixel differs from the model" % k


def test_a_launch_with_nothing_running_writes_nothing(fr, lib, torch):
    mcfg, lo, at_n = model("shallow_mandelbrot", 37)
    z, it, dz, mm = (np.array(a) for a in at_n)
    it[it == 37] = 38  # nothing is at N
    z.view(np.uint64)[...] = NAN_BITS
    dz.view(np.uint64)[...] = NAN_BITS
    mm[...] = 0xFFFFFFFF
    cfg = fr_cfg(fr, mcfg, 200)
    st = State(torch, it.size).upload((z, it, dz, mm))
    extend(lib, cfg, st, 37, lo)
    got = st.read(it.shape)
    assert np.array_equal(got[1], it) and np.array_equal(got[3], mm)
    assert (got[0].view(np.uint64) == NAN_BITS).all() and (got[2].view(np.uint64) == NAN_BITS).all()


# ---- host forms, colours ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["seahorse", "julia_rebase", "shallow_mandelbrot"])
def test_host_forms_equal_the_model(fr, name):
    n, m = 200, 333
    mcfg, lo, at_n = model(name, n)
    got = fr.escape_rows_pt_state(fr_cfg(fr, mcfg), pos_lo=lo)
    assert_state(got, at_n, "host state render")
    ext = fr.extend_rows_pt(fr_cfg(fr, mcfg, m), *got, n, pos_lo=lo)
    assert_state(ext, model(name, m)[2], "host extension")
    assert_state(got, at_n, "the arguments are left alone")
    piece = fr.extend_rows_pt(fr_cfg(fr, mcfg, m), *(a[5:20] for a in got), n, pos_lo=lo, y0=5, y1=20)
    assert_state(piece, tuple(a[5:20] for a in model(name, m)[2]), "host extension of rows [5, 20)")


@pytest.mark.parametrize("name,n,m", [("seahorse", 4000, 20000), ("shallow_mandelbrot", 37, 333), ("shallow_julia", 37, 333)])
def test_colour_pass_over_the_extended_state_is_the_pt_render(fr, lib, torch, name, n, m):
    """(the seahorse view's first escape is at step 8 940: under that cap its image is one colour)"""
    mcfg, lo, _ = model(name, n)
    cfg = fr_cfg(fr, mcfg)
    npx = cfg.width * cfg.height
    st = State(torch, npx)
    render(lib, cfg, st, lo)
    cfg.iterations = m
    extend(lib, cfg, st, n, lo)
    cfg.exposure = 3.0
    for channels in (3, 4):
        d_out = torch.zeros(channels * npx, dtype=torch.uint8, device="cuda")
        check(lib.fr_colour_rows_device(C.byref(cfg), st.ptrs[0], 2, st.ptrs[1], npx, channels, d_out.data_ptr(), channels * npx, None))
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().reshape(cfg.height, cfg.width, channels)
        if channels == 3:
            want = fr.get_image_rows(cfg, 0, cfg.height, fr.Precision.PT, pos_lo=lo)  # fr_render_rows_pt
            assert len(np.unique(want.reshape(-1, 3), axis=0)) > 2
        else:
            want = fr.get_image_rgba(cfg, fr.Precision.PT, pos_lo=lo)
        assert np.array_equal(got, want), channels


# ---- the orbit cache --------------------------------------------------------------------------------------------------------


def test_cache_continues_a_cut_orbit_by_the_missing_entries(fr, lib, torch):
    forget_orbit(fr)
    mcfg, lo, at_n = model("seahorse", 1500)
    cfg = fr_cfg(fr, mcfg)
    st = State(torch, 32 * 24)
    render(lib, cfg, st, lo)
    assert cache(lib) == (1500, 1502, 0, 1502)  # R_0 .. R_1501, all computed
    render(lib, cfg, st, lo)
    assert cache(lib) == (1500, 1502, 0, 0)  # served as it was
    cfg.iterations = 4000
    extend(lib, cfg, st, 1500, lo)
    assert cache(lib) == (4000, 4002, 0, 2500)  # the new entries, not M + 2
    assert_state(st.read((24, 32)), model("seahorse", 4000)[2], "after the continued orbit")
    z, it = fr.escape_rows(cfg, precision=fr.Precision.PT, pos_lo=lo)  # escape_pt_kernel on the continued orbit
    wz, wit = PM.escape_rows(mcfg.__class__.from_buffer_copy(bytes(cfg)), lo)
    assert cache(lib)[3] == 0 and np.array_equal(it, wit) and np.array_equal(z.view(np.uint64), wz.view(np.uint64))
    cfg.iterations = 37  # a lower cap recomputes
    render(lib, cfg, st, lo)
    assert cache(lib) == (37, 39, 0, 39)
    cfg.iterations = 38  # pos_lo is part of the view: without it this is another one
    render(lib, cfg, st, None)
    assert cache(lib) == (38, 40, 0, 40)


def test_cache_serves_orbits_ended_by_escape_as_they_are(fr, lib, torch):
    forget_orbit(fr)
    mcfg, lo, _ = model("early_escape", 38)
    cfg = fr_cfg(fr, mcfg)
    st = State(torch, 48 * 32)
    render(lib, cfg, st, lo)
    assert cache(lib) == (38, 31, 0, 31)  # R ends by escape at entry 30
    for n, m in ((38, 200), (200, 4000)):
        cfg.iterations = m
        extend(lib, cfg, st, n, lo)
        assert cache(lib) == (m, 31, 0, 0)
        assert_state(st.read((32, 48)), model("early_escape", m)[2], "early_escape %d -> %d" % (n, m))


def test_cache_continues_each_julia_orbit_on_its_own(fr, lib, torch):
    forget_orbit(fr)
    mcfg, lo, _ = model("julia_rebase", 200)
    cfg = fr_cfg(fr, mcfg)
    st = State(torch, 48 * 32)
    render(lib, cfg, st, lo)
    assert cache(lib) == (200, 201, 201, 402)  # V and K both cut at entry 200
    cfg.iterations = 333
    extend(lib, cfg, st, 200, lo)
    assert cache(lib) == (333, 202, 253, 1 + 52)  # V ends by escape at 201, K at 252
    assert_state(st.read((32, 48)), model("julia_rebase", 333)[2], "julia_rebase 200 -> 333")
    cfg.iterations = 1500
    extend(lib, cfg, st, 333, lo)
    assert cache(lib) == (1500, 202, 253, 0)
    assert_state(st.read((32, 48)), model("julia_rebase", 1500)[2], "julia_rebase 333 -> 1500")


@pytest.mark.parametrize("name", ["seahorse", "julia_rebase", "shallow_julia"])
def test_continued_and_fresh_orbits_give_the_same_results(fr, lib, torch, name):
    n, m = 38, 333
    mcfg, lo, _ = model(name, n)
    cfg = fr_cfg(fr, mcfg, m)
    shape = (cfg.height, cfg.width)
    forget_orbit(fr)
    first = State(torch, cfg.width * cfg.height)
    render(lib, cfg, first, lo)  # the render at M first: a fresh orbit
    assert cache(lib)[3] == cache(lib)[1] + cache(lib)[2]
    fresh = first.read(shape)
    forget_orbit(fr)
    cfg.iterations = n
    st = State(torch, cfg.width * cfg.height)
    render(lib, cfg, st, lo)
    cfg.iterations = m
    extend(lib, cfg, st, n, lo)
    assert 0 < cache(lib)[3] < cache(lib)[1] + cache(lib)[2]
    assert_state(st.read(shape), fresh, "continued against fresh")
    again = State(torch, cfg.width * cfg.height)
    render(lib, cfg, again, lo)  # the state render on the continued orbit
    assert cache(lib)[3] == 0
    assert_state(again.read(shape), fresh, "state render on the continued orbit")


# ---- the rest of the contract ---------------------------------------------------------------------------------------------------


def test_the_f64_extension_still_refuses_pt(fr, lib, torch):
    from fractal_renderer_amd import _native

    mcfg, lo, at_n = model("shallow_mandelbrot", 37)
    cfg = fr_cfg(fr, mcfg, 200)
    st = State(torch, cfg.width * cfg.height).upload(at_n)
    rc = lib.fr_escape_extend_device(C.byref(cfg), PT, None, 0, cfg.height, 37, 2, st.ptrs[0], st.ptrs[1], None, None)
    assert rc == _native.FR_ERR_INVALID_ARGUMENT and b"FR_PRECISION_PT" in lib.fr_last_error()
    assert_state(st.read((cfg.height, cfg.width)), at_n, "refused: nothing written")


def test_profiling_reports_the_new_kernels(fr, lib, torch):
    def last():
        buf, ms = C.create_string_buffer(256), C.c_float(-1.0)
        check(lib.fr_last_kernel_name(buf, len(buf)))
        check(lib.fr_last_kernel_ms(C.byref(ms)))
        return buf.value.decode(), ms.value

    check(lib.fr_set_profiling(1))
    try:
        for name in ("shallow_mandelbrot", "shallow_julia"):
            mcfg, lo, _ = model(name, 37)
            cfg = fr_cfg(fr, mcfg)
            st = State(torch, cfg.width * cfg.height)
            render(lib, cfg, st, lo)
            kname, ms = last()
            assert kname == "escape_pt_state_kernel" and ms > 0.0
            cfg.iterations = 200
            extend(lib, cfg, st, 37, lo)
            kname, ms = last()
            assert kname == "escape_extend_pt_kernel" and ms > 0.0
            assert_state(st.read((cfg.height, cfg.width)), model(name, 200)[2], "profiled")
    finally:
        check(lib.fr_set_profiling(0))


def test_fern_has_no_state(fr, lib, torch):
    cfg = fr.Config.new(fr.Algo.BarnsleyFern)
    cfg.width, cfg.height, cfg.iterations = 67, 45, 5
    st = State(torch, 67 * 45)
    render(lib, cfg, st)
    got = st.read((45, 67))
    assert all(not np.ascontiguousarray(a).view(np.uint8).any() for a in got)
    planted = (np.full((45, 67, 2), 1.5), np.full((45, 67), 5, dtype=np.uint32), np.full((45, 67, 2), 2.5),
               np.full((45, 67), 7, dtype=np.uint32))
    st.upload(planted)
    cfg.iterations = 50
    extend(lib, cfg, st, 5)
    assert_state(st.read((45, 67)), planted, "fern: the extension does nothing")


def test_offsets_past_4_gib(fr, lib, torch):
    """width 40 000, rows [0, 6 720): 268.8 M pixels, 4.3 GB each of z and dz — byte offsets past 2^32 in both kernels"""
    w, rows = 40000, 6720
    npx = w * rows
    assert npx * 16 > 2 ** 32
    dev = torch.device("cuda", 0)
    try:
        dz = torch.empty(npx * 2, dtype=torch.float64, device=dev)
        dd = torch.empty(npx * 2, dtype=torch.float64, device=dev)
        di = torch.empty(npx, dtype=torch.int32, device=dev)
        dm = torch.empty(npx, dtype=torch.int32, device=dev)
    except (RuntimeError, MemoryError) as e:  # torch.cuda.OutOfMemoryError is a RuntimeError
        pytest.skip("cannot allocate 10.8 GB of device memory: %s" % str(e)[:80])
    mcfg = O.config_new()
    SM.shallow_mandelbrot_view(mcfg, w, rows, 2)
    mcfg.limit, mcfg.pos.im = 2.0, -1.25  # the last rows cross the set along the real axis, the first lie outside |c| = 2
    cfg = fr_cfg(fr, mcfg)
    ptrs = (dz.data_ptr(), di.data_ptr(), dd.data_ptr(), dm.data_ptr())
    check(lib.fr_escape_rows_pt_state_device(C.byref(cfg), None, 0, rows, *ptrs, None))
    cfg.iterations = mcfg.iterations = 4
    check(lib.fr_escape_extend_pt_device(C.byref(cfg), None, 0, rows, 2, *ptrs, None))
    torch.cuda.synchronize()
    for y0, y1 in ((0, 8), (rows - 8, rows)):
        want = SM.state_rows(mcfg, (0.0, 0.0), y0, y1)
        if y0:
            assert {2, 3, 4} <= set(np.unique(want[1]).tolist())  # escapes at both caps and within the link, orbits still running
        got = (dz[2 * w * y0:2 * w * y1].cpu().numpy().reshape(y1 - y0, w, 2), di[w * y0:w * y1].cpu().numpy().view(np.uint32).reshape(y1 - y0, w),
               dd[2 * w * y0:2 * w * y1].cpu().numpy().reshape(y1 - y0, w, 2), dm[w * y0:w * y1].cpu().numpy().view(np.uint32).reshape(y1 - y0, w))
        assert_state(got, want, "rows [%d, %d) of 6720 x 40000" % (y0, y1))
    del dz, dd, di, dm
    torch.cuda.empty_cache()
