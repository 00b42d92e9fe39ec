"""A view kept on the device (include/fractal_hip.h: fr_escape_rows_device, fr_escape_extend_device, fr_escape_extend,
fr_colour_rows_device; kernels escape_extend_kernel<T>, escape_extend_dd_kernel, colour_rows_kernel), bit for bit:
  - the cap chain 0 -> 1 -> 5 -> 37 -> 38 -> 200 -> 333 on a 67 x 45 Mandelbrot and Julia view in F64 and F32, z (as bits)
    and iters against the oracle after every link, with the link's pixel classes asserted from the oracle first;
  - escapes on the very first step (limit 2), the speculative blocks on and off, one jump against the chain, row ranges,
    tiny images, more than 4 GiB of z;
  - untouched means untouched: finished pixels' z poisoned, foreign indices planted, guard bytes around every array;
  - DD (four doubles of state) against tests/dd_model.c, PT through the raw road and refused by the extension;
  - the host forms, two threads at once, profiling;
  - the colour pass over the extended arrays against the renders at the new cap and against the oracle's image."""
import ctypes as C
import threading

import numpy as np
import pytest

import dd_model as DM
import extend_cases as X
import oracle_lib as O

pytestmark = pytest.mark.gpu

F64, F32, DD, PT = X.F64, X.F32, X.DD, X.PT
GUARD = 64  # bytes, a multiple of 8: the arrays behind it keep their alignment
LO = (0.0, 2.0 ** -60)  # a normalised low part of the deep views' centre (0, 1)
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


def fr_cfg(fr, ocfg):
    """an oracle Config as the package's (same 104 bytes)"""
    return fr.Config.from_buffer_copy(bytes(ocfg))


def lo_ptr(pos_lo):
    from fractal_renderer_amd import _native

    return C.byref(_native.Imaginary(*pos_lo)) if pos_lo is not None else None


class Stored:
    """(z, iters) of `npx` pixels in device memory, guard bytes on both sides of each array"""

    def __init__(self, torch, npx, zw=2):
        dev = torch.device("cuda", 0)
        self.torch, self.npx, self.zw = torch, npx, zw
        self.zb, self.ib = npx * zw * 8, npx * 4
        self.dz = torch.full((GUARD + self.zb + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.di = torch.full((GUARD + self.ib + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        assert self.dz.data_ptr() % 16 == 0 and self.di.data_ptr() % 16 == 0
        self.z_ptr, self.it_ptr = self.dz.data_ptr() + GUARD, self.di.data_ptr() + GUARD

    def upload(self, z, it):
        t = self.torch
        assert z.size == self.npx * self.zw and it.size == self.npx
        self.dz[GUARD:GUARD + self.zb] = t.from_numpy(np.ascontiguousarray(z).reshape(-1).view(np.uint8).copy()).to(self.dz.device)
        self.di[GUARD:GUARD + self.ib] = t.from_numpy(np.ascontiguousarray(it, dtype=np.uint32).reshape(-1).view(np.uint8).copy()).to(self.di.device)
        t.cuda.synchronize()
        return self

    def read(self, shape):
        """-> (z float64 shape + (zw,), iters uint32 shape); the guards are checked"""
        self.torch.cuda.synchronize()
        hz, hi = self.dz.cpu().numpy(), self.di.cpu().numpy()
        for h, n in ((hz, self.zb), (hi, self.ib)):
            assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all(), "a write outside the array"
        z = hz[GUARD:GUARD + self.zb].copy().view(np.float64).reshape(tuple(shape) + (self.zw,))
        it = hi[GUARD:GUARD + self.ib].copy().view(np.uint32).reshape(shape)
        return z, it


def render_raw(lib, cfg, precision, st, y0=0, y1=None, pos_lo=None, opts=None, stream=None):
    y1 = cfg.height if y1 is None else y1
    check(lib.fr_escape_rows_device(C.byref(cfg), precision, lo_ptr(pos_lo), y0, y1, st.zw, st.z_ptr, st.it_ptr, stream,
                                    C.byref(opts) if opts is not None else None))


def extend(lib, cfg, precision, st, n, y0=0, y1=None, pos_lo=None, opts=None, stream=None):
    y1 = cfg.height if y1 is None else y1
    check(lib.fr_escape_extend_device(C.byref(cfg), precision, lo_ptr(pos_lo), y0, y1, n, st.zw, st.z_ptr, st.it_ptr, stream,
                                      C.byref(opts) if opts is not None else None))


def assert_is_reference(got, want, what):
    (z, it), (wz, wit) = got, want
    assert np.array_equal(it, wit), "%s: escape indices differ at %d pixels" % (what, int((it != wit).sum()))
    assert X.same_f64(z, wz), "%s: positions differ" % (what,)


def from_reference(torch, name, precision, n, rows=None):
    """a Stored holding the oracle's results at cap n (rows = (y0, y1) of them)"""
    z, it = X.reference(name, precision, n)
    if rows is not None:
        z, it = z[rows[0]:rows[1]], it[rows[0]:rows[1]]
    return Stored(torch, it.size).upload(z, it)


VIEWS = [("mandelbrot", F64), ("mandelbrot", F32), ("julia", F64), ("julia", F32)]
VIEW_IDS = ["%s_%s" % (n, "f32" if p else "f64") for n, p in VIEWS]


# ---- the chain --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,precision", VIEWS, ids=VIEW_IDS)
def test_cap_chain_is_the_oracle_after_every_link(fr, lib, torch, name, precision):
    st = Stored(torch, X.W * X.H)
    cfg = fr_cfg(fr, X.view_cfg(name, X.CHAIN[0]))
    render_raw(lib, cfg, precision, st)
    got = st.read((X.H, X.W))
    assert (got[1] == 0).all()  # cap 0: (start, 0) for every pixel
    assert_is_reference(got, X.reference(name, precision, 0), "cap 0")
    table = X.table(precision)
    for n, m in zip(X.CHAIN, X.CHAIN[1:]):
        cls = X.classes(X.reference(name, precision, n)[1], X.reference(name, precision, m)[1], n, m)
        assert cls[0] + cls[1] + cls[2] == X.W * X.H and cls[1] + cls[2] > 0, "nothing is running in this link"
        if (name, n, m) in table:
            assert cls == table[(name, n, m)], (n, m, cls)
        cfg.iterations = m
        extend(lib, cfg, precision, st, n)
        assert_is_reference(st.read((X.H, X.W)), X.reference(name, precision, m), "%d -> %d" % (n, m))


@pytest.mark.parametrize("precision", [F64, F32], ids=["f64", "f32"])
def test_escapes_on_the_very_first_step(fr, lib, torch, precision):
    """0 -> 1 has no escapes at the CLI's limit of 65 536; with limit = 2, 1 019 pixels of the Mandelbrot view escape at step 0"""
    want = X.reference("mandelbrot", precision, 1, limit=2.0)
    assert int((want[1] == 0).sum()) == 1019 and int((want[1] == 1).sum()) == X.W * X.H - 1019
    st = Stored(torch, X.W * X.H)
    cfg = fr_cfg(fr, X.view_cfg("mandelbrot", 0, limit=2.0))
    render_raw(lib, cfg, precision, st)
    cfg.iterations = 1
    extend(lib, cfg, precision, st, 0)
    assert_is_reference(st.read((X.H, X.W)), want, "limit 2, 0 -> 1")


@pytest.mark.parametrize("loop_mode", [-1, 5, 0])
@pytest.mark.parametrize("precision", [F64, F32], ids=["f64", "f32"])
def test_speculative_blocks_on_and_off_give_the_same_bytes(fr, lib, torch, precision, loop_mode):
    """the links of 162 and 133 iterations over the ~500 still-running Mandelbrot pixels run the speculative blocks (a wave
    speculates after 16 quiet iterations): the same arrays with them (default; loop_mode 0 = the unscaled loop, which has
    them too) and without (5)"""
    from fractal_renderer_amd import _native

    cfg = fr_cfg(fr, X.view_cfg("mandelbrot", 200))
    lm, skip, quiet = C.c_uint32(), C.c_double(), C.c_uint32()
    check(lib.fr_debug_loop_plan(C.byref(cfg), precision, C.byref(lm), C.byref(skip), C.byref(quiet)))
    assert 0 < quiet.value < 133, "the plan must allow speculative blocks on this view"
    opts = fr.RenderOpts(loop_mode=loop_mode)
    assert isinstance(opts, _native.fr_render_opts)
    for n, m in ((38, 200), (200, 333)):
        cls = X.classes(X.reference("mandelbrot", precision, n)[1], X.reference("mandelbrot", precision, m)[1], n, m)
        assert cls[2] >= 496 and cls[1] > 0
        st = from_reference(torch, "mandelbrot", precision, n)
        cfg.iterations = m
        extend(lib, cfg, precision, st, n, opts=opts)
        assert_is_reference(st.read((X.H, X.W)), X.reference("mandelbrot", precision, m), "%d -> %d, loop_mode %d" % (n, m, loop_mode))


@pytest.mark.parametrize("name,precision", VIEWS, ids=VIEW_IDS)
def test_one_jump_equals_the_chain(fr, lib, torch, name, precision):
    chain = from_reference(torch, name, precision, 5)
    cfg = fr_cfg(fr, X.view_cfg(name, 5))
    for n, m in ((5, 37), (37, 38), (38, 200), (200, 333)):
        cfg.iterations = m
        extend(lib, cfg, precision, chain, n)
    jump = from_reference(torch, name, precision, 5)
    extend(lib, cfg, precision, jump, 5)
    a, b = chain.read((X.H, X.W)), jump.read((X.H, X.W))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    assert_is_reference(b, X.reference(name, precision, 333), "5 -> 333")


# ---- untouched means untouched ------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,precision", VIEWS, ids=VIEW_IDS)
def test_finished_pixels_and_foreign_indices_are_left_alone(fr, lib, torch, name, precision):
    n, m = 37, 200
    z, it = (a.copy() for a in X.reference(name, precision, n))
    wz, wit = (a.copy() for a in X.reference(name, precision, m))
    finished, running = it != n, it == n
    assert finished.sum() > 1000 and running.sum() > 100
    zb = z.view(np.uint64)
    zb[finished] = NAN_BITS  # a finished pixel's z is never loaded, never stored
    # foreign indices, planted on finished and on running pixels alike: nothing of them may change
    fy, fx = np.nonzero(finished)
    ry, rx = np.nonzero(running)
    planted = [(fy[3], fx[3], 0xFFFFFFFF), (fy[-5], fx[-5], n + 1), (ry[2], rx[2], 0xFFFFFFFF), (ry[-7], rx[-7], n + 1),
               (ry[len(ry) // 2], rx[len(rx) // 2], n + 1)]
    foreign = np.zeros_like(finished)
    for y, x, v in planted:
        it[y, x] = v
        foreign[y, x] = True
    st = Stored(torch, X.W * X.H).upload(z, it)
    cfg = fr_cfg(fr, X.view_cfg(name, m))
    extend(lib, cfg, precision, st, n)
    gz, git = st.read((X.H, X.W))
    keep = finished | foreign
    assert np.array_equal(git[keep], it[keep]), "an index of a finished pixel changed"
    assert np.array_equal(gz.view(np.uint64)[keep], z.view(np.uint64)[keep]), "a finished pixel's z was written"
    go = ~keep
    assert go.sum() >= running.sum() - 3
    assert np.array_equal(git[go], wit[go]) and X.same_f64(gz[go], wz[go]), "the running pixels differ from the oracle"


# ---- row ranges and tiny images -------------------------------------------------------------------------------------


@pytest.mark.parametrize("rows", [(13, 30), (0, 1), (44, 45)], ids=lambda r: "rows_%d_%d" % r)
@pytest.mark.parametrize("name,precision", VIEWS, ids=VIEW_IDS)
def test_row_ranges(fr, lib, torch, name, precision, rows):
    y0, y1 = rows
    m = 200
    cfg = fr_cfg(fr, X.view_cfg(name, m))
    wz, wit = X.reference(name, precision, m)
    for n in (1, 5):  # at cap 1 every orbit of both views is still running; at cap 5 the corners have finished
        assert n != 1 or (X.reference(name, precision, n)[1][y0:y1] == n).all()
        st = from_reference(torch, name, precision, n, rows)
        extend(lib, cfg, precision, st, n, y0, y1)
        assert_is_reference(st.read((y1 - y0, X.W)), (wz[y0:y1], wit[y0:y1]), "rows [%d, %d), %d -> %d" % (y0, y1, n, m))
    # the raw road itself over the same rows
    st2 = Stored(torch, (y1 - y0) * X.W)
    render_raw(lib, cfg, precision, st2, y0, y1)
    assert_is_reference(st2.read((y1 - y0, X.W)), (wz[y0:y1], wit[y0:y1]), "raw rows [%d, %d)" % rows)


@pytest.mark.parametrize("size", [(9, 3), (1, 1)], ids=["9x3", "1x1"])
@pytest.mark.parametrize("name,precision", VIEWS, ids=VIEW_IDS)
def test_tiny_images(fr, lib, torch, name, precision, size):
    w, h = size
    st = Stored(torch, w * h)
    cfg = fr_cfg(fr, X.view_cfg(name, 0, w, h))
    render_raw(lib, cfg, precision, st)
    ran = 0
    for n, m in ((0, 5), (5, 37), (37, 333)):
        ran += int((X.reference(name, precision, n, w, h)[1] == n).sum())
        cfg.iterations = m
        extend(lib, cfg, precision, st, n)
        assert_is_reference(st.read((h, w)), X.reference(name, precision, m, w, h), "%dx%d, %d -> %d" % (w, h, n, m))
    assert ran > 0


# ---- DD -------------------------------------------------------------------------------------------------------------

DD_CHAIN = [0, 7, 300, 3000]
# (finished before, escapes within, still running after) of each link, from tests/dd_model.c: every orbit of these views is
# still running at cap 7 and all but the centre's (pos_lo = 0: the centre is c = i exactly) have escaped by 300
DD_CLASSES = {False: [(0, 0, 3072), (0, 3071, 1), (3071, 0, 1)], True: [(0, 0, 3072), (0, 3072, 0), (3072, 0, 0)]}


@pytest.mark.parametrize("with_lo", [False, True], ids=["lo_zero", "lo"])
@pytest.mark.parametrize("julia", [False, True], ids=["mandelbrot", "julia"])
def test_dd_chain_is_the_model_after_every_link(fr, lib, torch, julia, with_lo):
    pos_lo = LO if with_lo else (0.0, 0.0)
    cfg = DM.deep_view(fr.Config.new(), julia, 64, 48, 0)
    want = {}
    for cap in DD_CHAIN:
        cfg.iterations = cap
        want[cap] = DM.escape_rows(cfg, pos_lo)
    st = Stored(torch, 64 * 48, zw=4)
    cfg.iterations = 0
    render_raw(lib, cfg, DD, st, pos_lo=pos_lo if with_lo else None)
    assert_is_reference(st.read((48, 64)), want[0], "DD cap 0")
    for k, (n, m) in enumerate(zip(DD_CHAIN, DD_CHAIN[1:])):
        assert X.classes(want[n][1], want[m][1], n, m)[:3] == DD_CLASSES[with_lo][k], (n, m)
        cfg.iterations = m
        extend(lib, cfg, DD, st, n, pos_lo=pos_lo if with_lo else None)
        assert_is_reference(st.read((48, 64)), want[m], "DD %d -> %d" % (n, m))
    # one jump over the link in which everything escapes, and a row range of it
    st = Stored(torch, 64 * 48, zw=4).upload(*want[7])
    cfg.iterations = 3000
    extend(lib, cfg, DD, st, 7, pos_lo=pos_lo)
    assert_is_reference(st.read((48, 64)), want[3000], "DD 7 -> 3000")
    st = Stored(torch, 64 * 17, zw=4).upload(want[7][0][13:30], want[7][1][13:30])
    extend(lib, cfg, DD, st, 7, 13, 30, pos_lo=pos_lo)
    assert_is_reference(st.read((17, 64)), (want[3000][0][13:30], want[3000][1][13:30]), "DD rows [13, 30)")
    # z_width 2 through the raw road: the hi parts
    hi = Stored(torch, 64 * 48, zw=2)
    render_raw(lib, cfg, DD, hi, pos_lo=pos_lo)
    assert_is_reference(hi.read((48, 64)), (np.ascontiguousarray(want[3000][0][..., 0::2]), want[3000][1]), "DD hi parts")


@pytest.mark.parametrize("pos_lo,cap", [((0.0, 0.0), 55), (LO, 52)], ids=["lo_zero_cap55", "lo_cap52"])
@pytest.mark.parametrize("julia", [False, True], ids=["mandelbrot", "julia"])
def test_dd_finished_pixels_are_left_alone(fr, lib, torch, julia, pos_lo, cap):
    """the deep view's orbits escape between steps 51 and 82 (tests/dd_model.c): a cap inside that range splits the image into
    finished pixels and orbits that escape within the link — with pos_lo, on its very first step"""
    cfg = DM.deep_view(fr.Config.new(), julia, 64, 48, cap)
    z, it = DM.escape_rows(cfg, pos_lo)
    cfg.iterations = 3000
    wz, wit = DM.escape_rows(cfg, pos_lo)
    finished = it != cap
    assert 900 < finished.sum() < 64 * 48 - 900, "the cap must split this view"
    z = z.copy()
    z.view(np.uint64)[finished] = NAN_BITS
    st = Stored(torch, 64 * 48, zw=4).upload(z, it)
    extend(lib, cfg, DD, st, cap, pos_lo=pos_lo)
    gz, git = st.read((48, 64))
    assert np.array_equal(git, wit)
    assert np.array_equal(gz.view(np.uint64)[finished], z.view(np.uint64)[finished])
    assert X.same_f64(gz[~finished], wz[~finished])


# ---- PT ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("julia", [False, True], ids=["mandelbrot", "julia"])
def test_pt_goes_through_the_raw_road_and_is_refused_by_the_extension(fr, lib, torch, julia):
    from fractal_renderer_amd import _native

    cfg = DM.deep_view(fr.Config.new(), julia, 64, 48, 300)
    wz, wit = fr.escape_rows(cfg, precision=fr.Precision.PT, pos_lo=LO)
    assert len(np.unique(wit)) > 1 and wit.max() < 300
    st = Stored(torch, 64 * 48)
    render_raw(lib, cfg, PT, st, pos_lo=LO)
    assert_is_reference(st.read((48, 64)), (wz, wit), "PT raw")
    st2 = Stored(torch, 64 * 17)
    render_raw(lib, cfg, PT, st2, 13, 30, pos_lo=LO)
    assert_is_reference(st2.read((17, 64)), (wz[13:30], wit[13:30]), "PT raw rows")
    cfg.iterations = 600
    rc = lib.fr_escape_extend_device(C.byref(cfg), PT, lo_ptr(LO), 0, 48, 300, 2, st.z_ptr, st.it_ptr, None, None)
    assert rc == _native.FR_ERR_INVALID_ARGUMENT and b"FR_PRECISION_PT" in lib.fr_last_error()
    assert_is_reference(st.read((48, 64)), (wz, wit), "PT arrays after the refusal")


# ---- host forms -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,precision", VIEWS, ids=VIEW_IDS)
def test_host_forms_give_the_device_forms_bytes(fr, lib, name, precision):
    n, m = 5, 333
    z, it = (a.copy() for a in X.reference(name, precision, n))
    cfg = fr_cfg(fr, X.view_cfg(name, m))
    check(lib.fr_escape_extend(C.byref(cfg), precision, None, 0, X.H, n, 2, z.ctypes.data, it.ctypes.data))
    assert_is_reference((z, it), X.reference(name, precision, m), "fr_escape_extend")
    z0, it0 = X.reference(name, precision, n)
    z2, it2 = fr.extend_rows(cfg, z0, it0, n, precision=precision)
    assert_is_reference((z2, it2), X.reference(name, precision, m), "extend_rows")
    z3, it3 = fr.extend_rows(cfg, z0[13:30], it0[13:30], n, precision=precision, y0=13, y1=30)
    assert_is_reference((z3, it3), tuple(a[13:30] for a in X.reference(name, precision, m)), "extend_rows rows")


def test_host_form_dd(fr):
    cfg = DM.deep_view(fr.Config.new(), True, 64, 48, 7)
    z, it = DM.escape_rows(cfg, LO)
    cfg.iterations = 3000
    z2, it2 = fr.extend_rows(cfg, z, it, 7, precision=fr.Precision.DD, pos_lo=LO)
    assert z2.shape == (48, 64, 4)
    assert_is_reference((z2, it2), DM.escape_rows(cfg, LO), "extend_rows DD")


def test_python_device_wrappers(fr, torch):
    st = Stored(torch, X.W * X.H)
    cfg = fr_cfg(fr, X.view_cfg("julia", 5))
    fr.escape_rows_device(cfg, st.z_ptr, st.it_ptr)
    assert_is_reference(st.read((X.H, X.W)), X.reference("julia", F64, 5), "escape_rows_device")
    cfg.iterations = 200
    fr.extend_rows_device(cfg, st.z_ptr, st.it_ptr, 5, stream=torch.cuda.current_stream().cuda_stream)
    assert_is_reference(st.read((X.H, X.W)), X.reference("julia", F64, 200), "extend_rows_device")
    out = torch.zeros(4 * X.W * X.H, dtype=torch.uint8, device="cuda")
    fr.colour_rows_device(cfg, st.z_ptr, st.it_ptr, X.W * X.H, out.data_ptr(), channels=4)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(X.H, X.W, 4), fr.get_image_rgba(cfg))


# ---- colour -------------------------------------------------------------------------------------------------------------


def colour(torch, lib, cfg, st, n, channels, off=0, stream=None):
    """fr_colour_rows_device into a guarded destination `off` bytes behind an aligned base -> uint8 [n, channels]"""
    need = channels * n
    d_out = torch.full((GUARD + 16 + need + GUARD,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
    assert d_out.data_ptr() % 16 == 0
    at = GUARD + off
    torch.cuda.synchronize()
    check(lib.fr_colour_rows_device(C.byref(cfg), st.z_ptr, st.zw, st.it_ptr, n, channels, d_out.data_ptr() + at, need, stream))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:at] == 0xA5).all() and (host[at + need:] == 0xA5).all(), "the colour pass wrote outside its destination"
    return host[at:at + need].reshape(n, channels)


def oracle_image(cfg, precision):
    O.set_log2_mode(O.LOG2_SOFT)
    try:
        return O.get_image(O.Config.from_buffer_copy(bytes(cfg)), precision)
    finally:
        O.set_log2_mode(O.LOG2_LIBM)


@pytest.mark.parametrize("smooth,inside", [(1, 1), (1, 0), (0, 1), (0, 0)], ids=["smooth_inside", "smooth", "flat_inside", "flat"])
@pytest.mark.parametrize("name,precision", VIEWS, ids=VIEW_IDS)
def test_colour_pass_over_extended_results_is_the_render(fr, lib, torch, name, precision, smooth, inside):
    n, m = 5, 200
    st = from_reference(torch, name, precision, n)
    cfg = fr_cfg(fr, X.view_cfg(name, m))
    extend(lib, cfg, precision, st, n)
    npx = X.W * X.H
    for exposure in (5.0, 1.7):
        cfg.smooth, cfg.inside, cfg.exposure = smooth, inside, exposure
        want = fr.get_image_rows(cfg, 0, X.H, precision)
        assert len(np.unique(want.reshape(-1, 3), axis=0)) > (2 if smooth else 1)
        assert np.array_equal(want, oracle_image(cfg, precision)), "the render itself differs from the oracle"
        for off in (0, 1, 2, 3):  # 0: whole dwords for the full waves; the others: bytes
            got = colour(torch, lib, cfg, st, npx, 3, off)
            assert np.array_equal(got.reshape(X.H, X.W, 3), want), "RGB at byte offset %d, exposure %g" % (off, exposure)
        got4 = colour(torch, lib, cfg, st, npx, 4)
        assert np.array_equal(got4.reshape(X.H, X.W, 4), fr.get_image_rgba(cfg, precision)), "RGBA, exposure %g" % exposure
        assert (got4[:, 3] == 255).all() and np.array_equal(got4[:, :3].reshape(X.H, X.W, 3), want)
    # a row range of the stored arrays: any n pixels
    part = colour(torch, lib, cfg, st, 3 * X.W + 5, 3)
    assert np.array_equal(part, want.reshape(-1, 3)[:3 * X.W + 5])


@pytest.mark.parametrize("smooth,inside", [(1, 1), (0, 0)], ids=["smooth_inside", "flat"])
@pytest.mark.parametrize("julia", [False, True], ids=["mandelbrot", "julia"])
def test_colour_pass_dd(fr, lib, torch, julia, smooth, inside):
    ZERO = (0.0, 0.0)  # with this centre the view's orbits escape at two dozen different steps (tests/dd_model.c)
    cfg = DM.deep_view(fr.Config.new(), julia, 64, 48, 7)
    st = Stored(torch, 64 * 48, zw=4).upload(*DM.escape_rows(cfg, ZERO))
    cfg.iterations = 300
    extend(lib, cfg, DD, st, 7, pos_lo=ZERO)
    cfg.smooth, cfg.inside, cfg.exposure = smooth, inside, 3.0
    want = fr.get_image_rows(cfg, 0, 48, fr.Precision.DD, pos_lo=ZERO)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 2
    wz, wit = DM.escape_rows(cfg, ZERO)
    O.set_log2_mode(O.LOG2_SOFT)
    try:
        model = O.colour_rows(O.Config.from_buffer_copy(bytes(cfg)), np.ascontiguousarray(wz[..., 0::2]), wit)
    finally:
        O.set_log2_mode(O.LOG2_LIBM)
    assert np.array_equal(want, model)
    assert np.array_equal(colour(torch, lib, cfg, st, 64 * 48, 3).reshape(48, 64, 3), want)
    assert np.array_equal(colour(torch, lib, cfg, st, 64 * 48, 3, off=1).reshape(48, 64, 3), want)
    got4 = colour(torch, lib, cfg, st, 64 * 48, 4).reshape(48, 64, 4)
    assert np.array_equal(got4, fr.get_image_rgba(cfg, fr.Precision.DD, pos_lo=ZERO))


@pytest.mark.parametrize("precision", [F64, F32], ids=["f64", "f32"])
def test_colour_pass_strides_over_more_pixels_than_its_grid(fr, lib, torch, precision):
    """colour_rows_kernel's workgroups take up to four helpings of 256 pixels, a grid's width apart: 1031 x 521 = 537 151
    pixels are 2099 helpings for 525 workgroups — the last workgroups take three, and the last wave is ragged"""
    w, h = 1031, 521
    assert (w * h + 255) // 256 % 4 != 0 and (w * h) % 64 != 0
    cfg = fr_cfg(fr, X.view_cfg("mandelbrot", 20, w, h))
    st = Stored(torch, w * h)
    render_raw(lib, cfg, precision, st)
    cfg.iterations = 50
    extend(lib, cfg, precision, st, 20)
    wz, wit = O.escape_rows(O.Config.from_buffer_copy(bytes(cfg)), precision)
    assert_is_reference(st.read((h, w)), (wz, wit), "1031 x 521, 20 -> 50")
    want = fr.get_image_rows(cfg, 0, h, precision)
    assert np.array_equal(want, oracle_image(cfg, precision))
    for off in (0, 3):
        assert np.array_equal(colour(torch, lib, cfg, st, w * h, 3, off).reshape(h, w, 3), want), off
    assert np.array_equal(colour(torch, lib, cfg, st, w * h, 4).reshape(h, w, 4)[..., :3], want)


def test_fern_has_no_orbits_to_extend_and_colours_black(fr, lib, torch):
    cfg = fr.Config.new(fr.Algo.BarnsleyFern)
    cfg.width, cfg.height, cfg.iterations = X.W, X.H, 0
    st = Stored(torch, X.W * X.H)
    render_raw(lib, cfg, F64, st)
    cfg.iterations = 50
    extend(lib, cfg, F64, st, 0)
    z, it = st.read((X.H, X.W))
    assert (it == 0).all() and (z == 0).all()
    assert (colour(torch, lib, cfg, st, X.W * X.H, 3) == 0).all()
    got4 = colour(torch, lib, cfg, st, X.W * X.H, 4)
    assert (got4[:, :3] == 0).all() and (got4[:, 3] == 255).all()


# ---- past 4 GiB ---------------------------------------------------------------------------------------------------------


def test_offsets_past_4_gib(fr, lib, torch):
    """width 40 000, rows [0, 6 720): 268.8 M pixels, 4.3 GB of z and 1.1 GB of iters — element offsets past 2^31 and byte
    offsets past 2^32 in both kernels"""
    w, rows, height = 40000, 6720, 6720
    npx = w * rows
    assert npx * 16 > 2 ** 32 and npx > 2 ** 28
    dev = torch.device("cuda", 0)
    try:
        dz = torch.empty(npx * 2, dtype=torch.float64, device=dev)
        di = torch.empty(npx, dtype=torch.int32, device=dev)
    except (RuntimeError, MemoryError) as e:  # torch.cuda.OutOfMemoryError is a RuntimeError
        pytest.skip("cannot allocate 5.4 GB of device memory: %s" % str(e)[:80])
    cfg = fr_cfg(fr, X.view_cfg("mandelbrot", 2, w, height))
    check(lib.fr_escape_rows_device(C.byref(cfg), F64, None, 0, rows, 2, dz.data_ptr(), di.data_ptr(), None, None))
    cfg.iterations = 4
    check(lib.fr_escape_extend_device(C.byref(cfg), F64, None, 0, rows, 2, 2, dz.data_ptr(), di.data_ptr(), None, None))
    torch.cuda.synchronize()
    ocfg = O.Config.from_buffer_copy(bytes(cfg))
    for y0, y1 in ((0, 8), (rows - 8, rows)):
        wz, wit = O.escape_rows(ocfg, F64, y0, y1)
        assert len(np.unique(wit)) >= 3  # escapes within the link and orbits still running
        gz = dz[2 * w * y0:2 * w * y1].cpu().numpy().reshape(y1 - y0, w, 2)
        git = di[w * y0:w * y1].cpu().numpy().view(np.uint32).reshape(y1 - y0, w)
        assert_is_reference((gz, git), (wz, wit), "rows [%d, %d) of 6720 x 40000" % (y0, y1))
    del dz, di
    torch.cuda.empty_cache()


# ---- concurrency, profiling ------------------------------------------------------------------------------------------------


def test_two_threads_extend_and_colour_at_once(fr, lib, torch):
    jobs = [("mandelbrot", F64, 4), ("julia", F32, 3)]
    m = X.CHAIN[-1]
    serial, results, errors = {}, {}, []

    def run(key, name, precision, channels, stream):
        st = from_reference(torch, name, precision, X.CHAIN[1])
        cfg = fr_cfg(fr, X.view_cfg(name, m))
        need = channels * X.W * X.H
        d_out = torch.zeros(need, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h = stream.cuda_stream if stream is not None else None
        for a, b in zip(X.CHAIN[1:], X.CHAIN[2:]):  # ten launches per thread, nothing waited for in between
            cfg.iterations = b
            check(lib.fr_escape_extend_device(C.byref(cfg), precision, None, 0, X.H, a, 2, st.z_ptr, st.it_ptr, h, None))
            check(lib.fr_colour_rows_device(C.byref(cfg), st.z_ptr, 2, st.it_ptr, X.W * X.H, channels, d_out.data_ptr(), need, h))
        (stream.synchronize() if stream is not None else torch.cuda.synchronize())
        return st.read((X.H, X.W)) + (d_out.cpu().numpy(),)

    for k, (name, precision, channels) in enumerate(jobs):
        serial[k] = run(k, name, precision, channels, None)
        assert_is_reference(serial[k][:2], X.reference(name, precision, m), "serial")

    def worker(k, name, precision, channels):
        try:
            results[k] = run(k, name, precision, channels, torch.cuda.Stream())
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(k,) + job) for k, job in enumerate(jobs)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in serial:
        assert np.array_equal(results[k][1], serial[k][1])
        assert np.array_equal(results[k][0].view(np.uint64), serial[k][0].view(np.uint64))
        assert np.array_equal(results[k][2], serial[k][2])


def test_profiling_reports_the_new_kernels(fr, lib, torch):
    def last():
        buf, ms = C.create_string_buffer(256), C.c_float(-1.0)
        check(lib.fr_last_kernel_name(buf, len(buf)))
        check(lib.fr_last_kernel_ms(C.byref(ms)))
        return buf.value.decode(), ms.value

    check(lib.fr_set_profiling(1))
    try:
        for precision, want in ((F64, "escape_extend_kernel<double>"), (F32, "escape_extend_kernel<float>")):
            st = Stored(torch, X.W * X.H)
            cfg = fr_cfg(fr, X.view_cfg("mandelbrot", 5))
            render_raw(lib, cfg, precision, st)
            name, ms = last()
            assert name.startswith("escape_strip_kernel") and ms > 0.0
            cfg.iterations = 200
            extend(lib, cfg, precision, st, 5)
            name, ms = last()
            assert name == want and ms > 0.0
            assert_is_reference(st.read((X.H, X.W)), X.reference("mandelbrot", precision, 200), "profiled")
        cfg = DM.deep_view(fr.Config.new(), False, 64, 48, 7)
        st = Stored(torch, 64 * 48, zw=4)
        render_raw(lib, cfg, DD, st)
        assert last()[0] == "escape_dd_kernel"
        cfg.iterations = 300
        extend(lib, cfg, DD, st, 7)
        name, ms = last()
        assert name == "escape_extend_dd_kernel" and ms > 0.0
    finally:
        check(lib.fr_set_profiling(0))
