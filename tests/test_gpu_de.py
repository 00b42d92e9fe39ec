"""DE, distance estimation, on the device (include/fractal_hip.h, fr_precision: "DE"; csrc/fr_de.hip), bit for bit against
tests/de_model.py: z, iters, der, D and the RGB / RGBA bytes.  A NaN compares as a NaN; every other double by its bits.

Both algorithms on both roads; 40 x 24 and 37 x 23 (ragged workgroups in both axes); a row piece and an empty one; caps 0, 1
and caps that leave capped pixels; PT with and without pos_lo, a Julia view that rebases onto K, a view whose reference orbit
ends by escape, the 2^200 wide-centre view of the wide tests, and the view on c = i whose derivative overflows.  Each model
result is computed once and shared."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import de_model as D
import oracle_lib as O
import pt_model as PTM
import pt_wide_model as W
from test_de_cpu import misiurewicz_i

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes on both sides of every device array
FILL = 0xA5


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


# ---- the cases: a view, its road, and the model's answer ---------------------------------------------------------------------


class Case:
    def __init__(self, name, cfg, road, pos_lo=None, wide=None):
        import fractal_renderer_amd as fr
        from fractal_renderer_amd import _native

        self.name, self.road, self.pos_lo = name, road, pos_lo
        self.cfg = fr.Config.from_buffer_copy(bytes(cfg))
        self.centre = None
        if wide:  # (centre name, words)
            ints = W.centre_ints(*wide)
            self.words = W.to_words(ints[0], wide[1]), W.to_words(ints[1], wide[1])
            p64 = C.POINTER(C.c_uint64)
            self.centre = _native.fr_wide_centre(wide[1], self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64))
            self.orbits = W.Orbits(self.cfg, *ints, wide[1])
        self.z, self.it, self.der = self.model_rows()
        self.dist = D.distance(self.cfg, self.z, self.it, self.der)
        for a in (self.z, self.it, self.der, self.dist):
            a.setflags(write=False)

    def model_rows(self, y0=0, y1=None, cfg=None):
        cfg = self.cfg if cfg is None else cfg
        if self.centre is not None:
            return D.pt_wide_rows(cfg, self.orbits, y0, y1)
        if self.road == "pt":
            return D.pt_rows(cfg, self.pos_lo or (0.0, 0.0), y0, y1)
        return D.f64_rows(cfg, y0, y1)

    @functools.lru_cache(maxsize=None)
    def image(self, thickness, channels):
        a = D.colour(self.cfg, self.z, self.it, self.der, thickness, channels)
        a.setflags(write=False)
        return a


def _cfg(algo=0):
    return O.config_new(algo)


BUILDERS = {
    "f64-mandelbrot-40x24": lambda: Case("", D.default_view(_cfg(), 40, 24, 200), "f64"),
    "f64-mandelbrot-37x23": lambda: Case("", D.default_view(_cfg(), 37, 23, 200), "f64"),
    "f64-julia-40x24": lambda: Case("", D.julia_view(_cfg(), 40, 24, 300), "f64"),
    "f64-julia-37x23": lambda: Case("", D.julia_view(_cfg(), 37, 23, 300), "f64"),
    "f64-overflow": lambda: Case("", misiurewicz_i(_cfg()), "f64"),
    "pt-mandelbrot-37x23": lambda: Case("", D.default_view(_cfg(), 37, 23, 200), "pt"),
    "pt-julia-40x24": lambda: Case("", D.julia_view(_cfg(), 40, 24, 300), "pt"),
    "pt-overflow": lambda: Case("", misiurewicz_i(_cfg()), "pt"),
}


def _with_lo(make, *args):
    cfg = _cfg()
    lo = make(cfg, *args)
    return cfg, lo


BUILDERS["pt-seahorse-pos-lo"] = lambda: (lambda c: Case("", c[0], "pt", c[1]))(_with_lo(D.seahorse_shallow, 40, 24, 3000, 1e11))


def deep_view(cfg, width=37, height=23, iterations=300):
    """past the f64 limit, so the centre needs its low half: 1e18 around a point 2e-19 above c = i, a fifth of the view's height"""
    misiurewicz_i(cfg, width, height, iterations)
    cfg.scale.re = cfg.scale.im = 1e18
    return (0.0, 2e-19)


BUILDERS["pt-deep-pos-lo"] = lambda: (lambda c: Case("", c[0], "pt", c[1]))(_with_lo(deep_view))
BUILDERS["pt-julia-rebase"] = lambda: (lambda c: Case("", c[0], "pt"))(_with_lo(PTM.julia_rebase_view, 40, 24, 3000))
BUILDERS["pt-orbit-escapes"] = lambda: (lambda c: Case("", c[0], "pt"))(_with_lo(PTM.early_escape_view, 37, 23, 2000))
BUILDERS["wide-2^200"] = lambda: Case("", W.view(_cfg(), "M", 200, 16, 12, 3000), "pt", wide=("M", 5))
BUILDERS["wide-2^200-37x21"] = lambda: Case("", W.view(_cfg(), "M", 200, 37, 21, 3000), "pt", wide=("M", 5))
BUILDERS["wide-julia"] = lambda: Case("", W.view(_cfg(), "J", 100, 24, 16, 400), "pt", wide=("J", 3))

ALL = sorted(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    c.name = name
    return c


# ---- device memory with guards -------------------------------------------------------------------------------------------------


class Buf:
    def __init__(self, torch, nbytes):
        self.torch, self.nbytes = torch, nbytes
        self.t = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
        self.ptr = self.t.data_ptr() + GUARD
        assert self.ptr % 8 == 0

    def put(self, a):
        raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
        assert raw.size == self.nbytes
        self.t[GUARD:GUARD + self.nbytes] = self.torch.from_numpy(raw.copy()).to(self.t.device)
        return self

    def get(self, dtype, shape=None, offset=0):
        self.torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        assert (a[:GUARD + offset] == FILL).all() and (a[GUARD + self.nbytes:] == FILL).all(), "a write outside the array"
        out = a[GUARD + offset:GUARD + self.nbytes].copy().view(dtype)
        return out if shape is None else out.reshape(shape)

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.t == FILL).all().item())


class Rows:
    """(z, iters, der) of rows x width pixels in device memory"""

    def __init__(self, torch, rows, width):
        self.shape = (rows, width)
        n = rows * width
        self.n = n
        self.z, self.it, self.der = Buf(torch, 16 * n), Buf(torch, 4 * n), Buf(torch, 16 * n)

    def get(self):
        return self.z.get(np.float64, self.shape + (2,)), self.it.get(np.uint32, self.shape), self.der.get(np.float64, self.shape + (2,))


def render_device(lib, torch, c, y0=0, y1=None, cfg=None):
    cfg = c.cfg if cfg is None else cfg
    y1 = cfg.height if y1 is None else y1
    r = Rows(torch, y1 - y0, cfg.width)
    if c.centre is not None:
        check(lib.fr_escape_rows_de_pt_wide_device(C.byref(cfg), C.byref(c.centre), y0, y1, r.z.ptr, r.it.ptr, r.der.ptr, None))
    else:
        lo = None if c.pos_lo is None else C.byref(_lo(c.pos_lo))
        check(lib.fr_escape_rows_de_device(C.byref(cfg), 3 if c.road == "pt" else 0, lo, y0, y1, r.z.ptr, r.it.ptr, r.der.ptr, None))
    return r


def _lo(pos_lo):
    from fractal_renderer_amd import Imaginary

    return Imaginary(float(pos_lo[0]), float(pos_lo[1]))


def render_host(lib, c, y0=0, y1=None):
    y1 = c.cfg.height if y1 is None else y1
    shape = (y1 - y0, c.cfg.width)
    z, der = np.empty(shape + (2,), dtype=np.float64), np.empty(shape + (2,), dtype=np.float64)
    it = np.empty(shape, dtype=np.uint32)
    if c.centre is not None:
        check(lib.fr_escape_rows_de_pt_wide(C.byref(c.cfg), C.byref(c.centre), y0, y1, z.ctypes.data, it.ctypes.data, der.ctypes.data))
    else:
        lo = None if c.pos_lo is None else C.byref(_lo(c.pos_lo))
        check(lib.fr_escape_rows_de(C.byref(c.cfg), 3 if c.road == "pt" else 0, lo, y0, y1, z.ctypes.data, it.ctypes.data, der.ctypes.data))
    return z, it, der


def assert_rows(got, want, what):
    z, it, der = got
    wz, wit, wder = want
    assert np.array_equal(it, wit), "%s: escape indices differ at %d pixels" % (what, int((it != wit).sum()))
    assert D.same_doubles(z, wz), "%s: z differs" % what
    assert D.same_doubles(der, wder), "%s: der differs" % what


# ---- the renders ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ALL)
def test_rows_distance_and_colour_on_the_device(lib, torch, name):
    c = case(name)
    r = render_device(lib, torch, c)
    assert_rows(r.get(), (c.z, c.it, c.der), name)
    dist = Buf(torch, 8 * r.n)
    check(lib.fr_distance_rows_device(C.byref(c.cfg), r.z.ptr, r.it.ptr, r.der.ptr, r.n, dist.ptr, None))
    assert D.same_doubles(dist.get(np.float64, r.shape), c.dist), "%s: D differs" % name
    for channels in (3, 4):
        out = Buf(torch, channels * r.n)
        check(lib.fr_colour_de_rows_device(C.byref(c.cfg), r.z.ptr, r.it.ptr, r.der.ptr, r.n, 2.0, channels, out.ptr, None))
        assert np.array_equal(out.get(np.uint8, r.shape + (channels,)), c.image(2.0, channels)), "%s: %d channels" % (name, channels)


def test_the_cases_are_what_they_claim():
    """so that none can go trivial unnoticed (the model alone: no device is needed, but the cases live here)"""
    for name in ALL:
        c = case(name)
        escaped = c.it < c.cfg.iterations
        assert escaped.any(), name
        assert ((c.dist < 2.0) & escaped).sum() >= 40 and (c.image(2.0, 3) != c.image(0.0, 3)).any(), name
    for name in ("f64-overflow", "pt-overflow"):
        c = case(name)
        bad = ~np.isfinite(c.der).all(-1)
        assert bad.sum() >= 1 and (c.dist[bad] == 0.0).all()
    for name in ("f64-mandelbrot-40x24", "pt-mandelbrot-37x23", "pt-seahorse-pos-lo", "pt-orbit-escapes", "wide-julia"):
        c = case(name)
        assert (c.it == c.cfg.iterations).any(), name
    c = case("pt-orbit-escapes")
    assert len(PTM.reference_orbit(c.cfg)) < 100  # the reference orbit ends by escape long before the cap
    c = case("pt-julia-rebase")
    assert len(PTM.reference_orbit(c.cfg, which=0)) < 300 < int(c.it.max())  # V ends; the pixels go on on K


@pytest.mark.parametrize("name", ["f64-mandelbrot-37x23", "f64-julia-37x23", "pt-mandelbrot-37x23", "pt-julia-rebase", "wide-2^200-37x21"])
@pytest.mark.parametrize("cap", [0, 1])
def test_caps_zero_and_one(fr, lib, torch, name, cap):
    c = case(name)
    cfg = fr.Config.from_buffer_copy(bytes(c.cfg))
    cfg.iterations = cap
    if c.centre is not None:
        want = D.pt_wide_rows(cfg, W.Orbits(cfg, *W.centre_ints("M", 5), 5))
    else:
        want = c.model_rows(cfg=cfg)
    if cap == 0:
        assert not want[1].any() and (want[2] == [1.0, 0.0]).all()
    got = render_device(lib, torch, c, cfg=cfg).get()
    assert_rows(got, want, "%s at cap %d" % (name, cap))


@pytest.mark.parametrize("name", ["f64-mandelbrot-37x23", "pt-julia-rebase", "pt-seahorse-pos-lo", "wide-2^200-37x21"])
def test_a_row_piece_is_the_slice_and_no_rows_touch_nothing(lib, torch, name):
    c = case(name)
    piece = render_device(lib, torch, c, 5, 19).get()
    assert_rows(piece, (c.z[5:19], c.it[5:19], c.der[5:19]), name)
    r = Rows(torch, 2, c.cfg.width)
    if c.centre is not None:
        check(lib.fr_escape_rows_de_pt_wide_device(C.byref(c.cfg), C.byref(c.centre), 7, 7, r.z.ptr, r.it.ptr, r.der.ptr, None))
    else:
        check(lib.fr_escape_rows_de_device(C.byref(c.cfg), 3 if c.road == "pt" else 0, None, 7, 7, r.z.ptr, r.it.ptr, r.der.ptr, None))
    assert r.z.untouched() and r.it.untouched() and r.der.untouched()


@pytest.mark.parametrize("name", ["f64-julia-37x23", "pt-seahorse-pos-lo", "pt-overflow", "wide-julia"])
def test_host_forms_are_the_device_forms(fr, lib, name):
    c = case(name)
    z, it, der = render_host(lib, c)
    assert_rows((z, it, der), (c.z, c.it, c.der), name)
    piece = render_host(lib, c, 3, 11)
    assert_rows(piece, (c.z[3:11], c.it[3:11], c.der[3:11]), name)
    dist = np.empty(it.shape, dtype=np.float64)
    check(lib.fr_distance_rows(C.byref(c.cfg), z.ctypes.data, it.ctypes.data, der.ctypes.data, it.size, dist.ctypes.data))
    assert D.same_doubles(dist, c.dist)
    rgb = np.empty(it.shape + (3,), dtype=np.uint8)
    check(lib.fr_colour_de_rgb8(C.byref(c.cfg), z.ctypes.data, it.ctypes.data, der.ctypes.data, it.size, 2.0, rgb.ctypes.data, rgb.nbytes))
    assert np.array_equal(rgb, c.image(2.0, 3))
    # the Python surface over the same calls
    kw = {}
    if c.centre is not None:
        kw = dict(precision=fr.Precision.PT, centre=fr.WideCentre(len(c.words[0]), c.words[0], c.words[1]))
    elif c.road == "pt":
        kw = dict(precision=fr.Precision.PT, pos_lo=c.pos_lo)
    assert_rows(fr.escape_rows_de(c.cfg, **kw), (c.z, c.it, c.der), name)
    assert D.same_doubles(fr.distance_rows(c.cfg, z, it, der), c.dist)
    assert np.array_equal(fr.colour_image_de(c.cfg, z, it, der, 0.5), c.image(0.5, 3))
    assert np.array_equal(fr.get_image_de(c.cfg, 2.0, **kw), c.image(2.0, 3))


# ---- the shaded colour map ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["f64-mandelbrot-40x24", "pt-julia-rebase"])
def test_thickness_zero_is_the_plain_recolour(lib, torch, name):
    c = case(name)
    r = Rows(torch, *c.it.shape)
    r.z.put(c.z), r.it.put(c.it), r.der.put(c.der)
    for channels in (3, 4):
        plain, shaded = Buf(torch, channels * r.n), Buf(torch, channels * r.n)
        check(lib.fr_colour_rows_device(C.byref(c.cfg), r.z.ptr, 2, r.it.ptr, r.n, channels, plain.ptr, channels * r.n, None))
        check(lib.fr_colour_de_rows_device(C.byref(c.cfg), r.z.ptr, r.it.ptr, r.der.ptr, r.n, 0.0, channels, shaded.ptr, None))
        a, b = plain.get(np.uint8), shaded.get(np.uint8)
        assert np.array_equal(a, b) and np.array_equal(b.reshape(c.it.shape + (channels,)), c.image(0.0, channels))
    assert (c.image(0.0, 3) != c.image(2.0, 3)).any(-1).sum() >= 50  # and a thickness does change this view


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_three_channels_at_any_byte_offset(lib, torch, offset):
    c = case("f64-julia-37x23")
    r = Rows(torch, *c.it.shape)
    r.z.put(c.z), r.it.put(c.it), r.der.put(c.der)
    out = Buf(torch, 3 * r.n + offset)
    check(lib.fr_colour_de_rows_device(C.byref(c.cfg), r.z.ptr, r.it.ptr, r.der.ptr, r.n, 2.0, 3, out.ptr + offset, None))
    assert np.array_equal(out.get(np.uint8, c.it.shape + (3,), offset=offset), c.image(2.0, 3))


def test_thickness_is_a_recolour(lib, torch):
    """a kept view: one render, then thickness varied over the stored arrays"""
    c = case("f64-mandelbrot-37x23")
    r = render_device(lib, torch, c)
    for thickness in (0.25, 1.0, 8.0, 2.0 ** 20):
        out = Buf(torch, 4 * r.n)
        check(lib.fr_colour_de_rows_device(C.byref(c.cfg), r.z.ptr, r.it.ptr, r.der.ptr, r.n, thickness, 4, out.ptr, None))
        assert np.array_equal(out.get(np.uint8, r.shape + (4,)), c.image(thickness, 4)), thickness


def test_profiling_names_the_kernels(fr, lib, torch):
    check(lib.fr_set_profiling(1))
    try:
        for name, kernel in (("f64-julia-37x23", b"escape_de_kernel"), ("pt-mandelbrot-37x23", b"escape_pt_de_kernel")):
            render_device(lib, torch, case(name))
            torch.cuda.synchronize()
            buf = C.create_string_buffer(128)
            check(lib.fr_last_kernel_name(buf, 128))
            assert buf.value == kernel
    finally:
        check(lib.fr_set_profiling(0))


# ---- the command line ---------------------------------------------------------------------------------------------------------------

DEEP = ["--perturbation", "-x", "0", "-y", "1.0000000000000000000000000000000", "-s", "1e18", "-i", "3000"]


@pytest.mark.parametrize("view", ["plain", "perturbation"])
def test_the_cli_writes_get_image_de(fr, tmp_path, view):
    from test_cpp_host import CLI_EXE, _read_ppm, build_cli

    build_cli()
    if view == "plain":
        args, kw = ["-i", "300"], dict()
        cfg = fr.Config.from_buffer_copy(bytes(O.cli_config(64, 48, iterations=300)))
    else:
        args = DEEP
        cfg = fr.Config.from_buffer_copy(bytes(O.cli_config(64, 48, iterations=3000, scale=(1e18, 1e18))))
        kw = dict(precision=fr.Precision.PT, centre=fr.WideCentre.from_str(DEEP[2], DEEP[4], scale=1e18))
    out = str(tmp_path / "de")
    r = subprocess.run([CLI_EXE] + args + ["--distance-shade", "1.5", "64", "48", "-o", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    image = fr.get_image_de(cfg, 1.5, **kw)
    assert np.array_equal(_read_ppm(out + ".ppm"), image)
    plain = fr.get_image(cfg, **kw)
    assert (image != plain).any(-1).sum() >= 50 and (image <= plain).all()
