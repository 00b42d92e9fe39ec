"""DE ON SCALED PT on the device (include/fractal_hip.h, "DE ON SCALED PT"; fr_escape_rows_de_pt_scaled(_device); kernels
escape_pt_scaled_de_kernel and escape_bla_scaled_de_kernel), bit for bit against tests/de_scaled_model.py — orbits from
tests/pt_wide_model.py, tables from tests/pt_scaled_model.c, the pixel loops with their scaled derivative restated in
tests/de_scaled_model.c.  A NaN compares as a NaN; every other double by its bits.

  - M_900 (37 x 21, ragged against the 16 x 16 workgroup), J_900, N_900, MINI_861 (capped and interior pixels), MINI_OFF_860 (an
    odd scale with a negative axis), M_440 and J_300, for bits -1, 0 and 53, host and device forms, 64 guard bytes around every
    device array: z and iters are fr_escape_rows_pt_scaled's and the model's, der is the model's u;
  - rows [5, 11) equal the slice of the whole image; caps 0 to 3; an algorithm without orbits gives zeros;
  - the orbit and table caches are shared with fr_escape_rows_pt_scaled, both ways; the profiling names;
  - on M_440, on the device: der 2^e is fr_escape_rows_de_pt_wide's der and the distances are equal (claim 2);
  - get_image_de(scaled=True) is de_model.colour over the model's arrays on the scaled view; thickness 0 gives
    fr_render_rows_pt_scaled's bytes; the C++ overload gives the C calls' bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import de_model as D
import de_scaled_model as M
import deep_truth as T
import pt_scaled_model as S
import pt_wide_model as W
from test_gpu_de import Buf, Rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


class OffView:
    """deep_truth's MINI_OFF_860 as a pt_scaled_model.View is: cfg, words, orbits, shape and the fr_wide_centre"""

    def __init__(self, new_config, name):
        t = T.view(name)
        self.n, self.ints, self.words = t.n, t.ints, t.words
        self.cfg = t.fill(new_config())
        self.orbits = W.Orbits(self.cfg, *t.ints, t.n)
        self.x = self.orbits.x[0]
        self.k = self.orbits.k[0] if t.julia else None
        self.shape = t.shape

    centre = S.View.centre


SPECS = {"M_900": S.M_900, "J_900": S.J_900, "N_900": S.N_900, "MINI_861": S.MINI_861, "MINI_OFF_860": None, "M_440": S.M_440,
         "J_300": S.J_300}
_off = {}


def get_view(fr, name):
    if SPECS[name] is not None:
        return S.view(fr.Config.new, SPECS[name])
    if name not in _off:
        _off[name] = OffView(fr.Config.new, name)
    return _off[name]


def host_rows(lib, native, v, bits=-1, y0=0, y1=None, cfg=None):
    cfg = v.cfg if cfg is None else cfg
    y1 = cfg.height if y1 is None else y1
    st = v.centre(native)
    shape = (y1 - y0, cfg.width)
    z, der = np.full(shape + (2,), np.nan), np.full(shape + (2,), np.nan)
    it = np.full(shape, 0xFFFFFFFF, dtype=np.uint32)
    check(lib.fr_escape_rows_de_pt_scaled(C.byref(cfg), C.byref(st), bits, y0, y1, z.ctypes.data, it.ctypes.data, der.ctypes.data))
    return z, it, der


def device_rows(lib, native, torch, v, bits=-1, y0=0, y1=None, cfg=None):
    """the device form into guarded arrays -> Rows (tests/test_gpu_de.py)"""
    cfg = v.cfg if cfg is None else cfg
    y1 = cfg.height if y1 is None else y1
    st = v.centre(native)
    r = Rows(torch, y1 - y0, cfg.width)
    check(lib.fr_escape_rows_de_pt_scaled_device(C.byref(cfg), C.byref(st), bits, y0, y1, r.z.ptr, r.it.ptr, r.der.ptr, None))
    return r


def scaled_rows(lib, native, v, bits=-1):
    st = v.centre(native)
    z = np.full(v.shape + (2,), np.nan)
    it = np.full(v.shape, 0xFFFFFFFF, dtype=np.uint32)
    check(lib.fr_escape_rows_pt_scaled(C.byref(v.cfg), C.byref(st), bits, 0, v.shape[0], z.ctypes.data, it.ctypes.data))
    return z, it


def assert_rows(got, want, what):
    z, it, der = got
    wz, wit, wder = want[:3]
    assert np.array_equal(it, wit), "%s: escape indices differ at %d pixels" % (what, int((it != wit).sum()))
    assert S.same_bits(z, wz), "%s: z differs" % what
    assert D.same_doubles(der, wder), "%s: der differs" % what


def cache(lib):
    out = (C.c_uint32 * 4)()
    check(lib.fr_debug_bla_cache(out))
    return tuple(out)


def model_bits(bits):
    return 40 if bits == 0 else bits


# ---- the kernels against the model -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("bits", [-1, 0, 53])
@pytest.mark.parametrize("name", list(SPECS))
def test_the_kernel_is_the_model(fr, native, lib, torch, name, bits):
    v = get_view(fr, name)
    want = M.model(v, model_bits(bits))
    it = want[1]
    if name == "N_900":
        assert (it == v.cfg.iterations).all()
    elif name == "MINI_861":
        assert (it == v.cfg.iterations).sum() >= 50 and (it < v.cfg.iterations).sum() >= 250  # capped and interior pixels beside escaped ones
    else:
        assert (it < v.cfg.iterations).sum() * 10 >= 9 * it.size
    if bits >= 0 and name != "N_900":
        assert ((it < v.cfg.iterations) & (want[4] > 0)).sum() >= 1, "a view whose escaped pixels never skip checks no skipped derivative"
    sz, sit = scaled_rows(lib, native, v, bits)
    assert np.array_equal(sit, it) and S.same_bits(sz, want[0]), "CLAIM 1: z and iters are fr_escape_rows_pt_scaled's"
    assert_rows(host_rows(lib, native, v, bits), want, "%s, bits %d, host arrays" % (name, bits))
    r = device_rows(lib, native, torch, v, bits)
    assert_rows(r.get(), want, "%s, bits %d, device arrays" % (name, bits))
    # DE's distance over the arrays, on the device, on the scaled view
    view = fr.de_scaled_view(v.cfg)
    assert bytes(view) == bytes(M.scaled_view(v.cfg))
    dist = Buf(torch, 8 * r.n)
    check(lib.fr_distance_rows_device(C.byref(view), r.z.ptr, r.it.ptr, r.der.ptr, r.n, dist.ptr, None))
    want_d = D.distance(view, *want[:3])
    assert D.same_doubles(dist.get(np.float64, r.shape), want_d), "%s: D differs" % name
    if name == "N_900":
        assert (want_d == 0.0).all()
    else:
        assert ((want_d > 0.0) & np.isfinite(want_d)).sum() * 2 >= it.size


@pytest.mark.parametrize("bits", [-1, 0])
def test_row_pieces_equal_the_slices_of_the_whole(fr, native, lib, torch, bits):
    v = get_view(fr, "M_900")  # ragged edges, more than one workgroup on both axes
    want = M.model(v, model_bits(bits))
    for y0, y1 in ((5, 11), (0, 5), (11, 21), (20, 21)):
        assert_rows(device_rows(lib, native, torch, v, bits, y0, y1).get(), tuple(a[y0:y1] for a in want[:3]), "rows [%d, %d)" % (y0, y1))
        assert_rows(host_rows(lib, native, v, bits, y0, y1), tuple(a[y0:y1] for a in want[:3]), "host rows [%d, %d)" % (y0, y1))
    if bits >= 0:
        assert cache(lib)[3] == 0  # Dw is the image's: every piece is served from one table
    r = Rows(torch, 2, v.cfg.width)
    st = v.centre(native)
    check(lib.fr_escape_rows_de_pt_scaled_device(C.byref(v.cfg), C.byref(st), bits, 7, 7, r.z.ptr, r.it.ptr, r.der.ptr, None))
    assert r.z.untouched() and r.it.untouched() and r.der.untouched()


@pytest.mark.parametrize("name", ["M_900", "J_900", "MINI_861"])
@pytest.mark.parametrize("cap", [0, 1, 2, 3])
def test_small_caps(fr, native, lib, torch, name, cap):
    v = get_view(fr, name)
    cfg = fr.Config.from_buffer_copy(bytes(v.cfg))
    cfg.iterations = cap
    orbits = W.Orbits(cfg, *v.ints, v.n)
    x, k = orbits.x[0], orbits.k[0] if cfg.algo == 2 else None
    plain = M.escape_rows(cfg, x, k, -1)
    want = M.escape_rows(cfg, x, k, 40)
    if cap <= (2 if cfg.algo == 2 else 1):  # no level to skip with
        assert not want[4].any()
        assert_rows(want[:3], plain, "the model at cap %d" % cap)
    if cap == 0:
        sinv = 2.0 ** -S.exponent(cfg)
        assert not want[1].any() and (want[2] == [sinv, 0.0]).all()
    assert_rows(device_rows(lib, native, torch, v, -1, cfg=cfg).get(), plain, "%s at cap %d, plain" % (name, cap))
    assert_rows(device_rows(lib, native, torch, v, 0, cfg=cfg).get(), want, "%s at cap %d, table" % (name, cap))
    assert_rows(host_rows(lib, native, v, 0, cfg=cfg), want, "%s at cap %d, table, host" % (name, cap))
    assert_rows(host_rows(lib, native, v, -1, cfg=cfg), plain, "%s at cap %d, plain, host" % (name, cap))


def test_an_algorithm_without_orbits_writes_zeros(fr, native, lib, torch):
    v = get_view(fr, "M_900")
    cfg = fr.Config.from_buffer_copy(bytes(v.cfg))
    cfg.algo = int(fr.Algo.BarnsleyFern)
    cfg.width, cfg.height, cfg.iterations = 20, 9, 50
    st = v.centre(native)
    for bits in (-1, 0):
        r = Rows(torch, 9, 20)
        check(lib.fr_escape_rows_de_pt_scaled_device(C.byref(cfg), C.byref(st), bits, 0, 9, r.z.ptr, r.it.ptr, r.der.ptr, None))
        z, it, der = r.get()
        assert not z.any() and not it.any() and not der.any()
        z, der = np.full((9, 20, 2), np.nan), np.full((9, 20, 2), np.nan)
        it = np.full((9, 20), 7, dtype=np.uint32)
        check(lib.fr_escape_rows_de_pt_scaled(C.byref(cfg), C.byref(st), bits, 0, 9, z.ctypes.data, it.ctypes.data, der.ctypes.data))
        assert not z.any() and not it.any() and not der.any()


# ---- the caches, the profiling names -------------------------------------------------------------------------------------------------


def test_the_caches_are_shared_with_the_scaled_calls(fr, native, lib, torch):
    v, other = get_view(fr, "J_900"), get_view(fr, "M_900")
    scaled_rows(lib, native, other, 0)  # whatever came before, this is another view
    z, it = scaled_rows(lib, native, v, 0)
    built = cache(lib)
    assert built[0] == 40 and built[3] == 1
    assert_rows(host_rows(lib, native, v, 0), M.model(v, 40), "DE after SCALED PT")
    assert cache(lib) == built[:3] + (0,), "the DE call of the same view and bits is served from the cached table"
    # the plain forms in between use the orbits alone: the table is still served afterwards
    assert_rows(device_rows(lib, native, torch, v, -1).get(), M.model(v, -1), "plain DE in between")
    assert_rows(device_rows(lib, native, torch, v, 0).get(), M.model(v, 40), "DE again")
    assert cache(lib) == built[:3] + (0,)
    # and the other way round: a table the DE call built serves the SCALED PT call
    assert_rows(host_rows(lib, native, v, 53), M.model(v, 53), "other bits")
    assert cache(lib)[0] == 53 and cache(lib)[3] == 1
    z, it = scaled_rows(lib, native, v, 53)
    assert cache(lib)[3] == 0 and np.array_equal(it, v.model(53)[1]) and S.same_bits(z, v.model(53)[0])


def test_profiling_names_the_kernels(fr, native, lib, torch):
    check(lib.fr_set_profiling(1))
    try:
        for name in ("M_900", "J_900"):
            for bits, kernel in ((-1, b"escape_pt_scaled_de_kernel"), (0, b"escape_bla_scaled_de_kernel")):
                device_rows(lib, native, torch, get_view(fr, name), bits)
                torch.cuda.synchronize()
                buf = C.create_string_buffer(128)
                check(lib.fr_last_kernel_name(buf, 128))
                assert buf.value == kernel
    finally:
        check(lib.fr_set_profiling(0))


# ---- claim 2 on the device -----------------------------------------------------------------------------------------------------------


def test_in_the_common_domain_the_device_gives_the_wide_roads_derivative(fr, native, lib, torch):
    v = get_view(fr, "M_440")
    e = S.exponent(v.cfg)
    st = v.centre(native)
    r = device_rows(lib, native, torch, v, -1)
    w = Rows(torch, *v.shape)
    check(lib.fr_escape_rows_de_pt_wide_device(C.byref(v.cfg), C.byref(st), 0, v.shape[0], w.z.ptr, w.it.ptr, w.der.ptr, None))
    (z, it, u), (wz, wit, wd) = r.get(), w.get()
    assert np.array_equal(it, wit) and S.same_bits(z, wz)
    assert np.isfinite(wd).all() and D.same_doubles(np.ldexp(u, e), wd)
    view = fr.de_scaled_view(v.cfg)
    a, b = Buf(torch, 8 * r.n), Buf(torch, 8 * r.n)
    check(lib.fr_distance_rows_device(C.byref(view), r.z.ptr, r.it.ptr, r.der.ptr, r.n, a.ptr, None))
    check(lib.fr_distance_rows_device(C.byref(v.cfg), w.z.ptr, w.it.ptr, w.der.ptr, w.n, b.ptr, None))
    da, db = a.get(np.float64, r.shape), b.get(np.float64, r.shape)
    assert D.same_doubles(da, db) and (da > 0).sum() * 2 >= da.size


# ---- the shaded image ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,bla", [("M_900", None), ("MINI_861", 0), ("MINI_OFF_860", 0)])
def test_get_image_de_scaled_is_the_model_shaded(fr, native, lib, torch, name, bla):
    v = get_view(fr, name)
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    kw = dict(precision=fr.Precision.PT, centre=centre, bla=bla, scaled=True)
    want = M.model(v, -1 if bla is None else 40)
    assert_rows(fr.escape_rows_de(v.cfg, **kw), want, "escape_rows_de")
    assert_rows(fr.escape_rows_de(v.cfg, 5, 11, **kw), tuple(a[5:11] for a in want[:3]), "escape_rows_de, rows")
    view = M.scaled_view(v.cfg)
    for thickness in (1.5, 64.0):
        image = fr.get_image_de(v.cfg, thickness, **kw)
        assert np.array_equal(image, D.colour(view, *want[:3], thickness))
    plain = fr.get_image(v.cfg, fr.Precision.PT, centre=centre, bla=bla, scaled=True)
    assert (image != plain).any(-1).sum() >= 20, "the shading does change this view"
    r = Rows(torch, *v.shape)
    fr.escape_rows_de_device(v.cfg, r.z.ptr, r.it.ptr, r.der.ptr, **kw)
    assert_rows(r.get(), want, "escape_rows_de_device")


@pytest.mark.parametrize("name,bits", [("M_900", -1), ("J_900", 0), ("MINI_861", 0)])
def test_thickness_zero_is_the_scaled_render(fr, native, lib, torch, name, bits):
    v = get_view(fr, name)
    h, w = v.shape
    st = v.centre(native)
    view = fr.de_scaled_view(v.cfg)
    r = device_rows(lib, native, torch, v, bits)
    for channels in (3, 4):
        n = channels * r.n
        render, colour = Buf(torch, n), Buf(torch, n)
        check(lib.fr_render_rows_pt_scaled_device(C.byref(v.cfg), C.byref(st), bits, 0, h, channels, render.ptr, n, None))
        check(lib.fr_colour_de_rows_device(C.byref(view), r.z.ptr, r.it.ptr, r.der.ptr, r.n, 0.0, channels, colour.ptr, None))
        a, b = render.get(np.uint8, (h, w, channels)), colour.get(np.uint8, (h, w, channels))
        assert np.array_equal(a, b) and len(np.unique(a.reshape(-1, channels), axis=0)) > 1
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    kw = dict(precision=fr.Precision.PT, centre=centre, bla=None if bits < 0 else bits, scaled=True)
    assert np.array_equal(fr.get_image_de(v.cfg, 0.0, **kw), fr.get_image(v.cfg, **kw))


def test_cpp_overload_gives_the_c_calls_bytes(fr, native, lib, tmp_path):
    from test_gpu_bla import compile_cpp, decimal_centre

    exe = os.path.join(ROOT, "tests", "cpp", "test_de_scaled")
    compile_cpp(os.path.join(ROOT, "tests", "cpp", "test_de_scaled.cpp"), exe)
    tre, tim, centre = decimal_centre(fr, "M", 320, 2.0 ** 900)
    assert centre.words == 16
    cfg = W.view(fr.Config.new(), "M", 900, 37, 21, 6000)
    out = str(tmp_path / "image.rgb")
    r = subprocess.run([exe, tre, tim, "900", "37", "21", "6000", "40", "64.0", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.uint8).reshape(21, 37, 3)
    st = centre.c_struct()
    z, der = np.empty((21, 37, 2)), np.empty((21, 37, 2))
    it = np.empty((21, 37), dtype=np.uint32)
    check(lib.fr_escape_rows_de_pt_scaled(C.byref(cfg), C.byref(st), 40, 0, 21, z.ctypes.data, it.ctypes.data, der.ctypes.data))
    view = fr.de_scaled_view(cfg)
    want = np.empty((21, 37, 3), dtype=np.uint8)
    check(lib.fr_colour_de_rgb8(C.byref(view), z.ctypes.data, it.ctypes.data, der.ctypes.data, it.size, 64.0, want.ctypes.data, want.nbytes))
    assert np.array_equal(got, want) and len(np.unique(want.reshape(-1, 3), axis=0)) > 2
