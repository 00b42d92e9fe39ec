"""DE ON BLA-PT on the device (include/fractal_hip.h, "DE ON BLA-PT"; fr_escape_rows_de_pt_bla(_device); kernel
escape_bla_de_kernel), bit for bit against tests/de_bla_model.py — orbits from the PT models, tables from tests/bla_model.c,
the pixel loop with its derivative restated in tests/de_bla_model.c.  A NaN compares as a NaN; every other double by its bits.

  - every view of tests/bla_model.py's BLA tests (16 x 12, 37 x 21, 48 x 32), host and device forms, 64 guard bytes around every
    device array: z and iters are fr_escape_rows_pt_bla's and the model's, der is the model's;
  - M_37 in row pieces (ragged workgroups on both axes); 24, 40 and 53 bits; caps 0 and 1; an algorithm without orbits;
  - DE's own calls over the arrays: the colour map at thickness 0 is fr_render_rows_pt_bla_device's bytes, the distance is the
    distance model's;
  - the table cache is shared with the BLA-PT calls; the profiling name; the Python keyword and the C++ overload."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bla_model as B
import de_bla_model as M
import de_model as D
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


SPECS = {"M-16x12": B.M_16, "M-37x21": B.M_37, "M-2^440": B.M_DEEP, "N": B.N_16, "J": B.J_48, "seahorse": B.SEAHORSE,
         "early-escape": B.EARLY, "julia-rebase": B.JULIA_REBASE}


def host_rows(lib, native, v, bits=0, y0=0, y1=None, cfg=None):
    cfg = v.cfg if cfg is None else cfg
    y1 = cfg.height if y1 is None else y1
    lo, centre, _keep = v.args(native)
    shape = (y1 - y0, cfg.width)
    z, der = np.full(shape + (2,), np.nan), np.full(shape + (2,), np.nan)
    it = np.full(shape, 0xFFFFFFFF, dtype=np.uint32)
    check(lib.fr_escape_rows_de_pt_bla(C.byref(cfg), lo, centre, bits, y0, y1, z.ctypes.data, it.ctypes.data, der.ctypes.data))
    return z, it, der


def device_rows(lib, native, torch, v, bits=0, y0=0, y1=None, cfg=None):
    """the device form into guarded arrays -> Rows (tests/test_gpu_de.py)"""
    cfg = v.cfg if cfg is None else cfg
    y1 = cfg.height if y1 is None else y1
    lo, centre, _keep = v.args(native)
    r = Rows(torch, y1 - y0, cfg.width)
    check(lib.fr_escape_rows_de_pt_bla_device(C.byref(cfg), lo, centre, bits, y0, y1, r.z.ptr, r.it.ptr, r.der.ptr, None))
    return r


def bla_rows(lib, native, v, bits=0):
    lo, centre, _keep = v.args(native)
    z = np.full(v.shape + (2,), np.nan)
    it = np.full(v.shape, 0xFFFFFFFF, dtype=np.uint32)
    check(lib.fr_escape_rows_pt_bla(C.byref(v.cfg), lo, centre, bits, 0, v.shape[0], z.ctypes.data, it.ctypes.data))
    return z, it


def assert_rows(got, want, what):
    z, it, der = got
    wz, wit, wder = want[:3]
    assert np.array_equal(it, wit), "%s: escape indices differ at %d pixels" % (what, int((it != wit).sum()))
    assert B.same_bits(z, wz), "%s: z differs" % what
    assert D.same_doubles(der, wder), "%s: der differs" % what


def cache(lib):
    out = (C.c_uint32 * 4)()
    check(lib.fr_debug_bla_cache(out))
    return tuple(out)


# ---- the kernel against the model ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(SPECS))
def test_the_kernel_is_the_model(fr, native, lib, torch, name):
    v = B.view(fr.Config.new, *SPECS[name])
    want = M.model(v)
    escaped_with_skips = int(((want[1] < v.cfg.iterations) & (want[4] > 0)).sum())
    if name == "early-escape":
        assert not want[4].any()  # CLAIM 2's view: no pass skips, so the arrays are also DE's on plain PT
        assert_rows(want[:3], D.pt_rows_on(v.cfg, v.x, v.k), "the model on a view without skips")
    elif name == "N":
        assert (want[1] == v.cfg.iterations).all() and want[4].sum() > 0
    else:
        assert escaped_with_skips > 0, "a view whose escaped pixels never skip checks no skipped derivative"
    bz, bit = bla_rows(lib, native, v)
    assert np.array_equal(bit, want[1]) and B.same_bits(bz, want[0]), "CLAIM 1: z and iters are fr_escape_rows_pt_bla's"
    assert_rows(host_rows(lib, native, v), want, name + ", host arrays")
    r = device_rows(lib, native, torch, v)
    assert_rows(r.get(), want, name + ", device arrays")
    # DE's distance over the arrays, on the device
    dist = Buf(torch, 8 * r.n)
    check(lib.fr_distance_rows_device(C.byref(v.cfg), r.z.ptr, r.it.ptr, r.der.ptr, r.n, dist.ptr, None))
    want_d = D.distance(v.cfg, *want[:3])
    assert D.same_doubles(dist.get(np.float64, r.shape), want_d), "%s: D differs" % name
    if name == "N":
        assert (want_d == 0.0).all()
    else:
        assert (want_d > 0.0).sum() >= 100


def test_row_pieces_equal_the_slices_of_the_whole(fr, native, lib, torch):
    v = B.view(fr.Config.new, *B.M_37)  # ragged edges, more than one workgroup on both axes
    want = M.model(v)
    for y0, y1 in ((0, 8), (8, 13), (13, 21), (20, 21)):
        assert_rows(device_rows(lib, native, torch, v, 0, y0, y1).get(), tuple(a[y0:y1] for a in want[:3]), "rows [%d, %d)" % (y0, y1))
        assert_rows(host_rows(lib, native, v, 0, y0, y1), tuple(a[y0:y1] for a in want[:3]), "host rows [%d, %d)" % (y0, y1))
    assert cache(lib)[3] == 0  # D is the image's: every piece is served from one table
    r = Rows(torch, 2, v.cfg.width)
    lo, centre, _keep = v.args(native)
    check(lib.fr_escape_rows_de_pt_bla_device(C.byref(v.cfg), lo, centre, 0, 7, 7, r.z.ptr, r.it.ptr, r.der.ptr, None))
    assert r.z.untouched() and r.it.untouched() and r.der.untouched()


@pytest.mark.parametrize("bits", [24, 40, 53])
def test_bits(fr, native, lib, torch, bits):
    v = B.view(fr.Config.new, *B.M_16)
    want = M.model(v, bits)
    assert_rows(device_rows(lib, native, torch, v, bits).get(), want, "%d bits" % bits)
    assert cache(lib)[0] == bits
    if bits != 40:
        assert int(want[4].sum()) != int(M.model(v, 40)[4].sum())  # other radii, other skips


@pytest.mark.parametrize("name", ["M-37x21", "J", "seahorse"])
@pytest.mark.parametrize("cap", [0, 1])
def test_caps_zero_and_one(fr, native, lib, torch, name, cap):
    v = B.view(fr.Config.new, *SPECS[name])
    cfg = fr.Config.from_buffer_copy(bytes(v.cfg))
    cfg.iterations = cap
    if v.kind == "wide":
        orbits = W.Orbits(cfg, *v.ints, v.n)
        x, k = orbits.x[0], orbits.k[0] if cfg.algo == 2 else None
    else:
        import pt_model as P

        x, k = P.reference_orbit(cfg, v.pos_lo, 0), None
    want = M.escape_rows(cfg, x, k)
    assert not want[4].any()
    assert_rows(want[:3], D.pt_rows_on(cfg, x, k), "the model at cap %d" % cap)  # an empty table: DE's on plain PT
    if cap == 0:
        assert not want[1].any() and (want[2] == [1.0, 0.0]).all()
    assert_rows(device_rows(lib, native, torch, v, cfg=cfg).get(), want, "%s at cap %d" % (name, cap))
    assert_rows(host_rows(lib, native, v, cfg=cfg), want, "%s at cap %d, host" % (name, cap))


def test_an_algorithm_without_orbits_writes_zeros(fr, native, lib, torch):
    cfg = fr.Config.new(fr.Algo.BarnsleyFern)
    cfg.width, cfg.height, cfg.iterations = 20, 9, 50
    r = Rows(torch, 9, 20)
    check(lib.fr_escape_rows_de_pt_bla_device(C.byref(cfg), None, None, 0, 0, 9, r.z.ptr, r.it.ptr, r.der.ptr, None))
    z, it, der = r.get()
    assert not z.any() and not it.any() and not der.any()
    z, der = np.full((9, 20, 2), np.nan), np.full((9, 20, 2), np.nan)
    it = np.full((9, 20), 7, dtype=np.uint32)
    check(lib.fr_escape_rows_de_pt_bla(C.byref(cfg), None, None, 0, 0, 9, z.ctypes.data, it.ctypes.data, der.ctypes.data))
    assert not z.any() and not it.any() and not der.any()


# ---- DE's colour map over the arrays ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["M-37x21", "J", "seahorse"])
def test_thickness_zero_is_the_bla_render(fr, native, lib, torch, name):
    v = B.view(fr.Config.new, *SPECS[name])
    h, w = v.shape
    lo, centre, _keep = v.args(native)
    r = device_rows(lib, native, torch, v)
    want = M.model(v)
    for channels in (3, 4):
        n = channels * r.n
        render, colour, shaded = Buf(torch, n), Buf(torch, n), Buf(torch, n)
        check(lib.fr_render_rows_pt_bla_device(C.byref(v.cfg), lo, centre, 0, 0, h, channels, render.ptr, n, None))
        check(lib.fr_colour_de_rows_device(C.byref(v.cfg), r.z.ptr, r.it.ptr, r.der.ptr, r.n, 0.0, channels, colour.ptr, None))
        check(lib.fr_colour_de_rows_device(C.byref(v.cfg), r.z.ptr, r.it.ptr, r.der.ptr, r.n, 2.0, channels, shaded.ptr, None))
        a, b = render.get(np.uint8, (h, w, channels)), colour.get(np.uint8, (h, w, channels))
        assert np.array_equal(a, b) and len(np.unique(a.reshape(-1, channels), axis=0)) > 1
        assert np.array_equal(shaded.get(np.uint8, (h, w, channels)), D.colour(v.cfg, *want[:3], 2.0, channels))


# ---- the caches, the profiling name ----------------------------------------------------------------------------------------


def test_the_table_is_shared_with_the_bla_calls(fr, native, lib, torch):
    v = B.view(fr.Config.new, *B.M_16)
    other = B.view(fr.Config.new, *B.M_37)
    bla_rows(lib, native, other)  # whatever came before, this is another view
    z, it = bla_rows(lib, native, v)
    built = cache(lib)
    assert built[0] == 40 and built[3] == 1
    assert_rows(host_rows(lib, native, v), M.model(v), "DE after BLA-PT")
    assert cache(lib) == built[:3] + (0,), "the DE call of the same view and bits is served from the cached table"
    # PT of the same view in between: PT's bytes stay PT's, and the table is still served
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    pz, pit = fr.escape_rows(v.cfg, precision=fr.Precision.PT, centre=centre)
    assert np.array_equal(pit, v.pt[1]) and B.same_bits(pz, v.pt[0])
    assert_rows(device_rows(lib, native, torch, v).get(), M.model(v), "DE after PT")
    assert cache(lib) == built[:3] + (0,)
    # and the other way round: a table the DE call built serves the BLA-PT call
    assert_rows(host_rows(lib, native, v, 53), M.model(v, 53), "other bits")
    assert cache(lib)[0] == 53 and cache(lib)[3] == 1
    z, it = bla_rows(lib, native, v, 53)
    assert cache(lib)[3] == 0 and np.array_equal(it, v.model(53)[1]) and B.same_bits(z, v.model(53)[0])


def test_profiling_names_the_kernel(fr, native, lib, torch):
    check(lib.fr_set_profiling(1))
    try:
        for spec in (B.M_16, B.J_48):
            device_rows(lib, native, torch, B.view(fr.Config.new, *spec))
            torch.cuda.synchronize()
            buf = C.create_string_buffer(128)
            check(lib.fr_last_kernel_name(buf, 128))
            assert buf.value == b"escape_bla_de_kernel"
    finally:
        check(lib.fr_set_profiling(0))


# ---- the mirrors -----------------------------------------------------------------------------------------------------------


def c_image(lib, native, v, thickness, bits=0, cfg=None):
    cfg = v.cfg if cfg is None else cfg
    z, it, der = host_rows(lib, native, v, bits, cfg=cfg)
    rgb = np.empty(it.shape + (3,), dtype=np.uint8)
    check(lib.fr_colour_de_rgb8(C.byref(cfg), z.ctypes.data, it.ctypes.data, der.ctypes.data, it.size, thickness, rgb.ctypes.data, rgb.nbytes))
    return rgb


def test_python_bla_keyword_gives_the_c_calls_bytes(fr, native, lib, torch):
    v = B.view(fr.Config.new, *B.M_37)
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    kw = dict(precision=fr.Precision.PT, centre=centre)
    assert_rows(fr.escape_rows_de(v.cfg, bla=0, **kw), M.model(v), "escape_rows_de")
    assert_rows(fr.escape_rows_de(v.cfg, 4, 9, bla=24, **kw), tuple(a[4:9] for a in M.model(v, 24)[:3]), "rows and bits")
    want = c_image(lib, native, v, 1.5)
    assert np.array_equal(want, D.colour(v.cfg, *M.model(v)[:3], 1.5))
    assert np.array_equal(fr.get_image_de(v.cfg, 1.5, bla=0, **kw), want)
    assert np.array_equal(fr.get_image_de(v.cfg, 1.5, bla=40, **kw), want)
    assert (want != fr.get_image(v.cfg, bla=0, **kw)).any(-1).sum() >= 20  # the shading does change this view
    r = Rows(torch, *v.shape)
    fr.escape_rows_de_device(v.cfg, r.z.ptr, r.it.ptr, r.der.ptr, bla=0, **kw)
    assert_rows(r.get(), M.model(v), "escape_rows_de_device")
    # the (pos, pos_lo) road
    s = B.view(fr.Config.new, *B.SEAHORSE)
    assert_rows(fr.escape_rows_de(s.cfg, precision=fr.Precision.PT, pos_lo=s.pos_lo, bla=0), M.model(s), "pos_lo")
    assert np.array_equal(fr.get_image_de(s.cfg, 2.0, precision=fr.Precision.PT, pos_lo=s.pos_lo, bla=0), c_image(lib, native, s, 2.0))


def test_cpp_overload_gives_the_c_calls_bytes(fr, native, lib, tmp_path):
    from test_gpu_bla import compile_cpp, decimal_centre

    exe = os.path.join(ROOT, "tests", "cpp", "test_de_bla")
    compile_cpp(os.path.join(ROOT, "tests", "cpp", "test_de_bla.cpp"), exe)
    tre, tim, centre = decimal_centre(fr, "M", 140, 2.0 ** 300)
    cfg = W.view(fr.Config.new(), "M", 300, 37, 21, 5000)
    out = str(tmp_path / "image.rgb")
    r = subprocess.run([exe, tre, tim, "300", "37", "21", "5000", "24", "1.5", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.uint8).reshape(21, 37, 3)
    st = centre.c_struct()
    z, der = np.empty((21, 37, 2)), np.empty((21, 37, 2))
    it = np.empty((21, 37), dtype=np.uint32)
    check(lib.fr_escape_rows_de_pt_bla(C.byref(cfg), None, C.byref(st), 24, 0, 21, z.ctypes.data, it.ctypes.data, der.ctypes.data))
    want = np.empty((21, 37, 3), dtype=np.uint8)
    check(lib.fr_colour_de_rgb8(C.byref(cfg), z.ctypes.data, it.ctypes.data, der.ctypes.data, it.size, 1.5, want.ctypes.data, want.nbytes))
    assert np.array_equal(got, want) and len(np.unique(want.reshape(-1, 3), axis=0)) > 1
