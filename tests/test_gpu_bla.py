"""BLA-PT on the device (include/fractal_hip.h, fr_precision: "BLA-PT"; the fr_*_pt_bla calls; kernel escape_bla_kernel),
bit for bit against tests/bla_model.py — orbits from the PT models, the table and the pixel loop restated in
tests/bla_model.c:
  - z and iters of the Misiurewicz centre at 2^300 (16 x 12; 37 x 21 whole and in row pieces) and at 2^440, the edge of the
    domain; the period-3 nucleus, whose pixels all run to the cap; the Julia fixed point, with two tables; the seahorse dd
    view with pos_lo; an orbit of 31 entries met again and again; a Julia view that changes tables; 24, 40 and 53 bits;
    guard bytes around every device buffer;
  - RGB and RGBA renders, host and device forms, against fr_colour_rgb8 over the BLA escape rows;
  - fr_debug_bla_count against the model's passes and steps;
  - the table cache: built once per view, rebuilt for other bits or another size, undisturbed by PT calls in between;
  - the Python bla= road, the C++ overload and the CLI against the C call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bla_model as B
import oracle_lib as O
import pt_wide_model as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


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


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def escape_rows(lib, native, v, bits=0, y0=0, y1=None, cfg=None):
    cfg = v.cfg if cfg is None else cfg
    y1 = cfg.height if y1 is None else y1
    lo, centre, _keep = v.args(native)
    z = np.full((y1 - y0, cfg.width, 2), np.nan)
    it = np.full((y1 - y0, cfg.width), 0xFFFFFFFF, dtype=np.uint32)
    check(lib.fr_escape_rows_pt_bla(C.byref(cfg), lo, centre, bits, y0, y1, z.ctypes.data, it.ctypes.data))
    return z, it


def escape_rows_device(lib, native, torch, v, bits=0, y0=0, y1=None):
    """the device form into guarded buffers"""
    y1 = v.cfg.height if y1 is None else y1
    npx = (y1 - y0) * v.cfg.width
    lo, centre, _keep = v.args(native)
    zb = torch.full((GUARD + 16 * npx + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ib = torch.full((GUARD + 4 * npx + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    check(lib.fr_escape_rows_pt_bla_device(C.byref(v.cfg), lo, centre, bits, y0, y1, zb.data_ptr() + GUARD, ib.data_ptr() + GUARD, None))
    torch.cuda.synchronize()
    zh, ih = zb.cpu().numpy(), ib.cpu().numpy()
    for h, n in ((zh, 16 * npx), (ih, 4 * npx)):
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all(), "a write outside the array"
    z = zh[GUARD:GUARD + 16 * npx].copy().view(np.float64).reshape(y1 - y0, v.cfg.width, 2)
    it = ih[GUARD:GUARD + 4 * npx].copy().view(np.uint32).reshape(y1 - y0, v.cfg.width)
    return z, it


def assert_rows(got, want, what):
    assert np.array_equal(got[1], want[1]), "%s: escape indices differ at %d pixels" % (what, int((got[1] != want[1]).sum()))
    assert np.array_equal(bits_of(got[0]), bits_of(want[0])), "%s: z differs at %d doubles" % (
        what, int((bits_of(got[0]) != bits_of(want[0])).sum()))


def cache(lib):
    out = (C.c_uint32 * 4)()
    check(lib.fr_debug_bla_cache(out))
    return tuple(out)


# ---- the kernel against the model ------------------------------------------------------------------------------------------

SPECS = {"M-16x12": B.M_16, "M-37x21": B.M_37, "M-2^440": B.M_DEEP, "N": B.N_16, "J": B.J_48, "seahorse": B.SEAHORSE,
         "early-escape": B.EARLY, "julia-rebase": B.JULIA_REBASE}


@pytest.mark.parametrize("name", list(SPECS))
def test_the_kernel_is_the_model(fr, native, lib, torch, name):
    v = B.view(fr.Config.new, *SPECS[name])
    want = v.model()
    skipped = B.steps(v.cfg, want[1]) - int(want[2].sum())
    if name == "early-escape":  # a shallow view: |dz| ~ 2^-6 against radii of 2^-38, so every pass is a plain step and the
        assert skipped == 0 and B.same_bits(want[0], v.pt[0])  # search must refuse at every j; pixels meet m == last over and over
    else:
        assert skipped > 0, "a view on which the model never skips checks no table"
    assert_rows(escape_rows(lib, native, v), want, name + ", host arrays")
    assert_rows(escape_rows_device(lib, native, torch, v), want, name + ", device arrays")


def test_row_pieces_equal_the_slices_of_the_whole(fr, native, lib, torch):
    v = B.view(fr.Config.new, *B.M_37)  # ragged edges, more than one workgroup on both axes
    want = v.model()
    for y0, y1 in ((0, 8), (8, 13), (13, 21), (20, 21)):
        assert_rows(escape_rows_device(lib, native, torch, v, 0, y0, y1), (want[0][y0:y1], want[1][y0:y1]), "rows [%d, %d)" % (y0, y1))
    assert cache(lib)[3] == 0  # D is the image's: every piece is served from one table


@pytest.mark.parametrize("bits", [24, 40, 53])
def test_bits(fr, native, lib, bits):
    v = B.view(fr.Config.new, *B.M_16)
    want = v.model(bits)
    assert_rows(escape_rows(lib, native, v, bits), want, "%d bits" % bits)
    assert cache(lib)[0] == bits
    if bits != 40:
        assert int(want[2].sum()) != int(v.model(40)[2].sum())  # other radii, other skips


def test_only_one_array(fr, native, lib):
    v = B.view(fr.Config.new, *B.M_16)
    lo, centre, _keep = v.args(native)
    z = np.empty(v.shape + (2,))
    it = np.empty(v.shape, dtype=np.uint32)
    check(lib.fr_escape_rows_pt_bla(C.byref(v.cfg), lo, centre, 0, 0, v.shape[0], z.ctypes.data, None))
    check(lib.fr_escape_rows_pt_bla(C.byref(v.cfg), lo, centre, 0, 0, v.shape[0], None, it.ctypes.data))
    assert_rows((z, it), v.model(), "z alone, iters alone")


def test_an_algorithm_without_orbits_is_black(fr, native, lib):
    cfg = fr.Config.new(fr.Algo.BarnsleyFern)
    cfg.width, cfg.height, cfg.iterations = 20, 9, 50
    z = np.full((9, 20, 2), np.nan)
    it = np.full((9, 20), 7, dtype=np.uint32)
    check(lib.fr_escape_rows_pt_bla(C.byref(cfg), None, None, 0, 0, 9, z.ctypes.data, it.ctypes.data))
    assert (z == 0).all() and (it == 0).all()
    assert (fr.get_image(cfg, fr.Precision.PT, bla=0) == 0).all()


# ---- colours -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["M-37x21", "J", "seahorse"])
@pytest.mark.parametrize("smooth", [1, 0])
def test_renders_are_the_colour_map_over_the_escape_rows(fr, native, lib, torch, name, smooth):
    v = B.view(fr.Config.new, *SPECS[name])
    cfg = fr.Config.from_buffer_copy(bytes(v.cfg))
    cfg.smooth, cfg.exposure = smooth, 3.0
    h, w = v.shape
    lo, centre, _keep = v.args(native)
    z, it = escape_rows(lib, native, v, cfg=cfg)
    assert_rows((z, it), v.model(), name)
    want = fr.colour_image(cfg, z, it)
    assert len(np.unique(it)) > 5  # not a flat view (the model's counts: 16, 203 and 280 distinct indices)
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    check(lib.fr_render_rows_pt_bla(C.byref(cfg), lo, centre, 0, 0, h, 3, rgb.ctypes.data, rgb.nbytes))
    assert np.array_equal(rgb, want)
    rgba = np.zeros((h, w, 4), dtype=np.uint8)
    check(lib.fr_render_rows_pt_bla(C.byref(cfg), lo, centre, 0, 0, h, 4, rgba.ctypes.data, rgba.nbytes))
    assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all()
    for channels in (3, 4):
        n = channels * w * h
        buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        check(lib.fr_render_rows_pt_bla_device(C.byref(cfg), lo, centre, 0, 0, h, channels, buf.data_ptr() + GUARD, n, None))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:GUARD] == 0xA5).all() and (got[GUARD + n:] == 0xA5).all()
        img = got[GUARD:GUARD + n].reshape(h, w, channels)
        assert np.array_equal(img[..., :3], want) and (channels == 3 or (img[..., 3] == 255).all())
    # rows [3, 11) into the device form, and the device colour map over device escape rows
    n = 3 * w * 8
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    check(lib.fr_render_rows_pt_bla_device(C.byref(cfg), lo, centre, 0, 3, 11, 3, buf.data_ptr(), n, None))
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().reshape(8, w, 3), want[3:11])
    dz = torch.zeros(2 * w * h, dtype=torch.float64, device="cuda:0")
    di = torch.zeros(w * h, dtype=torch.int32, device="cuda:0")
    out = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda:0")
    check(lib.fr_escape_rows_pt_bla_device(C.byref(cfg), lo, centre, 0, 0, h, dz.data_ptr(), di.data_ptr(), None))
    check(lib.fr_colour_rows_device(C.byref(cfg), dz.data_ptr(), 2, di.data_ptr(), w * h, 4, out.data_ptr(), 4 * w * h, None))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(h, w, 4)[..., :3], want)
    # a misaligned RGBA destination is refused
    assert lib.fr_render_rows_pt_bla_device(C.byref(cfg), lo, centre, 0, 0, h, 4, out.data_ptr() + 1, 4 * w * h, None) == 1


# ---- the counts ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["M-37x21", "N", "J", "seahorse", "early-escape"])
def test_the_counts_are_the_models(fr, native, lib, name):
    v = B.view(fr.Config.new, *SPECS[name])
    z, it, passes = v.model()
    lo, centre, _keep = v.args(native)
    a, b = C.c_uint64(0), C.c_uint64(0)
    check(lib.fr_debug_bla_count(C.byref(v.cfg), lo, centre, 0, 0, v.shape[0], C.byref(a), C.byref(b)))
    assert (a.value, b.value) == (int(passes.astype(np.uint64).sum()), B.steps(v.cfg, it))
    check(lib.fr_debug_bla_count(C.byref(v.cfg), lo, centre, 0, 2, 9, C.byref(a), C.byref(b)))
    assert (a.value, b.value) == (int(passes[2:9].astype(np.uint64).sum()), B.steps(v.cfg, it[2:9]))


# ---- the cache ------------------------------------------------------------------------------------------------------------


def test_the_table_is_built_once_per_view(fr, native, lib):
    v = B.view(fr.Config.new, *B.M_16)
    other = B.view(fr.Config.new, *B.M_37)
    levels = (len(v.x) - 2).bit_length()
    entries = 2 * (len(v.x) - 2) - bin(len(v.x) - 2).count("1")
    escape_rows(lib, native, other)  # whatever came before, this is another view
    assert_rows(escape_rows(lib, native, v), v.model(), "first")
    assert cache(lib) == (40, levels, entries, 1)
    assert_rows(escape_rows(lib, native, v, 0, 3, 7), tuple(a[3:7] for a in v.model()[:2]), "rows")
    assert cache(lib) == (40, levels, entries, 0)
    recoloured = fr.Config.from_buffer_copy(bytes(v.cfg))
    recoloured.exposure, recoloured.smooth = 2.0, 0
    lo, centre, _keep = v.args(native)
    rgb = np.zeros(v.shape + (3,), dtype=np.uint8)
    check(lib.fr_render_rows_pt_bla(C.byref(recoloured), lo, centre, 40, 0, v.shape[0], 3, rgb.ctypes.data, rgb.nbytes))
    assert cache(lib)[3] == 0  # colours do not enter the key, and bits = 0 is 40
    assert_rows(escape_rows(lib, native, v, 24), v.model(24), "other bits")
    assert cache(lib) == (24, levels, entries, 1)
    assert_rows(escape_rows(lib, native, v), v.model(), "back to 40")
    assert cache(lib)[3] == 1
    assert_rows(escape_rows(lib, native, other), other.model(), "another size: another D")
    assert cache(lib)[3] == 1
    j = B.view(fr.Config.new, *B.J_48)
    assert_rows(escape_rows(lib, native, j), j.model(), "Julia")
    nx, nk = len(j.x) - 2, len(j.k) - 2
    assert cache(lib) == (40, nx.bit_length(), 2 * nx - bin(nx).count("1") + 2 * nk - bin(nk).count("1"), 1)


def test_pt_and_bla_alternate_on_one_context(fr, native, lib):
    v = B.view(fr.Config.new, *B.M_16)
    s = B.view(fr.Config.new, *B.SEAHORSE)
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    assert_rows(escape_rows(lib, native, v), v.model(), "BLA")
    built = cache(lib)
    # PT of the same view between two BLA renders: PT's bytes stay PT's, and the table is served
    z, it = fr.escape_rows(v.cfg, precision=fr.Precision.PT, centre=centre)
    assert_rows((z, it), v.pt, "PT of the same view")
    assert_rows(escape_rows(lib, native, v), v.model(), "BLA again")
    assert cache(lib) == built[:3] + (0,)
    # PT of ANOTHER view in between replaces the orbit: BLA rebuilds, and both stay right
    z, it = fr.escape_rows(s.cfg, precision=fr.Precision.PT, pos_lo=s.pos_lo)
    assert_rows((z, it), s.pt, "PT of the seahorse view")
    assert_rows(escape_rows(lib, native, v), v.model(), "BLA after another view's PT")
    assert cache(lib)[3] == 1
    assert_rows(escape_rows(lib, native, s), s.model(), "BLA of the seahorse view")
    z, it = fr.escape_rows(s.cfg, precision=fr.Precision.PT, pos_lo=s.pos_lo)
    assert_rows((z, it), s.pt, "PT after BLA, same orbit")
    assert not np.array_equal(s.pt[1], s.model()[1])  # the two are different renders of this view


# ---- the mirrors ----------------------------------------------------------------------------------------------------------


def test_python_bla_road_gives_the_c_calls_bytes(fr, native, lib):
    v = B.view(fr.Config.new, *B.M_37)
    h, w = v.shape
    lo, c, _keep = v.args(native)
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    want = np.zeros((h, w, 3), dtype=np.uint8)
    check(lib.fr_render_rows_pt_bla(C.byref(v.cfg), lo, c, 0, 0, h, 3, want.ctypes.data, want.nbytes))
    assert np.array_equal(want, fr.colour_image(v.cfg, *v.model()[:2]))
    assert np.array_equal(fr.get_image(v.cfg, fr.Precision.PT, centre=centre, bla=0), want)
    assert np.array_equal(fr.get_image(v.cfg, fr.Precision.PT, centre=centre, bla=40), want)
    assert np.array_equal(fr.get_image_rows(v.cfg, 3, 17, fr.Precision.PT, centre=centre, bla=0), want[3:17])
    rgba = fr.get_image_rgba(v.cfg, fr.Precision.PT, centre=centre, bla=0)
    assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all()
    assert_rows(fr.escape_rows(v.cfg, precision=fr.Precision.PT, centre=centre, bla=0), v.model(), "escape_rows")
    assert_rows(fr.escape_rows(v.cfg, 4, 9, precision=fr.Precision.PT, centre=centre, bla=24),
                tuple(a[4:9] for a in v.model(24)[:2]), "escape_rows, rows and bits")
    assert fr.bla_count(v.cfg, centre=centre) == (int(v.model()[2].sum()), B.steps(v.cfg, v.model()[1]))
    assert fr.bla_cache()[0] == 40
    # the (pos, pos_lo) road
    s = B.view(fr.Config.new, *B.SEAHORSE)
    assert_rows(fr.escape_rows(s.cfg, precision=fr.Precision.PT, pos_lo=s.pos_lo, bla=0), s.model(), "pos_lo")
    img = fr.get_image(s.cfg, fr.Precision.PT, pos_lo=s.pos_lo, bla=0)
    assert np.array_equal(img, fr.colour_image(s.cfg, *s.model()[:2]))
    e = B.view(fr.Config.new, *B.EARLY)
    assert_rows(fr.escape_rows(e.cfg, precision=fr.Precision.PT, bla=0), e.model(), "no pos_lo")


def decimal_centre(fr, name, digits, scale):
    re, im = W.centre(name)
    tre, tim = W.decimal_text(re, digits), W.decimal_text(im, digits)
    return tre, tim, fr.WideCentre.from_str(tre, tim, scale=scale)


def compile_cpp(source, exe):
    import __graft_entry__ as ge

    ge.build()
    pkg = os.path.join(ROOT, "fractal-renderer_amd")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(pkg, "host"), source, "-L" + pkg, "-lfractal_hip", "-Wl,-rpath," + pkg, "-o", exe], check=True)


def test_cpp_overload_gives_the_c_calls_bytes(fr, native, lib, tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "test_bla")
    compile_cpp(os.path.join(ROOT, "tests", "cpp", "test_bla.cpp"), exe)
    tre, tim, centre = decimal_centre(fr, "M", 140, 2.0 ** 300)
    assert centre.words == 6
    cfg = W.view(fr.Config.new(), "M", 300, 37, 21, 5000)
    out = str(tmp_path / "image.rgb")
    r = subprocess.run([exe, tre, tim, "300", "37", "21", "5000", "24", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.uint8).reshape(21, 37, 3)
    st = centre.c_struct()
    want = np.zeros((21, 37, 3), dtype=np.uint8)
    check(lib.fr_render_rows_pt_bla(C.byref(cfg), None, C.byref(st), 24, 0, 21, 3, want.ctypes.data, want.nbytes))
    assert np.array_equal(got, want) and len(np.unique(want.reshape(-1, 3), axis=0)) > 1


def test_cli_bla_gives_the_c_calls_bytes(fr, native, lib, tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "fractal_cli")
    compile_cpp(os.path.join(ROOT, "fractal-renderer_amd", "cli", "fractal_cli.cpp"), exe)
    scale = 2.0 ** 300
    tre, tim, centre = decimal_centre(fr, "M", 140, scale)
    ocfg = O.cli_config(48, 32, scale=(scale, scale), iterations=5000, limit=2.0, pos=(float(tre), float(tim)))
    cfg = fr.Config.from_buffer_copy(bytes(ocfg))
    st = centre.c_struct()
    for flags, bits in ((["--bla"], 0), (["--bla=24"], 24)):
        out = str(tmp_path / ("deep%d" % bits))
        r = subprocess.run([exe, "--perturbation"] + flags + ["48", "32", "-x", tre, "-y", tim, "-s", repr(scale), "-i", "5000", "-l", "2",
                                                               "-o", out, "--quiet"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        data = open(out + ".ppm", "rb").read().split(b"\n", 3)
        assert data[0] == b"P6" and data[1] == b"48 32"
        got = np.frombuffer(data[3], dtype=np.uint8).reshape(32, 48, 3)
        want = np.zeros((32, 48, 3), dtype=np.uint8)
        check(lib.fr_render_rows_pt_bla(C.byref(cfg), None, C.byref(st), bits, 0, 32, 3, want.ctypes.data, want.nbytes))
        assert np.array_equal(got, want) and len(np.unique(want.reshape(-1, 3), axis=0)) > 1
    # --bla without --perturbation, and bits outside 24 .. 53, are refused
    r = subprocess.run([exe, "--bla", "4", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "--perturbation" in r.stderr
    r = subprocess.run([exe, "--perturbation", "--bla=23", "4", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "24 .. 53" in r.stderr
