"""SCALED PT on the device (include/fractal_hip.h, fr_precision: "SCALED PT"; the fr_*_pt_scaled calls; kernels
escape_pt_scaled_kernel and escape_bla_scaled_kernel):
  - inside WIDE PT's domain, bit for bit against the existing roads ON THE DEVICE: bits = -1 against fr_escape_rows_pt_wide,
    bits = 40 against fr_escape_rows_pt_bla with a centre;
  - past the 2^440 edge, z and iters bit for bit against tests/pt_scaled_model.py (orbits from pt_wide_model's integers, the
    table and the pixel loops restated in tests/pt_scaled_model.c): the Misiurewicz point at 2^900 on 37 x 21 pixels (ragged
    against the 16 x 16 workgroup), the Julia fixed point at 2^900, a period-267 minibrot at 2^861; both loops; guard bytes
    around every device buffer;
  - row pieces against the whole (Dw is the image's), host forms against device forms;
  - RGB and RGBA renders against fr_colour_rgb8 over the scaled escape rows;
  - fr_debug_pt_scaled_count against the model's passes and steps;
  - the orbit cache shared with the wide road, the table slot shared with BLA-PT, the kernels' names."""
import ctypes as C

import numpy as np
import pytest

import pt_scaled_model as S

pytestmark = pytest.mark.gpu

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


def scaled_rows(lib, native, v, bits, y0=0, y1=None, cfg=None):
    """the host form"""
    cfg = v.cfg if cfg is None else cfg
    y1 = cfg.height if y1 is None else y1
    st = v.centre(native)
    z = np.full((y1 - y0, cfg.width, 2), np.nan)
    it = np.full((y1 - y0, cfg.width), 0xFFFFFFFF, dtype=np.uint32)
    check(lib.fr_escape_rows_pt_scaled(C.byref(cfg), C.byref(st), bits, y0, y1, z.ctypes.data, it.ctypes.data))
    return z, it


def scaled_rows_device(lib, native, torch, v, bits, y0=0, y1=None):
    """the device form into guarded buffers"""
    y1 = v.cfg.height if y1 is None else y1
    npx = (y1 - y0) * v.cfg.width
    st = v.centre(native)
    zb = torch.full((GUARD + 16 * npx + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ib = torch.full((GUARD + 4 * npx + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    check(lib.fr_escape_rows_pt_scaled_device(C.byref(v.cfg), C.byref(st), bits, y0, y1, zb.data_ptr() + GUARD, ib.data_ptr() + GUARD,
                                              None))
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


def kernel_name(lib):
    buf = C.create_string_buffer(128)
    check(lib.fr_last_kernel_name(buf, len(buf)))
    return buf.value.decode()


# ---- 1. inside the old domain: the existing roads, on the device ------------------------------------------------------------

INSIDE = {"M-2^200": S.M_200, "M-2^440-37x21": S.M_440, "N": S.N_300, "J": S.J_300}


@pytest.mark.parametrize("name", list(INSIDE))
def test_inside_wide_pts_domain_the_scaled_road_is_the_existing_roads(fr, native, lib, name):
    v = S.view(fr.Config.new, INSIDE[name])
    st = v.centre(native)
    h, w = v.shape
    z = np.full((h, w, 2), np.nan)
    it = np.full((h, w), 0xFFFFFFFF, dtype=np.uint32)
    check(lib.fr_escape_rows_pt_wide(C.byref(v.cfg), C.byref(st), 0, h, z.ctypes.data, it.ctypes.data))
    assert_rows(scaled_rows(lib, native, v, -1), (z, it), name + ": bits = -1 against fr_escape_rows_pt_wide")
    assert_rows((z, it), v.model()[:2], name + ": fr_escape_rows_pt_wide against the scaled model")
    zb = np.full((h, w, 2), np.nan)
    itb = np.full((h, w), 0xFFFFFFFF, dtype=np.uint32)
    check(lib.fr_escape_rows_pt_bla(C.byref(v.cfg), None, C.byref(st), 40, 0, h, zb.ctypes.data, itb.ctypes.data))
    assert_rows(scaled_rows(lib, native, v, 40), (zb, itb), name + ": bits = 40 against fr_escape_rows_pt_bla")


# ---- 2. past the edge: the model ----------------------------------------------------------------------------------------------

PAST = {"M-2^900-37x21": S.M_900, "J-2^900": S.J_900, "minibrot-2^861": S.MINI_861}


@pytest.mark.parametrize("bits", [-1, 40])
@pytest.mark.parametrize("name", list(PAST))
def test_past_the_edge_the_kernels_are_the_model(fr, native, lib, torch, name, bits):
    v = S.view(fr.Config.new, PAST[name])
    want = v.model(bits)
    assert len(np.unique(want[1])) > 10  # structure, not a flat image
    if bits >= 0:
        assert int(want[2].astype(np.uint64).sum()) < S.steps(v.cfg, want[1])  # the table is applied
    assert_rows(scaled_rows_device(lib, native, torch, v, bits), want, "%s, bits %d, device arrays" % (name, bits))
    assert_rows(scaled_rows(lib, native, v, bits), want, "%s, bits %d, host arrays" % (name, bits))  # 4. the forms agree


# ---- 3. row pieces ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("bits", [-1, 40])
def test_row_pieces_equal_the_slices_of_the_whole(fr, native, lib, torch, bits):
    v = S.view(fr.Config.new, S.M_900)  # ragged edges, more than one workgroup on both axes
    want = v.model(bits)
    for y0, y1 in ((5, 12), (0, 5), (5, 21)):
        assert_rows(scaled_rows_device(lib, native, torch, v, bits, y0, y1), (want[0][y0:y1], want[1][y0:y1]),
                    "rows [%d, %d), bits %d" % (y0, y1, bits))
    if bits >= 0:
        assert fr.bla_cache()[3] == 0  # Dw is the image's: every piece is served from one table


def test_only_one_array(fr, native, lib):
    v = S.view(fr.Config.new, S.J_900)
    st = v.centre(native)
    z = np.empty(v.shape + (2,))
    it = np.empty(v.shape, dtype=np.uint32)
    check(lib.fr_escape_rows_pt_scaled(C.byref(v.cfg), C.byref(st), 40, 0, v.shape[0], z.ctypes.data, None))
    check(lib.fr_escape_rows_pt_scaled(C.byref(v.cfg), C.byref(st), 40, 0, v.shape[0], None, it.ctypes.data))
    assert_rows((z, it), v.model(40), "z alone, iters alone")


# ---- 5. colours -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,bits", [("M-2^900-37x21", -1), ("M-2^900-37x21", 40), ("J-2^900", 40)])
@pytest.mark.parametrize("smooth", [1, 0])
def test_renders_are_the_colour_map_over_the_escape_rows(fr, native, lib, torch, name, bits, smooth):
    v = S.view(fr.Config.new, PAST[name])
    cfg = fr.Config.from_buffer_copy(bytes(v.cfg))
    cfg.smooth, cfg.exposure = smooth, 3.0
    h, w = v.shape
    st = v.centre(native)
    z, it = scaled_rows(lib, native, v, bits, cfg=cfg)
    assert_rows((z, it), v.model(bits), name)
    want = fr.colour_image(cfg, z, it)
    assert len(np.unique(it)) > 5 and len(np.unique(want.reshape(-1, 3), axis=0)) > 1  # not a flat view (15 and 42 indices)
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    check(lib.fr_render_rows_pt_scaled(C.byref(cfg), C.byref(st), bits, 0, h, 3, rgb.ctypes.data, rgb.nbytes))
    assert np.array_equal(rgb, want)
    rgba = np.zeros((h, w, 4), dtype=np.uint8)
    check(lib.fr_render_rows_pt_scaled(C.byref(cfg), C.byref(st), bits, 0, h, 4, rgba.ctypes.data, rgba.nbytes))
    assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all()
    for channels in (3, 4):
        n = channels * w * h
        buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        check(lib.fr_render_rows_pt_scaled_device(C.byref(cfg), C.byref(st), bits, 0, h, channels, buf.data_ptr() + GUARD, n, None))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:GUARD] == 0xA5).all() and (got[GUARD + n:] == 0xA5).all()
        img = got[GUARD:GUARD + n].reshape(h, w, channels)
        assert np.array_equal(img[..., :3], want) and (channels == 3 or (img[..., 3] == 255).all())
    # rows [3, 11) into the device form
    n = 3 * w * 8
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    check(lib.fr_render_rows_pt_scaled_device(C.byref(cfg), C.byref(st), bits, 3, 11, 3, buf.data_ptr(), n, None))
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().reshape(8, w, 3), want[3:11])
    # a misaligned RGBA destination and a short buffer are refused
    out = torch.zeros(4 * w * h + 4, dtype=torch.uint8, device="cuda:0")
    assert lib.fr_render_rows_pt_scaled_device(C.byref(cfg), C.byref(st), bits, 0, h, 4, out.data_ptr() + 1, 4 * w * h, None) == 1
    assert lib.fr_render_rows_pt_scaled_device(C.byref(cfg), C.byref(st), bits, 0, h, 4, out.data_ptr(), 4 * w * h - 1, None) != 0


def test_the_python_road(fr, native, lib):
    v = S.view(fr.Config.new, S.M_900)
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    PT = fr.Precision.PT
    assert_rows(fr.escape_rows(v.cfg, precision=PT, centre=centre, scaled=True), v.model(), "scaled=True")
    z, it = fr.escape_rows(v.cfg, precision=PT, centre=centre, bla=0, scaled=True)
    assert_rows((z, it), v.model(40), "scaled=True, bla=0")
    want = fr.colour_image(v.cfg, z, it)
    assert np.array_equal(fr.get_image(v.cfg, PT, centre=centre, bla=40, scaled=True), want)
    assert np.array_equal(fr.get_image_rows(v.cfg, 2, 9, PT, centre=centre, bla=40, scaled=True), want[2:9])
    rgba = fr.get_image_rgba(v.cfg, PT, centre=centre, bla=40, scaled=True)
    assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all()
    inside = S.view(fr.Config.new, S.M_200)  # the same bytes as the call without scaled=
    c2 = fr.WideCentre(inside.n, re=inside.words[0], im=inside.words[1])
    assert np.array_equal(fr.get_image(inside.cfg, PT, centre=c2, scaled=True), fr.get_image(inside.cfg, PT, centre=c2))


def test_an_algorithm_without_orbits_is_black(fr, native, lib):
    v = S.view(fr.Config.new, S.M_900)
    cfg = fr.Config.from_buffer_copy(bytes(v.cfg))
    cfg.algo = int(fr.Algo.BarnsleyFern)
    for bits in (-1, 40):
        z, it = scaled_rows(lib, native, v, bits, cfg=cfg)
        assert (z == 0).all() and (it == 0).all()


# ---- 6. the counts ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("bits", [-1, 40])
@pytest.mark.parametrize("name", list(PAST))
def test_the_counts_are_the_models(fr, native, lib, name, bits):
    v = S.view(fr.Config.new, PAST[name])
    z, it, passes, _ = v.model(bits)
    st = v.centre(native)
    a, b = C.c_uint64(0), C.c_uint64(0)
    check(lib.fr_debug_pt_scaled_count(C.byref(v.cfg), C.byref(st), bits, 0, v.shape[0], C.byref(a), C.byref(b)))
    assert (a.value, b.value) == (int(passes.astype(np.uint64).sum()), S.steps(v.cfg, it))
    check(lib.fr_debug_pt_scaled_count(C.byref(v.cfg), C.byref(st), bits, 2, 9, C.byref(a), C.byref(b)))
    assert (a.value, b.value) == (int(passes[2:9].astype(np.uint64).sum()), S.steps(v.cfg, it[2:9]))
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    assert fr.pt_scaled_count(v.cfg, centre, 2, 9, bla=None if bits < 0 else bits) == (a.value, b.value)


# ---- 7. the caches ---------------------------------------------------------------------------------------------------------------


def test_a_wide_call_is_served_the_orbit_of_a_scaled_call_and_back(fr, native, lib):
    v = S.view(fr.Config.new, S.M_300)
    other = S.view(fr.Config.new, S.N_300)
    st = v.centre(native)
    h, w = v.shape
    scaled_rows(lib, native, other, -1)  # whatever came before, this is another view
    assert_rows(scaled_rows(lib, native, v, -1), v.model(), "scaled first")
    assert fr.pt_orbit_cache() == (v.cfg.iterations, len(v.x), 0, len(v.x))  # computed by the scaled call
    z = np.empty((h, w, 2))
    it = np.empty((h, w), dtype=np.uint32)
    check(lib.fr_escape_rows_pt_wide(C.byref(v.cfg), C.byref(st), 0, h, z.ctypes.data, it.ctypes.data))
    assert fr.pt_orbit_cache() == (v.cfg.iterations, len(v.x), 0, 0)  # served, not recomputed
    assert_rows((z, it), v.model(), "wide after scaled")
    scaled_rows(lib, native, v, 40)
    assert fr.pt_orbit_cache()[3] == 0  # and the other way round


def test_the_table_slot_tells_a_scaled_table_from_bla_pts(fr, native, lib):
    v = S.view(fr.Config.new, S.M_300)
    st = v.centre(native)
    h, w = v.shape
    levels = (len(v.x) - 2).bit_length()
    entries = 2 * (len(v.x) - 2) - bin(len(v.x) - 2).count("1")
    scaled_rows(lib, native, S.view(fr.Config.new, S.N_300), 40)
    want = v.model(40)
    assert_rows(scaled_rows(lib, native, v, 40), want, "scaled table, first")
    assert fr.bla_cache() == (40, levels, entries, 1)
    assert_rows(scaled_rows(lib, native, v, 40, 3, 7), (want[0][3:7], want[1][3:7]), "scaled table, served")
    assert fr.bla_cache() == (40, levels, entries, 0)
    z = np.empty((h, w, 2))
    it = np.empty((h, w), dtype=np.uint32)
    check(lib.fr_escape_rows_pt_bla(C.byref(v.cfg), None, C.byref(st), 40, 0, h, z.ctypes.data, it.ctypes.data))
    assert fr.bla_cache() == (40, levels, entries, 1)  # same orbit, same bits: still another table
    assert_rows((z, it), want, "BLA-PT after the scaled table")
    assert_rows(scaled_rows(lib, native, v, 40), want, "the scaled table after BLA-PT's")
    assert fr.bla_cache()[3] == 1
    assert_rows(scaled_rows(lib, native, v, -1), v.model(), "no table")  # leaves the slot alone
    assert fr.bla_cache() == (40, levels, entries, 1)


# ---- 8. the names ------------------------------------------------------------------------------------------------------------------


def test_kernel_names(fr, native, lib, torch):
    v = S.view(fr.Config.new, S.J_900)
    check(lib.fr_set_profiling(1))
    try:
        scaled_rows_device(lib, native, torch, v, -1)
        assert kernel_name(lib) == "escape_pt_scaled_kernel"
        ms = C.c_float(-1.0)
        check(lib.fr_last_kernel_ms(C.byref(ms)))
        assert ms.value > 0.0
        scaled_rows_device(lib, native, torch, v, 40)
        assert kernel_name(lib) == "escape_bla_scaled_kernel"
    finally:
        check(lib.fr_set_profiling(0))
