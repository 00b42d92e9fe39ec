"""FR_PRECISION_DD on the device (fractal-renderer_amd/csrc/fr_dd.hip) against the host model tests/dd_model.c, bit for
bit: final positions (hi and lo parts), escape indices, RGB / RGBA bytes (the oracle's colour map over the model's hi
parts, libm log2), iteration counts; the entry points agree with each other; F64 renders are untouched by DD calls."""
import ctypes as C

import numpy as np
import pytest

import dd_model as M
import oracle_lib as O

pytestmark = pytest.mark.gpu

DD = 2
LO = (0.0, 2.0 ** -60)  # a normalised low part of the centre (0, 1): |LO| < half an ulp of 1


@pytest.fixture(scope="module")
def fr():
    import fractal_renderer_amd

    assert fractal_renderer_amd.device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    fractal_renderer_amd.init(0)
    assert fractal_renderer_amd.device_name().startswith("gfx950")
    return fractal_renderer_amd


def same_f64(a, b):
    """Bit-identical, zero signs included; any NaN matches any NaN (the platform picks the payload)."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(
        a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def view(fr, name, width=257, height=193, iterations=None):
    cfg = fr.Config.new()
    cfg.width, cfg.height = width, height
    if name == "default":
        cfg.iterations = 200 if iterations is None else iterations
    elif name == "default_julia":
        cfg.algo = 2
        cfg.iterations = 300 if iterations is None else iterations
        cfg.julia_set.re, cfg.julia_set.im = -0.8, 0.156
        cfg.scale.re = cfg.scale.im = 0.3
    else:
        M.deep_view(cfg, name == "deep_julia", width, height, 3000 if iterations is None else iterations)
    return cfg


def model_colours(fr, cfg, z4, it, rgba=False):
    ocfg = O.Config.from_buffer_copy(bytes(cfg))
    O.set_log2_mode(O.LOG2_LIBM)
    hi = np.ascontiguousarray(z4[..., 0::2])
    rgb = O.colour_rows(ocfg, hi, it)
    if not rgba:
        return rgb
    out = np.full(rgb.shape[:-1] + (4,), 255, dtype=np.uint8)
    out[..., :3] = rgb
    return out


CASES = [("default", None), ("default_julia", None), ("deep_mandelbrot", None), ("deep_mandelbrot", LO),
         ("deep_julia", None), ("deep_julia", LO)]


@pytest.mark.parametrize("name,pos_lo", CASES, ids=["%s%s" % (n, "_lo" if lo else "") for n, lo in CASES])
def test_escape_rows_dd_is_the_model_bit_for_bit(fr, name, pos_lo):
    cfg = view(fr, name)
    z, it = fr.escape_rows(cfg, precision=fr.Precision.DD, pos_lo=pos_lo or (0.0, 0.0), with_lo=True)
    wz, wit = M.escape_rows(cfg, pos_lo or (0.0, 0.0))
    assert np.array_equal(it, wit), "escape indices differ from the model at %d pixels" % int((it != wit).sum())
    assert same_f64(z, wz), "final positions differ from the model"
    if name.startswith("deep"):
        assert len(np.unique(it)) >= 2 and it.max() < cfg.iterations  # resolved, not flat blocks
    # hi parts through fr_escape_rows (pos_lo = 0) and the with_lo=False form
    if pos_lo is None:
        z2, it2 = fr.escape_rows(cfg, precision=fr.Precision.DD)
        assert np.array_equal(it2, wit) and same_f64(z2, np.ascontiguousarray(wz[..., 0::2]))
    z3, it3 = fr.escape_rows(cfg, 0, cfg.height, fr.Precision.DD, pos_lo=pos_lo or (0.0, 0.0))
    assert np.array_equal(it3, wit) and same_f64(z3, np.ascontiguousarray(wz[..., 0::2]))


@pytest.mark.parametrize("iterations", [0, 1, 37, 1000])
@pytest.mark.parametrize("name", ["default", "deep_julia"])
def test_caps_and_row_ranges(fr, name, iterations):
    cfg = view(fr, name, iterations=iterations)
    for y0, y1 in [(0, cfg.height), (17, 150), (192, 193), (5, 5)]:
        z, it = fr.escape_rows(cfg, y0, y1, fr.Precision.DD, pos_lo=LO if name.startswith("deep") else (0.0, 0.0),
                               with_lo=True)
        wz, wit = M.escape_rows(cfg, LO if name.startswith("deep") else (0.0, 0.0), y0, y1)
        assert np.array_equal(it, wit) and same_f64(z, wz), (y0, y1)
        img = fr.get_image_rows(cfg, y0, y1, fr.Precision.DD)
        if y1 > y0:
            wz0, wit0 = M.escape_rows(cfg, (0.0, 0.0), y0, y1)
            assert np.array_equal(img, model_colours(fr, cfg, wz0, wit0)), (y0, y1)


@pytest.mark.parametrize("smooth", [1, 0])
@pytest.mark.parametrize("inside", [1, 0])
@pytest.mark.parametrize("name,pos_lo", [("default", None), ("deep_mandelbrot", LO), ("deep_julia", None)])
def test_images_are_the_model_coloured(fr, name, pos_lo, smooth, inside):
    cfg = view(fr, name)
    cfg.smooth, cfg.inside = smooth, inside
    wz, wit = M.escape_rows(cfg, pos_lo or (0.0, 0.0))
    want = model_colours(fr, cfg, wz, wit)
    want4 = model_colours(fr, cfg, wz, wit, rgba=True)
    img = fr.get_image(cfg, fr.Precision.DD, pos_lo=pos_lo)
    assert np.array_equal(img, want), "RGB differs from the model at %d pixels" % int((img != want).any(-1).sum())
    assert np.array_equal(fr.get_image_rgba(cfg, fr.Precision.DD, pos_lo=pos_lo), want4)
    # re-colouring the hi parts with the library's own colour map gives the same image (include/fractal_hip.h)
    assert np.array_equal(fr.colour_image(cfg, np.ascontiguousarray(wz[..., 0::2]), wit), want)


def test_entry_points_agree(fr):
    import torch

    from fractal_renderer_amd import _native

    lib = _native.load()
    cfg = view(fr, "deep_mandelbrot")
    cfg.smooth = 1
    w, h = cfg.width, cfg.height
    host = fr.get_image(cfg, fr.Precision.DD)
    assert np.array_equal(fr.get_image_rows(cfg, 0, h, fr.Precision.DD, opts=fr.RenderOpts(tile=8, loop_mode=0)), host)
    rgba = fr.get_image_rgba(cfg, fr.Precision.DD)
    assert np.array_equal(rgba[..., :3], host) and (rgba[..., 3] == 255).all()
    dd3 = np.empty_like(host)
    _native.check(lib.fr_render_rows_dd(C.byref(cfg), None, 0, h, 3, dd3.ctypes.data, dd3.nbytes))
    assert np.array_equal(dd3, host)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    d3 = torch.zeros(h * w * 3, dtype=torch.uint8, device=dev)
    d4 = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
    e3 = torch.zeros(h * w * 3, dtype=torch.uint8, device=dev)
    o3 = torch.zeros(h * w * 3, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(stream):
        _native.check(lib.fr_render_rows_rgb8_device(C.byref(cfg), DD, 0, h, d3.data_ptr(), d3.numel(), stream.cuda_stream))
        _native.check(lib.fr_render_rows_rgba8_device(C.byref(cfg), DD, 0, h, d4.data_ptr(), d4.numel(), stream.cuda_stream))
        _native.check(lib.fr_render_rows_dd_device(C.byref(cfg), None, 0, h, 3, e3.data_ptr(), e3.numel(), stream.cuda_stream))
        o = fr.RenderOpts(tile=11)
        _native.check(lib.fr_render_rows_rgb8_device_opts(C.byref(cfg), DD, 0, h, o3.data_ptr(), o3.numel(), stream.cuda_stream,
                                                          C.byref(o)))
    stream.synchronize()
    for t in (d3, e3, o3):
        assert np.array_equal(t.cpu().numpy().reshape(h, w, 3), host)
    assert np.array_equal(d4.cpu().numpy().reshape(h, w, 4), rgba)
    for x, y in [(0, 0), (w - 1, h - 1), (128, 96), (3, 190), (200, 7)]:
        assert tuple(fr.get_recursive_pixel(cfg, x, y, fr.Precision.DD)) == tuple(host[y, x])


def test_start_hi_is_the_f64_start(fr):
    for name in ("default", "deep_mandelbrot", "deep_julia"):
        cfg = view(fr, name, iterations=0)
        zd, itd = fr.escape_rows(cfg, precision=fr.Precision.DD)
        z64, it64 = fr.escape_rows(cfg, precision=fr.Precision.F64)
        assert same_f64(zd, z64) and (itd == 0).all() and (it64 == 0).all(), name


@pytest.mark.parametrize("name", ["default", "default_julia", "deep_mandelbrot", "deep_julia"])
def test_count_iterations(fr, name):
    cfg = view(fr, name)
    total, npx = fr.count_iterations(cfg, precision=fr.Precision.DD)
    assert npx == cfg.width * cfg.height
    assert total == M.count_iterations(cfg)
    total2, _ = fr.count_iterations(cfg, 20, 120, precision=fr.Precision.DD)
    assert total2 == M.count_iterations(cfg, 20, 120)


def test_last_kernel_name_is_the_dd_kernel(fr):
    import torch

    from fractal_renderer_amd import _native

    lib = _native.load()
    cfg = view(fr, "deep_julia")
    out = torch.empty(cfg.width * cfg.height * 3, dtype=torch.uint8, device=torch.device("cuda", 0))
    name = C.create_string_buffer(160)
    ms = C.c_float()
    _native.check(lib.fr_set_profiling(1))
    try:
        _native.check(lib.fr_render_rows_rgb8_device(C.byref(cfg), DD, 0, cfg.height, out.data_ptr(), out.numel(), None))
        _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
        _native.check(lib.fr_last_kernel_name(name, len(name)))
    finally:
        _native.check(lib.fr_set_profiling(0))
    assert name.value == b"escape_dd_kernel" and ms.value > 0.0


def test_f64_renders_and_view_cache_are_untouched_by_dd(fr):
    """A shallow F64 view large enough for the view statistics (fr_set_dispatch_sampling): the same bytes and the same
    recorded choice before and after DD renders of the same view."""
    from fractal_renderer_amd import _native

    lib = _native.load()
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = 1536, 1024, 256

    def choice():
        st, ch, strip = C.c_int(), C.c_int(), C.c_uint32()
        _native.check(lib.fr_debug_view_choice(C.byref(cfg), 0, 0, cfg.height, C.byref(st), C.byref(ch), C.byref(strip)))
        return st.value, ch.value, strip.value

    before = fr.get_image(cfg)
    for _ in range(2):  # the next frames of the view read its statistics and settle the choice
        assert np.array_equal(fr.get_image(cfg), before)
    c0 = choice()
    assert c0[0] != 0, "the F64 view left no record"  # the check below would be empty
    for _ in range(2):
        fr.get_image(cfg, fr.Precision.DD)
        fr.get_image_rgba(cfg, fr.Precision.DD)
        fr.escape_rows(cfg, 0, 64, fr.Precision.DD)
        fr.count_iterations(cfg, 0, 64, precision=fr.Precision.DD)
        assert choice() == c0
    assert np.array_equal(fr.get_image(cfg), before)
