"""FR_PRECISION_PT on the device (fractal-renderer_amd/csrc/fr_pt.hip) against the host model tests/pt_model.c, bit for
bit: final positions, escape indices, RGB / RGBA bytes (the oracle's colour map over the model's z, libm log2),
iteration counts; the entry points agree with each other; two threads rendering two views at once each get their own
view (the context's orbit cache); F64 and DD renders and the view-choice cache are untouched by PT calls."""
import ctypes as C
import threading

import numpy as np
import pytest

import dd_model as D
import oracle_lib as O
import pt_model as M

pytestmark = pytest.mark.gpu

PT = 3
LO = (0.0, 2.0 ** -60)  # a normalised low part of the centre (0, 1)


@pytest.fixture(scope="module")
def fr():
    import fractal_renderer_amd

    assert fractal_renderer_amd.device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    fractal_renderer_amd.init(0)
    assert fractal_renderer_amd.device_name().startswith("gfx950")
    return fractal_renderer_amd


def same_f64(a, b):
    """Bit-identical, zero signs included; any NaN matches any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(
        a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def view(fr, name, width=257, height=193, iterations=None):
    """(config, the view's own pos_lo)"""
    cfg = fr.Config.new()
    cfg.width, cfg.height = width, height
    lo = (0.0, 0.0)
    if name == "default":
        cfg.iterations = 200 if iterations is None else iterations
    elif name == "default_julia":
        cfg.algo = 2
        cfg.iterations = 300 if iterations is None else iterations
        cfg.julia_set.re, cfg.julia_set.im = -0.8, 0.156
        cfg.scale.re = cfg.scale.im = 0.3
    elif name.startswith("deep"):
        D.deep_view(cfg, name == "deep_julia", width, height, 3000 if iterations is None else iterations)
    elif name == "seahorse":
        lo = M.seahorse_view(cfg, width, height, 20000 if iterations is None else iterations)
    elif name == "early":
        lo = M.early_escape_view(cfg, width, height, 2000 if iterations is None else iterations)
    elif name == "julia_rebase":
        lo = M.julia_rebase_view(cfg, width, height, 3000 if iterations is None else iterations)
    else:
        raise KeyError(name)
    return cfg, lo


def model_colours(cfg, z, it, rgba=False):
    ocfg = O.Config.from_buffer_copy(bytes(cfg))
    O.set_log2_mode(O.LOG2_LIBM)
    rgb = O.colour_rows(ocfg, np.ascontiguousarray(z), it)
    if not rgba:
        return rgb
    out = np.full(rgb.shape[:-1] + (4,), 255, dtype=np.uint8)
    out[..., :3] = rgb
    return out


CASES = [("default", None), ("default_julia", None), ("deep_mandelbrot", None), ("deep_mandelbrot", LO),
         ("deep_julia", None), ("deep_julia", LO), ("seahorse", "own"), ("early", None), ("julia_rebase", None),
         ("julia_rebase", LO)]


@pytest.mark.parametrize("name,pos_lo", CASES, ids=["%s%s" % (n, "_lo" if lo else "") for n, lo in CASES])
def test_escape_rows_pt_is_the_model_bit_for_bit(fr, name, pos_lo):
    kw = {"width": 128, "height": 96} if name == "seahorse" else {}
    cfg, own = view(fr, name, **kw)
    lo = own if pos_lo == "own" else (pos_lo or (0.0, 0.0))
    z, it = fr.escape_rows(cfg, precision=fr.Precision.PT, pos_lo=lo)
    wz, wit = M.escape_rows(cfg, lo)
    assert np.array_equal(it, wit), "escape indices differ from the model at %d pixels" % int((it != wit).sum())
    assert same_f64(z, wz), "final positions differ from the model"
    if name != "default" and name != "default_julia":
        assert len(np.unique(it)) >= 2  # resolved, not flat blocks
    if lo == (0.0, 0.0):  # fr_escape_rows(PT) is the same call with pos_lo = 0
        z2, it2 = fr.escape_rows(cfg, precision=fr.Precision.PT)
        assert np.array_equal(it2, wit) and same_f64(z2, wz)


@pytest.mark.parametrize("iterations", [0, 1, 2, 37, 1000])
@pytest.mark.parametrize("name", ["default", "deep_julia", "early"])
def test_caps_and_row_ranges(fr, name, iterations):
    cfg, _ = view(fr, name, iterations=iterations)
    lo = LO if name.startswith("deep") else (0.0, 0.0)
    wz, wit = M.escape_rows(cfg, lo)
    for y0, y1 in [(0, cfg.height), (17, 150), (192, 193), (5, 5)]:
        z, it = fr.escape_rows(cfg, y0, y1, fr.Precision.PT, pos_lo=lo)
        assert np.array_equal(it, wit[y0:y1]) and same_f64(z, wz[y0:y1]), (y0, y1)
        img = fr.get_image_rows(cfg, y0, y1, fr.Precision.PT, pos_lo=lo)
        if y1 > y0:
            assert np.array_equal(img, model_colours(cfg, wz[y0:y1], wit[y0:y1])), (y0, y1)


@pytest.mark.parametrize("smooth", [1, 0])
@pytest.mark.parametrize("inside", [1, 0])
@pytest.mark.parametrize("name,pos_lo", [("default", None), ("deep_mandelbrot", LO), ("julia_rebase", None)])
def test_images_are_the_model_coloured(fr, name, pos_lo, smooth, inside):
    cfg, _ = view(fr, name)
    cfg.smooth, cfg.inside = smooth, inside
    wz, wit = M.escape_rows(cfg, pos_lo or (0.0, 0.0))
    want = model_colours(cfg, wz, wit)
    img = fr.get_image(cfg, fr.Precision.PT, pos_lo=pos_lo)
    assert np.array_equal(img, want), "RGB differs from the model at %d pixels" % int((img != want).any(-1).sum())
    assert np.array_equal(fr.get_image_rgba(cfg, fr.Precision.PT, pos_lo=pos_lo), model_colours(cfg, wz, wit, True))
    assert np.array_equal(fr.colour_image(cfg, wz, wit), want)  # the library's own colour map over z


def test_entry_points_agree(fr):
    import torch

    from fractal_renderer_amd import _native

    lib = _native.load()
    cfg, _ = view(fr, "deep_mandelbrot")
    cfg.smooth = 1
    w, h = cfg.width, cfg.height
    host = fr.get_image(cfg, fr.Precision.PT)
    wz, wit = M.escape_rows(cfg)
    assert np.array_equal(host, model_colours(cfg, wz, wit))
    assert np.array_equal(fr.get_image_rows(cfg, 0, h, fr.Precision.PT, opts=fr.RenderOpts(tile=8, loop_mode=0)), host)
    rgba = fr.get_image_rgba(cfg, fr.Precision.PT)
    assert np.array_equal(rgba[..., :3], host) and (rgba[..., 3] == 255).all()
    pt3 = np.empty_like(host)
    _native.check(lib.fr_render_rows_pt(C.byref(cfg), None, 0, h, 3, pt3.ctypes.data, pt3.nbytes))
    assert np.array_equal(pt3, host)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    d3 = torch.zeros(h * w * 3, dtype=torch.uint8, device=dev)
    d4 = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
    e3 = torch.zeros(h * w * 3, dtype=torch.uint8, device=dev)
    e4 = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(stream):
        _native.check(lib.fr_render_rows_rgb8_device(C.byref(cfg), PT, 0, h, d3.data_ptr(), d3.numel(), stream.cuda_stream))
        _native.check(lib.fr_render_rows_rgba8_device(C.byref(cfg), PT, 0, h, d4.data_ptr(), d4.numel(), stream.cuda_stream))
        _native.check(lib.fr_render_rows_pt_device(C.byref(cfg), None, 0, h, 3, e3.data_ptr(), e3.numel(), stream.cuda_stream))
        _native.check(lib.fr_render_rows_pt_device(C.byref(cfg), None, 0, h, 4, e4.data_ptr(), e4.numel(), stream.cuda_stream))
    stream.synchronize()
    for t in (d3, e3):
        assert np.array_equal(t.cpu().numpy().reshape(h, w, 3), host)
    for t in (d4, e4):
        assert np.array_equal(t.cpu().numpy().reshape(h, w, 4), rgba)
    for x, y in [(0, 0), (w - 1, h - 1), (128, 96), (3, 190), (200, 7)]:
        assert tuple(fr.get_recursive_pixel(cfg, x, y, fr.Precision.PT)) == tuple(host[y, x])


@pytest.mark.parametrize("name", ["default", "default_julia", "deep_mandelbrot", "deep_julia", "early", "julia_rebase"])
def test_count_iterations(fr, name):
    cfg, _ = view(fr, name)
    total, npx = fr.count_iterations(cfg, precision=fr.Precision.PT)
    assert npx == cfg.width * cfg.height
    assert total == M.count_iterations(cfg)
    total2, _ = fr.count_iterations(cfg, 20, 120, precision=fr.Precision.PT)
    assert total2 == M.count_iterations(cfg, 20, 120)


def test_two_threads_render_two_views(fr):
    """Two threads, two different PT views, many frames each at the same time: the orbit cache of the context is
    replaced under the other thread's feet, and each thread still gets its own view's image every time.  A DD thread
    (host and device renders) and an F64 thread on the staged host-buffer road run beside them: the deep host path and
    the F64 road share the context's lock and scratch."""
    import torch

    from fractal_renderer_amd import _native

    lib = _native.load()
    views = [view(fr, "deep_mandelbrot", 160, 96, 3000)[0], view(fr, "julia_rebase", 160, 96)[0]]
    want = [model_colours(c, *M.escape_rows(c)) for c in views]
    dd_cfg = view(fr, "deep_julia", 160, 96)[0]
    dz, dit = D.escape_rows(dd_cfg)
    views.append(dd_cfg)
    want.append(model_colours(dd_cfg, np.ascontiguousarray(dz[..., 0::2]), dit))
    f64_cfg = view(fr, "default", 700, 500)[0]
    views.append(f64_cfg)
    O.set_log2_mode(O.LOG2_SOFT)  # the F64 kernels' log2
    want.append(O.get_image(O.Config.from_buffer_copy(bytes(f64_cfg))))
    O.set_log2_mode(O.LOG2_LIBM)
    errors = []

    def worker(k):
        try:
            cfg = views[k]
            stream = torch.cuda.Stream(torch.device("cuda", 0))
            d = torch.zeros(cfg.width * cfg.height * 3, dtype=torch.uint8, device=torch.device("cuda", 0))
            for frame in range(12):
                if k == 3:  # F64 through the host-buffer road
                    img = fr.get_image(cfg)
                elif frame % 2:
                    img = fr.get_image(cfg, fr.Precision.DD if k == 2 else fr.Precision.PT)
                else:
                    render = lib.fr_render_rows_dd_device if k == 2 else lib.fr_render_rows_pt_device
                    _native.check(render(C.byref(cfg), None, 0, cfg.height, 3, d.data_ptr(), d.numel(), stream.cuda_stream))
                    stream.synchronize()
                    img = d.cpu().numpy().reshape(cfg.height, cfg.width, 3)
                if not np.array_equal(img, want[k]):
                    errors.append((k, frame, int((img != want[k]).any(-1).sum())))
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(len(views))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_last_kernel_name_is_the_pt_kernel(fr):
    import torch

    from fractal_renderer_amd import _native

    lib = _native.load()
    cfg, _ = view(fr, "deep_julia")
    out = torch.empty(cfg.width * cfg.height * 3, dtype=torch.uint8, device=torch.device("cuda", 0))
    name = C.create_string_buffer(160)
    ms = C.c_float()
    _native.check(lib.fr_set_profiling(1))
    try:
        _native.check(lib.fr_render_rows_rgb8_device(C.byref(cfg), PT, 0, cfg.height, out.data_ptr(), out.numel(), None))
        _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
        _native.check(lib.fr_last_kernel_name(name, len(name)))
    finally:
        _native.check(lib.fr_set_profiling(0))
    assert name.value == b"escape_pt_kernel" and ms.value > 0.0


def test_f64_dd_and_view_cache_are_untouched_by_pt(fr):
    from fractal_renderer_amd import _native

    lib = _native.load()
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = 1536, 1024, 256

    def choice():
        st, ch, strip = C.c_int(), C.c_int(), C.c_uint32()
        _native.check(lib.fr_debug_view_choice(C.byref(cfg), 0, 0, cfg.height, C.byref(st), C.byref(ch), C.byref(strip)))
        return st.value, ch.value, strip.value

    before = fr.get_image(cfg)
    for _ in range(2):
        assert np.array_equal(fr.get_image(cfg), before)
    c0 = choice()
    assert c0[0] != 0, "the F64 view left no record"
    deep, _ = view(fr, "deep_julia")
    dd_before = fr.get_image(deep, fr.Precision.DD)
    for _ in range(2):
        fr.get_image(cfg, fr.Precision.PT)
        fr.get_image_rgba(cfg, fr.Precision.PT)
        fr.escape_rows(cfg, 0, 64, fr.Precision.PT)
        fr.count_iterations(cfg, 0, 64, precision=fr.Precision.PT)
        fr.get_image(deep, fr.Precision.PT)
        assert choice() == c0
    assert np.array_equal(fr.get_image(cfg), before)
    assert np.array_equal(fr.get_image(deep, fr.Precision.DD), dd_before)
