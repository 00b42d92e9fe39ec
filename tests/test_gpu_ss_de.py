"""SUPERSAMPLED DE on the device (include/fractal_hip.h, "SUPERSAMPLED DE"; csrc/fr_ss_de.hip: colour_de_filter_kernel), byte for
byte, no tolerance anywhere.  The yardstick is never the code under test: it is the composition of calls the library already
had — escape_rows_de(cfg_s) -> colour_image_de(cfg_s, T * s) -> box_filter — and, over the same arrays, the numpy model of
tests/ss_de_model.py.
  - the fused recolour (fr_colour_de_rows_ss_device, fr_colour_de_ss_rgb8) for every s in 2 .. 8, RGB at every byte misalignment
    and RGBA, sizes with a ragged last tile column and a ragged last tile row for every cf_tile_rows, with a teeth condition
    asserted from the composition's own arrays: enough samples are shaded, enough output pixels change, enough are capped;
    a row range of a view, s = 1, the fern, and 2^27 samples whose byte offsets pass 2^32;
  - the banded render (fr_render_rows_ss_de(_device)) on every road — F64, PT with a dd and with a wide centre, BLA-PT with
    both — with the smallest workspace (three bands) and the largest, row pieces, s = 1, T = 0, the caches, the host form;
  - special values placed by hand: der = 0, der = inf / NaN, iters == iterations."""
import ctypes as C

import numpy as np
import pytest

import de_model as DE
import pt_model as PM
import pt_wide_model as W
import ss_de_model as M

pytestmark = pytest.mark.gpu

GUARD = 64
T = 1.5
PLAIN, BLA = 0, 1


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


# ---- 1. the fused recolour against the composition of existing calls ---------------------------------------------------------------

# the kernel's tile (fr_ss_de.hip): 64 output pixels x cf_tile_rows(s) output rows
SIZES = [(67, 19), (65, 9), (1, 1), (63, 1)]
VIEWS = {"default": DE.default_view, "julia": DE.julia_view}
_arrays = {}


def arrays(fr, view, s, w, h):
    """(cfg, cfg_s, z, iters, der) of the view at w x h output pixels: the DE render of cfg_s by the existing call, made once"""
    key = (view, s, w, h)
    if key not in _arrays:
        cfg = VIEWS[view](fr.Config.new(), w, h)
        cfg_s = M.config_s(cfg, s)
        z, it, der = fr.escape_rows_de(cfg_s)
        for a in (z, it, der):
            a.setflags(write=False)
        _arrays[key] = cfg, cfg_s, z, it, der
    return _arrays[key]


def composition(fr, cfg_s, z, it, der, s, thickness, channels=3):
    """escape_rows_de's arrays -> colour_image_de at T * s -> box_filter: three calls the library already had"""
    return fr.box_filter(fr.colour_image_de(cfg_s, z, it, der, thickness * float(s)), s, channels)


def recolour_device(torch, lib, cfg, z, it, der, s, thickness, channels, dst_off=0, z_off=0, rows=None):
    """fr_colour_de_rows_ss_device over numpy arrays placed in guarded device buffers: the output dst_off bytes behind a 16-byte
    boundary, z and der z_off (0 or 8) bytes behind one"""
    dev = torch.device("cuda", 0)
    rows = it.shape[0] // s if rows is None else rows
    width = it.shape[1] // s

    def put(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        d = torch.zeros(a.size * 8 + 16, dtype=torch.uint8, device=dev)
        d[z_off:z_off + a.size * 8] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(dev)
        return d

    d_z, d_der = put(z), put(der)
    d_it = torch.from_numpy(np.ascontiguousarray(it).reshape(-1).view(np.int32).copy()).to(dev)
    need = channels * width * rows
    d_out = torch.full((GUARD + 16 + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert d_z.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    at = GUARD + dst_off
    torch.cuda.synchronize()
    check(lib.fr_colour_de_rows_ss_device(C.byref(cfg), d_z.data_ptr() + z_off, d_it.data_ptr(), d_der.data_ptr() + z_off, width, rows, s,
                                          thickness, channels, d_out.data_ptr() + at, need, None))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:at] == 0xA5).all() and (host[at + need:] == 0xA5).all(), "the kernel wrote outside its destination"
    return host[at:at + need].reshape(rows, width, channels)


@pytest.mark.parametrize("s", range(2, 9))
@pytest.mark.parametrize("view", list(VIEWS))
def test_fused_recolour_is_the_composition_of_existing_calls(fr, lib, torch, view, s):
    k = 0
    for w, h in SIZES:
        cfg, cfg_s, z, it, der = arrays(fr, view, s, w, h)
        want = {ch: composition(fr, cfg_s, z, it, der, s, T, ch) for ch in (3, 4)}
        plain = composition(fr, cfg_s, z, it, der, s, 0.0)
        if w * h > 64:  # the teeth, from the composition's own arrays
            D = fr.distance_rows(cfg_s, z, it, der)
            shaded = float(((it < cfg_s.iterations) & (D < T * s)).mean())
            changed = float((want[3] != plain).any(axis=-1).mean())
            capped = float((it == cfg_s.iterations).mean())
            print("%s %dx%d s=%d: %.1f%% of samples shaded, %.1f%% of output pixels changed, %.1f%% of samples capped"
                  % (view, w, h, s, 100 * shaded, 100 * changed, 100 * capped))
            assert shaded >= 0.05, "only %.1f%% of the samples are shaded" % (100 * shaded)
            assert changed >= 0.05, "only %.1f%% of the output pixels differ from the T = 0 output" % (100 * changed)
            if view == "default":
                assert capped >= 0.03, "only %.1f%% of the samples are capped" % (100 * capped)
        for ch in (3, 4):
            assert np.array_equal(M.colour(cfg, z, it, der, s, T, ch), want[ch]), ("the model and the composition", view, s, w, h, ch)
            assert np.array_equal(fr.colour_image_de_ss(cfg, z, it, der, s, T, channels=ch), want[ch]), ("host form", view, s, w, h, ch)
        for off in range(4):  # RGB rows start at every byte misalignment (odd widths), from every destination alignment
            got = recolour_device(torch, lib, cfg, z, it, der, s, T, 3, dst_off=off, z_off=8 * (k & 1))
            assert np.array_equal(got, want[3]), (view, s, w, h, off, int((got != want[3]).sum()))
            k += 1
        got = recolour_device(torch, lib, cfg, z, it, der, s, T, 4, dst_off=4 * (k % 3), z_off=8 * (k & 1))
        assert np.array_equal(got, want[4]), (view, s, w, h, "rgba")
        # T = 0 is the unshaded fused recolour, which is the unshaded composition
        got = recolour_device(torch, lib, cfg, z, it, der, s, 0.0, 3, dst_off=1)
        assert np.array_equal(got, plain) and np.array_equal(got, fr.colour_image_ss(cfg, z, it, s)), (view, s, w, h, "T = 0")


@pytest.mark.parametrize("s", [1, 2, 5, 8])
def test_a_row_range_of_the_view_is_shaded_with_the_whole_images_height(fr, lib, torch, s):
    """rows < cfg->height: the distance's last factor is (s * cfg->height) * min|scale|, whatever the arrays hold"""
    cfg, cfg_s, z, it, der = arrays(fr, "default", s, 67, 19)
    whole = composition(fr, cfg_s, z, it, der, s, T) if s > 1 else fr.colour_image_de(cfg, z, it, der, T)
    for y0, y1 in ((0, 7), (7, 19), (18, 19)):
        sub = tuple(a[s * y0:s * y1] for a in (z, it, der))
        assert np.array_equal(fr.colour_image_de_ss(cfg, *sub, s, T), whole[y0:y1]), (s, y0, y1, "host form")
        assert np.array_equal(recolour_device(torch, lib, cfg, *sub, s, T, 3, dst_off=3), whole[y0:y1]), (s, y0, y1)
        assert np.array_equal(M.colour(cfg, *sub, s, T), whole[y0:y1]), (s, y0, y1, "model")
    # and it matters: with the rows' own count as the height the bytes differ
    short = cfg.clone()
    short.height = 7
    assert not np.array_equal(fr.colour_image_de_ss(short, z[:7 * s], it[:7 * s], der[:7 * s], s, T), whole[:7])


def test_s_one_is_the_plain_shaded_recolour_and_the_fern_is_black(fr, lib, torch):
    cfg, _, z, it, der = arrays(fr, "julia", 1, 67, 19)
    want = fr.colour_image_de(cfg, z, it, der, T)
    assert np.array_equal(fr.colour_image_de_ss(cfg, z, it, der, 1, T), want)
    assert np.array_equal(recolour_device(torch, lib, cfg, z, it, der, 1, T, 3, dst_off=1), want)
    rgba = recolour_device(torch, lib, cfg, z, it, der, 1, T, 4)
    assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all()
    for s in (1, 3, 8):
        cfg, _, z, it, der = arrays(fr, "default", s, 65, 9)
        fern = cfg.clone()
        fern.algo = int(fr.Algo.BarnsleyFern)
        assert not recolour_device(torch, lib, fern, z, it, der, s, T, 3, dst_off=2).any()
        rgba = recolour_device(torch, lib, fern, z, it, der, s, T, 4)
        assert not rgba[..., :3].any() and (rgba[..., 3] == 255).all()


def test_special_values_placed_by_hand(fr, lib, torch):
    """der = 0 gives D = +inf: unshaded; der = inf or NaN gives D = 0: black; iters == iterations is never shaded"""
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = 5, 1, 100
    s = 2
    z = np.empty((2, 10, 2))
    z[...] = (300.0, 40.0)
    it = np.full((2, 10), 37, dtype=np.uint32)
    der = np.empty((2, 10, 2))
    der[...] = (1.0e-3, 0.0)  # far from the set: unshaded
    der[0, 0] = (0.0, 0.0)
    der[1, 2] = (np.inf, 1.0)
    der[0, 3] = (-np.inf, np.inf)
    der[1, 4] = (np.nan, 0.0)
    der[0, 5] = (0.0, np.nan)
    it[1, 6], z[1, 6] = 100, (0.1, 0.2)  # capped, inside: the inside colour, never shaded
    der[1, 6] = (np.inf, 0.0)
    it[0, 7], der[0, 7] = 100, (1e300, 1e300)  # capped with a z outside: still never shaded
    der[0, 8] = (900.0, 0.0)  # an ordinary shaded sample beside an unshaded one: D = 1.54 of Ts = 3 sample pixels
    want = M.colour(cfg, z, it, der, s, T)
    H = M.shaded(cfg, z, it, der, s, T)
    base = M.shaded(cfg, z, it, der, s, 0.0)
    assert base[0, 1].any() and np.array_equal(H[0, 0], base[0, 0]) and np.array_equal(H[0, 1], base[0, 1])
    for y, x in ((1, 2), (0, 3), (1, 4), (0, 5)):
        assert not H[y, x].any(), (y, x)
    assert np.array_equal(H[1, 6], base[1, 6]) and np.array_equal(H[0, 7], base[0, 7])
    assert H[0, 8].any() and (H[0, 8] < base[0, 8]).any()
    assert np.array_equal(want, composition(fr, M.config_s(cfg, s), z, it, der, s, T))
    for ch in (3, 4):
        want = M.colour(cfg, z, it, der, s, T, ch)
        assert np.array_equal(fr.colour_image_de_ss(cfg, z, it, der, s, T, channels=ch), want), ch
        assert np.array_equal(recolour_device(torch, lib, cfg, z, it, der, s, T, ch), want), ch


def test_fused_recolour_over_two_to_the_27_samples(fr, lib, torch):
    """2048 x 1024 output pixels at s = 8: 2^27 samples, 2.1 GB each of z and der and 0.5 GB of iters, so byte offsets pass 2^31
    and 2^32 (taken when the device has 12 GB free, which an MI355X has; otherwise 16384 x 1 at s = 8, and the print says
    which).  Built and compared on the device; the yardstick is the two existing device calls, fr_colour_de_rows_device and
    fr_box_filter_rgb8_device, through a 400 MB RGB image.  |z|^2 is log-uniform over 2^-20 .. 2^40 and |der| is set so that
    D / Ts is log-uniform over 2^-4 .. 2^4 where |z| > 1: about half of the escaped samples are shaded."""
    free, _total = torch.cuda.mem_get_info(0)
    s = 8
    width, rows = (2048, 1024) if free >= (12 << 30) else (16384, 1)
    print("fused DE recolour at %d x %d output pixels, s = 8 (%.1f GB free)" % (width, rows, free / 2 ** 30))
    n = s * s * width * rows
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(2028)
    cap = 1000
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = width, rows, cap
    cfg_s = M.config_s(cfg, s)
    pixels = float(cfg_s.height) * min(abs(cfg.scale.re), abs(cfg.scale.im))

    def polar(radius):
        a = torch.rand(n, device=dev, generator=g, dtype=torch.float64) * (2 * np.pi)
        return torch.stack([radius * torch.cos(a), radius * torch.sin(a)], dim=-1).contiguous()

    r2 = torch.exp2(torch.rand(n, device=dev, generator=g, dtype=torch.float64) * 60.0 - 20.0)
    ratio = torch.exp2(torch.rand(n, device=dev, generator=g, dtype=torch.float64) * 8.0 - 4.0)
    m = r2.sqrt() * torch.log2(r2).abs() * (0.5 * np.log(2.0) * pixels / (T * s)) / ratio
    z = polar(r2.sqrt())
    der = polar(m)
    del r2, ratio, m
    it = torch.randint(0, cap + 1, (n,), device=dev, generator=g, dtype=torch.int32)
    it[torch.rand(n, device=dev, generator=g) < 0.1] = cap
    rgb = torch.zeros(3 * n, dtype=torch.uint8, device=dev)
    plain = torch.zeros(3 * width * rows, dtype=torch.uint8, device=dev)
    check(lib.fr_colour_de_rows_device(C.byref(cfg_s), z.data_ptr(), it.data_ptr(), der.data_ptr(), n, 0.0, 3, rgb.data_ptr(), None))
    check(lib.fr_box_filter_rgb8_device(rgb.data_ptr(), width, rows, s, 3, plain.data_ptr(), plain.numel(), None))
    check(lib.fr_colour_de_rows_device(C.byref(cfg_s), z.data_ptr(), it.data_ptr(), der.data_ptr(), n, T * s, 3, rgb.data_ptr(), None))
    for channels in (3, 4):
        want = torch.zeros(channels * width * rows, dtype=torch.uint8, device=dev)
        check(lib.fr_box_filter_rgb8_device(rgb.data_ptr(), width, rows, s, channels, want.data_ptr(), want.numel(), None))
        got = torch.full((channels * width * rows,), 0xA5, dtype=torch.uint8, device=dev)
        check(lib.fr_colour_de_rows_ss_device(C.byref(cfg), z.data_ptr(), it.data_ptr(), der.data_ptr(), width, rows, s, T, channels,
                                              got.data_ptr(), got.numel(), None))
        torch.cuda.synchronize()
        assert torch.equal(got, want), (channels, int((got != want).sum()))
        if channels == 3:
            changed = float((want.view(-1, 3) != plain.view(-1, 3)).any(dim=1).double().mean())
            print("%.1f%% of the output pixels differ from the T = 0 output" % (100 * changed))
            assert changed >= 0.05 and int(want.max()) > 20 and len(torch.unique(want)) > 20  # the images are no constants


# ---- 2. the banded render on every road ----------------------------------------------------------------------------------------

W_OUT, H_OUT = 67, 19


def wide_centre(fr, name, words):
    ints = W.centre_ints(name, words)
    return fr.WideCentre(words, W.to_words(ints[0], words), W.to_words(ints[1], words))


def road_f64(fr):
    return DE.default_view(fr.Config.new(), W_OUT, H_OUT), dict()


def road_pt_dd(fr):
    cfg = fr.Config.new()
    lo = DE.seahorse_shallow(cfg, W_OUT, H_OUT)
    return cfg, dict(precision=fr.Precision.PT, pos_lo=lo)


def road_pt_wide(fr):  # the wide view of tests/test_gpu_de.py
    return W.view(fr.Config.new(), "M", 200, W_OUT, H_OUT, 3000), dict(precision=fr.Precision.PT, centre=wide_centre(fr, "M", 5))


def road_bla_wide(fr):  # tests/test_gpu_de_bla.py's M at 2^300: escaped pixels skip
    return W.view(fr.Config.new(), "M", 300, W_OUT, H_OUT, 5000), dict(precision=fr.Precision.PT, centre=wide_centre(fr, "M", 6), bla=0)


def road_bla_dd(fr):  # and its seahorse view on the dd centre
    cfg = fr.Config.new()
    lo = PM.seahorse_view(cfg, W_OUT, H_OUT)
    return cfg, dict(precision=fr.Precision.PT, pos_lo=lo, bla=0)


ROADS = {"f64": road_f64, "pt-dd": road_pt_dd, "pt-wide": road_pt_wide, "bla-wide": road_bla_wide, "bla-dd": road_bla_dd}


def c_args(kw):
    """(precision, pos_lo, centre, road, bits, keep-alive) of the C call for the Python keywords"""
    from fractal_renderer_amd import _native

    lo = None if kw.get("pos_lo") is None else _native.Imaginary(*kw["pos_lo"])
    st = None if kw.get("centre") is None else kw["centre"].c_struct()
    road, bits = (BLA, int(kw["bla"])) if kw.get("bla") is not None else (PLAIN, 0)
    return (int(kw.get("precision", 0)), None if lo is None else C.byref(lo), None if st is None else C.byref(st), road, bits), (lo, st)


def render_device(torch, lib, cfg, kw, s, thickness, y0, y1, channels, work_len):
    """fr_render_rows_ss_de_device into a guarded destination with a canary behind the workspace"""
    dev = torch.device("cuda", 0)
    pre, _keep = c_args(kw)
    need = channels * cfg.width * (y1 - y0)
    d_out = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_work = torch.full((work_len + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    check(lib.fr_render_rows_ss_de_device(C.byref(cfg), *pre, thickness, s, y0, y1, channels, d_out.data_ptr() + GUARD, need,
                                          d_work.data_ptr(), work_len, None))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    assert (d_work[work_len:].cpu().numpy() == 0x5A).all(), "wrote behind work_len"
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels)


def render_host(lib, cfg, kw, s, thickness, y0, y1, channels):
    pre, _keep = c_args(kw)
    need = channels * cfg.width * (y1 - y0)
    host = np.full(GUARD + need + GUARD, 0xA5, dtype=np.uint8)
    check(lib.fr_render_rows_ss_de(C.byref(cfg), *pre, thickness, s, y0, y1, channels, host.ctypes.data + GUARD, need))
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels)


def band_count(width, rows_out, s, work_len):
    """the band rule of include/fractal_hip.h (fr_ss_de_workspace_bytes) restated: the number of bands for a workspace length"""
    row_bytes, rows = 36 * s * width, s * rows_out
    bmax = work_len // row_bytes
    if bmax >= rows:
        return 1
    bmax -= bmax % (8 * s)
    nb = -(-rows // bmax)
    b = -(-rows // nb)
    b = -(-b // (8 * s)) * (8 * s)
    return -(-rows // b)


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", list(ROADS))
def test_banded_render_is_the_composition_on_every_road(fr, lib, torch, name, s):
    cfg, kw = ROADS[name](fr)
    cfg_s = M.config_s(cfg, s)
    z, it, der = fr.escape_rows_de(cfg_s, **kw)
    want = {ch: composition(fr, cfg_s, z, it, der, s, T, ch) for ch in (3, 4)}
    assert len(np.unique(want[3].reshape(-1, 3), axis=0)) > 8, "the view degenerated"
    plain = composition(fr, cfg_s, z, it, der, s, 0.0)
    print("%s s=%d: %.1f%% of the output pixels are shaded" % (name, s, 100 * float((want[3] != plain).any(axis=-1).mean())))
    assert (want[3] != plain).any(), "nothing is shaded: the road's distance is not tested"
    mn, best = fr.ss_de_workspace_bytes(cfg, s)
    assert band_count(W_OUT, H_OUT, s, mn) == 3 and band_count(W_OUT, H_OUT, s, best) == 1
    other = W.view(fr.Config.new(), "J", 300, 16, 12, 5000), wide_centre(fr, "J", 6)
    for work_len in (mn, best):
        for ch in (3, 4):
            got = render_device(torch, lib, cfg, kw, s, T, 0, H_OUT, ch, work_len)
            assert np.array_equal(got, want[ch]), (name, s, work_len, ch, int((got != want[ch]).sum()))
    # row pieces equal the whole
    pieces = [render_device(torch, lib, cfg, kw, s, T, y0, y1, 3, fr.ss_de_workspace_bytes(cfg, s, y0, y1)[0]) for y0, y1 in ((0, 7), (7, 19))]
    assert np.array_equal(np.concatenate(pieces), want[3]), (name, s, "row pieces")
    # the host form and the Python front end are the device form
    for ch in (3, 4):
        assert np.array_equal(render_host(lib, cfg, kw, s, T, 0, H_OUT, ch), want[ch]), (name, s, ch, "host form")
    assert np.array_equal(render_host(lib, cfg, kw, s, T, 7, 19, 3), want[3][7:19]), (name, s, "host form, rows")
    assert np.array_equal(fr.get_image_de(cfg, T, supersample=s, **kw), want[3]), (name, s, "get_image_de")
    assert np.array_equal(fr.get_image_de(cfg, T, supersample=s, y0=7, y1=19, channels=4, **kw), want[4][7:19])
    # T = 0 is the unshaded supersampled render of the same road
    unshaded = render_device(torch, lib, cfg, kw, s, 0.0, 0, H_OUT, 3, mn)
    assert np.array_equal(unshaded, plain)
    if name == "f64":
        assert np.array_equal(unshaded, fr.get_image(cfg, supersample=s))
    else:
        ss_kw = {k: v for k, v in kw.items() if k != "precision"}
        assert np.array_equal(unshaded, fr.get_image_ss_pt(cfg, s, **ss_kw)), (name, s, "T = 0")
    # one orbit — and for BLA one table — computed for all three bands: the last band found them in the caches
    if name != "f64":
        fr.escape_rows_de(other[0], precision=fr.Precision.PT, centre=other[1], bla=0)  # the caches now hold another view
        assert fr.pt_orbit_cache()[3] > 0 and fr.bla_cache()[3] == 1
        assert np.array_equal(render_device(torch, lib, cfg, kw, s, T, 0, H_OUT, 3, mn), want[3])
        assert fr.pt_orbit_cache()[3] == 0 and fr.pt_orbit_cache()[0] == cfg.iterations
        if "bla" in kw:
            assert fr.bla_cache()[3] == 0 and fr.bla_cache()[0] == fr.BLA_DEFAULT_BITS


@pytest.mark.parametrize("name", list(ROADS))
def test_supersample_one_is_get_image_de(fr, lib, torch, name):
    cfg, kw = ROADS[name](fr)
    want = fr.get_image_de(cfg, T, **kw)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 8
    mn, best = fr.ss_de_workspace_bytes(cfg, 1)
    assert band_count(W_OUT, H_OUT, 1, mn) == 3
    for work_len in (mn, best):
        assert np.array_equal(render_device(torch, lib, cfg, kw, 1, T, 0, H_OUT, 3, work_len), want), (name, work_len)
    rgba = render_device(torch, lib, cfg, kw, 1, T, 0, H_OUT, 4, mn)
    assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all()
    assert np.array_equal(render_host(lib, cfg, kw, 1, T, 0, H_OUT, 3), want)
    assert np.array_equal(fr.get_image_de(cfg, T, supersample=1, y0=7, y1=19, **kw), want[7:19])


def test_profiling_reports_the_roads_kernel(fr, lib, torch):
    ms, name = C.c_float(), C.create_string_buffer(160)
    check(lib.fr_set_profiling(1))
    try:
        for road, kernel in (("f64", b"escape_de_kernel"), ("pt-dd", b"escape_pt_de_kernel"), ("bla-dd", b"escape_bla_de_kernel")):
            cfg, kw = ROADS[road](fr)
            render_device(torch, lib, cfg, kw, 2, T, 0, H_OUT, 3, fr.ss_de_workspace_bytes(cfg, 2)[0])
            check(lib.fr_last_kernel_ms(C.byref(ms)))
            check(lib.fr_last_kernel_name(name, len(name)))
            assert name.value == kernel and ms.value > 0, (road, name.value, ms.value)
    finally:
        check(lib.fr_set_profiling(0))


def test_an_algorithm_without_orbits_renders_black(fr, lib, torch):
    cfg = DE.default_view(fr.Config.new(), W_OUT, H_OUT)
    cfg.algo = int(fr.Algo.BarnsleyFern)
    for s in (1, 2):
        mn = fr.ss_de_workspace_bytes(cfg, s)[0]
        assert not render_device(torch, lib, cfg, {}, s, T, 0, H_OUT, 3, mn).any()
        rgba = render_device(torch, lib, cfg, {}, s, T, 0, H_OUT, 4, mn)
        assert not rgba[..., :3].any() and (rgba[..., 3] == 255).all()


@pytest.mark.parametrize("channels", [3, 4])
def test_host_form_under_a_cap_below_min_bytes_is_the_device_form(fr, lib, torch, channels):
    """fr_render_rows_ss_de on the F64 road (test_gpu_ss.py: host_bands_are_the_device_forms)"""
    from test_gpu_ss import HOOK_H, HOOK_S, HOOK_W, HOOK_Y0, HOOK_Y1, host_bands_are_the_device_forms

    cfg = DE.default_view(fr.Config.new(), HOOK_W, HOOK_H)
    sizes = host_bands_are_the_device_forms(
        lib, 36, lambda n: render_device(torch, lib, cfg, {}, HOOK_S, T, HOOK_Y0, HOOK_Y1, channels, n),
        lambda: render_host(lib, cfg, {}, HOOK_S, T, HOOK_Y0, HOOK_Y1, channels))
    assert sizes == fr.ss_de_workspace_bytes(cfg, HOOK_S, HOOK_Y0, HOOK_Y1)
