"""Anti-aliased deep views on the device (fractal-renderer_amd/csrc/fr_ss.hip; include/fractal_hip.h, "supersampled rendering
on the deep roads"), byte for byte, no tolerance anywhere.  The yardstick is never the code under test:
  - fr_render_rows_ss_pt(_device) against the road's own plain call on cfg_s (fr_render_rows_pt_wide / _pt_bla / _pt_scaled,
    which tests/test_gpu_pt_wide.py, test_gpu_bla.py and test_gpu_pt_scaled.py tie to the models) filtered in numpy, with
    floors on the yardstick image so that a view that degenerates fails loudly: every road, s in {2, 3, 5}, the smallest and
    the largest workspace, row ranges, RGB and RGBA, guards and the workspace canary, host form = device form, s = 1, the
    Python front end and the command line, the orbit and table caches after a many-band call, profiling;
  - fr_colour_rows_ss_device / fr_colour_ss_rgb8 (colour_filter_kernel) against fr_box_filter_rgb8(fr_colour_rgb8(...)), two
    host calls the library already had, over real results and over synthetic arrays that reach byte boundaries: s = 1 .. 8,
    widths and rows around every boundary of the kernel's tile, every RGB destination alignment, RGBA, smooth and inside on
    and off, the fern, 2^27 samples, and a kept SCALED PT view extended and recoloured."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dd_model as DM
import oracle_lib as O
import pt_model as PM
import pt_scaled_model as S
import pt_wide_model as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT = 3
PLAIN, BLA, SCALED = 0, 1, 2
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


# ---- the definition, in numpy (tests/test_gpu_ss.py) -----------------------------------------------------------------------


def np_filter(big, s, channels=3):
    """big uint8 [s*rows, s*width, 3] -> uint8 [rows, width, channels]: (block sum + s*s // 2) // (s*s), alpha 255"""
    rows, width = big.shape[0] // s, big.shape[1] // s
    sums = big.reshape(rows, s, width, s, 3).astype(np.uint32).sum(axis=(1, 3))
    rgb = ((sums + (s * s) // 2) // (s * s)).astype(np.uint8)
    if channels == 3:
        return rgb
    out = np.full((rows, width, 4), 255, dtype=np.uint8)
    out[..., :3] = rgb
    return out


def mixed_share(big, s):
    """the share of s x s blocks that mix colours"""
    rows, width = big.shape[0] // s, big.shape[1] // s
    b = big.reshape(rows, s, width, s, 3)
    return float((b.max(axis=(1, 3)) != b.min(axis=(1, 3))).any(axis=-1).mean())


def band_count(width, rows_out, s, work_len):
    """the band rule of include/fractal_hip.h (fr_ss_workspace_bytes) restated: the number of bands for a workspace length"""
    row_bytes, rows = 3 * s * width, s * rows_out
    bmax = work_len // row_bytes
    if bmax >= rows:
        return 1
    bmax -= bmax % (8 * s)
    nb = -(-rows // bmax)
    b = -(-rows // nb)
    b = -(-b // (8 * s)) * (8 * s)
    return -(-rows // b)


def workspace(lib, cfg, s, y0, y1):
    mn, best = C.c_size_t(), C.c_size_t()
    check(lib.fr_ss_workspace_bytes(C.byref(cfg), s, y0, y1, C.byref(mn), C.byref(best)))
    return mn.value, best.value


# ---- the views: tests/pt_scaled_model.py's specs at s times the size --------------------------------------------------------

# name -> (centre, words, log2 scale, output width, height, cap, exposure or None, floor on the mixed share, [(road, bits)])
RENDER_VIEWS = {
    "J-2^300": ("J", 6, 300, 16, 12, 5000, None, 0.20, [(PLAIN, 0), (BLA, 0)]),
    "J-2^900": ("J", 16, 900, 16, 12, 5000, None, 0.20, [(SCALED, -1), (SCALED, 40)]),
    "M-2^300-e150": ("M", 6, 300, 16, 12, 5000, 150.0, 0.25, [(PLAIN, 0), (BLA, 0)]),
    "M-2^900-13x20": ("M", 16, 900, 13, 20, 6000, None, 0.03, [(SCALED, -1), (SCALED, 40)]),
}
_yard = {}


class Deep:
    """a view of RENDER_VIEWS at supersample s: cfg (the output's), cfg_s, the wide centre"""

    def __init__(self, fr, native, name, s, size=None):
        cname, n, log2, w, h, cap, exposure, self.floor, self.roads = RENDER_VIEWS[name]
        if size is not None:
            w, h = size
        self.name, self.s = name, s
        self.v = S.view(fr.Config.new, (cname, n, log2, s * w, s * h, cap))
        self.cfg_s = self.v.cfg.clone()  # the View's own config is shared: never written
        if exposure is not None:
            self.cfg_s.exposure = exposure
        self.cfg = self.cfg_s.clone()
        self.cfg.width, self.cfg.height = w, h
        self.st = self.v.centre(native)
        self.c = C.byref(self.st)

    def plain(self, lib, road, bits, cfg=None, y0=0, y1=None, channels=3):
        """the road's own plain call (host form) over rows [y0, y1) of cfg (default: cfg_s, whole)"""
        cfg = self.cfg_s if cfg is None else cfg
        y1 = cfg.height if y1 is None else y1
        out = np.zeros((y1 - y0, cfg.width, channels), dtype=np.uint8)
        tail = (y0, y1, channels, out.ctypes.data, out.nbytes)
        if road == PLAIN:
            check(lib.fr_render_rows_pt_wide(C.byref(cfg), self.c, *tail))
        elif road == BLA:
            check(lib.fr_render_rows_pt_bla(C.byref(cfg), None, self.c, bits, *tail))
        else:
            check(lib.fr_render_rows_pt_scaled(C.byref(cfg), self.c, bits, *tail))
        return out

    def yardstick(self, lib, road, bits):
        """the plain road's image of cfg_s, with the floor on its mixed share asserted: a condition on the yardstick"""
        key = (self.name, self.s, self.cfg.width, self.cfg.height, road, bits)
        if key not in _yard:
            big = self.plain(lib, road, bits)
            mixed = mixed_share(big, self.s)
            print("%s s=%d road=%d bits=%d: %.1f%% of blocks mixed" % (self.name, self.s, road, bits, 100 * mixed))
            if self.s > 1:
                assert mixed >= self.floor, "%s: only %.1f%% of the blocks mix colours" % (self.name, 100 * mixed)
            big.setflags(write=False)
            _yard[key] = big
        return _yard[key]


def ss_pt_device(torch, lib, cfg, centre, road, bits, s, y0, y1, channels, work_len, pos_lo=None, stream=None):
    """fr_render_rows_ss_pt_device into a guarded destination with a canary behind the workspace"""
    dev = torch.device("cuda", 0)
    need = channels * cfg.width * (y1 - y0)
    d_out = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_work = torch.full((work_len + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    check(lib.fr_render_rows_ss_pt_device(C.byref(cfg), pos_lo, centre, road, bits, s, y0, y1, channels, d_out.data_ptr() + GUARD, need,
                                          d_work.data_ptr() if work_len else None, work_len, stream))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    assert (d_work[work_len:].cpu().numpy() == 0x5A).all(), "wrote behind work_len"
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels)


def ss_pt_host(lib, cfg, centre, road, bits, s, y0, y1, channels, pos_lo=None):
    need = channels * cfg.width * (y1 - y0)
    host = np.full(GUARD + need + GUARD, 0xA5, dtype=np.uint8)
    check(lib.fr_render_rows_ss_pt(C.byref(cfg), pos_lo, centre, road, bits, s, y0, y1, channels, host.ctypes.data + GUARD, need))
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels)


# ---- 1. the renders ------------------------------------------------------------------------------------------------------------


def test_the_smallest_workspace_gives_the_band_counts_the_cases_rely_on(fr, lib):
    cfg = fr.Config.new()
    cfg.width, cfg.height = 13, 20
    assert band_count(13, 20, 3, workspace(lib, cfg, 3, 0, 20)[0]) == 3
    cfg.width, cfg.height = 16, 12
    assert band_count(16, 12, 2, workspace(lib, cfg, 2, 0, 12)[0]) == 2
    assert band_count(16, 12, 2, workspace(lib, cfg, 2, 0, 12)[1]) == 1


@pytest.mark.parametrize("s", [2, 3, 5])
@pytest.mark.parametrize("name", list(RENDER_VIEWS))
def test_supersampled_deep_render_is_the_filtered_plain_render(fr, native, lib, torch, name, s):
    d = Deep(fr, native, name, s)
    h = d.cfg.height
    for road, bits in d.roads:
        big = d.yardstick(lib, road, bits)
        want = {3: np_filter(big, s, 3), 4: np_filter(big, s, 4)}
        for y0, y1 in [(0, h), (5, 11)]:
            mn, best = workspace(lib, d.cfg, s, y0, y1)
            assert 0 < mn <= best
            for work_len in sorted({mn, best}):
                for channels in (3, 4):
                    got = ss_pt_device(torch, lib, d.cfg, d.c, road, bits, s, y0, y1, channels, work_len)
                    assert np.array_equal(got, want[channels][y0:y1]), (name, road, bits, y0, y1, work_len, channels,
                                                                        int((got != want[channels][y0:y1]).sum()))
            for channels in (3, 4):  # the host form is the device form
                got = ss_pt_host(lib, d.cfg, d.c, road, bits, s, y0, y1, channels)
                assert np.array_equal(got, want[channels][y0:y1]), (name, road, bits, y0, y1, channels, "host")


@pytest.mark.parametrize("name", list(RENDER_VIEWS))
def test_supersample_one_is_the_roads_plain_render(fr, native, lib, torch, name):
    d = Deep(fr, native, name, 1)
    h = d.cfg.height
    assert workspace(lib, d.cfg, 1, 0, h) == (0, 0)
    for road, bits in d.roads:
        for channels in (3, 4):
            want = d.plain(lib, road, bits, channels=channels)
            assert len(np.unique(want.reshape(-1, channels), axis=0)) > 1
            assert np.array_equal(ss_pt_device(torch, lib, d.cfg, d.c, road, bits, 1, 0, h, channels, 0), want)
            assert np.array_equal(ss_pt_device(torch, lib, d.cfg, d.c, road, bits, 1, 5, 11, channels, 0), want[5:11])
            assert np.array_equal(ss_pt_host(lib, d.cfg, d.c, road, bits, 1, 0, h, channels), want)


def test_plain_road_without_a_centre_is_fr_render_rows_ss_in_pt(fr, native, lib, torch):
    cfg = fr.Config.new()
    lo = PM.seahorse_view(cfg)
    plo = C.byref(native.Imaginary(*lo))
    for s in (1, 2, 3):
        for channels in (3, 4):
            want = np.zeros((cfg.height, cfg.width, channels), dtype=np.uint8)
            check(lib.fr_render_rows_ss(C.byref(cfg), PT, plo, s, 0, cfg.height, channels, want.ctypes.data, want.nbytes, None))
            assert len(np.unique(want.reshape(-1, channels), axis=0)) > 10
            mn, best = workspace(lib, cfg, s, 0, cfg.height)
            for work_len in sorted({mn, best}):
                got = ss_pt_device(torch, lib, cfg, None, PLAIN, 0, s, 0, cfg.height, channels, work_len, pos_lo=plo)
                assert np.array_equal(got, want), (s, channels, work_len)
            assert np.array_equal(ss_pt_host(lib, cfg, None, PLAIN, 0, s, 0, cfg.height, channels, pos_lo=plo), want)
    # BLA-PT on the dd centre
    want = np.zeros((2 * cfg.height, 2 * cfg.width, 3), dtype=np.uint8)
    cfg_s = cfg.clone()
    cfg_s.width, cfg_s.height = 2 * cfg.width, 2 * cfg.height
    check(lib.fr_render_rows_pt_bla(C.byref(cfg_s), plo, None, 0, 0, cfg_s.height, 3, want.ctypes.data, want.nbytes))
    got = ss_pt_device(torch, lib, cfg, None, BLA, 0, 2, 0, cfg.height, 3, workspace(lib, cfg, 2, 0, cfg.height)[0], pos_lo=plo)
    assert np.array_equal(got, np_filter(want, 2))
    assert np.array_equal(fr.get_image_ss_pt(cfg, 2, pos_lo=lo, bla=0), np_filter(want, 2))


def test_python_front_end(fr, native, lib):
    d = Deep(fr, native, "J-2^900", 3)
    centre = fr.WideCentre(d.v.n, d.v.words[0], d.v.words[1])
    big = d.yardstick(lib, SCALED, 40)
    assert np.array_equal(fr.get_image_ss_pt(d.cfg, 3, centre=centre, scaled=True, bla=40), np_filter(big, 3))
    assert np.array_equal(fr.get_image_ss_pt(d.cfg, 3, centre=centre, scaled=True, bla=40, y0=5, y1=11, channels=4), np_filter(big, 3, 4)[5:11])
    big = d.yardstick(lib, SCALED, -1)
    assert np.array_equal(fr.get_image_ss_pt(d.cfg, 3, centre=centre, scaled=True), np_filter(big, 3))
    d = Deep(fr, native, "J-2^300", 2)
    centre = fr.WideCentre(d.v.n, d.v.words[0], d.v.words[1])
    assert np.array_equal(fr.get_image_ss_pt(d.cfg, 2, centre=centre), np_filter(d.yardstick(lib, PLAIN, 0), 2))
    assert np.array_equal(fr.get_image_ss_pt(d.cfg, 2, centre=centre, bla=0), np_filter(d.yardstick(lib, BLA, 0), 2))


def test_cli_supersamples_the_deep_roads(fr, native, lib, tmp_path):
    import __graft_entry__ as ge

    ge.build()
    pkg = os.path.join(ROOT, "fractal-renderer_amd")
    exe = os.path.join(ROOT, "tests", "cpp", "fractal_cli")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(pkg, "host"), os.path.join(pkg, "cli", "fractal_cli.cpp"), "-L" + pkg, "-lfractal_hip",
                    "-Wl,-rpath," + pkg, "-o", exe], check=True)
    scale = 2.0 ** 300
    re, im = W.centre("M")
    tre, tim = W.decimal_text(re, 140), W.decimal_text(im, 140)
    centre = fr.WideCentre.from_str(tre, tim, scale=scale)
    st = centre.c_struct()
    for s, flags, road, bits, floor in ((2, [], PLAIN, 0, 0.25), (3, ["--scaled"], SCALED, -1, 0.25), (2, ["--bla"], BLA, 0, 0.25)):
        out = str(tmp_path / ("deep%d%d" % (s, road)))
        r = subprocess.run([exe, "--perturbation", *flags, "--supersample", str(s), "-x", tre, "-y", tim, "-s", repr(scale), "-i", "5000",
                            "-l", "2", "-e", "150", "16", "12", "-o", out, "--quiet"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        data = open(out + ".ppm", "rb").read().split(b"\n", 3)
        assert data[0] == b"P6" and data[1] == b"16 12"
        got = np.frombuffer(data[3], dtype=np.uint8).reshape(12, 16, 3)
        ocfg = O.cli_config(16 * s, 12 * s, scale=(scale, scale), iterations=5000, limit=2.0, exposure=150.0, pos=(float(tre), float(tim)))
        cfg_s = fr.Config.from_buffer_copy(bytes(ocfg))
        big = np.zeros((12 * s, 16 * s, 3), dtype=np.uint8)
        tail = (0, cfg_s.height, 3, big.ctypes.data, big.nbytes)
        if road == PLAIN:
            check(lib.fr_render_rows_pt_wide(C.byref(cfg_s), C.byref(st), *tail))
        elif road == BLA:
            check(lib.fr_render_rows_pt_bla(C.byref(cfg_s), None, C.byref(st), bits, *tail))
        else:
            check(lib.fr_render_rows_pt_scaled(C.byref(cfg_s), C.byref(st), bits, *tail))
        assert mixed_share(big, s) >= floor
        assert np.array_equal(got, np_filter(big, s)), (s, flags)
    # what --perturbation still does not combine with is refused
    r = subprocess.run([exe, "--perturbation", "--supersample", "2", "--devices", "0", "4", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "--perturbation" in r.stderr and "--supersample" not in r.stderr


def test_orbit_and_table_are_made_once_per_call(fr, native, lib, torch):
    """three bands: the first computes the orbit (and builds the table), the last finds them in the context's caches"""
    other = Deep(fr, native, "J-2^300", 2)
    d = Deep(fr, native, "M-2^300-e150", 3, size=(13, 20))
    mn, _ = workspace(lib, d.cfg, 3, 0, 20)
    assert band_count(13, 20, 3, mn) == 3
    want = np_filter(d.yardstick(lib, BLA, 0), 3)
    other.plain(lib, BLA, 0)  # the caches now hold another view
    assert fr.bla_cache()[3] == 1 and fr.pt_orbit_cache()[3] > 0
    assert np.array_equal(ss_pt_device(torch, lib, d.cfg, d.c, BLA, 0, 3, 0, 20, 3, mn), want)
    assert fr.bla_cache()[3] == 0 and fr.pt_orbit_cache()[3] == 0
    assert fr.pt_orbit_cache()[0] == d.cfg.iterations
    d = Deep(fr, native, "M-2^900-13x20", 3)
    for bits in (-1, 40):
        want = np_filter(d.yardstick(lib, SCALED, bits), 3)
        other.plain(lib, BLA, 0)
        assert fr.bla_cache()[3] == 1 and fr.pt_orbit_cache()[3] > 0
        assert np.array_equal(ss_pt_device(torch, lib, d.cfg, d.c, SCALED, bits, 3, 0, 20, 3, mn), want)
        assert fr.pt_orbit_cache()[3] == 0 and fr.pt_orbit_cache()[0] == d.cfg.iterations
        if bits >= 0:
            assert fr.bla_cache()[3] == 0 and fr.bla_cache()[0] == 40


def test_profiling_reports_the_roads_kernel_and_the_whole_span(fr, native, lib, torch):
    """On every road: the name is the road's kernel, and the span of a many-band call is at least what the road's plain call
    reports for the same rows of cfg_s, [s y0, s y1) in one call: the bands' kernels together do that kernel's work in two
    or three launches, and the filters and the gaps between the launches come on top.  Each side is the smallest of three
    measurements after a warm-up round: the usual estimator of a device time under other people's load.
    The sum of the plain call's figures over the BANDS, each called alone, is printed beside it and is no bound: every such
    call's events also hold the idle time between its first event and its kernel (the host finds the orbit and the table
    in between), which a banded call spends once, not once per band.  Measured on an MI355X, smallest of three, ms —
    SCALED bits -1: bands 0.334, span 0.349; bits 40: 0.076, 0.088; wide PT: 0.209, 0.212; BLA-PT: 0.6860, 0.6857."""
    dev = torch.device("cuda", 0)
    ms, name = C.c_float(), C.create_string_buffer(160)

    def plain_band(d, road, bits, ya, yb, big):
        tail = (ya, yb, 3, big.data_ptr(), big.numel(), None)
        if road == PLAIN:
            check(lib.fr_render_rows_pt_wide_device(C.byref(d.cfg_s), d.c, *tail))
        elif road == BLA:
            check(lib.fr_render_rows_pt_bla_device(C.byref(d.cfg_s), None, d.c, bits, *tail))
        else:
            check(lib.fr_render_rows_pt_scaled_device(C.byref(d.cfg_s), d.c, bits, *tail))

    three = Deep(fr, native, "M-2^900-13x20", 3), [(0, 24), (24, 48), (48, 60)]
    two = Deep(fr, native, "J-2^300", 2), [(0, 16), (16, 24)]
    cases = [(three, SCALED, -1, b"escape_pt_scaled_kernel"), (three, SCALED, 40, b"escape_bla_scaled_kernel"),
             (two, PLAIN, 0, b"escape_pt_kernel"), (two, BLA, 0, b"escape_bla_kernel")]
    check(lib.fr_set_profiling(1))
    try:
        for (d, bands), road, bits, kernel in cases:
            h = d.cfg.height
            mn, _ = workspace(lib, d.cfg, d.s, 0, h)
            assert band_count(d.cfg.width, h, d.s, mn) == len(bands) and bands[-1][1] == d.cfg_s.height
            big = torch.zeros(3 * d.cfg_s.width * d.cfg_s.height, dtype=torch.uint8, device=dev)
            plain_sums, plain_whole, spans = [], [], []
            for rep in range(4):
                plain_band(d, road, bits, 0, d.cfg_s.height, big)
                check(lib.fr_last_kernel_ms(C.byref(ms)))
                whole = ms.value
                total = 0.0
                for ya, yb in bands:
                    plain_band(d, road, bits, ya, yb, big)
                    check(lib.fr_last_kernel_ms(C.byref(ms)))
                    total += ms.value
                ss_pt_device(torch, lib, d.cfg, d.c, road, bits, d.s, 0, h, 3, mn)
                check(lib.fr_last_kernel_ms(C.byref(ms)))
                check(lib.fr_last_kernel_name(name, len(name)))
                assert name.value == kernel, name.value
                if rep:  # the first round warms up
                    plain_sums.append(total)
                    plain_whole.append(whole)
                    spans.append(ms.value)
            print("road %d bits %d: plain call %s ms, its bands summed %s ms, supersampled spans %s ms"
                  % (road, bits, plain_whole, plain_sums, spans))
            assert min(spans) >= min(plain_whole) > 0, (road, bits, spans, plain_whole)
    finally:
        check(lib.fr_set_profiling(0))


# ---- 2. the fused recolour: colour_filter_kernel --------------------------------------------------------------------------------

# the kernel's constants (fr_ss.hip): a tile is CF_TILE_W output pixels wide — one wave of 64 lanes per output row — and
# cf_tile_rows(s) output rows high; s = 1 goes to colour_rows_kernel, whose waves and helpings are 64 and 256 pixels
CF_TILE_W = 64
CF_THREADS = 256


def cf_tile_rows(s):
    return 4 if s <= 4 else 2 if s <= 6 else 1


WIDTHS = [1, 37, CF_TILE_W - 1, CF_TILE_W, CF_TILE_W + 1, 2 * CF_TILE_W - 1, 2 * CF_TILE_W, 2 * CF_TILE_W + 1, CF_THREADS + 1]


def rows_for(s):
    ro = cf_tile_rows(s)
    return sorted({1, ro - 1, ro, ro + 1, 2 * ro + 1} - {0})


def colour_config(fr, smooth=True, inside=True, cap=1000):
    cfg = fr.Config.new()
    cfg.iterations = cap
    cfg.smooth, cfg.inside = int(smooth), int(inside)
    return cfg


def synthetic(width, rows, s, cap, seed):
    """|z|^2 log-uniform over 2^-20 .. 2^40 at a random angle, iters uniform over 0 .. cap with a tenth at exactly cap"""
    rng = np.random.default_rng(seed)
    shape = (s * rows, s * width)
    r = np.exp2(rng.uniform(-20.0, 40.0, shape) / 2)
    a = rng.uniform(0.0, 2 * np.pi, shape)
    z = np.stack([r * np.cos(a), r * np.sin(a)], axis=-1)
    it = rng.integers(0, cap + 1, shape, dtype=np.uint32)
    it[rng.random(shape) < 0.1] = cap
    return z, it


def composition(lib, cfg, z2, it, s, channels):
    """fr_box_filter_rgb8(fr_colour_rgb8(...)): the yardstick, two host calls the library already had"""
    z2 = np.ascontiguousarray(z2, dtype=np.float64)
    n = it.size
    rgb = np.zeros((it.shape[0], it.shape[1], 3), dtype=np.uint8)
    check(lib.fr_colour_rgb8(C.byref(cfg), z2.ctypes.data, it.ctypes.data, n, rgb.ctypes.data, rgb.nbytes))
    rows, width = it.shape[0] // s, it.shape[1] // s
    out = np.zeros((rows, width, channels), dtype=np.uint8)
    check(lib.fr_box_filter_rgb8(rgb.ctypes.data, width, rows, s, channels, out.ctypes.data, out.nbytes))
    return out, rgb


def colour_ss_device(torch, lib, cfg, z, it, s, channels, dst_off=0, z_off=0):
    """fr_colour_rows_ss_device over numpy arrays placed in guarded device buffers: the output dst_off bytes behind a
    16-byte boundary, z z_off (0 or 8) bytes behind one"""
    dev = torch.device("cuda", 0)
    z = np.ascontiguousarray(z, dtype=np.float64)
    zw = z.shape[-1]
    rows, width = it.shape[0] // s, it.shape[1] // s
    d_z = torch.zeros(z.size * 8 + 16, dtype=torch.uint8, device=dev)
    d_z[z_off:z_off + z.size * 8] = torch.from_numpy(z.reshape(-1).view(np.uint8)).to(dev)
    d_it = torch.from_numpy(np.ascontiguousarray(it).reshape(-1).view(np.int32)).to(dev)
    need = channels * width * rows
    d_out = torch.full((GUARD + 16 + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert d_z.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    at = GUARD + dst_off
    torch.cuda.synchronize()
    check(lib.fr_colour_rows_ss_device(C.byref(cfg), d_z.data_ptr() + z_off, zw, d_it.data_ptr(), width, rows, s, channels,
                                       d_out.data_ptr() + at, need, None))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:at] == 0xA5).all() and (host[at + need:] == 0xA5).all(), "the kernel wrote outside its destination"
    return host[at:at + need].reshape(rows, width, channels)


@pytest.mark.parametrize("s", range(1, 9))
def test_fused_recolour_is_the_composition_on_synthetic_results(fr, lib, torch, s):
    cap = 1000
    flags = [(True, True), (True, False), (False, True), (False, False)]
    k = 0
    for width in WIDTHS:
        for rows in rows_for(s):
            z, it = synthetic(width, rows, s, cap, 100 * s + width + 7 * rows)
            for smooth, inside in flags:
                cfg = colour_config(fr, smooth, inside, cap)
                want3, rgb = composition(lib, cfg, z, it, s, 3)
                if width * rows >= 64:  # the inputs reach every branch of the colour map, and blocks mix
                    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > (8 if inside or smooth else 4)
                offs = range(4) if width in (37, CF_TILE_W + 1, 2 * CF_TILE_W + 1) else (k % 4,)
                for off in offs:
                    got = colour_ss_device(torch, lib, cfg, z, it, s, 3, dst_off=off, z_off=8 * (k & 1))
                    assert np.array_equal(got, want3), (s, width, rows, smooth, inside, off, int((got != want3).sum()))
                want4, _ = composition(lib, cfg, z, it, s, 4)
                got = colour_ss_device(torch, lib, cfg, z, it, s, 4, dst_off=4 * (k % 3), z_off=8 * (k & 1))
                assert np.array_equal(got, want4), (s, width, rows, smooth, inside, "rgba")
                k += 1
    # the host form and the Python front end
    z, it = synthetic(2 * CF_TILE_W + 1, 2 * cf_tile_rows(s) + 1, s, cap, 9000 + s)
    cfg = colour_config(fr, True, True, cap)
    for channels in (3, 4):
        want, _ = composition(lib, cfg, z, it, s, channels)
        assert np.array_equal(fr.colour_image_ss(cfg, z, it, s, channels=channels), want), (s, channels)


def real_results(fr, lib, s):
    """(name, colour config, z [s*rows, s*width, 2 or 4], iters) of real views at cfg_s"""
    w, h = 37, 21
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = s * w, s * h, 256
    z, it = fr.escape_rows(cfg)
    yield "default", cfg, z, it
    jul = fr.Config.from_buffer_copy(bytes(O.cli_config(s * w, s * h, O.JULIA, iterations=300, julia_set=(-0.8, 0.156))))
    z, it = fr.escape_rows(jul)
    yield "julia", jul, z, it
    deep = fr.Config.new()
    DM.deep_view(deep, False, s * 24, s * 16)
    deep.exposure = 150.0
    z4, it = fr.escape_rows(deep, precision=fr.Precision.DD, pos_lo=(0.0, 2.0 ** -66), with_lo=True)
    assert z4.shape[-1] == 4 and np.any(z4[..., 1::2] != 0)
    yield "deep-dd", deep, z4, it


@pytest.mark.parametrize("s", range(1, 9))
def test_fused_recolour_is_the_composition_on_real_results(fr, lib, torch, s):
    for name, cfg, z, it in real_results(fr, lib, s):
        z2 = z if z.shape[-1] == 2 else z[..., 0::2]  # colour on the hi parts
        for smooth, inside in ((True, True), (False, False)):
            c = cfg.clone()
            c.smooth, c.inside = int(smooth), int(inside)
            want3, rgb = composition(lib, c, z2, it, s, 3)
            assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 8, name
            if s > 1:
                assert mixed_share(rgb, s) >= 0.05, name
            for off in range(4):
                got = colour_ss_device(torch, lib, c, z, it, s, 3, dst_off=off)
                assert np.array_equal(got, want3), (name, s, smooth, inside, off, int((got != want3).sum()))
            want4, _ = composition(lib, c, z2, it, s, 4)
            assert np.array_equal(colour_ss_device(torch, lib, c, z, it, s, 4, z_off=8), want4), (name, s, "rgba")
            assert np.array_equal(fr.colour_image_ss(c, z, it, s), want3), (name, s, "host form")
        # s = 1 is fr_colour_rows_device
        if s == 1:
            assert np.array_equal(colour_ss_device(torch, lib, cfg, z, it, 1, 3), fr.colour_image(cfg, z2, it))


def test_fused_recolour_of_the_fern_is_black(fr, lib, torch):
    for s in (1, 2, 5, 8):
        z, it = synthetic(70, 5, s, 1000, s)
        cfg = colour_config(fr)
        cfg.algo = int(fr.Algo.BarnsleyFern)
        assert not colour_ss_device(torch, lib, cfg, z, it, s, 3, dst_off=1).any()
        rgba = colour_ss_device(torch, lib, cfg, z, it, s, 4)
        assert not rgba[..., :3].any() and (rgba[..., 3] == 255).all()


def test_fused_recolour_over_two_to_the_27_samples(fr, lib, torch):
    """2048 x 1024 output pixels at s = 8: 2^27 samples, 2.1 GB of z and 0.5 GB of iters, so byte offsets pass 2^31 and
    2^32 (taken when the device has 8 GB free, which an MI355X has; otherwise 16384 x 1 at s = 8, and the print says which).
    Built and compared on the device; the yardstick is the two existing device calls, fr_colour_rgb8_device and
    fr_box_filter_rgb8_device, through a 400 MB RGB workspace."""
    free, _total = torch.cuda.mem_get_info(0)
    s = 8
    width, rows = (2048, 1024) if free >= (8 << 30) else (16384, 1)
    print("fused recolour at %d x %d output pixels, s = 8 (%.1f GB free)" % (width, rows, free / 2 ** 30))
    n = s * s * width * rows
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(2027)
    cap = 1000
    r = torch.exp2(torch.rand(n, device=dev, generator=g, dtype=torch.float64) * 60.0 - 20.0).sqrt()
    a = torch.rand(n, device=dev, generator=g, dtype=torch.float64) * (2 * np.pi)
    z = torch.stack([r * torch.cos(a), r * torch.sin(a)], dim=-1).contiguous()
    del r, a
    it = torch.randint(0, cap + 1, (n,), device=dev, generator=g, dtype=torch.int32)
    it[torch.rand(n, device=dev, generator=g) < 0.1] = cap
    cfg = colour_config(fr, True, True, cap)
    rgb = torch.zeros(3 * n, dtype=torch.uint8, device=dev)
    check(lib.fr_colour_rgb8_device(C.byref(cfg), z.data_ptr(), it.data_ptr(), n, rgb.data_ptr(), rgb.numel(), None))
    for channels in (3, 4):
        want = torch.zeros(channels * width * rows, dtype=torch.uint8, device=dev)
        check(lib.fr_box_filter_rgb8_device(rgb.data_ptr(), width, rows, s, channels, want.data_ptr(), want.numel(), None))
        got = torch.full((channels * width * rows,), 0xA5, dtype=torch.uint8, device=dev)
        check(lib.fr_colour_rows_ss_device(C.byref(cfg), z.data_ptr(), 2, it.data_ptr(), width, rows, s, channels, got.data_ptr(),
                                           got.numel(), None))
        torch.cuda.synchronize()
        assert torch.equal(got, want), (channels, int((got != want).sum()))
        assert int(want.view(-1, channels)[:, :3].max()) > 100 and len(torch.unique(want)) > 50


def test_a_kept_scaled_view_extended_and_recoloured_is_the_render_at_the_higher_cap(fr, native, lib, torch):
    """the GUI's path: the state of cfg_s at cap N, extended in place to cap M, coloured by the
    fused kernel = fr_render_rows_ss_pt on SCALED PT's plain loop at cap M"""
    s, lower = 2, 560  # the view's escape indices run from 557 to 1341, half of them under 560
    d = Deep(fr, native, "J-2^900", s)
    hs, ws = d.cfg_s.height, d.cfg_s.width
    npx = hs * ws
    dev = torch.device("cuda", 0)
    z, w = (torch.zeros(2 * npx, dtype=torch.float64, device=dev) for _ in range(2))
    it, m = (torch.zeros(npx, dtype=torch.int32, device=dev) for _ in range(2))
    low = d.cfg_s.clone()
    low.iterations = lower
    check(lib.fr_escape_rows_pt_scaled_state_device(C.byref(low), d.c, 0, hs, z.data_ptr(), it.data_ptr(), w.data_ptr(), m.data_ptr(), None))
    torch.cuda.synchronize()
    running = int((it == lower).sum())
    assert 0 < running < npx, "the lower cap must leave some pixels running and some finished (%d of %d run)" % (running, npx)
    out = torch.zeros(3 * d.cfg.width * d.cfg.height, dtype=torch.uint8, device=dev)
    low_out = d.cfg.clone()
    low_out.iterations = lower
    check(lib.fr_colour_rows_ss_device(C.byref(low_out), z.data_ptr(), 2, it.data_ptr(), d.cfg.width, d.cfg.height, s, 3, out.data_ptr(),
                                       out.numel(), None))
    torch.cuda.synchronize()
    low_img = out.cpu().numpy().reshape(d.cfg.height, d.cfg.width, 3)
    assert np.array_equal(low_img, ss_pt_host(lib, low_out, d.c, SCALED, -1, s, 0, d.cfg.height, 3))
    check(lib.fr_escape_extend_pt_scaled_device(C.byref(d.cfg_s), d.c, 0, hs, lower, z.data_ptr(), it.data_ptr(), w.data_ptr(),
                                                m.data_ptr(), None))
    check(lib.fr_colour_rows_ss_device(C.byref(d.cfg), z.data_ptr(), 2, it.data_ptr(), d.cfg.width, d.cfg.height, s, 3, out.data_ptr(),
                                       out.numel(), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(d.cfg.height, d.cfg.width, 3)
    want = ss_pt_host(lib, d.cfg, d.c, SCALED, -1, s, 0, d.cfg.height, 3)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(want, np_filter(d.yardstick(lib, SCALED, -1), s)) and not np.array_equal(want, low_img)


@pytest.mark.parametrize("channels", [3, 4])
def test_host_form_under_a_cap_below_min_bytes_is_the_device_form(fr, native, lib, torch, channels):
    """fr_render_rows_ss_pt on BLA-PT (test_gpu_ss.py: host_bands_are_the_device_forms)"""
    from test_gpu_ss import HOOK_H, HOOK_S, HOOK_W, HOOK_Y0, HOOK_Y1, host_bands_are_the_device_forms

    d = Deep(fr, native, "J-2^300", HOOK_S, size=(HOOK_W, HOOK_H))
    sizes = host_bands_are_the_device_forms(
        lib, 3, lambda n: ss_pt_device(torch, lib, d.cfg, d.c, BLA, 0, HOOK_S, HOOK_Y0, HOOK_Y1, channels, n),
        lambda: ss_pt_host(lib, d.cfg, d.c, BLA, 0, HOOK_S, HOOK_Y0, HOOK_Y1, channels))
    assert sizes == workspace(lib, d.cfg, HOOK_S, HOOK_Y0, HOOK_Y1)
