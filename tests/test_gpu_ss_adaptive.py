"""ADAPTIVE SUPERSAMPLING on the device (fractal-renderer_amd/csrc/fr_ss_adaptive.hip; include/fractal_hip.h), byte for byte,
no tolerance anywhere.  The yardstick is always a call the library already had, never the code under test:
  - threshold -1 against fr_render_rows_ss / fr_render_rows_ss_pt;
  - threshold 255 against the strided samples of the road's plain render of cfg_s;
  - mixed thresholds against the numpy model of the definition (tests/ss_adaptive_model.py) applied to that plain render, the
    refined count included, with the yardstick's edge share asserted to lie in [0.05, 0.95]: a view that degenerates to
    all-edge or no-edge fails loudly;
  - row pieces, RGBA, guards and a canary behind the smallest workspace, the claim loop at forced grids, the fern, the Python
    front end and the command line.
Shapes: the smallest that exercise the kernels — 37 x 29 (odd, two mark tiles across, four down) for every lane mapping
s = 2, 3, 4, 5, 7, 8 (16, 7, 4, 2, 1, 1 entries per wave; idle lanes at 3, 5, 7), 64 x 48, and 1 x 1, 1 x 9, 9 x 1; the deep
roads on the four views of tests/test_gpu_ss_deep.py's RENDER_VIEWS at their own sizes (three at 16 x 12, one at 13 x 20) with
s in {2, 3}, where their edge shares at threshold 0 are 0.069 .. 0.76 (M-2^900-13x20 forced to 16 x 12 would have 0.047 at
s = 2, outside the condition), and PT and BLA-PT on a dd centre at threshold 8 (shares 0.18 and 0.25)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pt_model as PM
import ss_adaptive_model as A
from test_gpu_ss_deep import BLA, PLAIN, RENDER_VIEWS, SCALED, Deep

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, PT = 0, 3
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


def ad_device(torch, lib, cfg, s, tau, y0=0, y1=None, channels=3, precision=F64, pos_lo=None, centre=None, road=PLAIN, bits=0,
              want_refined=True, transfer=None):
    """fr_render_rows_ss_adaptive_device — with a transfer (0 included) fr_render_rows_ss_adaptive_tf_device — into a guarded
    destination, with the SMALLEST workspace and a canary behind it"""
    y1 = cfg.height if y1 is None else y1
    dev = torch.device("cuda", 0)
    need = channels * cfg.width * (y1 - y0)
    n = C.c_size_t()
    check(lib.fr_ss_adaptive_workspace_bytes(C.byref(cfg), s, y0, y1, C.byref(n)))
    work_len = n.value
    assert work_len == A.workspace_bytes(cfg.width, cfg.height, y0, y1)
    d_out = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_work = torch.full((work_len + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    d_n = torch.full((3,), -1, dtype=torch.int64, device=dev)
    assert d_work.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    tail = (tau, y0, y1, channels, d_out.data_ptr() + GUARD, need, d_work.data_ptr(), work_len, d_n.data_ptr() + 8 if want_refined else None,
            None)
    if transfer is not None:
        check(lib.fr_render_rows_ss_adaptive_tf_device(C.byref(cfg), precision, pos_lo, centre, road, bits, s, transfer, *tail))
    else:
        check(lib.fr_render_rows_ss_adaptive_device(C.byref(cfg), precision, pos_lo, centre, road, bits, s, *tail))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    assert (d_work[work_len:].cpu().numpy() == 0x5A).all(), "wrote behind work_len"
    cnt = d_n.cpu().numpy()
    assert cnt[0] == -1 and cnt[2] == -1, "wrote outside d_refined"
    assert want_refined or cnt[1] == -1
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels), int(cnt[1])


def ad_host(lib, cfg, s, tau, y0=0, y1=None, channels=3, precision=F64, pos_lo=None, centre=None, road=PLAIN, bits=0, transfer=None):
    y1 = cfg.height if y1 is None else y1
    need = channels * cfg.width * (y1 - y0)
    host = np.full(GUARD + need + GUARD, 0xA5, dtype=np.uint8)
    n = C.c_uint64(12345)
    tail = (tau, y0, y1, channels, host.ctypes.data + GUARD, need, C.byref(n))
    if transfer is not None:
        check(lib.fr_render_rows_ss_adaptive_tf(C.byref(cfg), precision, pos_lo, centre, road, bits, s, transfer, *tail))
    else:
        check(lib.fr_render_rows_ss_adaptive(C.byref(cfg), precision, pos_lo, centre, road, bits, s, *tail))
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels), n.value


# ---- the F64 views and their yardsticks -------------------------------------------------------------------------------------

F64_VIEWS = ["mandelbrot", "julia", "seahorse"]
_yard = {}


def f64_cfg(fr, view, w, h):
    cfg = fr.Config.new(fr.Algo.Julia) if view == "julia" else fr.Config.new()
    cfg.width, cfg.height = w, h
    if view == "seahorse":
        cfg.pos.re, cfg.pos.im = -0.745, 0.11
        cfg.scale.re = cfg.scale.im = 40.0
        cfg.iterations = 400
    return cfg


def scaled_up(cfg, s):
    c = cfg.clone()
    c.width, c.height = s * cfg.width, s * cfg.height
    return c


def f64_yardstick(fr, view, w, h, s):
    """(cfg, H): the existing plain render of cfg_s, computed once, shared, read-only"""
    key = (view, w, h, s)
    if key not in _yard:
        cfg = f64_cfg(fr, view, w, h)
        big = fr.get_image(scaled_up(cfg, s))
        big.setflags(write=False)
        _yard[key] = (cfg, big)
    return _yard[key]


def mixed(big, s, tau, tag):
    """the model's answer for a mixed threshold, with the condition on the yardstick: its edge share lies in [0.05, 0.95]"""
    share = A.edge_share(big, s, tau)
    print("%s s=%d tau=%d: edge share %.3f" % (tag, s, tau, share))
    assert 0.05 <= share <= 0.95, (tag, s, tau, share)
    return A.adaptive(big, s, tau)


@pytest.mark.parametrize("s", [2, 3, 4, 5, 7, 8])
@pytest.mark.parametrize("view", F64_VIEWS)
def test_f64_against_the_existing_calls_every_lane_mapping(fr, lib, torch, view, s):
    w, h = 37, 29
    cfg, big = f64_yardstick(fr, view, w, h, s)
    p = s // 2
    # threshold -1: the supersampled render's bytes, every pixel refined
    want = fr.get_image(cfg, supersample=s)
    assert np.array_equal(want, A.np_filter(big, s))  # the two yardsticks agree
    got, n = ad_device(torch, lib, cfg, s, -1)
    assert np.array_equal(got, want) and n == w * h, (view, s, int((got != want).sum()), n)
    # threshold 255: the probe image, nothing refined
    got, n = ad_device(torch, lib, cfg, s, 255)
    assert np.array_equal(got, big[p::s, p::s]) and n == 0, (view, s, int((got != big[p::s, p::s]).sum()), n)
    # mixed thresholds: the model on the plain render
    for tau in (8, 40):
        want, count = mixed(big, s, tau, view)
        got, n = ad_device(torch, lib, cfg, s, tau)
        assert np.array_equal(got, want) and n == count, (view, s, tau, int((got != want).sum()), n, count)
        got, n = ad_host(lib, cfg, s, tau)  # the host form is the device form
        assert np.array_equal(got, want) and n == count, (view, s, tau, "host")


@pytest.mark.parametrize("view", F64_VIEWS)
def test_f64_64_by_48_row_pieces_rgba_and_a_null_count(fr, lib, torch, view):
    w, h, s = 64, 48, 4
    cfg, big = f64_yardstick(fr, view, w, h, s)
    for tau in (8, 40):
        want, count = mixed(big, s, tau, view + " 64x48")
        got, n = ad_device(torch, lib, cfg, s, tau)
        assert np.array_equal(got, want) and n == count, (view, tau)
        # [0, 7), [7, 8), [8, h): the first and the last piece have no out-of-image neighbours, the middle one has a neighbour
        # row on either side; guards and canary are ad_device's
        pieces = [ad_device(torch, lib, cfg, s, tau, a, b) for a, b in ((0, 7), (7, 8), (8, h))]
        assert np.array_equal(np.concatenate([q[0] for q in pieces]), want), (view, tau)
        assert sum(q[1] for q in pieces) == count
        rgba, n = ad_device(torch, lib, cfg, s, tau, channels=4)
        assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all() and n == count
        rgba, n = ad_host(lib, cfg, s, tau, 7, 31, channels=4)
        assert np.array_equal(rgba[..., :3], want[7:31]) and (rgba[..., 3] == 255).all() and n == A.adaptive(big, s, tau, 7, 31)[1]
    got, n = ad_device(torch, lib, cfg, s, 8, want_refined=False)  # d_refined may be NULL
    assert np.array_equal(got, A.adaptive(big, s, 8)[0])
    assert lib.fr_render_rows_ss_adaptive(C.byref(cfg), F64, None, None, PLAIN, 0, s, 8, 0, h, 3, got.ctypes.data, got.nbytes, None) == 0


@pytest.mark.parametrize("size", [(1, 1), (1, 9), (9, 1)])
def test_f64_degenerate_sizes(fr, lib, torch, size):
    w, h = size
    for view in ("mandelbrot", "seahorse"):
        for s in (1, 2, 3, 8):
            cfg, big = f64_yardstick(fr, view, w, h, s)
            for tau in (-1, 0, 8, 255):
                want, count = A.adaptive(big, s, tau)
                got, n = ad_device(torch, lib, cfg, s, tau)  # 1 x 1 at the default grid: most waves claim nothing
                assert np.array_equal(got, want) and n == count, (view, size, s, tau)
                got, n = ad_device(torch, lib, cfg, s, tau, channels=4)
                assert np.array_equal(got[..., :3], want) and (got[..., 3] == 255).all() and n == count


@pytest.mark.parametrize("smooth,inside", [(False, True), (True, False), (False, False)])
def test_f64_colour_map_switches(fr, lib, torch, smooth, inside):
    """smooth off: the render takes its colours from a palette, the refine pass computes them per sample — the same bytes"""
    s = 3
    cfg = f64_cfg(fr, "seahorse", 37, 29)
    cfg.smooth, cfg.inside = smooth, inside
    big = fr.get_image(scaled_up(cfg, s))
    got, n = ad_device(torch, lib, cfg, s, -1)
    assert np.array_equal(got, fr.get_image(cfg, supersample=s)) and n == 37 * 29
    want, count = mixed(big, s, 8, "seahorse smooth=%s inside=%s" % (smooth, inside))
    got, n = ad_device(torch, lib, cfg, s, 8)
    assert np.array_equal(got, want) and n == count, (smooth, inside, int((got != want).sum()))


def test_supersample_one_is_the_plain_render_for_every_threshold(fr, lib, torch):
    for view in F64_VIEWS:
        cfg, big = f64_yardstick(fr, view, 37, 29, 1)
        for tau in (-1, 0, 8, 255):
            got, n = ad_device(torch, lib, cfg, 1, tau)
            assert np.array_equal(got, big) and n == A.adaptive(big, 1, tau)[1], (view, tau)


def test_claim_loop_at_forced_grids(fr, lib, torch):
    """one and two workgroups: every wave claims many times; the output does not depend on the grid"""
    try:
        for groups in (1, 2):
            check(lib.fr_debug_ss_adaptive_grid(groups))
            for view, s in (("mandelbrot", 2), ("seahorse", 3), ("julia", 8)):
                cfg, big = f64_yardstick(fr, view, 37, 29, s)
                for tau in (-1, 8):
                    want, count = A.adaptive(big, s, tau)
                    got, n = ad_device(torch, lib, cfg, s, tau)
                    assert np.array_equal(got, want) and n == count, (groups, view, s, tau)
    finally:
        check(lib.fr_debug_ss_adaptive_grid(0))
    assert lib.fr_debug_ss_adaptive_grid((1 << 20) + 1) == 1


def test_the_fern_is_black_and_refines_nothing(fr, lib, torch):
    cfg = fr.Config.new(fr.Algo.BarnsleyFern)
    cfg.width, cfg.height = 37, 29
    for tau in (-1, 8):
        got, n = ad_device(torch, lib, cfg, 3, tau)
        assert not got.any() and n == 0
        got, n = ad_device(torch, lib, cfg, 3, tau, channels=4)
        assert not got[..., :3].any() and (got[..., 3] == 255).all() and n == 0
        got, n = ad_host(lib, cfg, 3, tau)
        assert not got.any() and n == 0


# ---- the deep roads -------------------------------------------------------------------------------------------------------------


def deep_yardstick(d, lib, road, bits):
    """H of a deep view: the road's own plain call on cfg_s (test_gpu_ss_deep.py's Deep.plain), computed once, shared, read-only.
    The condition on it is the edge share, asserted where a mixed threshold is used."""
    key = ("deep", d.name, d.s, d.cfg.width, d.cfg.height, road, bits)
    if key not in _yard:
        big = d.plain(lib, road, bits)
        big.setflags(write=False)
        _yard[key] = big
    return _yard[key]


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", list(RENDER_VIEWS))
def test_deep_roads_against_the_existing_calls(fr, native, lib, torch, name, s):
    """the four views of test_gpu_ss_deep.py's RENDER_VIEWS at their own sizes: three at 16 x 12, one at 13 x 20"""
    d = Deep(fr, native, name, s)
    w, h = d.cfg.width, d.cfg.height
    p = s // 2
    taus = (0, 8) if name.startswith("J") else (0,)  # the M views' shares at 8 fall below 0.07
    for road, bits in d.roads:
        big = deep_yardstick(d, lib, road, bits)
        kw = dict(precision=PT, centre=d.c, road=road, bits=bits)
        want = np.zeros((h, w, 3), dtype=np.uint8)
        check(lib.fr_render_rows_ss_pt(C.byref(d.cfg), None, d.c, road, bits, s, 0, h, 3, want.ctypes.data, want.nbytes))
        got, n = ad_device(torch, lib, d.cfg, s, -1, **kw)
        assert np.array_equal(got, want) and n == w * h, (name, road, bits, int((got != want).sum()))
        got, n = ad_device(torch, lib, d.cfg, s, 255, **kw)
        assert np.array_equal(got, big[p::s, p::s]) and n == 0, (name, road, bits)
        for tau in taus:
            want, count = mixed(big, s, tau, "%s %dx%d road %d bits %d" % (name, w, h, road, bits))
            got, n = ad_device(torch, lib, d.cfg, s, tau, **kw)
            assert np.array_equal(got, want) and n == count, (name, road, bits, tau, int((got != want).sum()), n, count)
            pieces = [ad_device(torch, lib, d.cfg, s, tau, a, b, **kw) for a, b in ((0, 7), (7, 8), (8, h))]
            assert np.array_equal(np.concatenate([q[0] for q in pieces]), want) and sum(q[1] for q in pieces) == count
            rgba, n = ad_host(lib, d.cfg, s, tau, channels=4, **kw)
            assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all() and n == count


def test_pt_on_a_dd_centre(fr, native, lib, torch):
    cfg = fr.Config.new()
    lo = PM.seahorse_view(cfg, width=16, height=12)  # cap 20000: at threshold 8 its edge share is 0.18 (s = 2), 0.25 (s = 3)
    plo = C.byref(native.Imaginary(*lo))
    for s in (2, 3):
        cfg_s = scaled_up(cfg, s)
        big = fr.get_image(cfg_s, fr.Precision.PT, pos_lo=lo)
        p = s // 2
        want = fr.get_image(cfg, fr.Precision.PT, pos_lo=lo, supersample=s)
        got, n = ad_device(torch, lib, cfg, s, -1, precision=PT, pos_lo=plo)
        assert np.array_equal(got, want) and n == 16 * 12
        got, n = ad_device(torch, lib, cfg, s, 255, precision=PT, pos_lo=plo)
        assert np.array_equal(got, big[p::s, p::s]) and n == 0
        want, count = mixed(big, s, 8, "dd seahorse")
        got, n = ad_device(torch, lib, cfg, s, 8, precision=PT, pos_lo=plo)
        assert np.array_equal(got, want) and n == count
        # BLA-PT on the dd centre, and plain PT with neither pos_lo nor a centre
        big_bla = np.zeros_like(big)
        check(lib.fr_render_rows_pt_bla(C.byref(cfg_s), plo, None, 0, 0, cfg_s.height, 3, big_bla.ctypes.data, big_bla.nbytes))
        want, count = mixed(big_bla, s, 8, "dd seahorse, BLA-PT")
        got, n = ad_device(torch, lib, cfg, s, 8, precision=PT, pos_lo=plo, road=BLA)
        assert np.array_equal(got, want) and n == count
        big0 = fr.get_image(cfg_s, fr.Precision.PT)
        want, count = A.adaptive(big0, s, 8)  # pos alone is another point of the plane: compared, no condition on it
        got, n = ad_device(torch, lib, cfg, s, 8, precision=PT)
        assert np.array_equal(got, want) and n == count


# ---- the front ends ---------------------------------------------------------------------------------------------------------------


def test_python_front_end(fr, native, lib):
    cfg, big = f64_yardstick(fr, "seahorse", 37, 29, 3)
    want, count = A.adaptive(big, 3, 8)
    img, n = fr.get_image_ss_adaptive(cfg, 3)  # threshold 8 is the default
    assert np.array_equal(img, want) and n == count
    assert ad_host(lib, cfg, 3, 8)[1] == n
    img, n = fr.get_image_ss_adaptive(cfg, 3, threshold=40, y0=5, y1=11, channels=4)
    w2, c2 = A.adaptive(big, 3, 40, 5, 11, channels=4)
    assert np.array_equal(img, w2) and n == c2
    d = Deep(fr, native, "J-2^900", 3)
    centre = fr.WideCentre(d.v.n, d.v.words[0], d.v.words[1])
    for bla, bits in ((40, 40), (None, -1)):
        want, count = A.adaptive(deep_yardstick(d, lib, SCALED, bits), 3, 8)
        img, n = fr.get_image_ss_adaptive(d.cfg, 3, precision=fr.Precision.PT, centre=centre, scaled=True, bla=bla)
        assert np.array_equal(img, want) and n == count
    d = Deep(fr, native, "J-2^300", 2)
    centre = fr.WideCentre(d.v.n, d.v.words[0], d.v.words[1])
    for bla, road in ((None, PLAIN), (0, BLA)):
        want, count = A.adaptive(deep_yardstick(d, lib, road, 0), 2, 0)
        img, n = fr.get_image_ss_adaptive(d.cfg, 2, threshold=0, precision=fr.Precision.PT, centre=centre, bla=bla)
        assert np.array_equal(img, want) and n == count


def test_cli_adaptive(fr, native, lib, tmp_path):
    import __graft_entry__ as ge

    ge.build()
    pkg = os.path.join(ROOT, "fractal-renderer_amd")
    exe = os.path.join(ROOT, "tests", "cpp", "fractal_cli")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(pkg, "host"), os.path.join(pkg, "cli", "fractal_cli.cpp"), "-L" + pkg, "-lfractal_hip",
                    "-Wl,-rpath," + pkg, "-o", exe], check=True)

    def ppm(path, w, h):
        data = open(path + ".ppm", "rb").read().split(b"\n", 3)
        assert data[0] == b"P6" and data[1] == b"%d %d" % (w, h)
        return np.frombuffer(data[3], dtype=np.uint8).reshape(h, w, 3)

    # the F64 road, the default threshold and an explicit one; the refined share is printed unless --quiet
    for flag, tau in ((["--adaptive"], 8), (["--adaptive=40"], 40)):
        out = str(tmp_path / ("f64_%d" % tau))
        r = subprocess.run([exe, "--supersample", "3", *flag, "-x", "-0.745", "-y", "0.11", "-s", "40", "-i", "400", "37", "29", "-o", out],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        ocfg = O.cli_config(37, 29, scale=(40.0, 40.0), iterations=400, pos=(-0.745, 0.11))
        cfg = fr.Config.from_buffer_copy(bytes(ocfg))
        want, count = ad_host(lib, cfg, 3, tau)  # the C call
        assert 0 < count < 37 * 29
        assert np.array_equal(ppm(out, 37, 29), want), flag
        assert "refined %d of %d" % (count, 37 * 29) in r.stdout, r.stdout
        r = subprocess.run([exe, "--supersample", "3", *flag, "-x", "-0.745", "-y", "0.11", "-s", "40", "-i", "400", "37", "29", "-o", out,
                            "--quiet"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "refined" not in r.stdout
    # the deep roads
    import pt_wide_model as W

    scale = 2.0 ** 300
    re, im = W.centre("M")
    tre, tim = W.decimal_text(re, 140), W.decimal_text(im, 140)
    st = fr.WideCentre.from_str(tre, tim, scale=scale).c_struct()
    for s, flags, road, bits in ((2, [], PLAIN, 0), (3, ["--scaled"], SCALED, -1), (2, ["--bla"], BLA, 0)):
        out = str(tmp_path / ("deep%d%d" % (s, road)))
        r = subprocess.run([exe, "--perturbation", *flags, "--supersample", str(s), "--adaptive=0", "-x", tre, "-y", tim, "-s",
                            repr(scale), "-i", "5000", "-l", "2", "-e", "150", "16", "12", "-o", out, "--quiet"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        ocfg = O.cli_config(16, 12, scale=(scale, scale), iterations=5000, limit=2.0, exposure=150.0, pos=(float(tre), float(tim)))
        cfg = fr.Config.from_buffer_copy(bytes(ocfg))
        want, count = ad_host(lib, cfg, s, 0, precision=PT, centre=C.byref(st), road=road, bits=bits)
        assert 0 < count < 16 * 12
        assert np.array_equal(ppm(out, 16, 12), want), flags
    # refused without --supersample, and with --distance-shade
    r = subprocess.run([exe, "--adaptive", "4", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "--adaptive" in r.stderr and "--supersample" in r.stderr
    r = subprocess.run([exe, "--supersample", "2", "--adaptive", "--distance-shade", "1", "4", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "--adaptive" in r.stderr and "--distance-shade" in r.stderr


# ---- the host form's row pieces ---------------------------------------------------------------------------------------------------

HOOK_W, HOOK_H, HOOK_S, HOOK_Y0, HOOK_Y1 = 37, 21, 3, 2, 19
HOOK_CHAIN = [17, 9, 5, 3, 2, 1]  # the piece sizes the host form can arrive at from 17 rows: it halves, rounding up


def hook_caps(workspace_bytes):
    """piece size -> the cap that forces it: the workspace of a piece of n rows with a neighbour row on either side, which the next
    larger piece of the chain does not fit"""
    caps = {}
    for n in (5, 2, 1):  # 5 + 5 + 5 + 2, eight twos and a one, seventeen ones: the last piece is ragged in the first two
        caps[n] = workspace_bytes(HOOK_W, HOOK_H, HOOK_Y0, HOOK_Y0 + n)
        larger = HOOK_CHAIN[HOOK_CHAIN.index(n) - 1]
        assert caps[n] % 8 == 0 and workspace_bytes(HOOK_W, HOOK_H, HOOK_Y0, HOOK_Y0 + larger) > caps[n]
    return caps


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("road", ["f64", "pt"])
def test_host_form_by_row_pieces_is_the_device_form(fr, native, lib, torch, road, channels):
    """fr_debug_ss_host_work_cap forces the row-piece loop, which runs only above 256 MiB otherwise: pieces of 5, 2 and 1 rows
    give the device form's bytes over the whole range and its count"""
    if road == "f64":
        cfg, kw, tau = f64_cfg(fr, "seahorse", HOOK_W, HOOK_H), dict(), 8
    else:
        d = Deep(fr, native, "J-2^300", HOOK_S, size=(HOOK_W, HOOK_H))
        cfg, kw, tau = d.cfg, dict(precision=PT, centre=d.c, road=PLAIN, bits=0), 8
    want, count = ad_device(torch, lib, cfg, HOOK_S, tau, HOOK_Y0, HOOK_Y1, channels, **kw)
    assert 0 < count < HOOK_W * (HOOK_Y1 - HOOK_Y0), count
    assert lib.fr_debug_ss_host_work_cap(12) == 1  # not a multiple of 8
    try:
        for n, cap in hook_caps(A.workspace_bytes).items():
            check(lib.fr_debug_ss_host_work_cap(cap))
            got, refined = ad_host(lib, cfg, HOOK_S, tau, HOOK_Y0, HOOK_Y1, channels, **kw)
            assert np.array_equal(got, want) and refined == count, (n, cap, int((got != want).sum()), refined, count)
    finally:
        check(lib.fr_debug_ss_host_work_cap(0))
