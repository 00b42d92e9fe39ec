"""ADAPTIVE SUPERSAMPLED DE on the device (include/fractal_hip.h; csrc/fr_ss_adaptive_de.hip: ss_mark_de_kernel; fr_de.hip,
fr_de_bla.hip: ss_refine_de_*_kernel), byte for byte and count for count, no tolerance anywhere.  The yardstick is never the
code under test: it is the road's EXISTING DE call for cfg_s on the device (escape_rows_de: fr_escape_rows_de,
fr_escape_rows_de_pt_wide, fr_escape_rows_de_pt_bla), whose arrays are fed to the numpy model of tests/ss_adaptive_de_model.py.
Every output and every workspace lies between two 64-byte guards.  Each render case asserts on the yardstick that it cannot pass
emptily: 0 < refined < width * rows, and — where the reach is not 0 — at least one pixel that `near` marks and the colour rule does
not.  The degenerate sizes are exempt from the first condition only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import de_model as DE
import pt_model as PM
import pt_wide_model as W
import ss_adaptive_de_model as M
import ss_adaptive_model as A
import ss_de_model as SD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
T, TAU, REACH = 1.5, 8, 2.0
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


def c_args(kw):
    """(precision, pos_lo, centre, road, bits) of the C call for the Python keywords, and what keeps their memory alive; the
    keyword `c_call` holds the five as the C call takes them, kept alive by the caller"""
    from fractal_renderer_amd import _native

    if "c_call" in kw:
        return tuple(kw["c_call"]), None
    lo = None if kw.get("pos_lo") is None else _native.Imaginary(*kw["pos_lo"])
    st = None if kw.get("centre") is None else kw["centre"].c_struct()
    road, bits = (BLA, int(kw["bla"])) if kw.get("bla") is not None else (PLAIN, 0)
    return (int(kw.get("precision", 0)), None if lo is None else C.byref(lo), None if st is None else C.byref(st), road, bits), (lo, st)


def ad_device(torch, lib, cfg, kw, s, thickness, tau, reach, y0=0, y1=None, channels=3, want_refined=True, transfer=None):
    """fr_render_rows_ss_adaptive_de_device — with a transfer (0 included) fr_render_rows_ss_adaptive_de_tf_device — into a guarded
    destination, with the SMALLEST workspace between two guards"""
    y1 = cfg.height if y1 is None else y1
    dev = torch.device("cuda", 0)
    pre, _keep = c_args(kw)
    need = channels * cfg.width * (y1 - y0)
    n = C.c_size_t()
    check(lib.fr_ss_adaptive_de_workspace_bytes(C.byref(cfg), s, y0, y1, C.byref(n)))
    work_len = n.value
    assert work_len == M.workspace_bytes(cfg.width, cfg.height, y0, y1)
    d_out = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_work = torch.full((GUARD + work_len + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    d_n = torch.full((3,), -1, dtype=torch.int64, device=dev)
    assert d_work.data_ptr() % 8 == 0 and d_out.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    tail = (tau, reach, y0, y1, channels, d_out.data_ptr() + GUARD, need, d_work.data_ptr() + GUARD, work_len,
            d_n.data_ptr() + 8 if want_refined else None, None)
    if transfer is not None:
        check(lib.fr_render_rows_ss_adaptive_de_tf_device(C.byref(cfg), *pre, thickness, s, transfer, *tail))
    else:
        check(lib.fr_render_rows_ss_adaptive_de_device(C.byref(cfg), *pre, thickness, s, *tail))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    work = d_work.cpu().numpy()
    assert (work[:GUARD] == 0x5A).all() and (work[GUARD + work_len:] == 0x5A).all(), "wrote outside the workspace"
    cnt = d_n.cpu().numpy()
    assert cnt[0] == -1 and cnt[2] == -1, "wrote outside d_refined"
    assert want_refined or cnt[1] == -1
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels), int(cnt[1])


def ad_host(lib, cfg, kw, s, thickness, tau, reach, y0=0, y1=None, channels=3, transfer=None):
    y1 = cfg.height if y1 is None else y1
    pre, _keep = c_args(kw)
    need = channels * cfg.width * (y1 - y0)
    host = np.full(GUARD + need + GUARD, 0xA5, dtype=np.uint8)
    n = C.c_uint64(12345)
    tail = (tau, reach, y0, y1, channels, host.ctypes.data + GUARD, need, C.byref(n))
    if transfer is not None:
        check(lib.fr_render_rows_ss_adaptive_de_tf(C.byref(cfg), *pre, thickness, s, transfer, *tail))
    else:
        check(lib.fr_render_rows_ss_adaptive_de(C.byref(cfg), *pre, thickness, s, *tail))
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels), n.value


# ---- the views and their yardsticks ---------------------------------------------------------------------------------------------


def wide_centre(fr, name, words):
    ints = W.centre_ints(name, words)
    return fr.WideCentre(words, W.to_words(ints[0], words), W.to_words(ints[1], words))


def view_default(fr, w, h):
    return DE.default_view(fr.Config.new(), w, h), dict()


def view_julia(fr, w, h):
    return DE.julia_view(fr.Config.new(), w, h), dict()


def view_seahorse_f64(fr, w, h):  # F64 at 1e11, cap 3000: 18% of the samples are capped with a derivative past 2^1000
    cfg = fr.Config.new()
    DE.seahorse_shallow(cfg, w, h, 3000)
    return cfg, dict()


# The deep roads, set up as the supersampled DE tests set theirs, with the (t, R) chosen per view on the CPU models (de_model.pt_rows,
# pt_wide_model.Orbits + de_model.pt_wide_rows, de_bla_model.escape_rows) at 41 x 23, T = 1.5, s = 2 and 3.  Both seahorse views lie
# within a fraction of a pixel of the set almost everywhere (the median D of their escaped probes is 0.01 output pixels), so their
# reach is 1/8 pixel and the threshold 64; the wide views are sparse.
def road_pt_dd(fr, w, h):  # edge share 0.80 .. 0.81, 459 .. 479 near-only pixels
    cfg = fr.Config.new()
    lo = DE.seahorse_shallow(cfg, w, h)
    return cfg, dict(precision=fr.Precision.PT, pos_lo=lo)


def road_pt_wide(fr, w, h):  # edge share 0.10, 66 .. 69 near-only pixels
    return W.view(fr.Config.new(), "M", 200, w, h, 3000), dict(precision=fr.Precision.PT, centre=wide_centre(fr, "M", 5))


def road_bla_wide(fr, w, h):  # edge share 0.13, 101 .. 110 near-only pixels
    return W.view(fr.Config.new(), "M", 300, w, h, 5000), dict(precision=fr.Precision.PT, centre=wide_centre(fr, "M", 6), bla=0)


def road_bla_dd(fr, w, h):  # edge share 0.85 .. 0.86, 550 .. 579 near-only pixels
    cfg = fr.Config.new()
    lo = PM.seahorse_view(cfg, w, h)
    return cfg, dict(precision=fr.Precision.PT, pos_lo=lo, bla=0)


VIEWS = {"default": view_default, "julia": view_julia, "seahorse-f64": view_seahorse_f64, "pt-dd": road_pt_dd, "pt-wide": road_pt_wide,
         "bla-wide": road_bla_wide, "bla-dd": road_bla_dd}
DEEP = {"pt-dd": (64, 0.125), "pt-wide": (16, 2.0), "bla-wide": (16, 2.0), "bla-dd": (64, 0.125)}  # (t, R) per view
_yard = {}


def yardstick(fr, name, w, h, s):
    """(cfg, kw, z, iters, der): the road's existing DE call for cfg_s, made once, shared, read-only"""
    key = (name, w, h, s)
    if key not in _yard:
        cfg, kw = VIEWS[name](fr, w, h)
        z, it, der = fr.escape_rows_de(SD.config_s(cfg, s), **kw)
        for a in (z, it, der):
            a.setflags(write=False)
        _yard[key] = cfg, kw, z, it, der
    return _yard[key]


def expected(cfg, z, it, der, s, thickness, tau, reach, tag, degenerate=False):
    """the model's image and count over the yardstick's arrays, with the conditions that keep the case from passing emptily"""
    want, count = M.adaptive_de(cfg, z, it, der, s, thickness, tau, reach)
    lonely = int(M.near_only(cfg, z, it, der, s, thickness, tau, reach).sum())
    print("%s %dx%d s=%d T=%g t=%d R=%g: refined %d of %d, %d near-only" % (tag, cfg.width, cfg.height, s, thickness, tau, reach, count,
                                                                              cfg.width * cfg.height, lonely))
    if not degenerate:  # a 1-pixel-wide or 1-pixel-high image may be all edge or none: exempt from this condition only
        assert 0 < count < cfg.width * cfg.height, (tag, s, count)
    if reach > 0 and not degenerate:
        assert lonely >= 1, (tag, s, "no pixel is refined by the distance rule alone")
    return want, count


# ---- F64: every lane mapping of the claim loop -------------------------------------------------------------------------------------


@pytest.mark.parametrize("s", [2, 3, 4, 5, 7, 8])  # ppw = 16, 7, 4, 2, 1, 1
@pytest.mark.parametrize("view", ["default", "julia"])
def test_f64_every_lane_mapping(fr, lib, torch, view, s):
    for w, h in ((67, 19), (65, 9)):  # no multiple of the 32 x 8 mark tile: halo and ragged waves
        cfg, kw, z, it, der = yardstick(fr, view, w, h, s)
        want, count = expected(cfg, z, it, der, s, T, TAU, REACH, view)
        got, n = ad_device(torch, lib, cfg, kw, s, T, TAU, REACH)
        assert np.array_equal(got, want) and n == count, (view, s, w, h, int((got != want).sum()), n, count)
    got, n = ad_host(lib, cfg, kw, s, T, TAU, REACH)  # the host form is the device form
    assert np.array_equal(got, want) and n == count, (view, s, "host")


@pytest.mark.parametrize("view,w,h", [("julia", 1, 1), ("default", 1, 9), ("default", 63, 1)])
def test_degenerate_sizes(fr, lib, torch, view, w, h):
    """One pixel, one column, one row.  Exempt from 0 < refined < width * rows only — one pixel is all edge or none — and the
    distance rule must still bite: over the supersamples, the view has a pixel that `near` marks and the colour rule does not
    (the 1 x 1 Julia view's at s = 3, where the probe is the centre sample)."""
    lonely = 0
    for s in (2, 3, 8):
        cfg, kw, z, it, der = yardstick(fr, view, w, h, s)
        for tau, reach in ((TAU, REACH), (255, 8.0), (TAU, 0.0), (-1, 0.0)):
            want, count = expected(cfg, z, it, der, s, T, tau, reach, "degenerate " + view, degenerate=True)
            lonely += int(M.near_only(cfg, z, it, der, s, T, tau, reach).sum())
            got, n = ad_device(torch, lib, cfg, kw, s, T, tau, reach)
            assert np.array_equal(got, want) and n == count, (view, w, h, s, tau, reach, n, count)
    assert lonely >= 1, (view, w, h, "no pixel is refined by the distance rule alone")


@pytest.mark.parametrize("view", ["default", "julia"])
def test_row_pieces_rgba_and_a_null_count(fr, lib, torch, view):
    w, h, s = 67, 19, 3
    cfg, kw, z, it, der = yardstick(fr, view, w, h, s)
    want, count = expected(cfg, z, it, der, s, T, TAU, REACH, view)
    pieces, total = [], 0
    for y0, y1 in ((0, 1), (1, 8), (8, h)):
        got, _ = ad_device(torch, lib, cfg, kw, s, T, TAU, REACH, y0, y1, channels=4, want_refined=False)
        assert (got[..., 3] == 255).all()
        pieces.append(got[..., :3])
        m_img, m_n = M.adaptive_de(cfg, z, it, der, s, T, TAU, REACH, y0, y1, channels=4)
        assert np.array_equal(got, m_img), (view, y0, y1)
        got3, n = ad_device(torch, lib, cfg, kw, s, T, TAU, REACH, y0, y1)
        assert np.array_equal(got3, got[..., :3]) and n == m_n, (view, y0, y1, n, m_n)
        total += n
    assert np.array_equal(np.concatenate(pieces), want) and total == count
    got, n = ad_host(lib, cfg, kw, s, T, TAU, REACH, 1, 8, channels=4)
    assert np.array_equal(got[..., :3], want[1:8]) and (got[..., 3] == 255).all()


# ---- the corners of the rule, each against a call the library already had ----------------------------------------------------------------


@pytest.mark.parametrize("view", ["default", "julia"])
def test_rule_corners_against_the_existing_calls(fr, lib, torch, view):
    w, h, s = 67, 19, 4
    cfg, kw, z, it, der = yardstick(fr, view, w, h, s)
    p = s // 2
    H = SD.shaded(cfg, z, it, der, s, T)
    # t = -1: fr_render_rows_ss_de's bytes, every pixel refined, for every R
    full = fr.get_image_de(cfg, T, supersample=s)
    assert np.array_equal(full, SD.box(H, s))  # the two yardsticks agree
    for reach in (0.0, REACH):
        got, n = ad_device(torch, lib, cfg, kw, s, T, -1, reach)
        assert np.array_equal(got, full) and n == w * h, (view, reach, int((got != full).sum()), n)
    # t = 255 with R = 0: the probe image, nothing refined
    got, n = ad_device(torch, lib, cfg, kw, s, T, 255, 0.0)
    assert np.array_equal(got, H[p::s, p::s]) and n == 0
    # t = 255 with a reach: the distance rule alone
    want, count = expected(cfg, z, it, der, s, T, 255, REACH, view + " near alone")
    got, n = ad_device(torch, lib, cfg, kw, s, T, 255, REACH)
    assert np.array_equal(got, want) and n == count
    # R = 0: the colour rule on the shaded bytes
    want, count = A.adaptive(H, s, TAU)
    assert 0 < count < w * h
    got, n = ad_device(torch, lib, cfg, kw, s, T, TAU, 0.0)
    assert np.array_equal(got, want) and n == count, (view, "R = 0", n, count)
    # T = 0 with R = 0: fr_render_rows_ss_adaptive's bytes and count
    want, count = fr.get_image_ss_adaptive(cfg, s, TAU)
    assert 0 < count < w * h
    got, n = ad_device(torch, lib, cfg, kw, s, 0.0, TAU, 0.0)
    assert np.array_equal(got, want) and n == count, (view, "T = 0", n, count)
    # s = 1: the DE render coloured with T, for every t and R
    cfg1, kw1, z1, it1, der1 = yardstick(fr, view, w, h, 1)
    plain = fr.get_image_de(cfg1, T)
    assert np.array_equal(plain, fr.colour_image_de(cfg1, z1, it1, der1, T))
    for tau, reach in ((-1, 0.0), (0, 1.0), (TAU, REACH), (255, 0.0), (255, 3.0)):
        got, n = ad_device(torch, lib, cfg1, kw1, 1, T, tau, reach)
        assert np.array_equal(got, plain), (view, "s = 1", tau, reach)
        assert n == M.adaptive_de(cfg1, z1, it1, der1, 1, T, tau, reach)[1]


def test_tiny_distances_and_capped_probes_with_huge_derivatives(fr, lib, torch):
    """seahorse_shallow at cap 3000 on the F64 road: a sixth of the probes is capped with a derivative past 2^1000 — never near,
    whatever the reach — and the escaped probes' distances go down to 1e-13 pixels: the smallest reaches separate them.  R = 0
    refines none of them by distance.  (No escaped sample of this view has a derivative past 2^121, so none has D = 0: that rule
    is pinned on arrays made by hand in tests/test_ss_adaptive_de_cpu.py.)"""
    w, h = 40, 24
    for s in (2, 3):
        cfg, kw, z, it, der = yardstick(fr, "seahorse-f64", w, h, s)
        p = s // 2
        capped = it[p::s, p::s] == cfg.iterations
        assert 0.05 < capped.mean() < 0.5
        assert not (M.near(cfg, z, it, der, s, 2.0 ** 18) & capped).any()
        for tau, reach in ((255, 2.0 ** -40), (255, 0.125), (64, 0.125), (255, 2.0 ** 18)):
            want, count = expected(cfg, z, it, der, s, T, tau, reach, "seahorse-f64")
            got, n = ad_device(torch, lib, cfg, kw, s, T, tau, reach)
            assert np.array_equal(got, want) and n == count, (s, tau, reach, n, count)
        assert count == int((~capped).sum())  # the largest reach: every escaped probe and no capped one
        got, n = ad_device(torch, lib, cfg, kw, s, T, 255, 0.0)
        assert n == 0 and np.array_equal(got, SD.shaded(cfg, z, it, der, s, T)[p::s, p::s])


# ---- the deep roads -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", list(DEEP))
def test_deep_roads_and_their_caches(fr, lib, torch, name, s):
    w, h = 41, 23
    tau, reach = DEEP[name]
    cfg, kw, z, it, der = yardstick(fr, name, w, h, s)
    want, count = expected(cfg, z, it, der, s, T, tau, reach, name)
    # the caches hold another view: the probe computes and uploads the orbit (and the table), the refine pass finds them
    other = W.view(fr.Config.new(), "J", 300, 16, 12, 5000), wide_centre(fr, "J", 6)
    fr.escape_rows_de(other[0], precision=fr.Precision.PT, centre=other[1], bla=0)
    assert fr.pt_orbit_cache()[0] == other[0].iterations
    got, n = ad_device(torch, lib, cfg, kw, s, T, tau, reach)
    assert np.array_equal(got, want) and n == count, (name, s, int((got != want).sum()), n, count)
    assert fr.pt_orbit_cache()[3] == 0 and fr.pt_orbit_cache()[0] == cfg.iterations  # the last request, the refine pass's, was served
    if "bla" in kw:
        assert fr.bla_cache()[3] == 0 and fr.bla_cache()[0] == fr.BLA_DEFAULT_BITS
    # t = -1 is the supersampled DE render of the road; the host form and a row piece
    full = fr.get_image_de(cfg, T, supersample=s, **kw)
    got, n = ad_device(torch, lib, cfg, kw, s, T, -1, reach)
    assert np.array_equal(got, full) and n == w * h, (name, s, "t = -1")
    got, n = ad_host(lib, cfg, kw, s, T, tau, reach)
    assert np.array_equal(got, want) and n == count, (name, s, "host")
    got, n = ad_device(torch, lib, cfg, kw, s, T, tau, reach, 7, 16, channels=4)
    m_img, m_n = M.adaptive_de(cfg, z, it, der, s, T, tau, reach, 7, 16, channels=4)
    assert np.array_equal(got, m_img) and n == m_n, (name, s, "rows")


# ---- grids, colour switches, the fern, profiling, the front ends ---------------------------------------------------------------------


@pytest.mark.parametrize("name,s", [("default", 2), ("julia", 5), ("pt-wide", 3), ("bla-wide", 2)])
def test_forced_grids_give_the_same_bytes(fr, lib, torch, name, s):
    w, h = (67, 19) if name in ("default", "julia") else (41, 23)
    tau, reach = DEEP.get(name, (TAU, REACH))
    cfg, kw, z, it, der = yardstick(fr, name, w, h, s)
    want, count = expected(cfg, z, it, der, s, T, tau, reach, name)
    try:
        for groups in (1, 3):
            check(lib.fr_debug_ss_adaptive_grid(groups))
            got, n = ad_device(torch, lib, cfg, kw, s, T, tau, reach)
            assert np.array_equal(got, want) and n == count, (name, s, groups, int((got != want).sum()))
    finally:
        check(lib.fr_debug_ss_adaptive_grid(0))


@pytest.mark.parametrize("smooth,inside", [(False, True), (True, False), (False, False)])
def test_colour_map_switches(fr, lib, torch, smooth, inside):
    s, w, h = 3, 67, 19
    cfg = DE.default_view(fr.Config.new(), w, h)
    cfg.smooth, cfg.inside = smooth, inside
    z, it, der = fr.escape_rows_de(SD.config_s(cfg, s))
    want, count = expected(cfg, z, it, der, s, T, TAU, REACH, "smooth=%s inside=%s" % (smooth, inside))
    got, n = ad_device(torch, lib, cfg, {}, s, T, TAU, REACH)
    assert np.array_equal(got, want) and n == count, (smooth, inside, int((got != want).sum()))


def test_an_algorithm_without_orbits_renders_black_and_refines_nothing(fr, lib, torch):
    cfg = DE.default_view(fr.Config.new(), 67, 19)
    cfg.algo = int(fr.Algo.BarnsleyFern)
    for s in (1, 2):
        for tau in (-1, TAU):
            got, n = ad_device(torch, lib, cfg, {}, s, T, tau, REACH)
            assert not got.any() and n == 0
            rgba, n = ad_device(torch, lib, cfg, {}, s, T, tau, REACH, channels=4)
            assert not rgba[..., :3].any() and (rgba[..., 3] == 255).all() and n == 0
    got, n = ad_host(lib, cfg, {}, 2, T, TAU, REACH)
    assert not got.any() and n == 0


def test_profiling_reports_the_last_kernel_of_the_call(fr, lib, torch):
    ms, name = C.c_float(), C.create_string_buffer(160)
    check(lib.fr_set_profiling(1))
    try:
        for view, size, args, kernel in (("default", (67, 19), (2, T, TAU, REACH), b"ss_refine_de_f64_kernel"),
                                         ("default", (67, 19), (2, T, 255, 0.0), b"ss_mark_de_kernel"),
                                         ("default", (67, 19), (1, T, TAU, REACH), b"ss_mark_de_kernel"),
                                         ("pt-wide", (41, 23), (2, T, 16, 2.0), b"ss_refine_de_pt_kernel"),
                                         ("bla-wide", (41, 23), (2, T, 16, 2.0), b"ss_refine_de_bla_kernel")):
            cfg, kw = VIEWS[view](fr, *size)
            ad_device(torch, lib, cfg, kw, *args)
            check(lib.fr_last_kernel_ms(C.byref(ms)))
            check(lib.fr_last_kernel_name(name, len(name)))
            assert name.value == kernel and ms.value > 0, (view, args, name.value, ms.value)
    finally:
        check(lib.fr_set_profiling(0))


def test_python_front_end_is_the_c_call(fr, lib, torch):
    for name, s, (w, h) in (("default", 4, (67, 19)), ("pt-dd", 2, (41, 23)), ("pt-wide", 2, (41, 23)), ("bla-wide", 3, (41, 23))):
        tau, reach = DEEP.get(name, (TAU, REACH))
        cfg, kw, z, it, der = yardstick(fr, name, w, h, s)
        want, count = expected(cfg, z, it, der, s, T, tau, reach, name)
        got, n = fr.get_image_de_adaptive(cfg, T, s, tau, reach, **kw)
        assert np.array_equal(got, want) and n == count, (name, "python")
        got, n = fr.get_image_de_adaptive(cfg, thickness=T, supersample=s, threshold=tau, reach=reach, y0=3, y1=11, channels=4, **kw)
        m_img, m_n = M.adaptive_de(cfg, z, it, der, s, T, tau, reach, 3, 11, channels=4)
        assert np.array_equal(got, m_img) and n == m_n, (name, "python rows")
    assert fr.ss_adaptive_de_workspace_bytes(cfg, 3, 0, 5) == M.workspace_bytes(cfg.width, cfg.height, 0, 5)


def test_cpp_overload_gives_the_c_calls_bytes(fr, lib, tmp_path):
    import __graft_entry__ as ge

    ge.build()
    pkg = os.path.join(ROOT, "fractal-renderer_amd")
    exe = os.path.join(ROOT, "tests", "cpp", "test_de_adaptive")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "host"),
                    os.path.join(ROOT, "tests", "cpp", "test_de_adaptive.cpp"), "-L" + pkg, "-lfractal_hip", "-Wl,-rpath," + pkg, "-o", exe],
                   check=True)
    w, h, s = 67, 19, 3
    cfg, kw, z, it, der = yardstick(fr, "default", w, h, s)
    want, count = expected(cfg, z, it, der, s, T, TAU, REACH, "c++")
    out = str(tmp_path / "image.rgb")
    r = subprocess.run([exe, str(w), str(h), str(cfg.iterations), repr(T), str(s), str(TAU), repr(REACH), out], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(out, dtype=np.uint8).reshape(h, w, 3), want)
    assert r.stdout.split() == ["refined", str(count)]


# ---- the host form's row pieces ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("view", ["default", "pt-wide"])
def test_host_form_by_row_pieces_is_the_device_form(fr, lib, torch, view, channels):
    """fr_debug_ss_host_work_cap forces the row-piece loop, which runs only above 256 MiB otherwise: pieces of 5, 2 and 1 rows
    (test_gpu_ss_adaptive.py: hook_caps) give the device form's bytes over the whole range and its count"""
    from test_gpu_ss_adaptive import HOOK_H, HOOK_S, HOOK_W, HOOK_Y0, HOOK_Y1, hook_caps

    cfg, kw = VIEWS[view](fr, HOOK_W, HOOK_H)
    tau, reach = DEEP.get(view, (16, 1.0))
    want, count = ad_device(torch, lib, cfg, kw, HOOK_S, 1.5, tau, reach, HOOK_Y0, HOOK_Y1, channels)
    assert 0 < count < HOOK_W * (HOOK_Y1 - HOOK_Y0), count
    try:
        for n, cap in hook_caps(M.workspace_bytes).items():
            check(lib.fr_debug_ss_host_work_cap(cap))
            got, refined = ad_host(lib, cfg, kw, HOOK_S, 1.5, tau, reach, HOOK_Y0, HOOK_Y1, channels)
            assert np.array_equal(got, want) and refined == count, (n, cap, int((got != want).sum()), refined, count)
    finally:
        check(lib.fr_debug_ss_host_work_cap(0))
