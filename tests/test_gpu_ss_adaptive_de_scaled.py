"""ADAPTIVE SUPERSAMPLED SCALED DE on the device (include/fractal_hip.h; csrc/fr_ss_adaptive_de.hip: the scaled arm;
fr_de_scaled.hip: ss_refine_de_scaled_kernel<JULIA, BLA, LINEAR>), byte for byte and count for count, no tolerance anywhere.  The
yardstick is never the code under test: it is the EXISTING fr_escape_rows_de_pt_scaled on cfg_s, whose arrays are fed to the numpy
model of tests/ss_adaptive_de_model.py run on the scaled view (tests/de_scaled_model.py: scaled_view).  Every output and every
workspace lies between two 64-byte guards, the workspace is the smallest the call accepts, d_refined sits between two canaries.
The views are M_900 (37 x 21, cap 6000), J_900 (16 x 12, cap 5000), MINI_861 (24 x 16, cap 3204) and N_900 (16 x 12, every sample
capped: the empty list) of tests/pt_scaled_model.py as OUTPUT sizes; s in {2, 3}, bits in {-1, 40}, T = 1.0, t = 8, R = 2.0.
Each case asserts its teeth on the yardstick before it trusts a pass: 0 < refined < width * rows, a pixel that `near` marks and
the colour rule does not, and a pixel of the union whose F differs from its P — tests/test_ss_adaptive_de_scaled_cpu.py pins the
counts on the host model (85 / 83 of 777 on M_900, 76 / 74 of 192 on J_900, 346 / 347 of 384 on MINI_861, 0 on N_900) and that no
pixel outside the union has F != P, so a missed refinement shows in the bytes and an excess one in `refined`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import de_scaled_model as DSM
import pt_scaled_model as S
import ss_adaptive_de_model as M
import ss_adaptive_de_views as AV
import ss_adaptive_model as A
import ss_de_model as SD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
T, TAU, REACH = 1.0, 8, 2.0
PT, PLAIN, SCALED = 3, 0, 2
VIEWS = {"M_900": S.M_900, "J_900": S.J_900, "MINI_861": S.MINI_861, "N_900": S.N_900, "M_440": S.M_440, "J_300": S.J_300}
TOOTHED = ["M_900", "J_900", "MINI_861"]
UNION = {("M_900", 2): 85, ("M_900", 3): 83, ("J_900", 2): 76, ("J_900", 3): 74, ("MINI_861", 2): 346, ("MINI_861", 3): 347,
         ("N_900", 2): 0, ("N_900", 3): 0}  # by the host model, at bits -1 and 40 alike


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


def ref(centre):
    """a fr_wide_centre, or what C.byref made of one, as the calls take it"""
    return C.byref(centre) if isinstance(centre, C.Structure) else centre


def ads_device(torch, lib, cfg, centre, bits, s, thickness, tau, reach, y0=0, y1=None, channels=3, want_refined=True, transfer=None):
    """fr_render_rows_ss_adaptive_de_pt_scaled_device — with a transfer (0 included) its _tf twin — into a guarded destination, with
    the SMALLEST workspace between two guards and d_refined between two canaries.  centre: a fr_wide_centre or its byref."""
    y1 = cfg.height if y1 is None else y1
    dev = torch.device("cuda", 0)
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
        check(lib.fr_render_rows_ss_adaptive_de_pt_scaled_tf_device(C.byref(cfg), ref(centre), bits, thickness, s, transfer, *tail))
    else:
        check(lib.fr_render_rows_ss_adaptive_de_pt_scaled_device(C.byref(cfg), ref(centre), bits, thickness, s, *tail))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    work = d_work.cpu().numpy()
    assert (work[:GUARD] == 0x5A).all() and (work[GUARD + work_len:] == 0x5A).all(), "wrote outside the workspace"
    cnt = d_n.cpu().numpy()
    assert cnt[0] == -1 and cnt[2] == -1, "wrote outside d_refined"
    assert want_refined or cnt[1] == -1
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels), int(cnt[1])


def ads_host(lib, cfg, centre, bits, s, thickness, tau, reach, y0=0, y1=None, channels=3, transfer=None):
    y1 = cfg.height if y1 is None else y1
    need = channels * cfg.width * (y1 - y0)
    host = np.full(GUARD + need + GUARD, 0xA5, dtype=np.uint8)
    n = C.c_uint64(12345)
    tail = (tau, reach, y0, y1, channels, host.ctypes.data + GUARD, need, C.byref(n))
    if transfer is not None:
        check(lib.fr_render_rows_ss_adaptive_de_pt_scaled_tf(C.byref(cfg), ref(centre), bits, thickness, s, transfer, *tail))
    else:
        check(lib.fr_render_rows_ss_adaptive_de_pt_scaled(C.byref(cfg), ref(centre), bits, thickness, s, *tail))
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels), n.value


def last_kernel(lib):
    ms, name = C.c_float(), C.create_string_buffer(160)
    check(lib.fr_last_kernel_ms(C.byref(ms)))
    check(lib.fr_last_kernel_name(name, len(name)))
    return name.value.decode(), ms.value


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------

_kept = {}


def kept(fr, native, lib, name, s, bits):
    """(view of the OUTPUT size, its fr_wide_centre, the scaled view cfg_v, z, iters, u): fr_escape_rows_de_pt_scaled's arrays on
    cfg_s, made once, shared, read-only"""
    key = (name, s, bits)
    if key not in _kept:
        v = S.view(fr.Config.new, VIEWS[name])
        cfg_s = SD.config_s(v.cfg, s)
        h, w = cfg_s.height, cfg_s.width
        z, der, it = np.full((h, w, 2), np.nan), np.full((h, w, 2), np.nan), np.full((h, w), 0xFFFFFFFF, dtype=np.uint32)
        centre = v.centre(native)
        check(lib.fr_escape_rows_de_pt_scaled(C.byref(cfg_s), C.byref(centre), bits, 0, h, z.ctypes.data, it.ctypes.data, der.ctypes.data))
        for a in (z, it, der):
            a.setflags(write=False)
        cfg_v = DSM.scaled_view(v.cfg)
        assert bytes(fr.de_scaled_view(v.cfg)) == bytes(cfg_v)
        _kept[key] = v, centre, cfg_v, z, it, der
    return _kept[key]


def expected(cfg_v, z, it, u, s, thickness, tau, reach, tag, teeth=True, filter=None):
    """the model's image and count over the yardstick's arrays, with the conditions that keep the case from passing emptily"""
    want, count = M.adaptive_de(cfg_v, z, it, u, s, thickness, tau, reach, filter=filter)
    e, n = M.edge_sets(cfg_v, z, it, u, s, thickness, tau, reach)
    H = SD.shaded(cfg_v, z, it, u, s, thickness)
    differ = (SD.box(H, s) != A.probe(H, s)).any(axis=-1)
    print("%s s=%d T=%g t=%d R=%g: refined %d of %d, %d near-only, %d of the union with F != P" % (
        tag, s, thickness, tau, reach, count, e.size, int((n & ~e).sum()), int(((e | n) & differ).sum())))
    if teeth:
        assert 0 < count < e.size, (tag, s, count)
        assert (n & ~e).any(), (tag, s, "no pixel is refined by the distance rule alone")
        assert ((e | n) & differ).any(), (tag, s, "no refined pixel has F != P")
    return want, count


def same(got, n, want, count, *what):
    assert np.array_equal(got, want) and n == count, what + (int((got != want).any(axis=-1).sum()), n, count)


# ---- the device and the host form against the model -------------------------------------------------------------------------------


@pytest.mark.parametrize("bits", [-1, 40])
@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", ["M_900", "J_900", "MINI_861", "N_900"])
def test_device_and_host_form_are_the_model(fr, native, lib, torch, name, s, bits):
    v, centre, cfg_v, z, it, u = kept(fr, native, lib, name, s, bits)
    want, count = expected(cfg_v, z, it, u, s, T, TAU, REACH, "%s bits %d" % (name, bits), teeth=name != "N_900")
    assert count == UNION[name, s]
    got, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, TAU, REACH)
    same(got, n, want, count, name, s, bits, "device")
    got, n = ads_host(lib, v.cfg, centre, bits, s, T, TAU, REACH)
    same(got, n, want, count, name, s, bits, "host")
    if name == "N_900":  # every sample is capped: nothing is near, nothing is an edge, the image is the probe image
        assert (it == v.cfg.iterations).all() and count == 0
        check(lib.fr_set_profiling(1))
        try:
            got, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, TAU, 2.0 ** 18)  # whatever the reach
            same(got, n, want, 0, name, s, bits, "the largest reach")
            assert last_kernel(lib)[0] == "ss_refine_de_scaled_kernel"  # the pass runs over an empty list
            ads_device(torch, lib, v.cfg, centre, bits, s, T, 255, 0.0)
            assert last_kernel(lib)[0] == "ss_mark_de_kernel"  # no refine pass
        finally:
            check(lib.fr_set_profiling(0))


@pytest.mark.parametrize("transfer", [0, 1])
@pytest.mark.parametrize("bits", [-1, 40])
@pytest.mark.parametrize("name", ["M_900", "J_900"])
def test_all_eight_kernel_instances(fr, native, lib, torch, name, bits, transfer):
    """<JULIA, BLA, LINEAR>: Mandelbrot and Julia, the plain scaled loop and the table, the byte and the sRGB filter, each named by
    fr_last_kernel_name.  bits = 40: by the host model's `skips` some sample of a refined pixel took a table skip, so the table
    instance ran another loop.  transfer 1: some output pixel differs from transfer 0's."""
    s = 3
    v, centre, cfg_v, z, it, u = kept(fr, native, lib, name, s, bits)
    assert (v.cfg.algo == 2) == (name == "J_900")
    want, count = expected(cfg_v, z, it, u, s, T, TAU, REACH, "%s bits %d transfer %d" % (name, bits, transfer), filter=AV.FILTERS[transfer])
    bytes_want = M.adaptive_de(cfg_v, z, it, u, s, T, TAU, REACH)[0]
    if transfer:
        assert (want != bytes_want).any(), "the sRGB filter changes no pixel"
    if bits >= 0:
        vs = S.view(fr.Config.new, (VIEWS[name][:3] + (v.cfg.width * s, v.cfg.height * s) + VIEWS[name][5:]))
        skips = DSM.model(vs, bits)[4]
        e, n = M.edge_sets(cfg_v, z, it, u, s, T, TAU, REACH)
        assert (skips.reshape(v.cfg.height, s, v.cfg.width, s).sum(axis=(1, 3))[e | n] > 0).any(), "no refined sample took a skip"
    check(lib.fr_set_profiling(1))
    try:
        got, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, TAU, REACH, transfer=transfer)
        kernel, ms = last_kernel(lib)
    finally:
        check(lib.fr_set_profiling(0))
    same(got, n, want, count, name, bits, transfer)
    assert kernel == "ss_refine_de_scaled_kernel" and ms > 0, (kernel, ms)
    got, n = ads_host(lib, v.cfg, centre, bits, s, T, TAU, REACH, transfer=transfer)
    same(got, n, want, count, name, bits, transfer, "host")
    if transfer == 0:  # the plain spelling is the twin with FR_SS_TRANSFER_BYTES
        got, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, TAU, REACH)
        same(got, n, want, count, name, bits, "plain spelling")


@pytest.mark.parametrize("bits", [-1, 40])
@pytest.mark.parametrize("name", TOOTHED)
def test_row_pieces_rgba_and_a_null_count(fr, native, lib, torch, name, bits):
    s = 3
    v, centre, cfg_v, z, it, u = kept(fr, native, lib, name, s, bits)
    h = v.cfg.height
    want, count = expected(cfg_v, z, it, u, s, T, TAU, REACH, "%s bits %d" % (name, bits))
    pieces, total = [], 0
    for y0, y1 in ((0, 5), (5, 6), (6, h)):  # the middle piece is one row with a neighbour row on either side
        got, _ = ads_device(torch, lib, v.cfg, centre, bits, s, T, TAU, REACH, y0, y1, channels=4, want_refined=False)
        assert (got[..., 3] == 255).all()
        pieces.append(got[..., :3])
        m_img, m_n = M.adaptive_de(cfg_v, z, it, u, s, T, TAU, REACH, y0, y1, channels=4)
        assert np.array_equal(got, m_img), (name, bits, y0, y1)
        got3, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, TAU, REACH, y0, y1)
        assert np.array_equal(got3, got[..., :3]) and n == m_n, (name, bits, y0, y1, n, m_n)
        total += n
    assert np.array_equal(np.concatenate(pieces), want) and total == count
    got, n = ads_host(lib, v.cfg, centre, bits, s, T, TAU, REACH, 5, 6, channels=4)
    assert np.array_equal(got[..., :3], want[5:6]) and (got[..., 3] == 255).all()
    got, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, TAU, REACH, want_refined=False, transfer=1)  # d_refined = NULL
    assert np.array_equal(got, M.adaptive_de(cfg_v, z, it, u, s, T, TAU, REACH, filter=AV.srgb_filter)[0])


@pytest.mark.parametrize("name,s,bits", [("M_900", 2, -1), ("J_900", 3, 40), ("MINI_861", 2, 40)])
def test_forced_grid_gives_the_same_bytes(fr, native, lib, torch, name, s, bits):
    v, centre, cfg_v, z, it, u = kept(fr, native, lib, name, s, bits)
    want, count = expected(cfg_v, z, it, u, s, T, TAU, REACH, name)
    got, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, TAU, REACH)  # the default grid
    same(got, n, want, count, name, "default grid")
    try:
        for groups in (1, 3):
            check(lib.fr_debug_ss_adaptive_grid(groups))
            got, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, TAU, REACH)
            same(got, n, want, count, name, s, groups)
    finally:
        check(lib.fr_debug_ss_adaptive_grid(0))


# ---- each consequence against the call it names --------------------------------------------------------------------------------------


@pytest.mark.parametrize("bits", [-1, 40])
@pytest.mark.parametrize("name", TOOTHED)
def test_consequences_against_the_calls_they_name(fr, native, lib, torch, name, bits):
    s = 2
    v, centre, cfg_v, z, it, u = kept(fr, native, lib, name, s, bits)
    w, h, p = v.cfg.width, v.cfg.height, s // 2
    wide = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    bla = None if bits < 0 else bits
    H = SD.shaded(cfg_v, z, it, u, s, T)
    # t = -1: fr_render_rows_ss_de_pt_scaled's bytes, every pixel refined, for every R
    full = fr.get_image_de_scaled_ss(v.cfg, T, wide, s, bla=bla)
    assert np.array_equal(full, SD.box(H, s))  # the two yardsticks agree
    for reach in (0.0, REACH):
        got, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, -1, reach)
        same(got, n, full, w * h, name, bits, "t = -1", reach)
    # t = 255 with R = 0: the probe image, nothing refined
    got, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, 255, 0.0)
    same(got, n, H[p::s, p::s], 0, name, bits, "the probe image")
    # t = 255 with a reach: the distance rule alone
    want, count = M.adaptive_de(cfg_v, z, it, u, s, T, 255, REACH)
    assert 0 < count < w * h
    got, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, 255, REACH)
    same(got, n, want, count, name, bits, "near alone")
    # R = 0: the colour rule on the shaded bytes
    want, count = A.adaptive(H, s, TAU)
    assert 0 < count < w * h
    got, n = ads_device(torch, lib, v.cfg, centre, bits, s, T, TAU, 0.0)
    same(got, n, want, count, name, bits, "R = 0")
    # T = 0 with R = 0: fr_render_rows_ss_adaptive with FR_PT_ROAD_SCALED, bytes and count
    # (M_900's unshaded probe image is flat within 8 grey levels: by the host model the colour rule marks 0 pixels there at
    # t = 8, and 43 / 86 / 345 of the three views at t = 0, so t = 0 is where the list is neither empty nor full on all three)
    for tau in (0, TAU):
        want, count = fr.get_image_ss_adaptive(v.cfg, s, tau, precision=fr.Precision.PT, centre=wide, bla=bla, scaled=True)
        assert count < w * h and (tau or count > 0), (name, tau, count)
        got, n = ads_device(torch, lib, v.cfg, centre, bits, s, 0.0, tau, 0.0)
        same(got, n, want, count, name, bits, "T = 0", tau)
    # s = 1: fr_escape_rows_de_pt_scaled followed by fr_colour_de_rows_device(cfg_v, ..., T, channels), for every t and R
    _v, _c, _cv, z1, it1, u1 = kept(fr, native, lib, name, 1, bits)
    plain = fr.colour_image_de(fr.de_scaled_view(v.cfg), z1, it1, u1, T)
    assert (plain != fr.colour_image_de(fr.de_scaled_view(v.cfg), z1, it1, u1, 0.0)).any()
    for tau, reach in ((-1, 0.0), (0, 1.0), (TAU, REACH), (255, 0.0), (255, 3.0)):
        got, n = ads_device(torch, lib, v.cfg, centre, bits, 1, T, tau, reach)
        assert np.array_equal(got, plain), (name, bits, "s = 1", tau, reach)
        assert n == M.adaptive_de(cfg_v, z1, it1, u1, 1, T, tau, reach)[1]
    rgba, n = ads_device(torch, lib, v.cfg, centre, bits, 1, T, TAU, REACH, channels=4)
    assert np.array_equal(rgba[..., :3], plain) and (rgba[..., 3] == 255).all()


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", ["M_440", "J_300"])
def test_inside_wide_pt_the_plain_loop_is_adaptive_de_on_the_wide_road(fr, native, lib, torch, name, s):
    """DE ON SCALED PT's claim 2 carried through: with bits = -1 the bytes and the count are fr_render_rows_ss_adaptive_de's on
    FR_PRECISION_PT, FR_PT_ROAD_PLAIN with the same wide centre"""
    v, centre, cfg_v, z, it, u = kept(fr, native, lib, name, s, -1)
    want, count = expected(cfg_v, z, it, u, s, T, TAU, REACH, name)
    out = np.full((v.cfg.height, v.cfg.width, 3), 0x5A, dtype=np.uint8)
    n = C.c_uint64(0)
    check(lib.fr_render_rows_ss_adaptive_de(C.byref(v.cfg), PT, None, C.byref(centre), PLAIN, 0, T, s, TAU, REACH, 0, v.cfg.height, 3,
                                            out.ctypes.data, out.nbytes, C.byref(n)))
    same(out, n.value, want, count, name, s, "the wide road against the model on the scaled view")
    got, m = ads_device(torch, lib, v.cfg, centre, -1, s, T, TAU, REACH)
    same(got, m, out, n.value, name, s, "the scaled road against the wide road")


def test_an_algorithm_without_orbits_renders_black_and_refines_nothing(fr, native, lib, torch):
    v = S.view(fr.Config.new, VIEWS["M_900"])
    centre = v.centre(native)
    cfg = v.cfg.clone()
    cfg.algo = int(fr.Algo.BarnsleyFern)
    for s in (1, 2):
        for bits in (-1, 40):
            for tau in (-1, TAU):
                got, n = ads_device(torch, lib, cfg, centre, bits, s, T, tau, REACH)
                assert not got.any() and n == 0
                rgba, n = ads_device(torch, lib, cfg, centre, bits, s, T, tau, REACH, channels=4, transfer=1)
                assert not rgba[..., :3].any() and (rgba[..., 3] == 255).all() and n == 0
    got, n = ads_host(lib, cfg, centre, -1, 2, T, TAU, REACH)
    assert not got.any() and n == 0


# ---- the front ends ------------------------------------------------------------------------------------------------------------------


def test_python_front_end_is_the_c_call(fr, native, lib, torch):
    for name, s, bits in (("M_900", 2, -1), ("J_900", 3, 40), ("MINI_861", 3, 0)):
        model_bits = 40 if bits == 0 else bits  # 0 is FR_BLA_DEFAULT_BITS
        v, _centre, cfg_v, z, it, u = kept(fr, native, lib, name, s, model_bits)
        wide = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
        bla = None if bits < 0 else bits
        want, count = expected(cfg_v, z, it, u, s, T, TAU, REACH, name)
        got, n = fr.get_image_de_adaptive_scaled(v.cfg, T, wide, s, TAU, REACH, bla)
        same(got, n, want, count, name, "python")
        got, n = fr.get_image_de_adaptive_scaled(v.cfg, thickness=T, centre=wide, supersample=s, threshold=TAU, reach=REACH, bla=bla, y0=3,
                                                 y1=11, channels=4, transfer=1)
        m_img, m_n = M.adaptive_de(cfg_v, z, it, u, s, T, TAU, REACH, 3, 11, channels=4, filter=AV.srgb_filter)
        same(got, n, m_img, m_n, name, "python rows, rgba, sRGB")
        out = np.zeros((v.cfg.height, v.cfg.width, 3), dtype=np.uint8)
        got, n = fr.get_image_de_adaptive_scaled(v.cfg, T, wide, s, bla=bla, out=out)  # the defaults are t = 8, R = 2
        assert got is out
        same(out, n, want, count, name, "python out=")


def test_cpp_overload_gives_the_c_calls_bytes(fr, native, lib, tmp_path):
    from test_gpu_bla import compile_cpp, decimal_centre

    exe = os.path.join(ROOT, "tests", "cpp", "test_de_adaptive_scaled")
    compile_cpp(os.path.join(ROOT, "tests", "cpp", "test_de_adaptive_scaled.cpp"), exe)
    import pt_wide_model as W

    tre, tim, centre = decimal_centre(fr, "M", 320, 2.0 ** 900)
    assert centre.words == 16
    cfg = W.view(fr.Config.new(), "M", 900, 37, 21, 6000)
    st = centre.c_struct()
    for bits, s, transfer in ((-1, 2, 0), (40, 3, 1)):
        out = str(tmp_path / ("image_%d.rgb" % s))
        r = subprocess.run([exe, tre, tim, "900", "37", "21", "6000", str(bits), repr(T), str(s), str(TAU), repr(REACH), str(transfer), out],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        want, count = ads_host(lib, cfg, st, bits, s, T, TAU, REACH, transfer=transfer)
        assert 0 < count < 37 * 21
        assert np.array_equal(np.fromfile(out, dtype=np.uint8).reshape(21, 37, 3), want)
        assert r.stdout.split() == ["refined", str(count)]
    # the C call's bytes are the model's on this centre too: the decimal centre is the view's own, floored
    cfg_s = SD.config_s(cfg, 2)
    z, u, it = np.empty((42, 74, 2)), np.empty((42, 74, 2)), np.empty((42, 74), dtype=np.uint32)
    check(lib.fr_escape_rows_de_pt_scaled(C.byref(cfg_s), C.byref(st), -1, 0, 42, z.ctypes.data, it.ctypes.data, u.ctypes.data))
    want, count = expected(DSM.scaled_view(cfg), z, it, u, 2, T, TAU, REACH, "c++")
    got, n = ads_host(lib, cfg, st, -1, 2, T, TAU, REACH)
    same(got, n, want, count, "c++ centre")


# ---- the host form's row pieces ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("channels", [3, 4])
def test_host_form_by_row_pieces_is_the_device_form(fr, native, lib, torch, channels):
    """fr_debug_ss_host_work_cap forces the row-piece loop, which runs only above 256 MiB otherwise: pieces of 5, 2 and 1 rows
    (test_gpu_ss_adaptive.py: hook_caps; M_900 has its size) give the device form's bytes over the whole range and its count"""
    from test_gpu_ss_adaptive import HOOK_H, HOOK_W, HOOK_Y0, HOOK_Y1, hook_caps

    v, centre, cfg_v, z, it, u = kept(fr, native, lib, "M_900", 2, 40)
    assert (v.cfg.width, v.cfg.height) == (HOOK_W, HOOK_H)
    want, count = ads_device(torch, lib, v.cfg, centre, 40, 2, T, TAU, REACH, HOOK_Y0, HOOK_Y1, channels)
    m_img, m_n = M.adaptive_de(cfg_v, z, it, u, 2, T, TAU, REACH, HOOK_Y0, HOOK_Y1, channels=channels)
    same(want, count, m_img, m_n, "device rows")
    assert 0 < count < HOOK_W * (HOOK_Y1 - HOOK_Y0)
    try:
        for rows, cap in hook_caps(M.workspace_bytes).items():
            check(lib.fr_debug_ss_host_work_cap(cap))
            got, n = ads_host(lib, v.cfg, centre, 40, 2, T, TAU, REACH, HOOK_Y0, HOOK_Y1, channels)
            same(got, n, want, count, "host pieces", rows, cap)
    finally:
        check(lib.fr_debug_ss_host_work_cap(0))
