"""SUPERSAMPLED SCALED DE on the device (include/fractal_hip.h, "SUPERSAMPLED SCALED DE"; fr_render_rows_ss_de_pt_scaled(_device)),
byte for byte, no tolerance anywhere.  The views are M_900, J_900, MINI_861 and N_900 of tests/pt_scaled_model.py as OUTPUT sizes,
s in {2, 3}, T = 1.0, bits in {-1, 40}.  The yardsticks are never the code under test:
  - tests/ss_de_model.py's numpy restatement on tests/de_scaled_model.py's scaled view, over the arrays fr_escape_rows_de_pt_scaled
    gives on cfg_s, against the banded render with the smallest workspace (several bands) and with the largest;
  - fr_colour_de_rows_ss_device on cfg_v over the same kept arrays;
  - a row range with 4 channels; s = 1 and T = 0 against the calls the definition names; an algorithm without orbits;
  - a KEPT anti-aliased view: state-rendered on cfg_s at cap N, extended to M, recoloured by fr_colour_de_rows_ss_device, against
    the banded render at M with bits = -1.
The teeth are asserted from the MODEL (tests/de_scaled_model.py on cfg_s, limit 2, bits = -1, T = 1.0): "shaded" is iters < cap and
D < Ts; at least 4 % of the samples are shaded and at least 2 % of the output pixels hold both shaded and unshaded samples on the
first three views, and exactly no sample is shaded on N_900 (every sample is capped), so these tests cannot pass on unshaded
images."""
import ctypes as C

import numpy as np
import pytest

import de_model as DE
import de_scaled_model as DSM
import pt_scaled_model as S
import pt_scaled_state_model as T
import ss_de_model as M

pytestmark = pytest.mark.gpu

GUARD = 64
THICK = 1.0
VIEWS = {"M_900": S.M_900, "J_900": S.J_900, "MINI_861": S.MINI_861, "N_900": S.N_900}
SCALED_ROAD = 2  # FR_PT_ROAD_SCALED


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


def spec_s(spec, s):
    name, n, log2, w, h, cap = spec
    return (name, n, log2, w * s, h * s, cap)


_kept = {}


def kept(fr, native, lib, name, s, bits):
    """(view of the OUTPUT size, cfg_s, z, iters, u) — fr_escape_rows_de_pt_scaled's arrays on cfg_s, made once and read-only"""
    key = (name, s, bits)
    if key not in _kept:
        v = S.view(fr.Config.new, VIEWS[name])
        cfg_s = M.config_s(v.cfg, s)
        h, w = cfg_s.height, cfg_s.width
        z, der, it = np.full((h, w, 2), np.nan), np.full((h, w, 2), np.nan), np.full((h, w), 0xFFFFFFFF, dtype=np.uint32)
        centre = v.centre(native)
        check(lib.fr_escape_rows_de_pt_scaled(C.byref(cfg_s), C.byref(centre), bits, 0, h, z.ctypes.data, it.ctypes.data, der.ctypes.data))
        for a in (z, it, der):
            a.setflags(write=False)
        _kept[key] = v, cfg_s, z, it, der
    return _kept[key]


def teeth(fr, name, s):
    """from the model alone: (share of shaded samples, share of output pixels with both shaded and unshaded samples)"""
    vs = S.view(fr.Config.new, spec_s(VIEWS[name], s))  # the view of cfg_s: its own orbits, its own model
    v = S.view(fr.Config.new, VIEWS[name])
    assert bytes(vs.cfg) == bytes(M.config_s(v.cfg, s))
    z, it, u = DSM.model(vs)[:3]
    D = DE.distance(DSM.scaled_view(vs.cfg), z, it, u)
    shaded = (it < vs.cfg.iterations) & (D < THICK * s)
    per_pixel = shaded.reshape(v.cfg.height, s, v.cfg.width, s).sum(axis=(1, 3))
    mixed = (per_pixel > 0) & (per_pixel < s * s)
    return float(shaded.mean()), float(mixed.mean()), int(shaded.sum())


def render_device(torch, lib, native, v, bits, s, thickness, y0, y1, channels, work_len, cfg=None):
    """fr_render_rows_ss_de_pt_scaled_device into a guarded destination with a canary behind the workspace"""
    dev = torch.device("cuda", 0)
    cfg = v.cfg if cfg is None else cfg
    centre = v.centre(native)
    need = channels * cfg.width * (y1 - y0)
    d_out = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_work = torch.full((work_len + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    assert d_work.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    check(lib.fr_render_rows_ss_de_pt_scaled_device(C.byref(cfg), C.byref(centre), bits, thickness, s, y0, y1, channels,
                                                    d_out.data_ptr() + GUARD, need, d_work.data_ptr(), work_len, None))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    assert (d_work[work_len:].cpu().numpy() == 0x5A).all(), "wrote behind work_len"
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels)


def recolour_device(torch, lib, cfg_v, z, it, der, s, thickness, channels, ptrs=None):
    """fr_colour_de_rows_ss_device on the scaled view over kept arrays (numpy, or device pointers z, iters, der)"""
    dev = torch.device("cuda", 0)
    keep = None
    if ptrs is None:
        keep = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev) for a in (z, it, der)]
        ptrs = [t.data_ptr() for t in keep]
    need = channels * cfg_v.width * cfg_v.height
    d_out = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    check(lib.fr_colour_de_rows_ss_device(C.byref(cfg_v), *ptrs, cfg_v.width, cfg_v.height, s, thickness, channels, d_out.data_ptr() + GUARD,
                                          need, None))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    del keep
    return host[GUARD:GUARD + need].reshape(cfg_v.height, cfg_v.width, channels)


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
@pytest.mark.parametrize("name", list(VIEWS))
def test_the_views_have_teeth_by_the_model(fr, name, s):
    shaded, mixed, count = teeth(fr, name, s)
    print("%s s=%d: %.1f%% of the samples shaded, %.1f%% of the output pixels mixed" % (name, s, 100 * shaded, 100 * mixed))
    if name == "N_900":
        assert count == 0  # every sample is capped
    else:
        assert shaded >= 0.04 and mixed >= 0.02, (name, s, shaded, mixed)


@pytest.mark.parametrize("bits", [-1, 40])
@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", list(VIEWS))
def test_banded_render_is_the_model_and_the_fused_recolour_over_the_kept_arrays(fr, native, lib, torch, name, s, bits):
    shaded, mixed, count = teeth(fr, name, s)
    assert count == 0 if name == "N_900" else (shaded >= 0.04 and mixed >= 0.02)
    v, cfg_s, z, it, u = kept(fr, native, lib, name, s, bits)
    cfg_v = DSM.scaled_view(v.cfg)
    h = v.cfg.height
    want = {ch: M.colour(cfg_v, z, it, u, s, THICK, ch) for ch in (3, 4)}
    if name != "N_900":
        assert (want[3] != M.colour(cfg_v, z, it, u, s, 0.0)).any(), "nothing is shaded"
    lib_view = fr.de_scaled_view(v.cfg)
    assert bytes(lib_view) == bytes(cfg_v)
    mn, best = fr.ss_de_workspace_bytes(v.cfg, s)
    bands = band_count(v.cfg.width, h, s, mn)
    assert band_count(v.cfg.width, h, s, best) == 1 and (bands > 1 or h <= 8)
    if name == "M_900":
        assert bands == 3
    for work_len in (mn, best):
        got = render_device(torch, lib, native, v, bits, s, THICK, 0, h, 3, work_len)
        assert np.array_equal(got, want[3]), (name, s, bits, work_len, int((got != want[3]).sum()))
    # the fused recolour of the kept arrays on cfg_v
    for ch in (3, 4):
        assert np.array_equal(recolour_device(torch, lib, lib_view, z, it, u, s, THICK, ch), want[ch]), (name, s, bits, ch, "recolour")
    # a row range with 4 channels, the smallest workspace of that range
    y0, y1 = 3, h - 2
    got = render_device(torch, lib, native, v, bits, s, THICK, y0, y1, 4, fr.ss_de_workspace_bytes(v.cfg, s, y0, y1)[0])
    assert np.array_equal(got, want[4][y0:y1]), (name, s, bits, "rows, rgba")
    # the host form and the Python front end
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    bla = None if bits < 0 else bits
    assert np.array_equal(fr.get_image_de_scaled_ss(v.cfg, THICK, centre, s, bla=bla), want[3]), (name, s, bits, "host form")
    assert np.array_equal(fr.get_image_de_scaled_ss(v.cfg, THICK, centre, s, bla=bla, y0=y0, y1=y1, channels=4), want[4][y0:y1])


@pytest.mark.parametrize("bits", [-1, 40])
@pytest.mark.parametrize("name", ["M_900", "J_900", "MINI_861"])
def test_s_one_and_t_zero_are_the_calls_the_definition_names(fr, native, lib, torch, name, bits):
    v = S.view(fr.Config.new, VIEWS[name])
    h = v.cfg.height
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    bla = None if bits < 0 else bits
    # s = 1: fr_escape_rows_de_pt_scaled followed by fr_colour_de_rows_device(cfg_v, ..., T, channels)
    _v, _c, z, it, u = kept(fr, native, lib, name, 1, bits)
    cfg_v = fr.de_scaled_view(v.cfg)
    want = fr.colour_image_de(cfg_v, z, it, u, THICK)
    assert (want != fr.colour_image_de(cfg_v, z, it, u, 0.0)).any()
    mn, best = fr.ss_de_workspace_bytes(v.cfg, 1)
    for work_len in (mn, best):
        assert np.array_equal(render_device(torch, lib, native, v, bits, 1, THICK, 0, h, 3, work_len), want), (name, bits, work_len)
    rgba = render_device(torch, lib, native, v, bits, 1, THICK, 0, h, 4, mn)
    assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all()
    # T = 0: fr_render_rows_ss_pt with FR_PT_ROAD_SCALED
    for s in (2, 3):
        unshaded = fr.get_image_ss_pt(v.cfg, s, centre=centre, bla=bla, scaled=True)
        got = render_device(torch, lib, native, v, bits, s, 0.0, 0, h, 3, fr.ss_de_workspace_bytes(v.cfg, s)[0])
        assert np.array_equal(got, unshaded), (name, bits, s, "T = 0")
        assert len(np.unique(unshaded.reshape(-1, 3), axis=0)) > 1


def test_an_algorithm_without_orbits_renders_black(fr, native, lib, torch):
    v = S.view(fr.Config.new, VIEWS["M_900"])
    cfg = v.cfg.clone()
    cfg.algo = int(fr.Algo.BarnsleyFern)
    for s in (1, 2):
        for bits in (-1, 40):
            mn = fr.ss_de_workspace_bytes(cfg, s)[0]
            assert not render_device(torch, lib, native, v, bits, s, THICK, 0, cfg.height, 3, mn, cfg=cfg).any()
            rgba = render_device(torch, lib, native, v, bits, s, THICK, 0, cfg.height, 4, mn, cfg=cfg)
            assert not rgba[..., :3].any() and (rgba[..., 3] == 255).all()


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name,n,m", [("M_900", 560, 600), ("J_900", 632, 800)])
def test_a_kept_anti_aliased_view_extended_and_recoloured_is_the_render_at_the_new_cap(fr, native, lib, torch, name, n, m, s):
    c = T.chain(fr.Config.new, name)
    v = S.view(fr.Config.new, VIEWS[name])
    cfg_n, cfg_m = M.config_s(c.cfg(n), s), M.config_s(c.cfg(m), s)
    centre = c.centre(native)
    npx = cfg_n.width * cfg_n.height
    dev = torch.device("cuda", 0)
    d_z, d_w, d_der = (torch.zeros(2 * npx, dtype=torch.float64, device=dev) for _ in range(3))
    d_it, d_m = (torch.zeros(npx, dtype=torch.int32, device=dev) for _ in range(2))
    ptrs = [t.data_ptr() for t in (d_z, d_it, d_w, d_m, d_der)]
    check(lib.fr_escape_rows_de_pt_scaled_state_device(C.byref(cfg_n), C.byref(centre), 0, cfg_n.height, *ptrs, None))
    check(lib.fr_escape_extend_de_pt_scaled_device(C.byref(cfg_m), C.byref(centre), 0, cfg_m.height, n, *ptrs, None))
    torch.cuda.synchronize()
    running = int((d_it == n).sum())  # escaped at step n, or none: nothing is left at the old cap but those
    out_m = c.cfg(m)
    got = recolour_device(torch, lib, fr.de_scaled_view(out_m), None, None, None, s, THICK, 3, ptrs=[ptrs[0], ptrs[1], ptrs[4]])
    want = render_device(torch, lib, native, v, -1, s, THICK, 0, out_m.height, 3, fr.ss_de_workspace_bytes(out_m, s)[0], cfg=out_m)
    assert np.array_equal(got, want), (name, n, m, s, int((got != want).sum()), running)
    unshaded = render_device(torch, lib, native, v, -1, s, 0.0, 0, out_m.height, 3, fr.ss_de_workspace_bytes(out_m, s)[0], cfg=out_m)
    assert (want != unshaded).any(), "nothing is shaded at the new cap"


def test_profiling_reports_the_roads_kernel(fr, native, lib, torch):
    v = S.view(fr.Config.new, VIEWS["J_900"])
    ms, name = C.c_float(), C.create_string_buffer(160)
    check(lib.fr_set_profiling(1))
    try:
        for bits, kernel in ((-1, b"escape_pt_scaled_de_kernel"), (40, b"escape_bla_scaled_de_kernel")):
            render_device(torch, lib, native, v, bits, 2, THICK, 0, v.cfg.height, 3, fr.ss_de_workspace_bytes(v.cfg, 2)[0])
            check(lib.fr_last_kernel_ms(C.byref(ms)))
            check(lib.fr_last_kernel_name(name, len(name)))
            assert name.value == kernel and ms.value > 0, (bits, name.value, ms.value)
    finally:
        check(lib.fr_set_profiling(0))


@pytest.mark.parametrize("channels", [3, 4])
def test_host_form_under_a_cap_below_min_bytes_is_the_device_form(fr, native, lib, torch, channels):
    """fr_render_rows_ss_de_pt_scaled on its table road (test_gpu_ss.py: host_bands_are_the_device_forms)"""
    from test_gpu_ss import HOOK_H, HOOK_S, HOOK_W, HOOK_Y0, HOOK_Y1, host_bands_are_the_device_forms

    v = S.view(fr.Config.new, S.J_900[:3] + (HOOK_W, HOOK_H) + S.J_900[5:])
    centre = v.centre(native)

    def host():
        out = np.zeros((HOOK_Y1 - HOOK_Y0, HOOK_W, channels), dtype=np.uint8)
        check(lib.fr_render_rows_ss_de_pt_scaled(C.byref(v.cfg), C.byref(centre), 40, THICK, HOOK_S, HOOK_Y0, HOOK_Y1, channels,
                                                 out.ctypes.data, out.nbytes))
        return out

    sizes = host_bands_are_the_device_forms(
        lib, 36, lambda n: render_device(torch, lib, native, v, 40, HOOK_S, THICK, HOOK_Y0, HOOK_Y1, channels, n), host)
    assert sizes == fr.ss_de_workspace_bytes(v.cfg, HOOK_S, HOOK_Y0, HOOK_Y1)
