"""The colour map on the device at byte boundaries, window edges and in the reference's operation order, byte for byte.

tests/golden/colour_boundaries.npz (tests/golden/make_colour_boundaries.py) holds inputs whose true colour value lies a chosen
distance — from 2^-12 to 2^10 widths of the colour filter's bracket — from a chosen byte boundary, pixels at the ends of the
filter's range, and known answers that tell the reference's association of the exact paths from its neighbours.
tests/test_colour_boundaries_cpu.py shows on the CPU that these inputs convict a filter whose windows are too narrow.  Here they
go through the code that ships:
  - the recolour calls, which take any (z, iters): fr_colour_rgb8, fr_colour_rows_device (z_width 2 and 4, RGB and RGBA),
    fr_colour_rows_ss_device (colour_filter_kernel<S>, S = 2 .. 8, each block S * S copies of one rung, so that a wrong byte
    cannot vanish in the mean), under fr_set_colour_filter 1, 2 and 0, in whole waves of rungs and as single rungs among
    ordinary, non-finite, inside and capped neighbours (the roads are chosen per wave by ballot);
  - the render kernels, each with its own copy of the map and the f32 stage in its first-pass form: they take no z, so the
    EXPOSURE is aimed — bisected against the oracle to the value at which one pixel's byte flips, then moved off by a chosen
    number of bracket widths — and the whole image compared.
The truth is oracle_lib.colour_rows / get_image on the very arrays and configurations that are uploaded.  The filter knob is
process-wide: nothing here threads.
"""
import ctypes as C
import math
from contextlib import contextmanager

import numpy as np
import pytest

import colour_model as CM
import deep_edge_views as E
import oracle_lib as O

pytestmark = pytest.mark.gpu

GUARD = 64
SETTINGS = (1, 2, 0)  # fr_set_colour_filter: f32 stage + f64 stage, f64 stage alone, always the software log2


def fused_tile():
    """(tile width, cf_tile_rows) of colour_filter_kernel, read from fr_ss.hip so that the sizes below follow the kernel's"""
    import os
    import re

    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "fractal-renderer_amd", "csrc", "fr_ss.hip")) as f:
        src = f.read()
    width = re.search(r"constexpr uint32_t kCfTileW = (\d+);", src)
    rows = re.search(r"cf_tile_rows\(uint32_t s\) \{ return s <= (\d+) \? (\d+)u : s <= (\d+) \? (\d+)u : (\d+)u; \}", src)
    assert width and rows, "fr_ss.hip no longer states its tile as this test reads it"
    a, ra, b, rb, rc = (int(v) for v in rows.groups())
    return int(width.group(1)), (lambda s: ra if s <= a else rb if s <= b else rc)


CF_TILE_W, cf_tile_rows = fused_tile()


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


@pytest.fixture(scope="module")
def fx():
    O.set_log2_mode(O.LOG2_LIBM)
    return CM.Fixture()


def check(rc):
    from fractal_renderer_amd import _native

    _native.check(rc)


def truth_rows(ocfg, z, it):
    """the oracle's colour map on one thread: these arrays are small, and a team of threads per call costs more than the call"""
    return O.colour_rows(ocfg, z, it, threads=1)


def to_fr(fr, ocfg):
    return fr.Config.from_buffer_copy(bytes(ocfg))


@contextmanager
def colour_filter(lib, setting):
    check(lib.fr_set_colour_filter(setting))
    try:
        yield
    finally:
        check(lib.fr_set_colour_filter(1))


def colour_device(torch, lib, cfg, z, it, channels=3, zw=2, ss=None, dst_off=0):
    """fr_colour_rows_device (ss None) or fr_colour_rows_ss_device (ss = (width, rows, s)) over numpy arrays in guarded device
    buffers -> uint8 [pixels, channels].  zw = 4 spreads z to (re.hi, re.lo, im.hi, im.lo) with low parts that must not matter."""
    dev = torch.device("cuda", 0)
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, 2)
    it = np.ascontiguousarray(it, dtype=np.uint32).reshape(-1)
    if zw == 4:
        z4 = np.empty((z.shape[0], 4))
        z4[:, 0], z4[:, 2] = z[:, 0], z[:, 1]
        z4[:, 1], z4[:, 3] = 0.3, -0.7
        z = z4
    d_z = torch.from_numpy(z.reshape(-1).copy()).to(dev)
    d_it = torch.from_numpy(it.view(np.int32).copy()).to(dev)
    npx = it.size if ss is None else ss[0] * ss[1]
    need = channels * npx
    d_out = torch.full((GUARD + 16 + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    at = GUARD + dst_off
    torch.cuda.synchronize()
    if ss is None:
        check(lib.fr_colour_rows_device(C.byref(cfg), d_z.data_ptr(), zw, d_it.data_ptr(), it.size, channels, d_out.data_ptr() + at,
                                        need, None))
    else:
        assert it.size == npx * ss[2] * ss[2]
        check(lib.fr_colour_rows_ss_device(C.byref(cfg), d_z.data_ptr(), zw, d_it.data_ptr(), ss[0], ss[1], ss[2], channels,
                                           d_out.data_ptr() + at, need, None))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:at] == 0xA5).all() and (host[at + need:] == 0xA5).all(), "the kernel wrote outside its destination"
    out = host[at:at + need].reshape(npx, channels)
    if channels == 4:
        assert (out[:, 3] == 255).all()
    return out[:, :3]


def every_flat_call(fr, torch, lib, cfg, z, it, k):
    """(name, bytes [n, 3]) of every recolour call that takes a flat run of n results; k varies the cheap choices"""
    n = it.size
    yield "fr_colour_rgb8", fr.colour_image(cfg, z, it).reshape(n, 3)
    for zw in (2, 4):
        for channels in (3, 4):
            yield "fr_colour_rows_device zw %d ch %d" % (zw, channels), colour_device(torch, lib, cfg, z, it, channels, zw,
                                                                                      dst_off=(k % 4) if channels == 3 else 4 * (k % 3))
    yield "fr_colour_rows_ss_device s 1", colour_device(torch, lib, cfg, z, it, 3 + (k & 1), 2 + 2 * ((k >> 1) & 1), ss=(n, 1, 1))


def mismatch(fx, got, want, at=None):
    bad = np.flatnonzero((got != want).any(axis=-1))
    rows = []
    for j in bad[:6]:
        row = {"pixel": int(j), "got": got[j].tolist(), "want": want[j].tolist()}
        if at is not None:
            r = int(at[j])
            row.update(channel=int(fx.rung_channel[r]), boundary=int(fx.rung_boundary[r]), offset_W=float(fx.rung_offset_W[r]))
        rows.append(row)
    return len(bad), rows


# ---- the recolour calls ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", range(17))
def test_every_rung_through_every_recolour_call_and_filter_setting(fr, lib, torch, fx, c):
    """a configuration's rungs as one run: whole waves of aimed pixels, and a last, partial one"""
    assert len(fx.names) == 17  # 16 configurations and the range gates
    ocfg = fx.oracle_config(O, c)
    if c == len(fx.names) - 1:  # the ends of the filter's range of dist
        z, it, at = fx.gate_z, fx.gate_iters, None
        want = truth_rows(ocfg, z, it)
        assert np.array_equal(want, fx.gate_bytes)
    else:
        z, it, at = fx.rungs_of(c)
        want = truth_rows(ocfg, z, it)
        assert np.array_equal(want[np.arange(at.size), fx.rung_channel[at]], fx.rung_byte[at])
    cfg = to_fr(fr, ocfg)
    for setting in SETTINGS:
        with colour_filter(lib, setting):
            for name, got in every_flat_call(fr, torch, lib, cfg, z, it, c + setting):
                assert np.array_equal(got, want), (fx.names[c], setting, name) + mismatch(fx, got, want, at)


def test_order_kats_through_every_recolour_call(fr, lib, torch, fx):
    """each KAT 65 times over (a whole wave and a lane of the next): the reference's association, not its neighbour's"""
    for j in range(fx.kat_byte.size):
        ocfg = fx.kat_config(O, j)
        z, it = np.repeat(fx.kat_z[j:j + 1], 65, axis=0), np.repeat(fx.kat_iters[j:j + 1], 65)
        want = truth_rows(ocfg, z, it)
        assert (want == fx.kat_byte[j]).all() and fx.kat_alt_byte[j] != fx.kat_byte[j]
        cfg = to_fr(fr, ocfg)
        for setting in SETTINGS if str(fx.kat_path[j]) == "smooth" else (1,):
            with colour_filter(lib, setting):
                for name, got in every_flat_call(fr, torch, lib, cfg, z, it, j):
                    assert np.array_equal(got, want), (j, str(fx.kat_path[j]), str(fx.kat_alt[j]), setting, name, got[0].tolist(),
                                                       int(fx.kat_byte[j]), int(fx.kat_alt_byte[j]))


def close_rungs(fx, c, most=1.5):
    """the rungs of configuration c within `most` bracket widths of their boundary: undecided by the f32 stage, mostly by both"""
    z, it, at = fx.rungs_of(c)
    keep = np.abs(fx.rung_offset_W[at]) <= most
    return z[keep], it[keep], at[keep]


def ordinary(n, cap, seed):
    """pixels as a render leaves them: dist between limit^2 = 2^32 and its square, any index under the cap"""
    rng = np.random.default_rng(seed)
    r = np.exp2(rng.uniform(32.0, 64.0, n) / 2)
    a = rng.uniform(0.0, 2 * np.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=-1), rng.integers(0, cap, n, dtype=np.uint32)


@pytest.mark.parametrize("name", ["default-colours", "255-40-7", "n-77", "range-ends"])
def test_a_rung_keeps_its_bytes_whatever_its_wave_does(fr, lib, torch, fx, name):
    """one rung at lanes 0, 31 and 63 among ordinary pixels, and rungs beside lanes that leave the filter's range or the smooth
    branch altogether; n = 1, 63, 64, 65 and 1025 pixels.  "range-ends" is 255-40-7 with a stable_limit of 0.5: the same rungs,
    now beside the gate pixels — dist at 2 and 2^120 exactly and a step outside, still OUTSIDE colours — and a dist of 1.53."""
    c = fx.names.index(name)
    cap = int(fx.cfg_iterations[c])
    ocfg = fx.oracle_config(O, c)
    cfg = to_fr(fr, ocfg)
    gates = name == "range-ends"
    if gates:
        r = fx.names.index("255-40-7")
        assert (fx.cfg_iterations[r], fx.cfg_exposure[r], tuple(fx.cfg_primary[r])) == (cap, fx.cfg_exposure[c], tuple(fx.cfg_primary[c]))
        assert fx.cfg_stable_limit[c] == 0.5
    rz, rit, rat = close_rungs(fx, r if gates else c)
    assert rit.size >= 24
    inf, nan = math.inf, math.nan
    odd = [((1.2, 0.3), 7),  # dist = 1.53: the inside colour at the default stable_limit, outside and under the filter's range at 0.5
           ((0.0, 0.0), cap), ((3e5, 1.0), cap),  # iters == iterations, inside and (a caller's business) outside
           ((2.0 ** 61, 0.0), 9), ((1e200, 1e200), 10),  # dist > 2^120, dist = inf by overflow
           ((nan, 0.0), 11), ((1.0, nan), 12), ((inf, 0.0), 13), ((0.0, -inf), 14), ((inf, nan), 15)]
    if gates:
        odd = [((float(zr), float(zi)), int(i)) for (zr, zi), i in zip(fx.gate_z, fx.gate_iters)][::2] + odd[:2] + [((0.5, 0.3), 7)]
        assert sum(1 for (zr, zi), _i in odd if 0.5 < zr * zr + zi * zi < 2.0) >= 3
    k = 0
    for n in (1, 63, 64, 65, 1025):
        layouts = []
        # (a) one rung per wave at lane 0, 31 or 63, the rest ordinary
        for lane in (0, 31, 63):
            z, it = ordinary(n, cap, 100 * n + lane)
            for w, first in enumerate(range(0, n, 64)):
                if first + lane < n:
                    r = (7 * w + lane + n) % rit.size
                    z[first + lane], it[first + lane] = rz[r], rit[r]
            if n > lane:
                layouts.append(("lane %d" % lane, z, it))
        # (b) rungs with one odd neighbour per wave, at every other lane from the rung's
        z, it = np.empty((n, 2)), np.empty(n, dtype=np.uint32)
        pick = (np.arange(n) * 5 + n) % rit.size
        z[:], it[:] = rz[pick], rit[pick]
        for w, first in enumerate(range(0, n, 64)):
            where = first + (11 * w + 5) % min(64, n - first)
            if n > 1:
                z[where], it[where] = odd[w % len(odd)]
        layouts.append(("odd neighbours", z, it))
        # (c) every odd pixel in one wave of rungs
        if n >= 64:
            z, it = z.copy(), it.copy()
            for q, (pos, i) in enumerate(odd):
                z[3 + 6 * q], it[3 + 6 * q] = pos, i
            layouts.append(("all odd neighbours", z, it))
        for what, z, it in layouts:
            want = truth_rows(ocfg, z, it)
            for setting in SETTINGS:
                with colour_filter(lib, setting):
                    for call, got in every_flat_call(fr, torch, lib, cfg, z, it, k):
                        assert np.array_equal(got, want), (name, n, what, setting, call) + mismatch(fx, got, want)
            k += 1


@pytest.mark.parametrize("s", range(1, 9))
def test_fused_recolour_of_blocks_of_one_rung_each(fr, lib, torch, fx, s):
    """colour_filter_kernel<S> (S = 1: colour_rows_kernel) against the oracle: each output pixel's S x S samples are copies of one
    rung, so the box mean IS the rung's byte; widths on both sides of the 64-pixel tile, rows on both sides of cf_tile_rows(S)"""
    ro = cf_tile_rows(s)
    k = 0
    for name in ("255-40-7", "default-colours", "n-1000"):
        c = fx.names.index(name)
        ocfg = fx.oracle_config(O, c)
        cfg = to_fr(fr, ocfg)
        rz, rit, rat = fx.rungs_of(c)
        truth = truth_rows(ocfg, rz, rit)
        for width in (CF_TILE_W - 1, CF_TILE_W, CF_TILE_W + 1, 2 * CF_TILE_W + 1):
            for rows in sorted({max(ro - 1, 1), ro, ro + 1, 2 * ro + 1}):
                pick = ((np.arange(width * rows) * 3 + 17 * k) % rit.size).reshape(rows, width)
                big = np.repeat(np.repeat(pick, s, axis=0), s, axis=1)  # [s*rows, s*width]
                z, it = rz[big], rit[big]
                want = truth[pick].reshape(-1, 3)
                assert np.array_equal(truth_rows(ocfg, z, it), truth[big])  # the truth on the very arrays that go up
                for setting in SETTINGS:
                    with colour_filter(lib, setting):
                        got = colour_device(torch, lib, cfg, z, it, 3 + (k & 1), 2 + 2 * ((k >> 1) & 1), ss=(width, rows, s),
                                            dst_off=(k % 4) if not k & 1 else 4 * (k % 3))
                    assert np.array_equal(got, want), (name, s, width, rows, setting) + mismatch(fx, got, want, rat[pick.reshape(-1)])
                k += 1


# ---- the render kernels: aimed through the exposure ----------------------------------------------------------------------------------

VIEW = dict(iterations=300, pos=(-0.6, 0.0))
SIZES = ((96, 64), (97, 65))
OFFSETS_W = (0.25, 1.5, 64.0)


@pytest.mark.parametrize("palette", [1, 0])
def test_flat_order_kats_through_a_render(fr, lib, fx, palette):
    """smooth == false: the colour is a function of the escape index, so any view with a pixel of the KAT's index shows it"""
    seen = 0
    try:
        check(lib.fr_set_palette(palette))
        for j in np.flatnonzero(fx.kat_path == "flat"):
            p = int(fx.kat_colour[j])
            ocfg = O.cli_config(96, 64, iterations=int(fx.kat_iterations[j]), exposure=float(fx.kat_exposure[j]), smooth=0,
                                primary_color=(p, p, p))
            cfg = to_fr(fr, ocfg)
            for op, fp in ((O.F64, fr.Precision.F64), (O.F32, fr.Precision.F32)):
                z, it = O.escape_rows(ocfg, op, threads=1)
                hit = (it == fx.kat_iters[j]) & ((z ** 2).sum(axis=-1) > ocfg.stable_limit)
                assert hit.any(), (int(j), int(fx.kat_iters[j]))
                want = O.get_image(ocfg, op, threads=1)
                assert (want[hit] == fx.kat_byte[j]).all()
                got = fr.get_image(cfg, fp)
                assert np.array_equal(got, want), (int(j), palette, op, got[hit][0].tolist(), int(fx.kat_byte[j]), int(fx.kat_alt_byte[j]))
                seen += 1
    finally:
        lib.fr_set_palette(1)
    assert seen >= 2 * 16


def flip_exposure(ocfg, z1, it1, k, B):
    """the smallest f64 exposure at which the oracle's byte of channel k of the pixel (z1, it1) is >= B (the byte is monotone in
    the exposure), by bisection over the f64s"""
    def byte(e):
        ocfg.exposure = e
        return int(truth_rows(ocfg, z1, it1)[0, k])

    lo, hi = 1e-6, 1e6
    assert byte(lo) < B <= byte(hi)
    while math.nextafter(lo, math.inf) < hi:
        mid = math.sqrt(lo) * math.sqrt(hi)
        if not lo < mid < hi:
            mid = math.nextafter(lo, math.inf)
        if byte(mid) >= B:
            hi = mid
        else:
            lo = mid
    return hi


def aimed_exposures(ocfg, z, it):
    """(pixel, channel, boundary, offset in W, exposure): three escaped pixels with different indices, one (channel, boundary) each,
    the exposure E* (1 + d / B) for d = +- W * OFFSETS_W around the pixel's flip point E*"""
    n = ocfg.iterations
    dist = (z ** 2).sum(axis=-1)
    prim = (ocfg.primary_color.r, ocfg.primary_color.g, ocfg.primary_color.b)
    out, used = [], set()
    targets = [(0, 17), (1, 2), (2, 254)]
    flat_it, flat_dist = it.reshape(-1), dist.reshape(-1)
    for px in np.argsort(flat_dist, kind="stable")[::-1]:  # the farthest out first: ordinary escaped pixels, deterministic
        i = int(flat_it[px])
        if not 2 <= i < n or i in used or not 2.0 ** 33 < flat_dist[px] < 2.0 ** 60:
            continue
        used.add(i)
        k, B = targets[len(out) // (2 * len(OFFSETS_W))]
        z1, it1 = z.reshape(-1, 2)[px:px + 1], flat_it[px:px + 1]
        e_star = flip_exposure(ocfg, z1, it1, k, B)
        W = prim[CM.CH[k]] * (e_star / n) * 2.0 ** -18
        for m in OFFSETS_W:
            for sgn in (1.0, -1.0):
                out.append((int(px), k, B, sgn * m, e_star * (1.0 + sgn * m * W / B)))
        if len(out) == 3 * 2 * len(OFFSETS_W):
            return out
    raise AssertionError("the view has fewer than three usable escape indices")


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_render_kernels_at_exposures_aimed_at_a_pixels_boundary(fr, lib, fx, precision, size):
    """every first- and second-pass kernel's own copy of the map (tiles 0, 9, 10, 11, 13, 16): the whole image against get_image"""
    op, fp = (O.F64, fr.Precision.F64) if precision == "f64" else (O.F32, fr.Precision.F32)
    ocfg = O.cli_config(size[0], size[1], **VIEW)
    z, it = O.escape_rows(ocfg, op, threads=1)
    aims = aimed_exposures(ocfg, z, it)
    assert len({a[0] for a in aims}) == 3
    try:
        for px, k, B, m, e in aims:
            ocfg.exposure = e
            want = O.get_image(ocfg, op, threads=1)
            assert want.reshape(-1, 3)[px, k] == (B if m > 0 else B - 1), (px, k, B, m)
            cfg = to_fr(fr, ocfg)
            for tile in (0, 9, 10, 11, 13, 16):
                check(lib.fr_set_tile(tile))
                got = fr.get_image(cfg, fp)
                assert np.array_equal(got, want), (precision, size, tile, dict(pixel=px, channel=k, boundary=B, offset_W=m, exposure=e),
                                                   int((got != want).any(axis=-1).sum()), got.reshape(-1, 3)[px].tolist(),
                                                   want.reshape(-1, 3)[px].tolist())
    finally:
        lib.fr_set_tile(0)


@pytest.mark.parametrize("road", ["dd", "pt", "bla", "scaled"])
def test_deep_roads_at_exposures_aimed_at_a_pixels_boundary(fr, lib, fx, road):
    """fr_dd.hip's, fr_pt.hip's, fr_bla.hip's and fr_scaled.hip's copies of the map — DD and PT through fr_render_rows_rgb8 (and
    through their own row calls with pos_lo = 0) on the shallow view, BLA-PT and SCALED PT on tests/deep_edge_views.py's view of the point i at 1e18.  The image of a deep road is the colour
    map over the road's own fr_escape_rows* arrays (include/fractal_hip.h), so the aim and the truth are taken from those."""
    if road in ("dd", "pt"):
        prec = fr.Precision.DD if road == "dd" else fr.Precision.PT
        ocfg = O.cli_config(*SIZES[1], **VIEW)
        kw = dict(pos_lo=(0.0, 0.0))
    else:
        prec = fr.Precision.PT
        ocfg = O.config_new()
        E.make(ocfg, "deep_scale_a")
        ocfg.iterations = 300
        kw = dict(centre=fr.WideCentre.from_str("0", "1", scale=(ocfg.scale.re, ocfg.scale.im)))
        kw.update(dict(bla=0) if road == "bla" else dict(scaled=True))
    plain = road in ("dd", "pt")  # pos_lo = 0: the road is reached through the general calls, with the precision alone ...
    z, it = fr.escape_rows(to_fr(fr, ocfg), precision=prec, **({} if plain else kw))
    assert z.shape[-1] == 2
    if plain:  # ... and through its own calls with a zero pos_lo: the same arrays
        z0, it0 = fr.escape_rows(to_fr(fr, ocfg), precision=prec, **kw)
        assert np.array_equal(it0, it) and np.array_equal(z0.view(np.uint64), z.view(np.uint64))
    for px, k, B, m, e in aimed_exposures(ocfg, z, it):
        ocfg.exposure = e
        want = truth_rows(ocfg, z, it)
        assert want.reshape(-1, 3)[px, k] == (B if m > 0 else B - 1), (px, k, B, m)
        cfg = to_fr(fr, ocfg)
        where = (road, dict(pixel=px, channel=k, boundary=B, offset_W=m, exposure=e))
        if plain:
            got = np.zeros_like(want)
            check(lib.fr_render_rows_rgb8(C.byref(cfg), int(prec), 0, cfg.height, got.ctypes.data, got.nbytes))
            assert np.array_equal(got, want), ("fr_render_rows_rgb8",) + where + (int((got != want).any(axis=-1).sum()),)
        got = fr.get_image(cfg, prec, **kw)
        assert np.array_equal(got, want), where + (int((got != want).any(axis=-1).sum()),)
