"""Statistics of a kept view on the device (include/fractal_hip.h, "statistics of a kept view": fr_view_stats_device,
fr_view_stats; kernels view_stats_range_kernel, view_stats_hist_kernel), field for field and exactly against
tests/view_stats_model.py:
  - tails of every size around the wave, the workgroup and the tile, both z widths, a z that is 8- but not 16-byte aligned;
  - a stale record, the same record twice, an empty array;
  - the edges of the three classes (the limit itself, NaN, infinities, it around the cap, cap 0, the low parts of z_width 4)
    and of the range (shift 0 .. 22, the last bin, a non-zero minimum);
  - everything in one bin, and one pixel in 64 elsewhere (the wave's aggregated and mixed paths); no escaped pixel at all;
  - stream order behind the render that fills the arrays; one array past 2^32 bytes;
  - real views on every road: the record, the exposure it gives, and the recoloured bytes against the library's own render
    (and the oracle's, for F64) of the same config at that exposure; and that the deep view the feature was built for shows
    more colours with it than without."""
import importlib.util
import math
import os

import numpy as np
import pytest

import deep_edge_views as E
import oracle_lib as O
import view_stats_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # bytes, a multiple of 8
U32_MAX = 2 ** 32 - 1


@pytest.fixture(scope="module")
def fr():
    import fractal_renderer_amd

    assert fractal_renderer_amd.device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    fractal_renderer_amd.init(0)
    assert fractal_renderer_amd.device_name().startswith("gfx950")
    return fractal_renderer_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def config(fr, iterations=50, stable_limit=2.0, algo=0):
    cfg = fr.Config.new(algo)
    cfg.iterations, cfg.stable_limit = iterations, stable_limit
    return cfg


class Record:
    """the 8248 bytes of a record in device memory between guard bytes, pre-filled with 0xFF: stale contents must not matter"""

    def __init__(self, torch):
        self.torch = torch
        self.buf = torch.full((GUARD + M.SIZEOF + GUARD,), 0xFF, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 8 == 0
        self.ptr = self.buf.data_ptr() + GUARD

    def read(self, fr):
        self.torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        assert (raw[:GUARD] == 0xFF).all() and (raw[GUARD + M.SIZEOF:] == 0xFF).all(), "a write outside the record"
        return M.from_struct(fr.ViewStats.from_bytes(raw[GUARD:GUARD + M.SIZEOF].tobytes()))


def upload(torch, z, it, misalign=False):
    """numpy z float64 [n, zw], it uint32 [n] -> (keep-alive, z pointer, iters pointer); misalign: z 8 bytes off a 16-byte
    boundary"""
    flat = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
    pad = 1 if misalign else 0
    dz = torch.from_numpy(np.concatenate([np.zeros(pad), flat])).to("cuda:0")
    di = torch.from_numpy(np.ascontiguousarray(it, dtype=np.uint32).reshape(-1).view(np.int32).copy()).to("cuda:0")
    assert dz.data_ptr() % 16 == 0
    return (dz, di), dz.data_ptr() + 8 * pad, di.data_ptr()


def device_stats(fr, torch, cfg, z, it, misalign=False, record=None):
    z = np.asarray(z, dtype=np.float64)
    z = z.reshape(-1, z.shape[-1])
    keep, zp, ip = upload(torch, z, it, misalign)
    record = record or Record(torch)
    fr.view_stats_device(cfg, zp, ip, z.shape[0], record.ptr, z_width=z.shape[1])
    got = record.read(fr)
    del keep
    return got


def field(rec, name):
    return rec["hist"][int(name[5:-1])] if name.startswith("hist[") else rec[name]


def assert_record(got, want, what):
    d = M.diff(got, want)
    assert not d, "%s: %d fields differ, (field, got, want) of the first: %s" % (what, len(d), [(f, field(got, f), field(want, f)) for f in d[:4]])


def check(fr, torch, cfg, z, it, what, misalign=False):
    z = np.asarray(z, dtype=np.float64)
    want = M.view_stats(z, it, cfg.iterations, cfg.stable_limit)
    assert_record(device_stats(fr, torch, cfg, z, it, misalign), want, what)
    return want


# ---- tails --------------------------------------------------------------------------------------------------------

TAILS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 1000003]  # around the wave, the workgroup (1024) and its tile (4096)


@pytest.fixture(scope="module")
def noise():
    """1 000 003 pixels of every class: positions around the stable limit, indices around the cap of 50"""
    rng = np.random.default_rng(77)
    z = rng.normal(0.0, 1.3, size=(TAILS[-1], 4))
    it = rng.integers(0, 54, size=TAILS[-1], dtype=np.uint32)
    z.setflags(write=False)
    it.setflags(write=False)
    return z, it


@pytest.mark.parametrize("zw", [2, 4])
@pytest.mark.parametrize("n", TAILS)
def test_tails(fr, torch, noise, n, zw):
    z, it = noise
    cfg = config(fr)
    # the array's END is what a tail gets wrong: take the last n pixels, so that every size sees other data
    zs, its = z[-n:, :zw], it[-n:]
    want = check(fr, torch, cfg, zs, its, "n = %d" % n)
    if n >= 4097:
        assert min(want["stable"], want["capped"], want["escaped"]) > 0 and want["shift"] == 0
    check(fr, torch, cfg, zs, its, "n = %d, z 8 bytes off a 16-byte boundary" % n, misalign=True)
    host = M.from_struct(fr.view_stats(cfg, zs, its))  # the host form: context scratch, one small download
    assert_record(host, want, "fr_view_stats, n = %d" % n)


# ---- a stale record -------------------------------------------------------------------------------------------------


def test_a_stale_record_the_same_record_twice_and_an_empty_array(fr, torch, noise):
    z, it = noise
    cfg = config(fr)
    rec = Record(torch)  # 0xFF everywhere
    a = (z[:5000, :2], it[:5000])
    b = (z[5000:5300, :2] * 3.0, it[5000:5300] % np.uint32(7))
    for zs, its in (a, b, a):
        assert_record(device_stats(fr, torch, cfg, zs, its, record=rec), M.view_stats(zs, its, 50, 2.0), "a record used before")
    fr.view_stats_device(cfg, 0, 0, 0, rec.ptr)  # n == 0: the all-zero record, queued like any other
    got = rec.read(fr)
    assert got == M.view_stats(np.empty((0, 2)), np.empty(0, dtype=np.uint32), 50, 2.0) and not any(got["hist"])
    # two calls into the same record with nothing between them: the stream orders them
    (k1, zp1, ip1), (k2, zp2, ip2) = upload(torch, *a), upload(torch, *b)
    fr.view_stats_device(cfg, zp1, ip1, 5000, rec.ptr)
    fr.view_stats_device(cfg, zp2, ip2, 300, rec.ptr)
    assert_record(rec.read(fr), M.view_stats(*b, 50, 2.0), "the second of two queued calls")


# ---- class edges ----------------------------------------------------------------------------------------------------

INF, NAN = math.inf, math.nan
EDGE_POSITIONS = [(1.5, 0.5), (0.0, 0.0), (-0.0, 0.0), (1.0, 1.0), (3.0, -4.0), (NAN, 0.0), (0.0, NAN), (INF, NAN), (INF, 0.0),
                  (-INF, 1.0), (INF, -INF), (1e200, 1e200), (1e-200, 1e-200), (5e-324, 0.0), (1.3407807929942596e154, 0.0)]


def edge_arrays(n_cap):
    its = sorted({0, 1, max(n_cap - 1, 0), n_cap, min(n_cap + 1, U32_MAX), U32_MAX, U32_MAX - 1})
    z = np.array([p for p in EDGE_POSITIONS for _ in its], dtype=np.float64)
    it = np.array([i for _ in EDGE_POSITIONS for i in its], dtype=np.uint32)
    return z, it


@pytest.mark.parametrize("n_cap", [0, 1, 50, U32_MAX], ids=lambda v: "cap%d" % v)
def test_class_edges(fr, torch, n_cap):
    z, it = edge_arrays(n_cap)
    assert 1.5 * 1.5 + 0.5 * 0.5 == 2.5
    limits = [2.5, math.nextafter(2.5, 0.0), math.nextafter(2.5, 3.0), 2.0, 0.0, -0.0, -1.0, INF, -INF, 1e308, 5e-324]
    for limit in limits:
        cfg = config(fr, n_cap, limit)
        want = check(fr, torch, cfg, z, it, "stable_limit %r, cap %d" % (limit, n_cap))
        if limit == INF:
            assert want["stable"] == want["n"]
        if n_cap == 0:
            assert want["escaped"] == 0 and want["shift"] == 0 and want["max_iters"] == 0
    # dist == stable_limit is S, the next double above it is E: the pixel (1.5, 0.5) on either side of the comparison
    one = (np.array([[1.5, 0.5]]), np.array([3], dtype=np.uint32))
    if n_cap > 3:
        assert check(fr, torch, config(fr, n_cap, 2.5), *one, "dist == limit")["stable"] == 1
        assert check(fr, torch, config(fr, n_cap, math.nextafter(2.5, 0.0)), *one, "dist one ulp above the limit")["escaped"] == 1


def test_z_width_4_reads_the_hi_parts_only(fr, torch):
    cfg = config(fr, 50, 2.0)
    # re.hi, re.lo, im.hi, im.lo: low parts that would change the class if they were read, in either direction
    z = np.array([[1.0, 9.0, 1.0, 9.0], [2.0, NAN, 2.0, NAN], [0.5, INF, 0.5, -INF], [3.0, -3.0, 0.0, 0.0], [NAN, 5.0, 0.0, 5.0]] * 70)
    it = np.arange(len(z), dtype=np.uint32) % np.uint32(60)
    want = check(fr, torch, cfg, z, it, "z_width 4")
    as_two = M.view_stats(np.ascontiguousarray(z[:, 0::2]), it, 50, 2.0)
    assert want == as_two and want["stable"] == 3 * 70 and want["escaped"] > 0


# ---- range edges ----------------------------------------------------------------------------------------------------

RANGES = [(7, 0, 0), (7, 1023, 0), (7, 1024, 1), (0, 1023, 0), (123456, 2 ** 24 - 1, 14), (0, 2 ** 32 - 2, 22), (5, 2 ** 32 - 7, 22),
          (2 ** 31 - 3, 2048, 2)]


@pytest.mark.parametrize("lo,span,shift", RANGES, ids=["min%d_span%d" % r[:2] for r in RANGES])
def test_range_edges(fr, torch, lo, span, shift):
    rng = np.random.default_rng(lo + span)
    hi = lo + span
    it = np.concatenate([rng.integers(lo, hi + 1, size=3000, dtype=np.uint64), [lo, hi, hi, (lo + hi) // 2]]).astype(np.uint32)
    rng.shuffle(it)
    z = np.tile([3.0, 0.0], (len(it), 1))
    cfg = config(fr, min(hi + 1, U32_MAX), 2.0)
    want = check(fr, torch, cfg, z, it, "indices %d .. %d" % (lo, hi))
    assert (want["min_iters"], want["max_iters"], want["shift"], want["escaped"]) == (lo, hi, shift, len(it))
    assert want["hist"][span >> shift] >= 2 and not any(want["hist"][(span >> shift) + 1:])  # the last bin used is hi's
    if span == 1023 or span == 2 ** 32 - 2:
        assert want["hist"][1023] >= 2


# ---- one bin ----------------------------------------------------------------------------------------------------------


def test_one_bin_and_one_pixel_in_64_elsewhere(fr, torch):
    n = 200000
    cfg = config(fr, 3000, 2.0)
    z = np.tile([0.0, -2.5], (n, 1))
    same = np.full(n, 137, dtype=np.uint32)
    want = check(fr, torch, cfg, z, same, "one index")
    assert want["hist"][0] == n and want["shift"] == 0 and want["sum_iters"] == 137 * n
    mixed = same.copy()
    mixed[5::64] = 900  # one lane of every wave in another bin: the wave's second round
    want = check(fr, torch, cfg, z, mixed, "every 64th pixel different")
    assert want["hist"][0] == n - len(mixed[5::64]) and want["hist"][763] == len(mixed[5::64])
    three = same.copy()
    three[5::64], three[6::64], three[40::64] = 900, 901, 2999  # four bins in every wave: two rounds, then the lanes left over
    check(fr, torch, cfg, z, three, "four bins in a wave")
    holes = mixed.copy()
    z2 = z.copy()
    z2[0::3] = (0.1, 0.1)  # S pixels between them: the first active lane is not lane 0
    holes[1::5] = 3000     # and capped ones
    check(fr, torch, cfg, z2, holes, "one bin with holes")


def test_no_escaped_pixel_at_all(fr, torch):
    n = 70001
    cfg = config(fr, 50, 2.0)
    it = np.arange(n, dtype=np.uint32) % np.uint32(50)
    for z, its, field in ((np.tile([0.5, 0.5], (n, 1)), it, "stable"), (np.tile([2.0, 2.0], (n, 1)), it + np.uint32(50), "capped")):
        want = check(fr, torch, cfg, z, its, "no E, all %s" % field)
        assert want[field] == n and want["escaped"] == 0
        assert (want["min_iters"], want["max_iters"], want["shift"], want["sum_iters"]) == (0, 0, 0, 0) and not any(want["hist"])


# ---- stream order -----------------------------------------------------------------------------------------------------


def test_statistics_queued_behind_the_render_on_one_stream(fr, torch):
    cfg = config(fr, 200)
    cfg.width, cfg.height = 160, 90
    npx = cfg.width * cfg.height
    dz = torch.full((2 * npx,), NAN, dtype=torch.float64, device="cuda:0")
    di = torch.full((npx,), -1, dtype=torch.int32, device="cuda:0")
    rec = Record(torch)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    fr.escape_rows_device(cfg, dz.data_ptr(), di.data_ptr(), stream=stream.cuda_stream)
    fr.view_stats_device(cfg, dz.data_ptr(), di.data_ptr(), npx, rec.ptr, stream=stream.cuda_stream)  # no synchronisation between
    stream.synchronize()
    got = rec.read(fr)
    z, it = dz.cpu().numpy().reshape(npx, 2), di.cpu().numpy().view(np.uint32)
    want = M.view_stats(z, it, 200, cfg.stable_limit)
    assert_record(got, want, "behind fr_escape_rows_device")
    assert want["escaped"] > 0 and want["stable"] > 0


# ---- 64-bit indexing ---------------------------------------------------------------------------------------------------


def test_an_array_past_four_gigabytes(fr, torch):
    n = 2 ** 28 + 77
    free = torch.cuda.mem_get_info()[0]
    if free < 16 * 2 ** 30:
        pytest.skip("the device has %.1f GiB free; the 2^28 + 77 pixel case needs 16" % (free / 2 ** 30))
    dev = "cuda:0"
    cap = 5000
    k = torch.arange(n, dtype=torch.int64, device=dev)
    it = (k * 2654435761 + 12345) % 4099  # 0 .. 4098, all below the cap
    it[-77:] = 4500 + torch.arange(77, dtype=torch.int64, device=dev)  # the maximum lives in the tail, past 2^32 bytes of z
    it[2 ** 28 - 3] = 5000                                              # one capped pixel just under the boundary
    re = ((k + 5) % 7).to(torch.float64) * 0.5  # dist = 0, .25, 1, 2.25, 4, 6.25, 9 against a limit of 2: S for (k + 5) % 7 < 3
    del k
    z = torch.stack([re, torch.zeros_like(re)], dim=1).contiguous()
    outside = (re * re) > 2.0
    del re
    capped = outside & (it >= cap)
    esc = outside & ~capped
    ie = it[esc]
    lo, hi = int(ie.min()), int(ie.max())
    want = dict(n=n, stable=int((~outside).sum()), capped=int(capped.sum()), escaped=int(esc.sum()), sum_iters=int(ie.sum()), min_iters=lo,
                max_iters=hi, shift=M.shift_of(lo, hi), reserved=0)
    want["hist"] = [int(v) for v in torch.bincount((ie - lo) >> want["shift"], minlength=M.BINS).cpu()]
    assert (hi, want["capped"], want["shift"]) == (4576, 1, 3) and z.numel() * 8 > 2 ** 32
    di = it.to(torch.int32)
    del it, ie, outside, capped, esc
    rec = Record(torch)
    fr.view_stats_device(config(fr, cap, 2.0), z.data_ptr(), di.data_ptr(), n, rec.ptr)
    assert_record(rec.read(fr), want, "n = 2^28 + 77")
    del z, di
    torch.cuda.empty_cache()


# ---- real views ---------------------------------------------------------------------------------------------------------


def recolour_on_device(fr, torch, cfg, z, it):
    """fr_colour_rows_device over the uploaded arrays -> uint8 [rows, width, 3]"""
    zw = z.shape[-1]
    keep, zp, ip = upload(torch, z.reshape(-1, zw), it)
    out = torch.zeros(3 * it.size, dtype=torch.uint8, device="cuda:0")
    fr.colour_rows_device(cfg, zp, ip, it.size, out.data_ptr(), z_width=zw)
    torch.cuda.synchronize()
    del keep
    return out.cpu().numpy().reshape(it.shape + (3,))


def with_exposure(cfg, exposure):
    shown = cfg.clone()
    shown.exposure = exposure
    return shown


def view_and_exposure(fr, torch, cfg, z, it, p=0.99):
    """the record of (z, iters) on both forms against the model; -> the exposure, checked against the model's"""
    want = M.view_stats(z, it, cfg.iterations, cfg.stable_limit)
    st = fr.view_stats(cfg, z, it)
    assert_record(M.from_struct(st), want, "fr_view_stats")
    assert_record(device_stats(fr, torch, cfg, z, it), want, "fr_view_stats_device")
    assert want["escaped"] > 0
    exposure = fr.auto_exposure(cfg, st, p)
    assert exposure == M.auto_exposure(cfg.iterations, cfg.exposure, want, p) and fr.stats_percentile(st, p) == M.percentile(want, p)
    return exposure


@pytest.mark.parametrize("algo", [0, 2], ids=["mandelbrot", "julia"])
@pytest.mark.parametrize("precision", [0, 1], ids=["f64", "f32"])
def test_default_views(fr, torch, algo, precision):
    cfg = fr.Config.new(algo)
    cfg.width, cfg.height = 96, 64
    z, it = fr.escape_rows(cfg, precision=precision)
    exposure = view_and_exposure(fr, torch, cfg, z, it)
    shown = with_exposure(cfg, exposure)
    render = fr.get_image(shown, precision=precision)
    assert np.array_equal(recolour_on_device(fr, torch, shown, z, it), render)
    image, e = fr.get_image_auto(cfg, precision=precision)
    assert e == exposure and np.array_equal(image, render)
    if precision == 0:
        O.lib()
        O.set_log2_mode(O.LOG2_SOFT)  # the log2 the kernels carry
        try:
            assert np.array_equal(O.get_image(O.Config.from_buffer_copy(bytes(shown))), render)
        finally:
            O.set_log2_mode(O.LOG2_LIBM)
    image, e = fr.get_image_auto(cfg, percentile=1.0, precision=precision)
    assert e == cfg.iterations / max(int(it[it < cfg.iterations].max()), 1) and np.array_equal(image, fr.get_image(with_exposure(cfg, e), precision=precision))


def test_dd_view_with_its_low_parts(fr, torch):
    cfg = fr.Config.new()
    E.make(cfg, "deep_scale_a")
    cfg.width, cfg.height = 64, 48
    z, it = fr.escape_rows(cfg, precision=fr.Precision.DD, pos_lo=E.LO_I, with_lo=True)
    assert z.shape == (48, 64, 4)
    exposure = view_and_exposure(fr, torch, cfg, z, it)
    shown = with_exposure(cfg, exposure)
    render = fr.get_image(shown, precision=fr.Precision.DD, pos_lo=E.LO_I)
    assert np.array_equal(recolour_on_device(fr, torch, shown, z, it), render)
    image, e = fr.get_image_auto(cfg, precision=fr.Precision.DD, pos_lo=E.LO_I)
    assert e == exposure and np.array_equal(image, render)


DEEP_ROADS = {"wide": dict(), "bla": dict(bla=0), "scaled": dict(scaled=True)}


@pytest.mark.parametrize("road", list(DEEP_ROADS))
def test_deep_roads(fr, torch, road):
    kw = DEEP_ROADS[road]
    cfg = fr.Config.new()
    E.make(cfg, "deep_scale_a")  # 96 x 64 at (0, 1), scale (1e18, -3e17), cap 3000
    centre = fr.WideCentre.from_str("0", "1", scale=(cfg.scale.re, cfg.scale.im))
    z, it = fr.escape_rows(cfg, precision=fr.Precision.PT, centre=centre, **kw)
    exposure = view_and_exposure(fr, torch, cfg, z, it)
    shown = with_exposure(cfg, exposure)
    render = fr.get_image(shown, precision=fr.Precision.PT, centre=centre, **kw)
    assert np.array_equal(recolour_on_device(fr, torch, shown, z, it), render)
    image, e = fr.get_image_auto(cfg, precision=fr.Precision.PT, centre=centre, **kw)
    assert e == exposure and np.array_equal(image, render)
    # anti-aliased: the statistics are those of the twice larger view, the image is the road's supersampled render
    image, e = fr.get_image_auto(cfg, precision=fr.Precision.PT, centre=centre, supersample=2, **kw)
    big = cfg.clone()
    big.width, big.height = 2 * cfg.width, 2 * cfg.height
    zb, itb = fr.escape_rows(big, precision=fr.Precision.PT, centre=centre, **kw)
    assert e == M.auto_exposure(cfg.iterations, cfg.exposure, M.view_stats(zb, itb, cfg.iterations, cfg.stable_limit), 0.99)
    assert np.array_equal(image, fr.get_image_ss_pt(with_exposure(cfg, e), 2, centre=centre, **kw))


def test_the_deep_view_shows_more_colours_with_it(fr):
    """the 2^200 Misiurewicz view of profiles/pt_wide_orbit.txt (rows escape at 122 .. 191 under a cap of 3000, 20 distinct
    colours at 1080p), reduced to 96 x 54"""
    spec = importlib.util.spec_from_file_location("pt_wide_orbit", os.path.join(ROOT, "tools", "pt_wide_orbit.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    mis = tool.newton([1, 2, 2, 2], -0.22815549, 1.11514251)
    view = fr.Config.new()
    view.width, view.height, view.iterations, view.limit = 96, 54, 3000, 2.0
    view.scale.re = view.scale.im = 2.0 ** 200
    centre = tool.wide_centre(mis[0], mis[1], 5)
    plain = fr.get_image(view, precision=fr.Precision.PT, centre=centre)
    auto, exposure = fr.get_image_auto(view, precision=fr.Precision.PT, centre=centre)
    colours = [len(np.unique(im.reshape(-1, 3), axis=0)) for im in (plain, auto)]
    print("distinct colours: %d at exposure %g, %d at the chosen %g" % (colours[0], view.exposure, colours[1], exposure))
    assert exposure > view.exposure and colours[1] > colours[0]
