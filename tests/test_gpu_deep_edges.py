"""FR_PRECISION_DD (csrc/fr_dd.hip) and FR_PRECISION_PT (csrc/fr_pt.hip) against their host models (tests/dd_model.c,
tests/pt_model.c) bit for bit, away from the nice views of test_gpu_dd.py / test_gpu_pt.py: subnormal and tiny values,
views on the domain's bounds, unequal and negative scales, portrait, ragged and extreme shapes, outputs past 4 GiB, strided
counts, pixels outside the image, the iteration caps, a seeded random differential, and the PT orbit cache changed one
key field at a time.  Colours are the oracle's colour map in soft-log2 mode (the log2 the kernels carry) over the models'
final positions (DD: the hi parts)."""
import ctypes as C
import math

import numpy as np
import pytest

import dd_model as D
import deep_edge_views as V
import oracle_lib as O
import pt_model as P
from test_gpu_dd import fr, same_f64  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

DD, PT = 2, 3
LO_I = V.LO_I
PRECS = ["dd", "pt"]


def soft_colours(cfg, z2, it, rgba=False):
    """the oracle's colour map (soft log2) over f64 positions z2 [..., 2] and indices; Barnsley fern is black"""
    if cfg.algo not in (0, 2):
        rgb = np.zeros(np.shape(it) + (3,), dtype=np.uint8)
    else:
        O.set_log2_mode(O.LOG2_SOFT)
        try:
            rgb = O.colour_rows(O.Config.from_buffer_copy(bytes(cfg)), np.ascontiguousarray(z2), it)
        finally:
            O.set_log2_mode(O.LOG2_LIBM)
    if not rgba:
        return rgb
    out = np.full(rgb.shape[:-1] + (4,), 255, dtype=np.uint8)
    out[..., :3] = rgb
    return out


def model_rows(prec, cfg, lo=(0.0, 0.0), y0=0, y1=None):
    """(z as the library returns it: DD [.., 4] with the lo parts, PT [.., 2]; the f64 positions coloured; indices)"""
    if prec == "dd":
        z, it = D.escape_rows(cfg, lo, y0, y1)
        return z, np.ascontiguousarray(z[..., 0::2]), it
    z, it = P.escape_rows(cfg, lo, y0, y1)
    return z, z, it


def device_rows(fr, prec, cfg, lo=(0.0, 0.0), y0=0, y1=None):
    if prec == "dd":
        return fr.escape_rows(cfg, y0, y1, fr.Precision.DD, pos_lo=lo, with_lo=True)
    return fr.escape_rows(cfg, y0, y1, fr.Precision.PT, pos_lo=lo)


def model_count(prec, cfg, y0=0, y1=None):
    return (D if prec == "dd" else P).count_iterations(cfg, y0, y1)


def executed(it, cap):
    """the executed iterations of escape indices `it` (escape at i -> i + 1, exhaustion -> cap)"""
    it = np.asarray(it, dtype=np.uint64)
    return int(np.where(it < cap, it + 1, cap).sum())


def desc(cfg, lo, *more):
    return (bytes(cfg).hex(), float(lo[0]).hex(), float(lo[1]).hex()) + more


def check_all(fr, prec, cfg, lo, what=""):
    """escape rows (DD with lo parts), RGB, RGBA and the whole image's count against the model; returns the indices"""
    p = fr.Precision.DD if prec == "dd" else fr.Precision.PT
    d = desc(cfg, lo, prec, what)
    wz, wz2, wit = model_rows(prec, cfg, lo)
    z, it = device_rows(fr, prec, cfg, lo)
    assert np.array_equal(it, wit), d + ("escape indices differ at %d pixels" % int((it != wit).sum()),)
    assert same_f64(z, wz), d + ("final positions differ",)
    want = soft_colours(cfg, wz2, wit)
    img = fr.get_image(cfg, p, pos_lo=lo)
    assert np.array_equal(img, want), d + ("RGB differs at %d pixels" % int((img != want).any(-1).sum()),)
    assert np.array_equal(fr.get_image_rgba(cfg, p, pos_lo=lo), soft_colours(cfg, wz2, wit, rgba=True)), d + ("RGBA",)
    total, npx = fr.count_iterations(cfg, precision=p)
    assert npx == cfg.width * cfg.height, d
    assert total == model_count(prec, cfg), d + ("count",)
    return wit


# ---- 1. edge views ----------------------------------------------------------------------------------------------------


def edge_view(fr, name):
    cfg = fr.Config.new(V.VIEWS[name][0])
    V.make(cfg, name)
    return cfg


@pytest.mark.parametrize("case", V.cases(flat=False), ids=V.case_id)
@pytest.mark.parametrize("prec", PRECS)
def test_edge_views_are_the_model_bit_for_bit(fr, prec, case):
    name, lo = case
    cfg = edge_view(fr, name)
    wit = check_all(fr, prec, cfg, lo)
    assert len(np.unique(wit)) >= 2, "the view is meant to be resolved"


@pytest.mark.parametrize("case", V.cases(flat=True), ids=V.case_id)
@pytest.mark.parametrize("prec", PRECS)
def test_flat_edge_views_are_the_model_bit_for_bit(fr, prec, case):
    """views with one escape index over the whole image: the comparison is on the final positions' bits"""
    name, lo = case
    cfg = edge_view(fr, name)
    wit = check_all(fr, prec, cfg, lo)
    assert len(np.unique(wit)) == 1


# ---- 2. seeded random differential ------------------------------------------------------------------------------------

DEEP_CENTRES = [(0.0, 1.0), (P.SEAHORSE_RE, P.SEAHORSE_IM), ("-1.7548776662466927600495", "0"), ("-0.75", "0.1"),
                ("0.26", "0"), ("-0.1011", "0.9563"), ("0.3602404434376143632361", "-0.6413130610648031748603"),
                ("-2", "0"), ("0", "0"), ("-1.25", "0")]


def random_config(fr, rng):
    """(Config, pos_lo) inside the DD / PT domain"""
    r = rng.random()
    algo = 0 if r < 0.5 else (2 if r < 0.9 else 1)
    cfg = fr.Config.new(algo)
    cfg.width, cfg.height = int(rng.integers(1, 161)), int(rng.integers(1, 161))
    centre = DEEP_CENTRES[int(rng.integers(len(DEEP_CENTRES)))]
    if rng.random() < 0.2:
        centre = (str(rng.uniform(-2.0, 0.5)), "0")  # the real axis
    (re, re_lo), (im, im_lo) = P.split(str(centre[0])), P.split(str(centre[1]))
    cfg.pos.re, cfg.pos.im = re, im

    def lo(p, dflt):
        if p == 0.0:
            return math.copysign(0.0, rng.choice([1.0, -1.0]))
        if rng.random() < 0.4:
            return dflt
        return math.ulp(p) * float(rng.uniform(-0.25, 0.25))

    pos_lo = (lo(re, re_lo), lo(im, im_lo))
    s = float(10 ** rng.uniform(-1, 300))
    other = s * float(rng.choice([1.0, 0.7, 1.9, -1.0, -0.3]))
    cfg.scale.re, cfg.scale.im = (s, other) if rng.random() < 0.5 else (other, s)
    cfg.iterations = int(rng.choice([0, 1, 2, 3, 17, 64, 255, 1000, 3000]))
    cfg.limit = float(rng.choice([2.0, 4.0, 0.5, 1000.5, 65536.0, 2.0 ** 500, 1e-300]))
    cfg.stable_limit = float(rng.choice([2.0, 0.5, 0.0, -1.0, 100.0]))
    cfg.exposure = float(rng.choice([5.0, 2.0, 0.3, 50.0, -1.0]))
    cfg.inside, cfg.smooth = int(rng.random() < 0.7), int(rng.random() < 0.7)
    cfg.primary_color.r, cfg.primary_color.g, cfg.primary_color.b = (int(v) for v in rng.integers(0, 256, 3))
    cfg.secondary_color.r, cfg.secondary_color.g, cfg.secondary_color.b = (int(v) for v in rng.integers(0, 256, 3))
    js = [(-0.8, 0.156), (0.0, 1.0), (-1.0, 0.0), (0.0, 0.0), (1e-310, -3e-320), (1e-200, 1e-170), (0.285, 0.01),
          (float(rng.uniform(-1.2, 0.6)), float(rng.uniform(-0.8, 0.8)))]
    cfg.julia_set.re, cfg.julia_set.im = js[int(rng.integers(len(js)))]
    return cfg, pos_lo


@pytest.mark.parametrize("seed", range(16))
@pytest.mark.parametrize("prec", PRECS)
def test_random_deep_configs_differential(fr, prec, seed):
    rng = np.random.default_rng(7000 + seed + (0 if prec == "dd" else 500))
    p = fr.Precision.DD if prec == "dd" else fr.Precision.PT
    for _ in range(3):
        cfg, lo = random_config(fr, rng)
        d = desc(cfg, lo, prec, seed)
        wz, wz2, wit = model_rows(prec, cfg, lo)
        z, it = device_rows(fr, prec, cfg, lo)
        assert np.array_equal(it, wit), d
        assert same_f64(z, wz), d
        if cfg.algo == 1:
            assert not wz.any() and not wit.any(), d
        assert np.array_equal(fr.get_image(cfg, p, pos_lo=lo), soft_colours(cfg, wz2, wit)), d
        assert np.array_equal(fr.get_image_rgba(cfg, p, pos_lo=lo), soft_colours(cfg, wz2, wit, rgba=True)), d
        y0 = int(rng.integers(0, cfg.height + 1))
        y1 = int(rng.integers(y0, cfg.height + 1))
        total, npx = fr.count_iterations(cfg, y0, y1, precision=p)
        assert npx == cfg.width * (y1 - y0), d
        assert total == model_count(prec, cfg, y0, y1), d + (y0, y1)


# ---- 3. shapes, addressing, entry points -------------------------------------------------------------------------------


def deep_mandelbrot(fr, w, h, iterations=500):
    cfg = fr.Config.new()
    D.deep_view(cfg, False, w, h, iterations)
    return cfg


@pytest.mark.parametrize("w,h", [(1, 1), (1, 17), (17, 1), (15, 15), (16, 16), (17, 17), (31, 33), (33, 31)])
@pytest.mark.parametrize("prec", PRECS)
def test_ragged_sizes(fr, prec, w, h):
    cfg = deep_mandelbrot(fr, w, h)
    cfg.scale.re, cfg.scale.im = 1e18 * 64 / w, 1e18 * 48 / h  # every size shows about the same patch
    check_all(fr, prec, cfg, LO_I, "%dx%d" % (w, h))
    check_all(fr, prec, cfg, (0.0, 0.0), "%dx%d" % (w, h))


@pytest.mark.parametrize("w,h", [(3, 300001), (500003, 2)])
@pytest.mark.parametrize("prec", PRECS)
def test_extreme_aspect_ratios(fr, prec, w, h):
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = w, h, 40
    cfg.pos.re = -0.6
    cfg.scale.re, cfg.scale.im = (0.4 * w / h, 0.4) if w > h else (0.4, 0.4)
    check_all(fr, prec, cfg, (0.0, 0.0), "%dx%d" % (w, h))


@pytest.mark.parametrize("prec", PRECS)
def test_device_renders_past_four_gigabytes(fr, prec):
    """40 000 x 36 000 into device memory: RGB is 4.32 GB and RGBA 5.76 GB, so pixel offsets pass 2^32"""
    import torch

    from fractal_renderer_amd import _native

    lib = _native.load()
    w, h = 40000, 36000
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = w, h, 50
    cfg.scale.re = cfg.scale.im = 0.01  # almost every pixel escapes within a few iterations
    assert 3 * w * h > 2 ** 32
    s = torch.cuda.current_stream()
    code = DD if prec == "dd" else PT
    lo_render = lib.fr_render_rows_dd_device if prec == "dd" else lib.fr_render_rows_pt_device
    d3 = torch.empty(3 * w * h, dtype=torch.uint8, device="cuda:0")
    _native.check(lib.fr_render_rows_rgb8_device(C.byref(cfg), code, 0, h, d3.data_ptr(), d3.numel(), s.cuda_stream))
    d4 = torch.empty(4 * w * h, dtype=torch.uint8, device="cuda:0")
    _native.check(lo_render(C.byref(cfg), None, 0, h, 4, d4.data_ptr(), d4.numel(), s.cuda_stream))
    torch.cuda.synchronize()
    rgb, rgba = d3.view(h, w, 3), d4.view(h, w, 4)
    for y in (0, h // 2 + 1, h - 1):
        _, wz2, wit = model_rows(prec, cfg, (0.0, 0.0), y, y + 1)
        assert np.array_equal(rgb[y].cpu().numpy(), soft_colours(cfg, wz2, wit)[0]), y
    for y0 in range(0, h, 4000):  # in slabs: a strided comparison of the whole image would copy it
        assert torch.equal(rgba[y0:y0 + 4000, :, :3], rgb[y0:y0 + 4000]), y0
        assert bool((rgba[y0:y0 + 4000, :, 3] == 255).all()), y0


@pytest.mark.parametrize("prec", PRECS)
def test_host_render_larger_than_the_scratch(fr, prec):
    """a host-buffer render that grows the context's scratch (6000 x 4000 RGBA, 96 MB), then a small one"""
    p = fr.Precision.DD if prec == "dd" else fr.Precision.PT
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = 6000, 4000, 50
    cfg.scale.re = cfg.scale.im = 0.01
    rgba = fr.get_image_rgba(cfg, p)
    for y in (0, 1, 2001, 3999):
        _, wz2, wit = model_rows(prec, cfg, (0.0, 0.0), y, y + 1)
        assert np.array_equal(rgba[y], soft_colours(cfg, wz2, wit, rgba=True)[0]), y
    rgb = fr.get_image_rows(cfg, 1000, 4000, p)
    assert np.array_equal(rgb, rgba[1000:, :, :3])
    check_all(fr, prec, deep_mandelbrot(fr, 40, 30), LO_I, "after the large render")


STRIDES = [(2, 3), (7, 1), (1, 5), (16, 16), ("w", "h"), (1000, 1000)]


@pytest.mark.parametrize("prec", PRECS)
def test_strided_counts(fr, prec):
    p = fr.Precision.DD if prec == "dd" else fr.Precision.PT
    for cfg in (deep_mandelbrot(fr, 257, 193, 3000), edge_view(fr, "deep_julia_scale_a")):
        w, h = cfg.width, cfg.height
        _, _, wit = model_rows(prec, cfg)
        for sx, sy in STRIDES:
            sx, sy = (w if sx == "w" else sx), (h if sy == "h" else sy)
            for y0, y1 in [(0, h), (1, h), (5, 150), (17, 18), (h - 1, h), (3, 3)]:
                y1 = min(y1, h)
                rows = [y for y in range(y0, y1) if y % sy == 0]
                want = executed(wit[rows][:, ::sx], cfg.iterations) if rows else 0
                total, npx = fr.count_iterations(cfg, y0, y1, sx, sy, precision=p)
                d = desc(cfg, (0.0, 0.0), prec, sx, sy, y0, y1)
                assert npx == len(range(0, w, sx)) * len(rows), d
                assert total == want, d


@pytest.mark.parametrize("prec", PRECS)
def test_get_recursive_pixel_outside_the_image(fr, prec):
    """get_recursive_pixel does not clamp x, y (calc/src/lib.rs:199-207); off_re depends on the width"""
    p = fr.Precision.DD if prec == "dd" else fr.Precision.PT
    base = fr.Config.new()
    base.width, base.height, base.iterations = 64, 48, 80
    for cfg in (base, deep_mandelbrot(fr, 64, 48, 3000), edge_view(fr, "deep_julia_scale_b")):
        w, h = cfg.width, cfg.height
        for x, y in [(0, 0), (w - 1, h - 1), (w, h), (1000, 3), (5, 4000), (4294967295, 4294967295)]:
            if prec == "dd":
                z, it = D.pixel(cfg, x, y)
                z2 = z[0::2]
            else:
                z2, it = P.pixel(cfg, x, y)
            want = soft_colours(cfg, z2.reshape(1, 2), np.array([it], dtype=np.uint32))[0]
            assert tuple(fr.get_recursive_pixel(cfg, x, y, p)) == tuple(want), desc(cfg, (0.0, 0.0), prec, x, y)


# ---- 4. caps ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("algo", ["mandelbrot", "julia"])
def test_pt_at_the_iteration_cap(fr, algo):
    """iterations = FR_PT_MAX_ITERATIONS on views where every pixel runs to the cap without a rebase: m reaches the last
    orbit entry (2^24 + 1 for R, 2^24 for V; a Julia view keeps both V and K)"""
    from fractal_renderer_amd import _native

    cfg = fr.Config.new(0 if algo == "mandelbrot" else 2)
    cfg.width, cfg.height = 8, 8
    cfg.scale.re = cfg.scale.im = 1e3
    if algo == "mandelbrot":
        cfg.pos.re, cfg.pos.im = -0.1, 0.0
    else:
        cfg.pos.re, cfg.pos.im = 0.05, 0.02
        cfg.julia_set.re, cfg.julia_set.im = -0.1, 0.1
    cfg.iterations = 1 << 24
    n = C.c_uint32(0)
    lib = _native.load()
    entries = [(0, (1 << 24) + 2)] if algo == "mandelbrot" else [(0, (1 << 24) + 1), (1, (1 << 24) + 1)]
    for which, want in entries:
        _native.check(lib.fr_debug_reference_orbit(C.byref(cfg), None, which, None, 0, C.byref(n)))
        assert n.value == want, (which, n.value)
    check_all(fr, "pt", cfg, (0.0, 0.0))
    _, it = fr.escape_rows(cfg, precision=fr.Precision.PT)
    assert (it == cfg.iterations).all()


def test_dd_at_the_u32_cap(fr):
    """iterations = u32::MAX and u32::MAX - 1 with a limit every orbit passes at once"""
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.limit, cfg.stable_limit = 40, 24, 1e-3, 0.0
    cfg.pos.re = -0.6
    cfg.iterations = 5
    _, _, wit = model_rows("dd", cfg)
    assert (wit == 0).all(), "a pixel that does not escape at once would run for minutes"
    for it in (4294967295, 4294967294):
        cfg.iterations = it
        for lo in ((0.0, 0.0), V.lo_for((-0.6, 0.0))):
            check_all(fr, "dd", cfg, lo, it)


# ---- 5. the PT orbit cache and concurrency ---------------------------------------------------------------------------


def test_pt_orbit_cache_one_field_at_a_time(fr):
    """A sequence of views on one thread, each differing from the one before in one field.  The fields of the orbit's
    key (algo, iterations, pos, pos_lo, julia_set) must miss the cache — each such step changes the model's result, so a
    stale orbit would show — and the others (limit, scale, size, colours, exposure) must give the new view's image."""
    cfg = fr.Config.new()
    own = P.seahorse_view(cfg, 48, 32, iterations=5000, scale=1e14)
    ure, uim = math.ulp(cfg.pos.re), math.ulp(cfg.pos.im)  # the low parts stay below a quarter of these
    steps = [("first", {}, own)]
    steps.append(("pos_lo.im", {}, (own[0], own[1] + 0.2 * uim)))
    steps.append(("pos_lo.re", {}, (own[0] + 0.3 * ure, own[1] + 0.2 * uim)))
    steps.append(("iterations - 1", dict(iterations=4999), steps[-1][2]))
    steps.append(("iterations + 1", dict(iterations=5000), steps[-1][2]))
    steps.append(("pos_lo +0", {}, (0.0, 0.0)))
    steps.append(("pos_lo -0", {}, (-0.0, -0.0)))
    steps.append(("pos_lo +0 again", {}, (0.0, 0.0)))
    steps.append(("limit", dict(limit=1000.5), (0.0, 0.0)))
    steps.append(("scale", dict(scale=(3e14, -1e14)), (0.0, 0.0)))
    steps.append(("size", dict(width=40, height=50), (0.0, 0.0)))
    steps.append(("colours", dict(primary_color=(9, 200, 77), secondary_color=(255, 1, 128)), (0.0, 0.0)))
    steps.append(("exposure", dict(exposure=0.7), (0.0, 0.0)))
    steps.append(("algo", dict(algo=2, julia_set=(0.0, 0.0)), (0.0, 0.0)))
    steps.append(("julia_set.im", dict(julia_set=(0.0, 5e-324)), (0.0, 0.0)))
    steps.append(("back to the first", "first", own))
    must_differ = {"pos_lo.im", "pos_lo.re", "iterations - 1", "pos_lo +0", "algo", "julia_set.im", "back to the first"}
    first = cfg.clone()
    prev = None
    for what, change, lo in steps:
        if change == "first":
            cfg = first.clone()
        else:
            for k, v in change.items():
                if k in ("pos", "scale", "julia_set"):
                    getattr(cfg, k).re, getattr(cfg, k).im = v
                elif k in ("primary_color", "secondary_color"):
                    c = getattr(cfg, k)
                    c.r, c.g, c.b = v
                else:
                    setattr(cfg, k, v)
        d = desc(cfg, lo, what)
        wz, _, wit = model_rows("pt", cfg, lo)
        if what in must_differ:
            assert prev is not None and (prev[0].shape != wz.shape or not same_f64(prev[0], wz)
                                         or not np.array_equal(prev[1], wit)), d + ("the step changes nothing",)
        prev = (wz, wit)
        z, it = fr.escape_rows(cfg, precision=fr.Precision.PT, pos_lo=lo)  # the first call of the step: hit or miss
        assert np.array_equal(it, wit) and same_f64(z, wz), d
        want = soft_colours(cfg, wz, wit)
        assert np.array_equal(fr.get_image(cfg, fr.Precision.PT, pos_lo=lo), want), d
        if all(v == 0.0 and math.copysign(1.0, v) > 0 for v in lo):  # the calls that take no pos_lo: the same key
            assert np.array_equal(fr.get_image(cfg, fr.Precision.PT), want), d
            for x, y in [(0, 0), (cfg.width - 1, cfg.height - 1), (cfg.width // 2, 3)]:
                assert tuple(fr.get_recursive_pixel(cfg, x, y, fr.Precision.PT)) == tuple(want[y, x]), d + (x, y)
            assert fr.count_iterations(cfg, 2, cfg.height, precision=fr.Precision.PT)[0] == executed(wit[2:], cfg.iterations), d
