"""Parity of the HIP path (through the C ABI) against the CPU oracle and the golden vectors.

Bar: byte-exact colours, integer-exact escape indices, bit-exact final positions (f64), at the
same precision and iteration cap as the CPU path.
"""
import ctypes as C
import math

import numpy as np
import pytest

import golden_util as G
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fr():
    import fractal_renderer_amd

    assert fractal_renderer_amd.device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    fractal_renderer_amd.init(0)
    assert fractal_renderer_amd.device_name().startswith("gfx950")
    return fractal_renderer_amd


def to_fr(fr, ocfg):
    return fr.Config.from_buffer_copy(bytes(ocfg))


def same_f64(a, b):
    """Bit-identical, except that any NaN matches any NaN: the sign/payload of a generated NaN is
    the platform's (x86 SSE makes 0xFFF8.., gfx950 0x7FF8..) — in the reference too."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(
        a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def oracle_image(ocfg, prec=O.F64, soft=True, **kw):
    O.set_log2_mode(O.LOG2_SOFT if soft else O.LOG2_LIBM)
    try:
        return O.get_image(ocfg, prec, **kw)
    finally:
        O.set_log2_mode(O.LOG2_LIBM)


# ---- device arithmetic the colour pass relies on -------------------------------------------


def _debug_math(fr, which, x):
    from fractal_renderer_amd import _native

    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    _native.check(_native.load().fr_debug_math(which, x.ctypes.data, y.ctypes.data, x.size))
    return y


def test_device_sqrt_is_correctly_rounded(fr):
    rng = np.random.default_rng(11)
    x = np.concatenate([
        np.exp(rng.uniform(-700, 700, 400_000)),
        rng.uniform(0, 4, 400_000),
        rng.uniform(2.0 ** 32, 2.0 ** 64, 200_000),
        (rng.integers(1, 2 ** 26, 200_000).astype(np.float64)) ** 2,          # perfect squares
        np.nextafter((rng.integers(1, 2 ** 26, 200_000).astype(np.float64)) ** 2, np.inf),
        np.array([0.0, -0.0, np.inf, 1.0, 2.0, 4.0, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308]),
    ])
    got = _debug_math(fr, 1, x)
    assert np.array_equal(got.view(np.uint64), np.sqrt(x).view(np.uint64))


def test_device_division_is_correctly_rounded(fr):
    rng = np.random.default_rng(12)
    x = np.concatenate([np.exp(rng.uniform(-300, 300, 500_000)) * rng.choice([-1.0, 1.0], 500_000),
                        rng.integers(1, 70000, 500_000).astype(np.float64)])
    got = _debug_math(fr, 2, x)
    want = x / np.roll(x, -1)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_device_saturating_cast(fr):
    """Rust `f64 as u8` (calc/src/lib.rs:135-137): truncate toward zero, saturate, NaN -> 0."""
    rng = np.random.default_rng(14)
    x = np.concatenate([rng.uniform(-10, 300, 200_000), rng.uniform(0, 1, 1000), np.arange(0, 258, dtype=np.float64),
                        np.nextafter(np.arange(0, 258, dtype=np.float64), -np.inf),
                        np.array([np.nan, -np.nan, np.inf, -np.inf, 1e300, -1e300, 4294967295.0, 4294967296.0,
                                  1e19, -0.0, 0.0, 0.9999999999999999, 254.99999999999997, 255.0, 5e-324, -5e-324])])
    got = _debug_math(fr, 3, x)
    with np.errstate(invalid="ignore"):
        want = np.where(np.isnan(x), 0.0, np.clip(np.trunc(x), 0, 255))
    assert np.array_equal(got, want)


def test_device_packed_saturating_cast(fr):
    """The colour filter's f32 stage casts with v_floor_f32 + v_cvt_pk_u8_f32 (fr_kernels.hip: sat_u8_pack): the
    same bytes as the plain cast on EVERY f32 bit pattern, in every byte position, other bytes left alone."""
    got = _debug_math(fr, 6, np.array([0.0, float(0xFFFFFFFF)]))
    assert got[0] == 0.0, "%d f32 patterns differ" % got[0]
    x = np.array([0.0, 0.4, 0.5, 0.6, 1.5, 2.5, 127.99999, 254.5, 254.9, 255.0, 255.5, 256.0, 1e9, -0.4, -0.6, -1.0, -1e9,
                  np.nan, np.inf, -np.inf])
    with np.errstate(invalid="ignore"):
        want = np.where(np.isnan(x), 0.0, np.clip(np.trunc(x.astype(np.float32).astype(np.float64)), 0, 255))
    assert np.array_equal(_debug_math(fr, 5, x), 0xAABB00DD + want * 256.0)


def test_device_log2_equals_host_soft_log2_and_tracks_libm(fr):
    rng = np.random.default_rng(13)
    x = np.concatenate([
        np.exp(rng.uniform(-700, 700, 100_000)), rng.uniform(0.5, 2, 100_000), 1 + rng.uniform(-0.04, 0.04, 100_000),
        rng.uniform(8, 16, 100_000), rng.uniform(65536, 2.0 ** 32, 100_000),
        np.array([0.0, -0.0, 1.0, 2.0, 0.5, np.inf, 5e-324, 1e-310, 65536.0, 0.96875, 1.03125]),
    ])
    got = _debug_math(fr, 0, x)
    O.set_log2_mode(O.LOG2_SOFT)
    soft = np.array([O.log2(v) for v in x.tolist()])
    O.set_log2_mode(O.LOG2_LIBM)
    assert np.array_equal(got.view(np.uint64), soft.view(np.uint64)), "device log2 != host build of the same source"
    libm = np.log2(x)
    fin = np.isfinite(libm)
    ulp = np.abs(got[fin].view(np.int64) - libm[fin].view(np.int64))
    assert ulp.max() <= 1
    assert math.isnan(_debug_math(fr, 0, np.array([-1.0]))[0]) and math.isnan(_debug_math(fr, 0, np.array([np.nan]))[0])


# ---- known answers through the reference-shaped API ------------------------


def test_kat_recursive(fr):
    pos, it = fr.recursive(50, (2, 0), (2, 0), 65536)
    assert (tuple(pos), it) == ((2090918.0, 0.0), 3)
    pos, it = fr.recursive(50, (2, 0), (2, 0), 2)
    assert (tuple(pos), it) == ((6.0, 0.0), 0)
    pos, it = fr.recursive(50, (-2, 0), (-2, 0), 65536)
    assert (tuple(pos), it) == ((2.0, 0.0), 50)
    assert fr.recursive(50, (-1, 0), (-1, 0), 65536)[1] == 50
    pos, it = fr.recursive(51, (-1, 0), (-1, 0), 65536)
    assert (tuple(pos), it) == ((0.0, 0.0), 51)
    for n in (0, 1, 50):
        pos, it = fr.recursive(n, (0, 0), (0, 0), 65536)
        assert (tuple(pos), it) == ((0.0, 0.0), n)


def test_kat_pixels_and_4x4_image(fr):
    cfg = fr.Config.new()
    cfg.width = cfg.height = 4
    cfg.scale.re = cfg.scale.im = 0.25
    assert fr.get_recursive_pixel(cfg, 0, 2) == (83, 83, 255)
    assert fr.get_recursive_pixel(cfg, 1, 2) == (240, 170, 0)
    img = fr.get_image(cfg)
    want = [[(0, 0, 5), (1, 1, 8), (1, 1, 9), (0, 0, 6)],
            [(1, 1, 12), (3, 3, 22), (240, 170, 0), (2, 2, 13)],
            [(83, 83, 255), (240, 170, 0), (0, 0, 0), (2, 2, 18)],
            [(1, 1, 12), (3, 3, 22), (240, 170, 0), (2, 2, 13)]]
    assert [[tuple(p) for p in row] for row in img.tolist()] == want
    cfg.smooth = 0
    img = fr.get_image(cfg)
    want = [[(4, 4, 30)] * 4,
            [(6, 6, 40), (8, 8, 51), (240, 170, 0), (6, 6, 40)],
            [(80, 80, 255), (240, 170, 0), (0, 0, 0), (6, 6, 40)],
            [(6, 6, 40), (8, 8, 51), (240, 170, 0), (6, 6, 40)]]
    assert [[tuple(p) for p in row] for row in img.tolist()] == want
    assert fr.get_recursive_pixel(cfg, 0, 2) == (80, 80, 255)


def test_recursive_batch_matches_oracle(fr):
    rng = np.random.default_rng(5)
    n = 5000
    start = rng.uniform(-2, 2, (n, 2))
    c = np.where(rng.random((n, 1)) < 0.5, start, rng.uniform(-1, 1, (n, 2)))
    for prec, f32 in ((fr.Precision.F64, False), (fr.Precision.F32, True)):
        for limit in (65536.0, 2.0):
            pos, it = fr.recursive_batch(300, start, c, limit, prec)
            for k in range(0, n, 7):
                wpos, wit = O.recursive(300, tuple(start[k]), tuple(c[k]), limit, f32=f32)
                assert it[k] == wit and tuple(pos[k]) == wpos, (k, prec, limit)


# ---- golden vectors ---------------------------------------------------------------------------


@pytest.mark.parametrize("key", G.KEYS)
def test_golden_vectors(fr, key):
    ocfg = G.oracle_config(key)
    cfg = to_fr(fr, ocfg)
    prec = fr.Precision.F32 if G.precision_of(key) == O.F32 else fr.Precision.F64
    v = G.vectors()
    z, it = fr.escape_rows(cfg, precision=prec)
    assert np.array_equal(it, v[key + "/iters"])
    if key + "/z" in v.files:
        assert same_f64(z, v[key + "/z"])
    img = fr.get_image(cfg, prec)
    assert np.array_equal(img, v[key + "/rgb"])
    total, npx = fr.count_iterations(cfg, precision=prec)
    assert total == G.MANIFEST[key]["executed_iterations"] and npx == cfg.width * cfg.height


@pytest.mark.parametrize("tile", [0, 1, 2, 4, 8, 9, 6401, 3202, 1604, 808])
def test_every_tile_shape_gives_the_same_bytes(fr, tile):
    from fractal_renderer_amd import _native

    v = G.vectors()
    try:
        _native.check(_native.load().fr_set_tile(tile))
        for key in ("mandelbrot_default/257x193/f64", "julia_m08_0156/257x193/f32", "limit_2/257x193/f64",
                    "deep_5e5/64x64/f64", "unsmooth/257x193/f32"):
            cfg = to_fr(fr, G.oracle_config(key))
            prec = fr.Precision.F32 if key.endswith("f32") else fr.Precision.F64
            assert np.array_equal(fr.get_image(cfg, prec), v[key + "/rgb"]), (tile, key)
            assert fr.count_iterations(cfg, precision=prec)[0] == G.MANIFEST[key]["executed_iterations"]
    finally:
        _native.load().fr_set_tile(0)


@pytest.mark.parametrize("mode", [-1, 0, 2, 4])
def test_every_orbit_loop_gives_the_same_bytes(fr, mode):
    """The scaled / check-skipping loops (fr_kernels.hip) against the golden vectors, forced on."""
    from fractal_renderer_amd import _native

    v = G.vectors()
    keys = [k for k in G.KEYS if k.split("/")[1] == "64x64"] + [
        "golden_fringe_i400/257x193/f64", "julia_m08_0156/257x193/f32", "deep_5e5/257x193/f64",
        "c1_view_1e6/257x193/f64", "limit_2/257x193/f32"]
    try:
        _native.check(_native.load().fr_set_loop_mode(mode))
        for key in keys:
            cfg = to_fr(fr, G.oracle_config(key))
            prec = fr.Precision.F32 if key.endswith("f32") else fr.Precision.F64
            z, it = fr.escape_rows(cfg, precision=prec)
            assert np.array_equal(it, v[key + "/iters"]), (mode, key)
            if key + "/z" in v.files:
                assert same_f64(z, v[key + "/z"]), (mode, key)
            assert np.array_equal(fr.get_image(cfg, prec), v[key + "/rgb"]), (mode, key)
    finally:
        _native.load().fr_set_loop_mode(-1)


@pytest.mark.parametrize("limit", [1000.5, 3.7, 77777.123, 2.0 ** 20 + 1.0, 1e9, 1e100, 0.9])
@pytest.mark.parametrize("mode", [-1, 0, 4])
def test_limits_with_nonzero_low_mantissa_bits(fr, limit, mode):
    """limit^2 travels to the loop as a 64-bit scalar; every bit of it must arrive."""
    from fractal_renderer_amd import _native

    ocfg = O.cli_config(160, 96, iterations=150, limit=limit)
    cfg = to_fr(fr, ocfg)
    try:
        _native.check(_native.load().fr_set_loop_mode(mode))
        for op, fp in ((O.F64, fr.Precision.F64), (O.F32, fr.Precision.F32)):
            if op == O.F32 and limit > 1e30:
                continue  # (f32)limit^2 overflows to inf: nothing escapes; covered by huge_limit golden
            z, it = fr.escape_rows(cfg, precision=fp)
            wz, wit = O.escape_rows(ocfg, op)
            assert np.array_equal(it, wit), (limit, mode, op)
            assert same_f64(z, wz)
            assert np.array_equal(fr.get_image(cfg, fp), oracle_image(ocfg, op))
    finally:
        _native.load().fr_set_loop_mode(-1)


@pytest.mark.parametrize("palette", [1, 0])
@pytest.mark.parametrize("iterations", [1, 3, 50, 1024, 1279, 1280, 3000])
def test_unsmooth_palette_lookup(fr, palette, iterations):
    """smooth == false (-u): the LDS-staged palette path and the per-pixel path give the oracle's bytes."""
    from fractal_renderer_amd import _native

    ocfg = O.cli_config(200, 120, iterations=iterations, smooth=0, exposure=7.0)
    cfg = to_fr(fr, ocfg)
    try:
        _native.check(_native.load().fr_set_palette(palette))
        for op, fp in ((O.F64, fr.Precision.F64), (O.F32, fr.Precision.F32)):
            assert np.array_equal(fr.get_image(cfg, fp), oracle_image(ocfg, op, soft=False)), (palette, iterations, op)
        jcfg = O.cli_config(120, 90, O.JULIA, julia_set=(-0.8, 0.156), iterations=iterations, smooth=0, inside=0)
        assert np.array_equal(fr.get_image(to_fr(fr, jcfg)), oracle_image(jcfg, soft=False))
    finally:
        _native.load().fr_set_palette(1)


def _random_config(rng):
    algo = O.JULIA if rng.random() < 0.4 else O.MANDELBROT
    w, h = int(rng.integers(1, 200)), int(rng.integers(1, 160))
    centres = [(-0.6, 0.0), (-0.7436447860, 0.1318252536), (0.0, 0.0), (-1.25, 0.0), (0.3, 0.5), (-2.0, 0.0), (5.0, -3.0)]
    cx, cy = centres[int(rng.integers(len(centres)))]
    scale = float(10 ** rng.uniform(-1.5, 7))
    kw = dict(
        iterations=int(rng.choice([0, 1, 2, 3, 5, 17, 64, 100, 255, 300])),
        pos=(cx + float(rng.normal(0, 0.3 / scale)), cy + float(rng.normal(0, 0.3 / scale))),
        scale=(scale, scale * float(rng.choice([1.0, 1.0, 0.7, 1.9]))),
        limit=float(rng.choice([65536.0, 65536.0, 2.0, 4.0, 100.0, 1000.5, 0.5, 1e10, 3.3e7])),
        stable_limit=float(rng.choice([2.0, 2.0, 0.5, 1.5, 100.0, 0.0])),
        exposure=float(rng.choice([5.0, 2.0, 0.3, 50.0, -1.0])),
        inside=int(rng.random() < 0.7), smooth=int(rng.random() < 0.7),
        primary_color=tuple(int(v) for v in rng.integers(0, 256, 3)),
        secondary_color=tuple(int(v) for v in rng.integers(0, 256, 3)),
    )
    if algo == O.JULIA:
        kw["julia_set"] = (float(rng.uniform(-1.2, 0.6)), float(rng.uniform(-0.8, 0.8)))
        kw["pos"] = (float(rng.normal(0, 0.5)), float(rng.normal(0, 0.5)))
        kw["scale"] = (float(10 ** rng.uniform(-0.7, 2)),) * 2
    return O.cli_config(w, h, algo, **kw)


@pytest.mark.parametrize("seed", range(40))
def test_random_configs_differential(fr, seed):
    """Seeded random Configs (sizes, views, limits, flags, colours, both algorithms, both precisions,
    every kernel variant and loop form): colours, escape indices and final positions vs the oracle."""
    from fractal_renderer_amd import _native

    rng = np.random.default_rng(1000 + seed)
    lib = _native.load()
    try:
        for _ in range(4):
            ocfg = _random_config(rng)
            cfg = to_fr(fr, ocfg)
            f32 = rng.random() < 0.35
            op, fp = (O.F32, fr.Precision.F32) if f32 else (O.F64, fr.Precision.F64)
            _native.check(lib.fr_set_tile(int(rng.choice([0, 0, 1, 2, 4, 8, 9, 9, 9, 808, 1604, 3202, 6401]))))
            _native.check(lib.fr_set_loop_mode(int(rng.choice([-1, -1, 0, 2, 4]))))
            _native.check(lib.fr_set_palette(int(rng.random() < 0.7)))
            _native.check(lib.fr_set_cycle_shortcut(int(rng.random() < 0.5)))
            desc = (seed, bytes(ocfg).hex(), f32)
            z, it = fr.escape_rows(cfg, precision=fp)
            wz, wit = O.escape_rows(ocfg, op)
            assert np.array_equal(it, wit), desc
            assert same_f64(z, wz), desc
            assert np.array_equal(fr.get_image(cfg, fp), oracle_image(ocfg, op)), desc
            assert fr.count_iterations(cfg, precision=fp)[0] == O.count_iterations(ocfg, op), desc
    finally:
        lib.fr_set_tile(0)
        lib.fr_set_loop_mode(-1)
        lib.fr_set_palette(1)
        lib.fr_set_cycle_shortcut(0)


CYCLE_VIEWS = {
    "default_1024": dict(iterations=1024),
    "default_5000": dict(iterations=5000),
    "seahorse_3000": dict(iterations=3000, pos=(-0.75, 0.1), scale=(8.0, 8.0)),
    "minibrot_4096": dict(iterations=4096, pos=(-1.7548776662, 0.0), scale=(40.0, 40.0)),
    "julia_filled_2000": dict(algo=O.JULIA, julia_set=(-0.123, 0.745), iterations=2000),
    "julia_c_minus1_999": dict(algo=O.JULIA, julia_set=(-1.0, 0.0001), iterations=999),
    "odd_cap_1023_limit_100": dict(iterations=1023, limit=100.0),
}


@pytest.mark.parametrize("view", sorted(CYCLE_VIEWS))
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_exact_cycle_shortcut_is_bit_identical(fr, view, prec):
    """fr_set_cycle_shortcut(1): orbits that return bitwise to an earlier state are fast-forwarded to
    the cap.  Final positions (bit for bit), escape indices, colours and the reference-defined
    executed-iteration sum must be exactly those of the plain loop / the oracle."""
    from fractal_renderer_amd import _native

    kw = dict(CYCLE_VIEWS[view])
    algo = kw.pop("algo", O.MANDELBROT)
    ocfg = O.cli_config(448, 320, algo, **kw)
    cfg = to_fr(fr, ocfg)
    op, fp = (O.F32, fr.Precision.F32) if prec == "f32" else (O.F64, fr.Precision.F64)
    wz, wit = O.escape_rows(ocfg, op)
    want = oracle_image(ocfg, op)
    lib = _native.load()
    try:
        _native.check(lib.fr_set_cycle_shortcut(1))
        for tile in (9, 0):
            _native.check(lib.fr_set_tile(tile))
            z, it = fr.escape_rows(cfg, precision=fp)
            assert np.array_equal(it, wit), (view, prec, tile)
            assert same_f64(z, wz), (view, prec, tile)
            assert np.array_equal(fr.get_image(cfg, fp), want), (view, prec, tile)
            assert fr.count_iterations(cfg, precision=fp)[0] == O.count_iterations(ocfg, op)
    finally:
        lib.fr_set_cycle_shortcut(0)
        lib.fr_set_tile(0)


def test_palette_path_is_stable_over_a_long_call_history(fr):
    """Regression for an intermittent failure the soak (tools/soak_differential.py) found when the
    palette lived in stream-ordered (hipMallocAsync) memory: after hundreds of mixed calls a palette
    was read back as zeros.  700 mixed configurations, palette on vs off, must agree every time."""
    from fractal_renderer_amd import _native

    lib = _native.load()
    bad = []
    try:
        for seed in range(700):
            rng = np.random.default_rng(50_000 + seed)
            ocfg = _random_config(rng)
            if rng.random() < 0.3:
                ocfg.width, ocfg.height = int(rng.integers(300, 700)), int(rng.integers(200, 500))
                ocfg.iterations = int(rng.choice([500, 1024, 2000, 4100]))
            cfg = to_fr(fr, ocfg)
            fp = fr.Precision.F32 if rng.random() < 0.35 else fr.Precision.F64
            lib.fr_set_tile(int(rng.choice([0, 1, 2, 4, 8, 9, 9, 808, 1604, 3202, 6401])))
            lib.fr_set_loop_mode(int(rng.choice([-1, -1, 0, 2, 4])))
            lib.fr_set_palette(1)
            lib.fr_set_cycle_shortcut(int(rng.random() < 0.5))
            fr.escape_rows(cfg, precision=fp)
            a = fr.get_image(cfg, fp)
            fr.count_iterations(cfg, precision=fp)
            lib.fr_set_palette(0)
            if not np.array_equal(a, fr.get_image(cfg, fp)):
                bad.append(seed)
    finally:
        lib.fr_set_tile(0)
        lib.fr_set_loop_mode(-1)
        lib.fr_set_palette(1)
        lib.fr_set_cycle_shortcut(0)
    assert not bad, bad


TINY_CASES = {
    # orbits whose products pass through the subnormal range: the scaled loop must not be used
    "julia_c_zero": dict(algo=O.JULIA, julia_set=(0.0, 0.0), iterations=40),
    "julia_c_subnormal": dict(algo=O.JULIA, julia_set=(1e-310, -3e-320), iterations=40),
    "julia_c_tiny": dict(algo=O.JULIA, julia_set=(1e-200, 1e-170), iterations=60),
    "julia_c_real": dict(algo=O.JULIA, julia_set=(-1.0, 0.0), iterations=300),
    "mandelbrot_tiny_offsets": dict(iterations=80, pos=(1e-300, -1e-305)),
    "mandelbrot_zoom_at_origin": dict(iterations=60, pos=(0.0, 0.0), scale=(1e150, 1e150)),
    "mandelbrot_zoom_at_origin_deeper": dict(iterations=30, pos=(0.0, 0.0), scale=(1e300, 1e300)),
}


@pytest.mark.parametrize("name", sorted(TINY_CASES))
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_tiny_and_subnormal_orbits(fr, name, prec):
    kw = dict(TINY_CASES[name])
    algo = kw.pop("algo", O.MANDELBROT)
    ocfg = O.cli_config(96, 64, algo, **kw)
    cfg = to_fr(fr, ocfg)
    op = O.F32 if prec == "f32" else O.F64
    fp = fr.Precision.F32 if prec == "f32" else fr.Precision.F64
    z, it = fr.escape_rows(cfg, precision=fp)
    wz, wit = O.escape_rows(ocfg, op)
    assert np.array_equal(it, wit)
    assert same_f64(z, wz)
    assert np.array_equal(fr.get_image(cfg, fp), oracle_image(ocfg, op))


# ---- shapes, ranges, edge cases ----------------------------------------------------------------


def test_row_ranges_and_empty_inputs(fr):
    ocfg = G.oracle_config("mandelbrot_default/257x193/f64")
    cfg = to_fr(fr, ocfg)
    full = G.vectors()["mandelbrot_default/257x193/f64/rgb"]
    parts = [fr.get_image_rows(cfg, a, b) for a, b in ((0, 1), (1, 100), (100, 193))]
    assert np.array_equal(np.concatenate(parts), full)
    assert fr.get_image_rows(cfg, 7, 7).shape == (0, 257, 3)
    cfg.height = 0
    assert fr.get_image(cfg).shape == (0, 257, 3)
    cfg.height, cfg.width = 5, 0
    assert fr.get_image(cfg).shape == (5, 0, 3)
    with pytest.raises(fr.FractalHipError):
        fr.get_image_rows(cfg, 3, 9)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (63, 65), (1025, 7), (17, 1031)])
def test_ragged_sizes(fr, w, h):
    ocfg = O.cli_config(w, h, iterations=120)
    cfg = to_fr(fr, ocfg)
    assert np.array_equal(fr.get_image(cfg), oracle_image(ocfg))
    z, it = fr.escape_rows(cfg)
    wz, wit = O.escape_rows(ocfg)
    assert np.array_equal(it, wit) and same_f64(z, wz)


@pytest.mark.parametrize("world,block_rows", [(2, 64), (3, 16), (8, 8), (4, 1)])
def test_logical_block_cyclic_partitions_on_one_device(fr, world, block_rows):
    """The multi-GPU partition rendered as `world` logical shares on ONE device and reassembled
    must be byte-identical to the single render."""
    import torch

    from fractal_renderer_amd import _native
    from fractal_renderer_amd import partition as P

    ocfg = G.oracle_config("golden_fringe_i400/257x193/f64")
    cfg = to_fr(fr, ocfg)
    want = G.vectors()["golden_fringe_i400/257x193/f64/rgb"]
    rb = 3 * cfg.width
    max_rows = P.local_rows(cfg.height, block_rows, 0, world)
    gathered = np.zeros((world, max_rows * rb), dtype=np.uint8)
    for r in range(world):
        rows = C.c_uint64(0)
        _native.check(_native.load().fr_render_block_cyclic_rgb8(
            C.byref(cfg), 0, block_rows, r, world, gathered[r].ctypes.data, gathered[r].nbytes, C.byref(rows)))
        assert rows.value == P.local_rows(cfg.height, block_rows, r, world)
    img = P.assemble(torch.from_numpy(gathered), cfg.height, rb, block_rows, world).numpy()
    assert np.array_equal(img.reshape(cfg.height, cfg.width, 3), want)


@pytest.mark.parametrize("w,h", [(3, 300001), (500003, 2), (8, 262145 + 64)])
def test_extreme_aspect_ratios(fr, w, h):
    """More than 32768 row tiles (3-D grid path) and very wide images; every pixel against the oracle."""
    ocfg = O.cli_config(w, h, iterations=40, scale=(0.4 * w / max(h, 1), 0.4) if w > h else (0.4, 0.4))
    cfg = to_fr(fr, ocfg)
    assert np.array_equal(fr.get_image(cfg), oracle_image(ocfg))
    assert fr.count_iterations(cfg)[0] == O.count_iterations(ocfg)


def test_iteration_cap_extremes(fr):
    """iterations = u32::MAX with a limit every orbit exceeds at once, and iterations not a multiple
    of the unroll factors."""
    for it in (4294967295, 4294967294, 7, 6, 5):
        ocfg = O.cli_config(40, 24, iterations=it, limit=1e-3, stable_limit=0.0)
        cfg = to_fr(fr, ocfg)
        z, iters = fr.escape_rows(cfg)
        wz, wit = O.escape_rows(ocfg)
        assert np.array_equal(iters, wit) and same_f64(z, wz), it
        assert np.array_equal(fr.get_image(cfg), oracle_image(ocfg)), it


@pytest.mark.parametrize("world,block_rows,h", [(1, 8, 193), (2, 16, 193), (3, 8, 200), (8, 8, 193), (4, 64, 1000)])
def test_chunked_block_cyclic_rendering_packed_and_in_place(fr, world, block_rows, h):
    """What each rank of the pipelined multi-GPU gather launches (partition.DistributedRenderer): its
    blocks chunk by chunk, packed (ranks > 0) or straight into the whole image (rank 0) — all logical
    ranks on one device here; the reassembled image must equal the single render."""
    import torch

    from fractal_renderer_amd import partition as P

    ocfg = O.cli_config(257, h, iterations=120)
    cfg = to_fr(fr, ocfg)
    want = fr.get_image(cfg)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    rb = 3 * cfg.width
    nblocks = P.num_blocks(h, block_rows)
    nb_max = (nblocks + world - 1) // world
    image = torch.zeros(h * rb, dtype=torch.uint8, device=dev)
    for r in range(world):
        for (j0, j1) in P.chunk_schedule(nb_max):
            mine = [j * world + r for j in range(j0, j1) if j * world + r < nblocks]
            if not mine:
                continue
            if r == 0:
                P.render_chunk_hip(cfg, 0, block_rows, mine[0], world, len(mine), True, image, stream.cuda_stream)
            else:
                rows = sum(P.block_range(h, block_rows, b)[1] - P.block_range(h, block_rows, b)[0] for b in mine)
                chunk = torch.empty(rows * rb, dtype=torch.uint8, device=dev)
                got_rows = P.render_chunk_hip(cfg, 0, block_rows, mine[0], world, len(mine), False, chunk, stream.cuda_stream)
                assert got_rows == rows
                off = 0
                for b in mine:  # what the P2P receive does on rank 0
                    y0, y1 = P.block_range(h, block_rows, b)
                    image[y0 * rb : y1 * rb] = chunk[off : off + (y1 - y0) * rb]
                    off += (y1 - y0) * rb
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy().reshape(h, cfg.width, 3), want)
    # and the renderer object itself, block by block on one rank
    renderer = P.DistributedRenderer(cfg, 0, block_rows, device=dev, force_blocks=True)
    for _ in range(2):
        img = renderer.render()
        torch.cuda.synchronize()
        assert np.array_equal(img.cpu().numpy(), want)


@pytest.mark.parametrize("key", ["mandelbrot_default/257x193/f64", "julia_m08_0156/257x193/f32", "stable_limit_half/64x64/f64",
                                 "huge_limit_nan_orbits/64x64/f64", "iterations_0/64x64/f64"])
def test_recolour_without_reiterating(fr, key):
    """fr_colour_rgb8 over stored (z, iters) reproduces get_image, and with changed colour-map inputs
    (exposure, smooth, inside, colours, stable_limit) the image of the changed Config — the GUI's
    sliders (src/gui.rs:183-203) never need a second orbit pass."""
    ocfg = G.oracle_config(key)
    prec = fr.Precision.F32 if key.endswith("f32") else fr.Precision.F64
    op = O.F32 if key.endswith("f32") else O.F64
    cfg = to_fr(fr, ocfg)
    z, it = fr.escape_rows(cfg, precision=prec)
    assert np.array_equal(fr.colour_image(cfg, z, it), G.vectors()[key + "/rgb"])
    for change in (dict(exposure=17.5), dict(smooth=0), dict(inside=0), dict(stable_limit=0.75),
                   dict(primary_color=(9, 200, 77), secondary_color=(255, 1, 128), exposure=0.4)):
        ocfg2 = O.Config.from_buffer_copy(bytes(ocfg))
        O.apply_overrides(ocfg2, change)
        assert np.array_equal(fr.colour_image(to_fr(fr, ocfg2), z, it), oracle_image(ocfg2, op)), (key, change)


DEGENERATE = {
    "limit_nan": dict(limit=float("nan")), "limit_inf": dict(limit=float("inf")), "limit_negative": dict(limit=-3.0),
    "limit_zero": dict(limit=0.0), "limit_1e300": dict(limit=1e300),
    "stable_nan": dict(stable_limit=float("nan")), "stable_inf": dict(stable_limit=float("inf")),
    "stable_negative": dict(stable_limit=-1.0),
    "exposure_nan": dict(exposure=float("nan")), "exposure_inf": dict(exposure=float("inf")), "exposure_zero": dict(exposure=0.0),
    "scale_zero": dict(scale=(0.0, 0.4)), "scale_negative": dict(scale=(-0.4, -0.4)), "scale_nan": dict(scale=(float("nan"), 0.4)),
    "scale_inf": dict(scale=(float("inf"), float("inf"))), "scale_tiny": dict(scale=(1e-300, 1e-300)),
    "pos_inf": dict(pos=(float("inf"), 0.0)), "pos_nan": dict(pos=(0.0, float("nan"))), "pos_huge": dict(pos=(1e200, -1e200)),
    "julia_nan": dict(algo=O.JULIA, julia_set=(float("nan"), 0.1)), "julia_inf": dict(algo=O.JULIA, julia_set=(float("inf"), 0.0)),
    "julia_huge": dict(algo=O.JULIA, julia_set=(1e300, -1e300)),
}


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_nonfinite_and_degenerate_parameters(fr, name):
    """NaN / infinite / zero / negative parameters: whatever the reference's arithmetic does with them
    (NaN never compares greater, `as u8` maps NaN to 0, ...) the device must do too, in every loop form."""
    from fractal_renderer_amd import _native

    kw = dict(DEGENERATE[name])
    algo = kw.pop("algo", O.MANDELBROT)
    ocfg = O.cli_config(72, 40, algo, iterations=30, **kw)
    cfg = to_fr(fr, ocfg)
    lib = _native.load()
    try:
        for mode in (-1, 0, 4):
            lib.fr_set_loop_mode(mode)
            for op, fp in ((O.F64, fr.Precision.F64), (O.F32, fr.Precision.F32)):
                z, it = fr.escape_rows(cfg, precision=fp)
                wz, wit = O.escape_rows(ocfg, op)
                assert np.array_equal(it, wit), (name, mode, op)
                assert same_f64(z, wz), (name, mode, op)
                assert np.array_equal(fr.get_image(cfg, fp), oracle_image(ocfg, op)), (name, mode, op)
    finally:
        lib.fr_set_loop_mode(-1)


@pytest.mark.parametrize("key", ["mandelbrot_default/257x193/f64", "julia_m08_0156/257x193/f32", "unsmooth/257x193/f64"])
@pytest.mark.parametrize("tile", [0, 9, 808])
def test_rgba8_output(fr, key, tile):
    """RGBA8 variant (the GUI's upload format, src/gui.rs:71-72): same r,g,b as get_image, alpha 255."""
    from fractal_renderer_amd import _native

    cfg = to_fr(fr, G.oracle_config(key))
    prec = fr.Precision.F32 if key.endswith("f32") else fr.Precision.F64
    try:
        _native.check(_native.load().fr_set_tile(tile))
        rgba = fr.get_image_rgba(cfg, prec)
    finally:
        _native.load().fr_set_tile(0)
    assert np.array_equal(rgba[..., :3], G.vectors()[key + "/rgb"])
    assert (rgba[..., 3] == 255).all()


def test_get_recursive_pixel_outside_the_image(fr):
    # get_recursive_pixel does not clamp x, y to width/height (calc/src/lib.rs:199-207)
    ocfg = O.cli_config(64, 48, iterations=80)
    cfg = to_fr(fr, ocfg)
    O.set_log2_mode(O.LOG2_SOFT)
    try:
        for (x, y) in [(0, 0), (63, 47), (64, 48), (1000, 3), (5, 4000), (4294967295, 4294967295)]:
            assert tuple(fr.get_recursive_pixel(cfg, x, y)) == O.get_recursive_pixel(ocfg, x, y), (x, y)
    finally:
        O.set_log2_mode(O.LOG2_LIBM)


BASELINE_VIEWS = {
    "C2_default": dict(iterations=1024),
    "C1_C3_zoom_1e6": dict(iterations=1024, scale=(1e6, 1e6), pos=(-0.7436447860, 0.1318252536)),
    "C4_julia": dict(algo=O.JULIA, julia_set=(-0.8, 0.156), iterations=4096),
}


@pytest.mark.parametrize("view", sorted(BASELINE_VIEWS))
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_baseline_views_1024_crop(fr, view, prec):
    """1024x1024 renders of each BASELINE.md view, all bytes against the oracle in both log2 modes."""
    kw = dict(BASELINE_VIEWS[view])
    algo = kw.pop("algo", O.MANDELBROT)
    ocfg = O.cli_config(1024, 1024, algo, **kw)
    cfg = to_fr(fr, ocfg)
    op = O.F32 if prec == "f32" else O.F64
    fp = fr.Precision.F32 if prec == "f32" else fr.Precision.F64
    img = fr.get_image(cfg, fp)
    assert np.array_equal(img, oracle_image(ocfg, op, soft=True))
    assert np.array_equal(img, oracle_image(ocfg, op, soft=False))
    assert fr.count_iterations(cfg, precision=fp)[0] == O.count_iterations(ocfg, op)


def test_concurrent_callers(fr):
    """src/gui.rs:56-60 + 322-326: the render thread and the screenshot thread call get_image
    at the same time with different sizes."""
    import threading

    ocfgs = [O.cli_config(375, 250, iterations=200), O.cli_config(750, 500, iterations=200)]
    want = [oracle_image(c) for c in ocfgs]
    errs = []

    def work(i):
        try:
            cfg = to_fr(fr, ocfgs[i])
            for _ in range(5):
                if not np.array_equal(fr.get_image(cfg), want[i]):
                    errs.append("mismatch in thread %d" % i)
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    ts = [threading.Thread(target=work, args=(i,)) for i in (0, 1, 0, 1)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs


# ---- BASELINE.json full sizes: size-independent properties + strided comparison ---------------


def oracle_sample_both_modes(ocfg, step, prec=O.F64):
    """The oracle on every `step`-th pixel in x and y with the platform libm's log2 — what the reference's
    f64::log2 calls (calc/src/lib.rs:222-223), the mode the device is compared with — after checking that the
    software log2 the kernels carry gives the very same bytes and iteration sum on that sample."""
    O.set_log2_mode(O.LOG2_SOFT)
    try:
        soft = O.sample_image(ocfg, step, step, prec)
    finally:
        O.set_log2_mode(O.LOG2_LIBM)
    libm = O.sample_image(ocfg, step, step, prec)
    assert soft[:2] == libm[:2] and np.array_equal(soft[2], libm[2]), "libm and software log2 differ in output bytes"
    return libm


def test_full_size_c2_sampled_against_oracle(fr):
    """C2 (16384^2, 1024 iterations): every 16th pixel in x and y, colours and executed-iteration
    sum, against the oracle; plus row-split invariance of the full image.  (The WHOLE C2 image is compared with the CPU
    oracle, byte for byte, by bench.py's cpu_baseline leg in every --full run: 8 s of CPU there, not repeated here.)"""
    ocfg = O.cli_config(16384, 16384, iterations=1024)
    cfg = to_fr(fr, ocfg)
    img = fr.get_image(cfg)
    total, npx, want = oracle_sample_both_modes(ocfg, 16)
    assert np.array_equal(img[::16, ::16], want)
    assert fr.count_iterations(cfg, sx=16, sy=16) == (total, npx)
    # vertical symmetry of the default view about row 8192 (im(y) = -im(16384 - y) exactly and the
    # iteration is conjugation-symmetric): rows 1..8191 mirror rows 16383..8193
    assert np.array_equal(img[1:8192], img[16383:8192:-1])
    # any row band rendered on its own equals the same rows of the full render
    band = fr.get_image_rows(cfg, 8000, 8192)
    assert np.array_equal(band, img[8000:8192])


@pytest.mark.parametrize("prec_name", ["f32", "f64"])
def test_full_size_c4_julia_whole_image_against_oracle(fr, prec_name):
    """C4 (Julia c = -0.8+0.156i, 16384^2, 4096 iterations) through the default dispatch (two passes at this size), f32
    and f64: ALL 805 306 368 bytes and the exact executed-iteration sum against the oracle in libm mode (the whole image
    is 1.2e10 pixel-iterations — seconds of CPU — so nothing is sampled: VERDICT r02 #3), after checking on every 16th
    pixel that the software log2 the kernels carry and the platform libm's give the same bytes."""
    ocfg = O.cli_config(16384, 16384, O.JULIA, julia_set=(-0.8, 0.156), iterations=4096)
    cfg = to_fr(fr, ocfg)
    oprec, prec = (O.F32, fr.Precision.F32) if prec_name == "f32" else (O.F64, fr.Precision.F64)
    oracle_sample_both_modes(ocfg, 16, oprec)  # soft == libm on a sample; the full comparison below is in libm mode
    img = fr.get_image(cfg, prec)
    total, npx, want = O.sample_image(ocfg, 1, 1, oprec)
    assert npx == 16384 * 16384 and np.array_equal(img, want)
    del want
    assert fr.count_iterations(cfg, precision=prec) == (total, npx)
    # the Julia set of a c is symmetric under z -> -z: the image equals itself rotated by 180 degrees
    # about the centre pixel grid point (x, y) -> (W - x, H - y) for x, y >= 1
    assert np.array_equal(img[1:, 1:], img[:0:-1, :0:-1])


def test_full_size_c3_deep_zoom_sampled_and_shortcut(fr):
    """C3 (16384^2, zoom 10^6, 65536 iterations, f64): every 64th pixel against the oracle — SAMPLED because the whole
    image is 7e12 pixel-iterations, ~14 minutes of this box's 16 host threads — and the exact-periodicity shortcut must
    reproduce the plain render byte for byte at full size."""
    from fractal_renderer_amd import _native

    ocfg = O.cli_config(16384, 16384, iterations=65536, scale=(1e6, 1e6), pos=(-0.7436447860, 0.1318252536))
    cfg = to_fr(fr, ocfg)
    img = fr.get_image(cfg)
    total, npx, want = oracle_sample_both_modes(ocfg, 64)
    assert np.array_equal(img[::64, ::64], want)
    assert fr.count_iterations(cfg, sx=64, sy=64) == (total, npx)
    lib = _native.load()
    try:
        _native.check(lib.fr_set_cycle_shortcut(1))
        assert np.array_equal(fr.get_image(cfg), img)
    finally:
        lib.fr_set_cycle_shortcut(0)


def test_full_size_c5_65536_squared_on_one_device(fr):
    """BASELINE C5's image (65536^2 = 2^32 pixels, 12.9 GB) rendered whole on ONE device: every
    index is past 32 bits.  Every 64th pixel in x and y against the oracle (SAMPLED: the whole image is 1.1e12
    pixel-iterations, ~2 minutes of CPU and 12.9 GB twice over), the exact iteration sum on that sample, and the mirror
    symmetry of the default view."""
    ocfg = O.cli_config(65536, 65536, iterations=1024)
    cfg = to_fr(fr, ocfg)
    img = fr.get_image(cfg)
    total, npx, want = oracle_sample_both_modes(ocfg, 64)
    assert np.array_equal(img[::64, ::64], want)
    assert fr.count_iterations(cfg, sx=64, sy=64) == (total, npx)
    assert np.array_equal(img[1:4096], img[65535:61440:-1])          # top rows mirror the bottom rows
    assert np.array_equal(img[32768 - 2048:32768], img[32768 + 2048:32768:-1])
    # the last rows rendered on their own (byte offsets > 2^33 in the full image) equal the full render
    band = fr.get_image_rows(cfg, 65536 - 24, 65536)
    assert np.array_equal(band, img[65536 - 24:])
    del img


def test_device_pointer_api_from_concurrent_threads_and_streams(fr):
    """fr_render_rows_rgb8_device is lock-free: several host threads, each on its own HIP stream
    (torch streams used only as plumbing), render different configs at once — smooth and palette
    paths mixed — into their own device buffers; every result must equal the serial render."""
    import threading

    import torch

    from fractal_renderer_amd import partition as P

    ocfgs = [O.cli_config(320, 200, iterations=300), O.cli_config(200, 320, iterations=150, smooth=0),
             O.cli_config(256, 256, O.JULIA, julia_set=(-0.8, 0.156), iterations=400),
             O.cli_config(400, 120, iterations=90, smooth=0, inside=0)]
    cfgs = [to_fr(fr, c) for c in ocfgs]
    want = [fr.get_image(c) for c in cfgs]
    errs = []

    def work(i):
        try:
            cfg = cfgs[i]
            dev = torch.device("cuda", 0)
            stream = torch.cuda.Stream(dev)
            with torch.cuda.stream(stream):
                out = torch.empty(cfg.height * cfg.width * 3, dtype=torch.uint8, device=dev)
            for _ in range(25):
                with torch.cuda.stream(stream):
                    out.zero_()  # same stream as the render: ordered before it
                    P.render_rows_hip(cfg, 0, 0, cfg.height, out, stream.cuda_stream)
                stream.synchronize()
                got = out.cpu().numpy().reshape(cfg.height, cfg.width, 3)
                if not np.array_equal(got, want[i]):
                    errs.append("thread %d: mismatch" % i)
                    return
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(cfgs))]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errs, errs


def test_bench_smoke_small():
    """bench.py end to end on a small image: torch-first import order, HIP-event timing, roofline and
    cpu_baseline objects, and its own GPU-vs-CPU byte comparison."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--size", "2048", "--steps", "2", "--warmup", "1", "--full"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["metric"] == "pixel_iterations_per_sec" and d["n_gpus"] == 1 and d["value"] > 1e9
    assert d["roofline"]["achieved"] > 0 and 0 < d["roofline"]["frac"] < 1
    assert d["cpu_baseline"]["gpu_bytes_identical_on_sample"] is True
    assert d["cpu_baseline"]["gpu_iteration_sum_identical_on_sample"] is True
    # the box's own reference: the same workload without the speculative blocks, same bytes
    ref = d["roofline"]["same_box_without_speculative_blocks"]
    assert ref["byte_sums_identical"] is True and ref["kernel_ms_avg"] > 0 and -0.5 < ref["speculative_blocks_gain"] < 0.5


def test_bench_plain_run_and_dump_outputs(fr, tmp_path):
    """A plain bench.py run times exactly --steps steps, prints the headline without the --full legs, and
    --dump-outputs writes the image of the last timed step: whole for a small image, a fixed sample of pixels for a
    large one — both equal to the library's own render of the same Config."""
    import json
    import os
    import subprocess
    import sys

    import bench

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for edge in (2048, 4608):
        out_dir = tmp_path / str(edge)
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--size", str(edge), "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert d["metric"] == "pixel_iterations_per_sec" and d["unit"] == "pixel-iterations/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f64" and d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 1e9
        assert not {"cpu_baseline", "end_to_end", "exact_cycle_shortcut", "other_configs", "gui_latency"} & set(d)
        assert "same_box_without_speculative_blocks" not in d["roofline"]
        want = fr.get_image(bench.make_config(fr, "default", edge, 1024))
        files = sorted(os.listdir(out_dir))
        assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 * 2**20
        if edge == 2048:
            assert files == ["image.npy"]
            got = np.load(out_dir / "image.npy")
            assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
        else:
            assert files == ["image_sample.npy", "image_sample_index.npy"]
            got, idx = np.load(out_dir / "image_sample.npy"), np.load(out_dir / "image_sample_index.npy")
            assert got.dtype == np.float32 and idx.dtype == np.float64 and len(got) == len(idx) == bench.DUMP_SAMPLE_PIXELS
            assert np.array_equal(got, want.reshape(-1, 3)[idx.astype(np.int64)].astype(np.float32))


def test_rccl_p2p_call_pattern_self_send():
    """The torch.distributed (RCCL) call pattern of the multi-GPU gather — P2POp batches on a side
    stream behind an event of the compute stream — exercised on one GPU by sending to self
    (tools/nccl_p2p_selftest.py).  A real N > 1 run is the driver's; this proves the plumbing."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "nccl_p2p_selftest.py")], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0 and "nccl p2p self-test: ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
