"""The edge views of FR_PRECISION_DD and FR_PRECISION_PT (include/fractal_hip.h, fr_precision), shared by the GPU tests
(tests/test_gpu_deep_edges.py: the kernels against the host models) and the CPU test of the models against the header
text (tests/test_deep_definition_cpu.py).

Each view is Config::new(algo) at 96 x 64 with a few fields changed, plus the pos_lo values it is rendered with: (0, 0)
always, and a normalised nonzero low part wherever the centre allows one (a zero component of pos takes only +-0).
`flat` views have one escape index over the whole image (every pixel runs to the cap, or escapes at the same step): they
are compared on the z bits, and the "resolved" assertion of the other views does not apply to them."""
import math

MANDELBROT, JULIA = 0, 2
W, H = 96, 64


def lo_for(pos, frac=0.2113):
    """a normalised low part of `pos`, +0 on an axis where pos is 0: |lo| < ulp(pos)/4, so pos + lo rounds to pos even
    where pos is a power of two and lo points into the binade below, whose ulp is half as large"""
    return tuple(math.ulp(p) * frac * (1 if k == 0 else -1) if p != 0.0 else 0.0 for k, p in enumerate(pos))


DEEP = dict(pos=(0.0, 1.0), scale=(1e18, 1e18), julia_set=(0.0, 1.0), iterations=3000)

Z = (0.0, 0.0)
NZ = (-0.0, -0.0)
LO_I = (0.0, 2.0 ** -60)  # a normalised low part of a centre (0, 1)

# name -> (algo, fields, [(pos_lo, flat), ...]); pos_lo "lo" = lo_for(pos)
VIEWS = {
    # ---- subnormal and tiny values ----
    "origin_1e150": (MANDELBROT, dict(iterations=60, scale=(1e150, 1e150)), [(Z, True), (NZ, True)]),
    "origin_1e300": (MANDELBROT, dict(iterations=60, scale=(1e300, 1e300)), [(Z, True)]),
    "origin_1e308": (MANDELBROT, dict(iterations=60, scale=(1e308, 1e308)), [(Z, True)]),  # the offsets are subnormal
    "julia_c_zero": (JULIA, dict(iterations=40), [(Z, False)]),
    "julia_c_subnormal": (JULIA, dict(iterations=40, julia_set=(1e-310, -3e-320)), [(Z, False)]),
    "julia_c_tiny": (JULIA, dict(iterations=60, julia_set=(1e-200, 1e-170)), [(Z, False)]),
    "julia_c_real": (JULIA, dict(iterations=300, julia_set=(-1.0, 0.0)), [(Z, False)]),
    "tiny_centre": (MANDELBROT, dict(iterations=80, pos=(1e-300, -1e-305)), [(Z, False), ((2.0 ** -1060, -2.0 ** -1070), False)]),
    "centre_i_1e300": (MANDELBROT, dict(iterations=200, pos=(0.0, 1.0), scale=(1e300, 1e300)), [(Z, True), (LO_I, True)]),
    # ---- domain bounds, accepted side ----
    "limit_2p500": (MANDELBROT, dict(iterations=100, limit=2.0 ** 500), [(Z, False), (NZ, False)]),
    "limit_2p500_julia": (JULIA, dict(iterations=100, limit=2.0 ** 500, julia_set=(-0.8, 0.156)), [(Z, False)]),
    "pos_re_2p64": (MANDELBROT, dict(iterations=50, limit=2.0 ** 500, pos=(-2.0 ** 64, 0.5)), [(Z, True), ("lo", True)]),
    "julia_re_2p64": (JULIA, dict(iterations=50, limit=2.0 ** 500, julia_set=(2.0 ** 64, 0.0)), [(Z, True)]),
    "scale_2m64": (MANDELBROT, dict(iterations=50, pos=(-0.75, 0.125), scale=(2.0 ** -64, -2.0 ** -64)),
                   [(Z, False), ("lo", False)]),
    "limit_1e-300": (MANDELBROT, dict(iterations=70, limit=1e-300), [(Z, False)]),
    "limit_1e-300_deep": (MANDELBROT, dict(DEEP, limit=1e-300, iterations=70), [(Z, True), (LO_I, True)]),
    "lo_bounds_deep": (MANDELBROT, dict(DEEP), [((0.0, 2.0 ** -53), False), ((0.0, -2.0 ** -54), True), (NZ, False)]),
    "lo_bounds_deep_julia": (JULIA, dict(DEEP), [((0.0, 2.0 ** -53), True), ((0.0, -2.0 ** -54), True), (NZ, False)]),
    "colour_extremes_a": (MANDELBROT, dict(iterations=200, pos=(-0.6, 0.0), stable_limit=0.0, exposure=1e300,
                                           color_weight=-1e300), [(Z, False)]),
    "colour_extremes_b": (MANDELBROT, dict(iterations=200, pos=(-0.6, 0.0), stable_limit=-1.0, exposure=-1e300,
                                           color_weight=1e300, smooth=0), [(Z, False)]),
    # ---- geometry: unequal and negative scales, a portrait image ----
    "deep_scale_a": (MANDELBROT, dict(DEEP, scale=(1e18, -3e17)), [(Z, False), (LO_I, False)]),
    "deep_scale_b": (MANDELBROT, dict(DEEP, scale=(2e17, 1e18)), [(Z, False), (LO_I, False)]),
    "deep_julia_scale_a": (JULIA, dict(DEEP, scale=(1e18, -3e17)), [(Z, False), (LO_I, False)]),
    "deep_julia_scale_b": (JULIA, dict(DEEP, scale=(2e17, 1e18)), [(Z, False), (LO_I, False)]),
    "deep_portrait": (MANDELBROT, dict(DEEP, width=97, height=203), [(Z, False), (LO_I, False)]),
}


def make(cfg, name):
    """fill `cfg` (Config::new of either binding, changed in place) with view `name`; returns its pos_lo values"""
    algo, fields, _ = VIEWS[name]
    cfg.algo = algo
    cfg.width, cfg.height = W, H
    for k, v in fields.items():
        if k in ("pos", "scale", "julia_set"):
            getattr(cfg, k).re, getattr(cfg, k).im = v
        else:
            setattr(cfg, k, v)
    return pos_los(name)


def pos_los(name, flat=None):
    """the pos_lo values of view `name` (only the flat or only the resolved ones if `flat` is given)"""
    _, fields, los = VIEWS[name]
    return [lo_for(fields.get("pos", Z)) if lo == "lo" else lo for lo, f in los if flat is None or f == flat]


def cases(flat):
    """(view name, pos_lo) pairs with flat or with resolved escape indices"""
    return [(n, lo) for n in VIEWS for lo in pos_los(n, flat)]


def case_id(case):
    name, lo = case
    if all(v == 0.0 and math.copysign(1.0, v) > 0 for v in lo):
        return name
    return "%s-lo(%s,%s)" % (name, float(lo[0]).hex(), float(lo[1]).hex())
