"""Generated and edge records for the calls that sit on the FR_PRECISION_F64, FR_PRECISION_F32 and FR_PRECISION_DD roads — the kept
view (fr_escape_rows_device, fr_escape_extend_device, fr_colour_rows_device, fr_colour_rows_ss_device, fr_view_stats_device with
fr_stats_percentile and fr_auto_exposure) and the F64 DE family — shared by tests/test_shallow_random_cpu.py (the host models
alone: is the set worth running) and tests/test_gpu_shallow_random.py (the kernels against the models on the same records).  No
device and no library: numpy's seeded generator, the oracle's Config, and tests/de_model.py for a record's thickness.

A record is an fr_config image (the oracle's Config, 104 bytes, at the chain's last cap) and what the chains of the GPU file need:
  precision   F64, F32 or DD;  `de`: the record also goes through the F64 DE chain (F64 and limit <= 2^20, DE's domain);
  chain       caps N0 < N1 < ... = cfg.iterations, 2 to 4 links;  piece: the link that first runs on the rows `split` = [y0, y1);
  s           the supersample, 1 .. 8, lowered until s * s * width * height * max(iterations, 1) <= 2^26 (DD: 2^22) so that a
              model of cfg_s takes a second or two at the most;
  thickness   DE records: the median finite positive D of the escaped pixels at the last cap, clamped to 2^20 / s; 1.5 where no
              pixel has one; None without DE;
  tile, loop_mode   the selectors of tests/test_gpu_parity.py's differential (they select nothing for DD);  host: the host forms
              are compared as well (one record in four);  pos_lo: DD's low parts.
draw(rng) draws the F64 and F32 records:
  algo      Mandelbrot 0.5, Julia 0.44, algo 1 (no orbits: zeros and black) 0.06;
  centre    Mandelbrot: a boundary point of MANDELBROT_CENTRES; Julia: the repelling fixed point (1 +- sqrt(1 - 4c)) / 2 of larger
            modulus of a constant of JULIA_CONSTANTS, whose filled Julia sets keep capped pixels beside escaping ones at every
            depth; both moved by up to 0.35 of the view's height on either axis;
  scale     f 2^e with 2^e the binade of 10^U(-0.5, 9) (F32: 10^U(-0.5, 4), where an f32 start still tells pixels apart) and f in
            [0.5, 1) with its last mantissa bit set; the other axis is the first times one of RATIOS; both negated in one draw of
            four; either axis first;
  caps      CAPS;  limit: LIMITS, and in one draw of eight PLAIN_LIMITS (no DE then);  stable_limit, exposure, inside, smooth and
            the two colours as tests/test_gpu_parity.py draws them;
  size      1 .. 79 by 1 .. 59, one draw in ten from FIXED_SIZES: the smallest shapes that cross the 16 x 16 workgroups of 8 x 8
            waves of the DE kernels and the 64-pixel tiles of the filter kernels; records(seed) also hands the first record of every
            seed and the third of every even seed the next size of that list in turn.
dd_record(rng) takes a view of tests/test_gpu_deep_edges.py::random_config — its algo, centre with pos_lo, scales, limit, look and
Julia constant — and gives it a size, a cap chain, a split and a supersample of this file's; every such view lies inside DD's
domain, which dd_domain restates and the CPU test asserts.  EDGES are hand-placed records on the borders of the domains."""
import cmath
import ctypes as C
import functools
import math

import numpy as np

import de_model as D
import oracle_lib as O

F64, F32, DD = 0, 1, 2
SEEDS = range(30)
BASE_SEED = 11500
DD_BASE_SEED = 11900
PER_SEED = 4  # F64 / F32 records of a seed; one DD record more

MANDELBROT_CENTRES = ((0.0, 1.0), (-2.0, 0.0), (-0.75, 0.1), (-0.7436447860, 0.1318252536), (-1.401155189, 0.0), (0.25, 0.0),
                      (-1.7548776662, 0.0))
JULIA_CONSTANTS = ((-0.123, 0.745), (-1.0, 0.0), (-0.8, 0.156), (0.25, 0.0), (0.0, 0.0), (-0.4, 0.6))
RATIOS = (1.0, 1.0, 0.7, 1.9, -1.0)
CAPS = (0, 1, 2, 17, 64, 100, 255, 300, 1000, 2000)
LIMITS = (65536.0, 65536.0, 2.0, 4.0, 0.5, 100.0, 1000.5, 2.0 ** 20)
PLAIN_LIMITS = (1e10, 3.3e7)
STABLE_LIMITS = (2.0, 2.0, 0.5, 1.5, 100.0, 0.0)
EXPOSURES = (5.0, 2.0, 0.3, 50.0, -1.0)
FIXED_SIZES = ((1, 1), (1, 37), (37, 1), (16, 17), (17, 16), (33, 2), (65, 5))
TILES = (0, 0, 1, 2, 4, 8, 9, 9, 9, 808, 1604, 3202, 6401)
LOOP_MODES = (-1, -1, 0, 2, 4)
DE_MAX = 2.0 ** 20  # DE's largest limit and largest thickness * s
WORK = 2 ** 26  # samples * cap of cfg_s on the F64 / F32 roads
WORK_DD = 2 ** 22  # and in DD, whose host model takes twenty times as long a step


class Record:
    def __init__(self, label, cfg, precision, chain, piece, split, s, thickness=None, de=None, tile=0, loop_mode=-1, host=False,
                 pos_lo=None):
        assert C.sizeof(cfg) == 104 and len(chain) >= 2 and all(a < b for a, b in zip(chain, chain[1:]))
        assert 0 <= piece < len(chain) - 1 and 0 <= split[0] <= split[1] <= cfg.height and 1 <= s <= 8
        self.label, self.precision, self.chain, self.piece, self.split, self.s = label, precision, tuple(chain), piece, tuple(split), s
        self.cfg = O.Config.from_buffer_copy(bytes(cfg))
        self.cfg.iterations = self.chain[-1]
        self.de = (precision == F64 and self.cfg.limit <= DE_MAX) if de is None else de
        self.tile, self.loop_mode, self.host, self.pos_lo = tile, loop_mode, host, pos_lo
        assert (pos_lo is not None) == (precision == DD) and not (self.de and precision != F64)
        self.thickness = thickness
        if self.de and thickness is None:
            self.thickness = median_thickness(self.cfg, s)
        assert not self.de or 0.0 <= self.thickness * s <= DE_MAX

    @property
    def shape(self):
        return (self.cfg.height, self.cfg.width)

    @property
    def z_width(self):
        return 4 if self.precision == DD else 2

    def cfg_at(self, cap, s=1, config=None):
        """a copy of the config at a cap — of cfg_s, s times as wide and as high, for s > 1 — as an oracle Config or as `config`"""
        cfg = (config or O.Config).from_buffer_copy(bytes(self.cfg))
        cfg.iterations = cap
        cfg.width, cfg.height = self.cfg.width * s, self.cfg.height * s
        return cfg

    def links(self):
        return list(zip(self.chain, self.chain[1:]))

    def describe(self):
        """a Python expression that rebuilds the record from the config's bytes and its extras"""
        lo = "None" if self.pos_lo is None else "(float.fromhex(%r), float.fromhex(%r))" % tuple(float(v).hex() for v in self.pos_lo)
        t = "None" if self.thickness is None else "float.fromhex(%r)" % float(self.thickness).hex()
        return ("%s: shallow_random_views.replay(%r, precision=%d, chain=%r, piece=%d, split=%r, s=%d, thickness=%s, de=%r, tile=%d, "
                "loop_mode=%d, host=%r, pos_lo=%s)" % (self.label, bytes(self.cfg).hex(), self.precision, self.chain, self.piece, self.split,
                                                     self.s, t, self.de, self.tile, self.loop_mode, self.host, lo))


def replay(image, **extras):
    """the record of a failure message"""
    return Record("replayed", O.Config.from_buffer_copy(bytes.fromhex(image)), **extras)


def median_thickness(cfg, s):
    """the median finite positive D of the escaped pixels (tests/de_model.py at cfg's cap), clamped to 2^20 / s; 1.5 without one"""
    z, it, der = D.f64_rows(cfg)
    dist = D.distance(cfg, z, it, der)[it < cfg.iterations]
    dist = dist[np.isfinite(dist) & (dist > 0.0)]
    t = float(np.median(dist)) if dist.size else 1.5
    return min(t, DE_MAX / s)


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _mantissa(rng):
    """in [0.5, 1) with the last of its 53 bits set"""
    return math.ldexp(int(rng.integers(1 << 52, 1 << 53)) | 1, -53)


def fixed_point(c):
    """the repelling fixed point of z^2 + c: the root of z^2 - z + c of larger modulus"""
    r = cmath.sqrt(1.0 - 4.0 * complex(*c))
    a, b = (1.0 + r) / 2.0, (1.0 - r) / 2.0
    return a if abs(a) >= abs(b) else b


def _size(rng, fixed=None):
    if fixed is not None:
        return FIXED_SIZES[fixed % len(FIXED_SIZES)]
    if rng.random() < 0.1:
        return _pick(rng, FIXED_SIZES)
    return int(rng.integers(1, 80)), int(rng.integers(1, 60))


def _chain(rng):
    caps = sorted(int(c) for c in rng.choice(CAPS, size=int(rng.integers(2, 5)) + 1, replace=False))
    return tuple(caps), int(rng.integers(len(caps) - 1))


def _split(rng, height):
    y0 = int(rng.integers(0, height))
    return y0, int(rng.integers(y0 + 1, height + 1))


def _supersample(rng, width, height, cap, work):
    s = int(rng.integers(1, 9))
    while s > 1 and s * s * width * height * max(cap, 1) > work:
        s -= 1
    return s


def _look(rng, cfg):
    cfg.stable_limit, cfg.exposure = float(_pick(rng, STABLE_LIMITS)), float(_pick(rng, EXPOSURES))
    cfg.inside, cfg.smooth = int(rng.random() < 0.7), int(rng.random() < 0.7)
    cfg.primary_color = O.RGB(*(int(v) for v in rng.integers(0, 256, 3)))
    cfg.secondary_color = O.RGB(*(int(v) for v in rng.integers(0, 256, 3)))


def draw(rng, label="", fixed=None):
    """one F64 or F32 record from a numpy Generator; fixed: the size is FIXED_SIZES[fixed modulo their number]"""
    precision = F32 if rng.random() < 0.22 else F64
    r = rng.random()
    algo = O.MANDELBROT if r < 0.5 else (O.JULIA if r < 0.94 else O.BARNSLEY_FERN)
    cfg = O.config_new(O.MANDELBROT)
    cfg.algo = algo
    cfg.width, cfg.height = _size(rng, fixed)
    first = math.ldexp(_mantissa(rng), math.frexp(10.0 ** rng.uniform(-0.5, 4.0 if precision == F32 else 9.0))[1])
    other = first * float(_pick(rng, RATIOS))
    if rng.random() < 0.25:
        first, other = -first, -other
    cfg.scale = O.Imaginary(first, other) if rng.random() < 0.5 else O.Imaginary(other, first)
    constant = _pick(rng, JULIA_CONSTANTS)
    cfg.julia_set = O.Imaginary(*constant)
    if algo == O.JULIA:
        p = fixed_point(constant)
        centre = (p.real, p.imag)
    else:
        centre = _pick(rng, MANDELBROT_CENTRES)
    cfg.pos = O.Imaginary(centre[0] + float(rng.uniform(-0.35, 0.35)) / abs(cfg.scale.re),
                          centre[1] + float(rng.uniform(-0.35, 0.35)) / abs(cfg.scale.im))
    chain, piece = _chain(rng)
    cfg.iterations = chain[-1]
    cfg.limit = float(_pick(rng, PLAIN_LIMITS if rng.random() < 0.125 else LIMITS))
    _look(rng, cfg)
    split = _split(rng, cfg.height)
    s = _supersample(rng, cfg.width, cfg.height, chain[-1], WORK)
    tile, loop_mode, host = int(_pick(rng, TILES)), int(_pick(rng, LOOP_MODES)), bool(rng.random() < 0.25)
    return Record(label, cfg, precision, chain, piece, split, s, tile=tile, loop_mode=loop_mode, host=host)


class _OracleConfigs:
    """what tests/test_gpu_deep_edges.py::random_config asks of the package: Config.new(algo)"""

    class Config:
        new = staticmethod(lambda algo=0: O.config_new(int(algo)))


def dd_domain(cfg, pos_lo):
    """DD's domain of include/fractal_hip.h, restated"""
    vals = [cfg.limit, cfg.stable_limit, cfg.pos.re, cfg.pos.im, cfg.scale.re, cfg.scale.im, cfg.exposure, cfg.color_weight,
            cfg.julia_set.re, cfg.julia_set.im, pos_lo[0], pos_lo[1]]
    return (all(math.isfinite(v) for v in vals) and 0.0 < cfg.limit <= 2.0 ** 500
            and max(abs(cfg.pos.re), abs(cfg.pos.im), abs(cfg.julia_set.re), abs(cfg.julia_set.im)) <= 2.0 ** 64
            and min(abs(cfg.scale.re), abs(cfg.scale.im)) >= 2.0 ** -64
            and cfg.pos.re + pos_lo[0] == cfg.pos.re and cfg.pos.im + pos_lo[1] == cfg.pos.im)


def dd_record(rng, label=""):
    """a DD record, or None where random_config's view lies outside DD's domain"""
    from test_gpu_deep_edges import random_config

    cfg, pos_lo = random_config(_OracleConfigs, rng)
    cfg.width, cfg.height = _size(rng)
    chain, piece = _chain(rng)
    cfg.iterations = chain[-1]
    split = _split(rng, cfg.height)
    s = min(_supersample(rng, cfg.width, cfg.height, chain[-1], WORK_DD), 3)
    if not dd_domain(cfg, pos_lo):
        return None
    return Record(label, cfg, DD, chain, piece, split, s, pos_lo=tuple(float(v) for v in pos_lo))


@functools.lru_cache(maxsize=None)
def records(seed):
    """the F64 and F32 records of a seed, the same on every machine"""
    rng = np.random.default_rng(BASE_SEED + seed)
    # the first record of every seed and the third of every even one walk through FIXED_SIZES: 45 records, six or seven of each size
    fixed = {0: seed, 2: len(SEEDS) + seed // 2 if seed % 2 == 0 else None}
    return tuple(draw(rng, "seed %d record %d" % (seed, k), fixed.get(k)) for k in range(PER_SEED))


@functools.lru_cache(maxsize=None)
def dd_records(seed):
    rng = np.random.default_rng(DD_BASE_SEED + seed)
    r = dd_record(rng, "seed %d DD record" % seed)
    return () if r is None else (r,)


# ---- the edge records ---------------------------------------------------------------------------------------------------------------


def _view(width, height, algo=O.MANDELBROT, **kw):
    return O.cli_config(width, height, algo, **kw)


def _seahorse(width, height, **kw):
    return _view(width, height, pos=(-0.75, 0.1), scale=(8.0, 8.0), **kw)


def _overflow():
    from test_de_cpu import misiurewicz_i

    return misiurewicz_i(O.config_new(O.MANDELBROT), 40, 24, 1200)


def _scale_re_zero():
    # an even width: x / h == (w / h) / 2 at x = w / 2, so that column is 0 / 0 = NaN and the others are -inf and +inf
    return _view(12, 6, pos=(-0.5, 0.0), scale=(0.0, 0.4), limit=2.0)


EDGES = {
    # DE's domain limits: the largest limit, both ends of the thickness, and T * s on the bound with s > 1
    "limit_2^20": lambda n: Record(n, _seahorse(37, 23, limit=2.0 ** 20), F64, (17, 64, 300), 1, (5, 17), 2),
    "thickness_0": lambda n: Record(n, _seahorse(37, 23), F64, (17, 64, 300), 0, (5, 17), 3, thickness=0.0),
    "thickness_2^20": lambda n: Record(n, _seahorse(37, 23), F64, (17, 64, 300), 1, (0, 23), 1, thickness=2.0 ** 20),
    "Ts_2^20": lambda n: Record(n, _seahorse(37, 23), F64, (17, 64, 300), 0, (22, 23), 4, thickness=2.0 ** 18),
    # caps 0 and 1; at limit 2 pixels of the default view escape on the very first step.  Cap 0 returns (start, 0, (1, 0))
    "caps_0_1_2": lambda n: Record(n, _view(37, 23, limit=2.0), F64, (0, 1, 2), 0, (3, 20), 5, host=True),
    # the derivative of the centre pixel overflows (tests/test_de_cpu.py::misiurewicz_i at cap 1200): |d| >= 2^512, dn2 = +inf, at
    # cap 500; (-inf, -inf) at cap 820, which the link 820 -> 821 continues into (NaN, NaN); NaN from there on
    "overflow": lambda n: Record(n, _overflow(), F64, (500, 820, 821, 1200), 1, (5, 17), 2, host=True),
    # scale.re = 0: the coordinates are the IEEE result, +-inf and NaN, and min |scale| = 0 in D's last factor
    "scale_re_0": lambda n: Record(n, _scale_re_zero(), F64, (0, 2, 17), 1, (1, 4), 2, host=True),
    # every pixel, or none, in the stable class
    "stable_+inf": lambda n: Record(n, _seahorse(37, 23, stable_limit=math.inf), F64, (17, 64, 300), 1, (5, 17), 2),
    "stable_-1": lambda n: Record(n, _seahorse(37, 23, stable_limit=-1.0), F64, (17, 64, 300), 1, (5, 17), 2),
    # one output row and one output column under the filter kernels' tiles of 64 pixels by 1 (s = 8) and by 2 rows (s = 5)
    "65x1_s8": lambda n: Record(n, _seahorse(65, 1), F64, (17, 64, 300), 0, (0, 1), 8),
    "65x1_s5": lambda n: Record(n, _seahorse(65, 1), F64, (17, 64, 300), 1, (0, 1), 5),
    "1x9_s8": lambda n: Record(n, _seahorse(1, 9), F64, (17, 64, 300), 0, (2, 7), 8),
    "1x9_s5": lambda n: Record(n, _seahorse(1, 9), F64, (17, 64, 300), 1, (8, 9), 5),
}


@functools.lru_cache(maxsize=None)
def edge(name):
    return EDGES[name]("edge record " + name)
