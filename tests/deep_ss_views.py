"""What the generated and edge views of tests/deep_random_views.py gain for the supersampled, adaptive and kept scaled-DE calls,
shared by tests/test_deep_ss_random_cpu.py (the models alone: does the set have teeth) and tests/test_gpu_deep_ss_random.py (the
kernels against the models on the same views).  No device and no library: everything is derived from the seed and from the HOST
MODELS — pt_scaled_model.escape_rows, de_scaled_model.escape_rows and test_gpu_deep_edges.soft_colours' colour map on cfg_s, the view's config
with width * s and height * s.  The orbits are the view's own: the centre and the cap do not change with s.

A view gains:
  s          drawn from S_VALUES by default_rng([BASE_SEED + seed, 7]), lowered by one while it is above 2 and
             s * s * width * height * max(cap, 1) is above WORK (a host model of cfg_s then stays under a second or two); an edge
             view takes the fixed s of EDGE_S, chosen so that all six values occur;
  piece      a drawn row piece [y0, y1), y0 < y1;  a: on a view with height >= 3 the drawn row of the three-way split
             [0, a), [a, a + 1), [a + 1, height), whose middle piece has a neighbour row on either side;
  H          soft_colours of the scaled model (bits -1) on cfg_s;  tau: with d(X, Y) the largest channel difference of H's probe
             image to any of the 8 neighbours inside the image, the distinct value v of d whose share of pixels with d > v is
             nearest to 0.5 (the smallest such v); 0 on a flat view;
  thickness  the median finite positive distance of the escaped samples of cfg_s by de_scaled_model, clamped so that
             thickness * s <= 2^20; 1.0 where no sample has one;
  split      the band split N: the median escaped index of the view (at its own size) + 1, clamped to cap - 1; None where no pixel
             escapes or the cap is under 2.
EXTRA lists the views added from seeds 16 upward (deep_random_views.views(seed)[k], with s and the pieces drawn as above): those
the models call mixed and that fill a floor of tests/test_deep_ss_random_cpu.py which the 60 views alone miss.  They were picked
by scripts run on the host models; nothing a device returns took part.  The CPU test asserts that each of them is mixed."""
import functools

import numpy as np

import bla_model as B
import de_bla_model as DB
import de_model as D
import de_scaled_model as M
import deep_random_views as G
import oracle_lib as O
import pt_scaled_model as S
import pt_wide_model as W
import ss_adaptive_model as A

S_VALUES = (2, 3, 4, 5, 7, 8)
WORK = 2 ** 26  # samples * cap of cfg_s
DE_MAX = 2.0 ** 20  # the largest thickness * s of the DE calls
EDGE_S = {"below_2^440": 3, "e_951": 2, "ratio_2^-32": 8, "F_e+64_n8": 7, "F_e+64_n3": 5, "n16_e70": 8, "limit_2^20": 4,
          "limit_2^20_J": 4, "1x1": 7, "outside": 5, "on_a_pixel": 5, "on_a_pixel_J": 7}
# the mixed views with `smooth` off that the draws of seeds 16 .. 45 hold besides (34, 1) and (41, 0): the 60 views have two such,
# the floor is three.  (39, 2) also is a mixed view at s = 8 past 2^440.
EXTRA = ((17, 1), (21, 0), (24, 2), (28, 0), (39, 2))


def soft_colours(cfg, z, it):
    """test_gpu_deep_edges.soft_colours — the oracle's colour map with the software log2; an algorithm without orbits is black —
    through de_model.base_colours, which gives the oracle at most 16 threads where its own default is a thread per processor of
    the machine (tests/test_deep_ss_random_cpu.py asserts that the two are one)"""
    if cfg.algo not in (0, 2):
        return np.zeros(np.shape(it) + (3,), dtype=np.uint8)
    return D.base_colours(cfg, np.ascontiguousarray(z), it)


def lowered(s, width, height, cap):
    while s > 2 and s * s * width * height * max(cap, 1) > WORK:
        s -= 1
    return s


def config_s(cfg, s, cap=None):
    """a copy of cfg with width * s and height * s, at its cap or at another"""
    big = type(cfg).from_buffer_copy(bytes(cfg))
    big.width, big.height = cfg.width * s, cfg.height * s
    if cap is not None:
        big.iterations = cap
    return big


def neighbour_difference(P, neighbours=8, y0=0, y1=None):
    """d(X, Y) of a probe image uint8 [h, w, 3]: the largest channel difference to any of the 8 (or 4) neighbours inside rows
    [y0, y1) of the image (the definition: the whole image), -1 where a pixel has no neighbour; int32 [h, w]"""
    P = P.astype(np.int32)
    h, w = P.shape[:2]
    y1 = h if y1 is None else y1
    d = np.full((h, w), -1, dtype=np.int32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dy == 0 and dx == 0) or (neighbours == 4 and dy != 0 and dx != 0):
                continue
            ys = slice(max(y0, y0 - dy), y1 - max(0, dy))
            xs = slice(max(0, -dx), w - max(0, dx))
            yn = slice(max(y0, y0 - dy) + dy, y1 - max(0, dy) + dy)
            xn = slice(max(0, -dx) + dx, w - max(0, dx) + dx)
            if ys.start >= ys.stop or xs.start >= xs.stop:
                continue
            d[ys, xs] = np.maximum(d[ys, xs], np.abs(P[ys, xs] - P[yn, xn]).max(axis=-1))
    return d


def median_tau(big, s):
    """the distinct value of d whose share of pixels with d > v is nearest to 0.5, the smallest of them; 0 on a flat view"""
    d = neighbour_difference(A.probe(big, s))
    values = np.unique(d[d >= 0])
    if values.size == 0 or values[-1] == 0:
        return 0
    shares = np.array([(d > v).mean() for v in values])
    return int(values[int(np.argmin(np.abs(shares - 0.5)))])


class Ss:
    """a view of deep_random_views with what this file derives; the models' arrays are computed once, on first use, read-only"""

    def __init__(self, g, key, s, piece, a):
        self.g, self.key, self.s, self.piece, self.a = g, key, s, piece, a
        self.cfg = g.cfg(O.config_new)  # the oracle's Config: the same 104 bytes as the library's
        self.cfg_s = config_s(self.cfg, s)
        self.h, self.w = g.shape

    @functools.cached_property
    def orbits(self):
        return self.g.orbits(self.cfg)

    @property
    def x(self):
        return self.orbits.x[0]

    @property
    def k(self):
        return self.orbits.k[0] if self.g.julia else None

    def _frozen(self, arrays):
        for a in arrays:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return arrays

    @functools.lru_cache(maxsize=None)
    def rows(self, mode, bits=-1):
        """a model's arrays on cfg_s: "wide" (z, iters) of WIDE PT, "bla" and "scaled" (z, iters, ...) at a table's bits or -1,
        "de_wide", "de_bla" and "de_scaled" (z, iters, der or u, ...)"""
        cfg, x, k = self.cfg_s, self.x, self.k
        if mode == "wide":
            (z, it, _, _), _ = W.state_rows(cfg, self.orbits, rule=1)
            r = (z, it)
        elif mode == "bla":
            r = B.escape_rows(cfg, x, k, bits)
        elif mode == "scaled":
            r = S.escape_rows(cfg, x, k, bits)
        elif mode == "de_wide":
            r = D.pt_wide_rows(cfg, self.orbits)
        elif mode == "de_bla":
            r = DB.escape_rows(cfg, x, k, bits)
        elif mode == "de_scaled":
            r = M.escape_rows(cfg, x, k, bits)
        else:
            raise KeyError(mode)
        return self._frozen(r)

    def scaled(self, bits=-1):
        """(z, iters, ...) of pt_scaled_model on cfg_s"""
        return self.rows("scaled", bits)

    def de_scaled(self, bits=-1):
        """(z, iters, u, ...) of de_scaled_model on cfg_s"""
        return self.rows("de_scaled", bits)

    @functools.lru_cache(maxsize=None)
    def plain(self):
        """(z, iters, ...) of pt_scaled_model (bits -1) on the view at its own size"""
        return self._frozen(S.escape_rows(self.cfg, self.x, self.k, -1))

    @functools.lru_cache(maxsize=None)
    def image(self, bits=-1, mode="scaled"):
        """H by the scaled model, or by another road's: uint8 [s*h, s*w, 3]"""
        z, it = self.rows(mode, bits)[:2]
        big = soft_colours(self.cfg_s, z, it)
        big.setflags(write=False)
        return big

    @functools.cached_property
    def tau(self):
        return median_tau(self.image(), self.s)

    @functools.cached_property
    def thickness(self):
        z, it, u = self.de_scaled()[:3]
        dist = D.distance(M.scaled_view(self.cfg_s), z, it, u)[it < self.g.cap]
        dist = dist[np.isfinite(dist) & (dist > 0.0)]
        t = float(np.median(dist)) if dist.size else 1.0
        return min(t, DE_MAX / self.s)

    @functools.cached_property
    def split(self):
        it = self.plain()[1]
        escaped = it[it < self.g.cap]
        if self.g.cap < 2 or escaped.size == 0:
            return None
        return min(int(np.median(escaped)) + 1, self.g.cap - 1)

    def split_classes(self):
        """(pixels finished before N, pixels escaping at N or later, pixels at the cap) of the band split; None without one"""
        n = self.split
        if n is None:
            return None
        it = self.plain()[1]
        return int((it < n).sum()), int(((it >= n) & (it < self.g.cap)).sum()), int((it == self.g.cap).sum())

    def edge_share(self, tau=None):
        return A.edge_share(self.image(), self.s, self.tau if tau is None else tau)

    @functools.cached_property
    def mixed(self):
        """tau gives an edge share in [0.05, 0.95] and at least one edge pixel has F != P"""
        big, s = self.image(), self.s
        e = A.edges(big, s, self.tau)
        differ = (A.np_filter(big, s) != A.probe(big, s)).any(axis=-1)
        return bool(0.05 <= e.mean() <= 0.95 and (e & differ).any())

    def three_way(self):
        """[(0, a), (a, a + 1), (a + 1, h)] on a view with height >= 3, else None"""
        return None if self.a is None else [(0, self.a), (self.a, self.a + 1), (self.a + 1, self.h)]

    def describe(self):
        return "%s, s %d, tau %d" % (self.g.describe(self.cfg), self.s, self.tau)


def _drawn(rng, g):
    d = g.draw
    s = lowered(int(S_VALUES[int(rng.integers(len(S_VALUES)))]), d.width, d.height, d.cap)
    y0 = int(rng.integers(0, d.height))
    y1 = int(rng.integers(y0 + 1, d.height + 1))
    a = int(rng.integers(1, d.height - 1)) if d.height >= 3 else None
    return s, (y0, y1), a


@functools.lru_cache(maxsize=None)
def all_of(seed):
    """the three views of a seed with what they gain, the same on every machine"""
    rng = np.random.default_rng([G.BASE_SEED + seed, 7])
    return tuple(Ss(g, (seed, k), *_drawn(rng, g)) for k, g in enumerate(G.views(seed)))


@functools.lru_cache(maxsize=None)
def views(seed):
    """the views of a seed that the tests run: all three of deep_random_views.SEEDS, those of EXTRA from the seeds above"""
    if seed in G.SEEDS:
        return all_of(seed)
    return tuple(v for v in all_of(seed) if v.key in EXTRA)


SEEDS = tuple(G.SEEDS) + tuple(sorted({seed for seed, _ in EXTRA}))


@functools.lru_cache(maxsize=None)
def edge(name):
    g = G.edge(name)
    d = g.draw
    rng = np.random.default_rng([G.BASE_SEED, 8, list(G.EDGES).index(name)])
    _, piece, a = _drawn(rng, g)
    return Ss(g, name, lowered(EDGE_S[name], d.width, d.height, d.cap), piece, a)


def everything():
    """every view the tests run: generated, extra, edge"""
    return [v for seed in SEEDS for v in views(seed)] + [edge(name) for name in G.EDGES]


# ---- the dd-centre views: one drawn s each ----------------------------------------------------------------------------------------


def dd_supersample(seed, k, cfg):
    """the s of dd-centre view k of a seed (test_gpu_deep_edges.random_config's draws are left alone: this has its own generator)"""
    rng = np.random.default_rng([G.DD_BASE_SEED + seed, 7, k])
    return lowered(int(S_VALUES[int(rng.integers(len(S_VALUES)))]), cfg.width, cfg.height, cfg.iterations)


# ---- the F64 records of tests/shallow_random_views.py on the adaptive call ------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def f64_records():
    """every F64 record, generated and edge, algo 1 included"""
    import shallow_random_views as R

    out = [rec for seed in R.SEEDS for rec in R.records(seed) if rec.precision == R.F64]
    return tuple(out) + tuple(R.edge(name) for name in R.EDGES)


_f64_images = {}


def f64_image(rec):
    """H of an F64 record: soft_colours of the oracle's F64 rows of cfg_s at the record's last cap, read-only, made once"""
    if rec.label not in _f64_images:
        cfg_s = rec.cfg_at(rec.chain[-1], rec.s)
        if cfg_s.algo in (0, 2):
            z, it = O.escape_rows(cfg_s, O.F64, threads=D.THREADS)
        else:
            z, it = np.zeros((cfg_s.height, cfg_s.width, 2)), np.zeros((cfg_s.height, cfg_s.width), dtype=np.uint32)
        big = soft_colours(cfg_s, z, it)
        big.setflags(write=False)
        _f64_images[rec.label] = big
    return _f64_images[rec.label]


def f64_mixed(rec):
    """(tau, mixed) of an F64 record, by the definition of Ss.mixed"""
    big, s = f64_image(rec), rec.s
    tau = median_tau(big, s)
    e = A.edges(big, s, tau)
    differ = (A.np_filter(big, s) != A.probe(big, s)).any(axis=-1)
    return tau, bool(0.05 <= e.mean() <= 0.95 and (e & differ).any())
