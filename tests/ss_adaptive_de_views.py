"""What the F64 DE records of tests/shallow_random_views.py and the wide views of tests/deep_ss_views.py gain for ADAPTIVE
SUPERSAMPLED DE, shared by tests/test_ss_adaptive_de_random_cpu.py (the models alone: does the set have teeth) and
tests/test_gpu_ss_adaptive_de_random.py (the kernels against the models on the same inputs).  No device and no library: everything
is derived from the HOST MODELS' (z, it, der) of cfg_s — de_model.f64_rows for a record, deep_ss_views.Ss.rows("de_wide") and
rows("de_bla", table_bits) for a view — and from the thickness the record or the view already carries.

The inputs:
  records()  every record of shallow_random_views with `de` true, generated and edge (algo 1 and s = 1 included);
  wide()     every view of deep_ss_views.everything() that lies inside 2^440, on the roads of ROADS: WIDE PT and BLA-PT.
An input gains:
  H_de     ss_de_model.shaded(cfg, z, it, der, s, thickness), uint8 [s*height, s*width, 3];
  tau_de   deep_ss_views.median_tau(H_de, s);
  reach    with Dp = de_model.distance(cfg_s, ...) of the probes a[p::s, p::s], p = s // 2: the median of Dp over the escaped probes
           with a finite Dp > 0, divided by s, clamped to 2^20 / s; 1.0 where no probe qualifies.  With an odd number of such
           probes the median is a probe's own D, so R * s lands on or beside that probe's distance and the strict D < Rs is
           decided on its boundary;
  de_mixed with (e, n) = ss_adaptive_de_model.edge_sets at (tau_de, reach): some pixel is near without being a colour edge, the
           union is neither empty nor the whole image, and some pixel of it has box(H_de) != probe(H_de);
  describe()  everything that replays the input: the config's bytes in hex (and, for a view, n and the centre's words), s and the
           thickness, tau and reach as float.hex."""
import functools
import importlib.util
import os

import numpy as np

import de_model as D
import deep_ss_views as V
import shallow_random_views as R
import ss_adaptive_de_model as M
import ss_adaptive_model as A
import ss_de_model as SD
import ss_linear_model as LM

DE_MAX = 2.0 ** 20  # the largest reach * s the sets use
ROADS = ("de_wide", "de_bla")  # deep_ss_views.Ss.rows modes of WIDE PT and BLA-PT


@functools.lru_cache(maxsize=None)
def srgb_tables():
    """(L, T) by the arithmetic of csrc/gen_srgb_table.py, as test_gpu_ss_linear.LT makes them: the definition, not the library's copy"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fractal-renderer_amd", "csrc", "gen_srgb_table.py")
    spec = importlib.util.spec_from_file_location("_gen_srgb", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen.tables()


def srgb_filter(big, s, channels=3):
    """F of LINEAR-LIGHT SUPERSAMPLING under the sRGB transfer: ss_linear_model.ss_filter with the generator's tables"""
    L, T = srgb_tables()
    return LM.ss_filter(np.asarray(big), s, LM.SRGB, L, T, channels)


FILTERS = {0: None, 1: srgb_filter}  # transfer -> the filter argument of the adaptive models


def probes(s, *arrays):
    """a[p::s, p::s], p = s // 2, contiguous"""
    p = s // 2
    return tuple(np.ascontiguousarray(a[p::s, p::s]) for a in arrays)


def probe_distance(cfg, z, it, der, s):
    """(D of the probes in sample pixels float64 [height, width], escaped bool [height, width])"""
    zp, ip, dp = probes(s, z, it, der)
    return D.distance(SD.config_s(cfg, s), zp, ip, dp), ip < cfg.iterations


def median_reach(cfg, z, it, der, s):
    """the median finite positive D of the escaped probes, in output pixels, clamped to 2^20 / s; 1.0 without one"""
    dist, escaped = probe_distance(cfg, z, it, der, s)
    dist = dist[escaped]
    dist = dist[np.isfinite(dist) & (dist > 0.0)]
    if dist.size == 0:
        return 1.0
    return min(float(np.median(dist)) / s, DE_MAX / s)


class Input:
    """a record or a (view, road) with what this file derives; the models' arrays are computed once, on first use, read-only"""

    def __init__(self, label, cfg, s, thickness, source, what):
        self.label, self.cfg, self.s, self.thickness = label, cfg, s, float(thickness)
        self.h, self.w = cfg.height, cfg.width
        self.orbits = cfg.algo in (0, 2)
        self._source, self._what = source, what

    @functools.cached_property
    def arrays(self):
        """(z, it, der) of cfg_s by the host model"""
        out = tuple(self._source()[:3])
        for a in out:
            if a.flags.writeable:
                a.setflags(write=False)
        return out

    @functools.cached_property
    def H(self):
        big = M.shaded(self.cfg, *self.arrays, self.s, self.thickness)
        big.setflags(write=False)
        return big

    @functools.cached_property
    def tau(self):
        return V.median_tau(self.H, self.s)

    @functools.cached_property
    def reach(self):
        return median_reach(self.cfg, *self.arrays, self.s)

    def edge_sets(self, tau=None, reach=None):
        """(colour edge, near) at the input's (tau_de, reach) or at others"""
        tau = self.tau if tau is None else tau
        reach = self.reach if reach is None else reach
        return A.edges(self.H, self.s, tau), M.near(self.cfg, *self.arrays, self.s, reach)

    @functools.cached_property
    def sets(self):
        return self.edge_sets()

    @functools.cached_property
    def differ(self):
        """box(H_de) != probe(H_de), bool [height, width]"""
        return (SD.box(self.H, self.s) != A.probe(self.H, self.s)).any(axis=-1)

    @functools.cached_property
    def de_mixed(self):
        if not self.orbits:
            return False
        e, n = self.sets
        u = e | n
        return bool((n & ~e).any() and 0 < u.sum() < self.w * self.h and (u & self.differ).any())

    def model(self, tau, reach, y0=0, y1=None, channels=3, filter=None):
        """ss_adaptive_de_model.adaptive_de over the input's arrays (H is shaded once)"""
        H = self.H if self.orbits else None
        return M.adaptive_de(self.cfg, *self.arrays, self.s, self.thickness, tau, reach, y0, y1, channels, filter=filter, H=H)

    def describe(self):
        return "%s, s %d, thickness float.fromhex(%r), tau %d, reach float.fromhex(%r)" % (
            self._what(), self.s, self.thickness.hex(), self.tau, float(self.reach).hex())


# ---- (a) the F64 DE records -------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def de_records():
    """every record with `de` true, generated and edge"""
    out = [rec for seed in R.SEEDS for rec in R.records(seed) if rec.de]
    return tuple(out) + tuple(R.edge(name) for name in R.EDGES if R.edge(name).de)


@functools.lru_cache(maxsize=None)
def of_record(rec):
    cfg_s = rec.cfg_at(rec.chain[-1], rec.s)
    inp = Input(rec.label, rec.cfg, rec.s, rec.thickness, lambda: D.f64_rows(cfg_s), rec.describe)
    inp.rec = rec
    return inp


def records():
    return [of_record(rec) for rec in de_records()]


def records_of(seed):
    return [of_record(rec) for rec in R.records(seed) if rec.de]


# ---- (b) the wide views ---------------------------------------------------------------------------------------------------------------------


def wide_views():
    return [v for v in V.everything() if v.g.wide]


@functools.lru_cache(maxsize=None)
def of_view(v, mode):
    assert v.g.wide and mode in ROADS
    bits = v.g.table_bits if mode == "de_bla" else -1
    name = "BLA-PT, bits %d" % v.g.call_bits if mode == "de_bla" else "WIDE PT"
    inp = Input("%s, %s" % (v.g.label, name), v.cfg, v.s, v.thickness, lambda: v.rows(mode, bits), lambda: "%s, %s" % (name, v.g.describe(v.cfg)))
    inp.v, inp.mode = v, mode
    return inp


def wide(mode="de_wide"):
    """the inputs of the wide views on one road"""
    return [of_view(v, mode) for v in wide_views()]
