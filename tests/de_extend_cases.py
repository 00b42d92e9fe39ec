"""The views and caps of the RESUMABLE DE tests (tests/test_de_state_model_cpu.py, tests/test_gpu_de_extend.py) and the model's
answers for them, each computed once.  A case is a view, its road, and a cap change N -> M; `counts`, where given, are the
pixels (finished below N, escaping in [N, M), capped at M) that the case was chosen for."""
import ctypes as C
import functools

import de_model as D
import de_state_model as S
import oracle_lib as O
import pt_model as PTM
import pt_wide_model as W
from test_de_cpu import misiurewicz_i


class Case:
    def __init__(self, name, road, cfg, n, pos_lo=None, wide=None, counts=None, chain=None):
        self.name, self.road, self.n, self.pos_lo, self.wide, self.counts = name, road, n, pos_lo, wide, counts
        self.cfg = cfg  # at the cap M
        self.m = cfg.iterations
        self.chain = chain or (n, self.m)
        if wide:  # (centre name, words)
            self.ints = W.centre_ints(*wide)

    def cfg_at(self, cap):
        cfg = type(self.cfg).from_buffer_copy(bytes(self.cfg))
        cfg.iterations = cap
        return cfg

    @functools.lru_cache(maxsize=None)
    def orbits(self, cap):
        """a wide centre's orbits at the cap"""
        return W.Orbits(self.cfg_at(cap), *self.ints, self.wide[1])

    @functools.lru_cache(maxsize=None)
    def state(self, cap):
        """the model's state at the cap from the initial state: (z, iters, der) on F64, (z, iters, dz, m, der) on PT"""
        cfg = self.cfg_at(cap)
        if self.road == "f64":
            st = D.f64_rows(cfg)
        elif self.wide:
            st = S.pt_wide_state_rows(cfg, self.orbits(cap))
        else:
            st = S.pt_state_rows(cfg, self.pos_lo or (0.0, 0.0))
        for a in st:
            a.setflags(write=False)
        return st

    def continued(self, state, n, cap, y0=0, y1=None):
        """the model's continuation of `state` (rows [y0, y1)) from n to cap"""
        cfg = self.cfg_at(cap)
        if self.road == "f64":
            return S.f64_continue(cfg, state, n, y0, y1)
        if self.wide:
            return S.pt_wide_continue(cfg, self.orbits(cap), state, n, y0, y1)
        return S.pt_continue(cfg, state, n, self.pos_lo or (0.0, 0.0), y0, y1)

    def de_rows(self, cap):
        """DE's own (z, iters, der) at the cap (tests/de_model.py)"""
        cfg = self.cfg_at(cap)
        if self.road == "f64":
            return D.f64_rows(cfg)
        if self.wide:
            return D.pt_wide_rows(cfg, self.orbits(cap))
        return D.pt_rows(cfg, self.pos_lo or (0.0, 0.0))

    @functools.lru_cache(maxsize=None)
    def image(self, thickness, channels):
        st = self.state(self.m)
        a = D.colour(self.cfg, st[0], st[1], st[-1], thickness, channels)
        a.setflags(write=False)
        return a

    def same(self, a, b):
        return S.same_f64_state(a, b) if self.road == "f64" else S.same_state(a, b)


def _cfg(algo=0):
    return O.config_new(algo)


def _with_lo(make, *args):
    cfg = _cfg()
    lo = make(cfg, *args)
    return cfg, lo


def _seahorse():
    cfg, lo = _with_lo(D.seahorse_shallow, 40, 24, 3000, 1e11)
    return Case("", "pt", cfg, 2200, pos_lo=lo, counts=(551, 232, 177))


BUILDERS = {
    "f64-mandelbrot-40x24": lambda: Case("", "f64", D.default_view(_cfg(), 40, 24, 200), 10, counts=(745, 67, 148)),
    "f64-mandelbrot-37x23": lambda: Case("", "f64", D.default_view(_cfg(), 37, 23, 200), 10),
    "pt-mandelbrot-40x24": lambda: Case("", "pt", D.default_view(_cfg(), 40, 24, 200), 10, counts=(745, 67, 148)),
    "pt-mandelbrot-37x23": lambda: Case("", "pt", D.default_view(_cfg(), 37, 23, 200), 10),
    "f64-julia-40x24": lambda: Case("", "f64", D.julia_view(_cfg(), 40, 24, 300), 20, counts=(863, 93, 4)),
    "pt-julia-40x24": lambda: Case("", "pt", D.julia_view(_cfg(), 40, 24, 300), 20, counts=(863, 93, 4)),
    "f64-overflow": lambda: Case("", "f64", misiurewicz_i(_cfg(), 40, 24, 1200), 500, counts=(959, 0, 1)),
    "pt-overflow": lambda: Case("", "pt", misiurewicz_i(_cfg(), 40, 24, 1200), 500, counts=(959, 0, 1)),
    "pt-seahorse-pos-lo": _seahorse,
    "pt-julia-rebase": lambda: Case("", "pt", _with_lo(PTM.julia_rebase_view, 40, 24, 3000)[0], 300, counts=(886, 74, 0),
                                    chain=(150, 300, 3000)),
    "pt-orbit-escapes": lambda: Case("", "pt", _with_lo(PTM.early_escape_view, 37, 23, 2000)[0], 20, counts=(96, 106, 649)),
    "wide-2^200-16x12": lambda: Case("", "pt", W.view(_cfg(), "M", 200, 16, 12, 3000), 120, wide=("M", 5), counts=(0, 192, 0)),
    "wide-2^200-37x21": lambda: Case("", "pt", W.view(_cfg(), "M", 200, 37, 21, 3000), 120, wide=("M", 5)),
    "wide-julia": lambda: Case("", "pt", W.view(_cfg(), "J", 100, 24, 16, 400), 100, wide=("J", 3), counts=(325, 53, 6)),
}

ALL = sorted(BUILDERS)
PT = [n for n in ALL if not n.startswith("f64")]
F64 = [n for n in ALL if n.startswith("f64")]


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    c.name = name
    return c


def classes(it, n, m):
    """pixels (finished below n, escaping in [n, m), capped at m) of the escape indices at the cap m"""
    return int((it < n).sum()), int(((it >= n) & (it < m)).sum()), int((it == m).sum())
