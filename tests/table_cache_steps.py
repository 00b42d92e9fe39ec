"""The step lists of the table-cache tests (tests/test_table_cache_cpu.py, tests/test_gpu_table_cache.py): sequences of views,
each differing from the one before in one thing, with what the MODELS say about the table slot of a context (Ctx::bla_table,
fractal-renderer_amd/csrc/fr_bla.hip: bla_table_for) at every step.

A step holds its config, its centre, its bits, its orbits (tests/pt_wide_model.py's integers or tests/pt_model.py's dd
recurrence, never the library's) and, computed once, its model result and its whole tables.  classes() compares every step with
the step whose tables the slot holds — the one before, or the one before a step that reads no table:
  must_build   an orbit differs, or the tables differ in any bit: a library that serves the slot's tables here is wrong;
  may_serve    neither differs: serving and building give the same kernel arguments.
Nothing here reads the library beyond fr.Config.new (the defaults of a config)."""
import ctypes as C
import math

import numpy as np

import bla_model as B
import pt_model as P
import pt_scaled_model as S
import pt_wide_model as W

MUST_BUILD, MAY_SERVE = "must_build", "may_serve"
DEFAULT_BITS = 40  # FR_BLA_DEFAULT_BITS: what bits = 0 asks for
NO_TABLE = S.NO_TABLE


def changed(cfg, **kw):
    """a copy of cfg with the given fields; pairs for pos, scale, julia_set, triples for the colours"""
    out = cfg.clone()
    for k, v in kw.items():
        if k in ("pos", "scale", "julia_set"):
            getattr(out, k).re, getattr(out, k).im = v
        elif k in ("primary_color", "secondary_color"):
            c = getattr(out, k)
            c.r, c.g, c.b = v
        else:
            setattr(out, k, v)
    return out


def _readonly(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


_wide_orbits = {}


def wide_orbits(cfg, ints, n):
    """(x, k or None, every orbit ended by escape) from pt_wide_model's integers, computed once per key of the orbit"""
    julia = cfg.algo == 2
    key = (ints, n, int(cfg.algo), int(cfg.iterations), (cfg.julia_set.re.hex(), cfg.julia_set.im.hex()) if julia else None)
    if key not in _wide_orbits:
        o = W.Orbits(cfg, ints[0], ints[1], n)
        x, k = o.x[0], o.k[0] if julia else None
        _readonly([a for a in (x, k) if a is not None])
        _wide_orbits[key] = (x, k, bool(o.x[1] and o.k[1]))
    return _wide_orbits[key]


class Step:
    """what: the change against the step before; bits: as the call is given them (0: the default; -1, SCALED PT only: no
    table); extra: a further check the GPU test makes at this step — "served": the repeat of the call and a row piece find the
    slot's tables; "render": the RGB render; "rekey": the orbit cache computes nothing"""

    scaled = False
    pos_lo = None
    n = ints = words = None

    def __init__(self, what, cfg, bits, extra=None):
        self.what, self.cfg, self.bits, self.extra = what, cfg, bits, extra
        self.shape = (cfg.height, cfg.width)
        self._model = self._tables = None

    @property
    def table_bits(self):
        """the bits of the table the call reads; None: it reads none"""
        return None if self.bits < 0 else DEFAULT_BITS if self.bits == 0 else self.bits

    def orbits(self):
        return [self.x] if self.k is None else [self.x, self.k]

    def model(self):
        """(z, iters, passes, ...) of the road's model over the whole image"""
        if self._model is None:
            self._model = _readonly(list(self._escape_rows()))
        return self._model

    def passes(self, y0=0, y1=None):
        return int(self.model()[2][y0:y1].astype(np.uint64).sum())

    def tables(self):
        """the whole tables: per orbit a list of levels, each float64 [n_k, 5]"""
        if self._tables is None:
            self._tables = [self._table(o) for o in self.orbits()]
        return self._tables

    def cache_triple(self):
        """what fr_debug_bla_cache reports of these tables: (bits, levels of the first orbit's table, entries of all)"""
        t = self.tables()
        return self.table_bits, len(t[0]), sum(len(level) for table in t for level in table)

    def centre(self, native):
        """the fr_wide_centre of the step (it points into self.words)"""
        p64 = C.POINTER(C.c_uint64)
        return native.fr_wide_centre(self.n, self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64))

    def kw(self, fr):
        """the keywords the package's calls select this step's centre with"""
        if self.ints is None:
            return dict(pos_lo=self.pos_lo)
        return dict(centre=fr.WideCentre(self.n, re=self.words[0], im=self.words[1]))


class ScaledStep(Step):
    """SCALED PT on a wide centre: the integers `ints` of n words"""

    scaled = True

    def __init__(self, what, cfg, n, ints, bits=40, extra=None):
        Step.__init__(self, what, cfg, bits, extra)
        self.n, self.ints = n, ints
        self.words = W.to_words(ints[0], n), W.to_words(ints[1], n)
        self.x, self.k, self.ended = wide_orbits(cfg, ints, n)

    def D(self):
        return float(S.lib().ptsm_Dw(C.byref(S._view(self.cfg))))

    def _escape_rows(self):
        return S.escape_rows(self.cfg, self.x, self.k, NO_TABLE if self.table_bits is None else self.table_bits)

    def _table(self, orbit):
        return S.table(self.cfg, orbit, self.table_bits)

    def model_with_table_of(self, other):
        """the model on this view with the tables built for `other`'s Dw and S: what a stale slot gives"""
        return S.escape_rows_table_of(self.cfg, other.cfg, self.x, self.k, self.table_bits)


class BlaStep(Step):
    """BLA-PT on a dd centre (pos + pos_lo) or, with n and ints, on a wide one"""

    def __init__(self, what, cfg, pos_lo=None, n=None, ints=None, bits=40, extra=None):
        Step.__init__(self, what, cfg, bits, extra)
        if ints is None:
            self.pos_lo = (float(pos_lo[0]), float(pos_lo[1]))
            self.x = P.reference_orbit(cfg, self.pos_lo, 0)
            self.k = P.reference_orbit(cfg, self.pos_lo, 1) if cfg.algo == 2 else None
            _readonly([a for a in (self.x, self.k) if a is not None])
        else:
            self.n, self.ints = n, ints
            self.words = W.to_words(ints[0], n), W.to_words(ints[1], n)
            self.x, self.k, _ = wide_orbits(cfg, ints, n)

    def D(self):
        return float(B.lib().blam_D(C.byref(B._view(self.cfg))))

    def _escape_rows(self):
        return B.escape_rows(self.cfg, self.x, self.k, self.table_bits)

    def _table(self, orbit):
        return B.table(self.cfg, orbit, self.table_bits)

    def args(self, native):
        """(pos_lo, centre) of the fr_*_pt_bla calls and what keeps them alive"""
        if self.ints is not None:
            st = self.centre(native)
            return None, C.byref(st), st
        lo = native.Imaginary(*self.pos_lo)
        return C.byref(lo), None, lo


# ---- what the models say about the slot -------------------------------------------------------------------------------------


def same_orbits(a, b):
    oa, ob = a.orbits(), b.orbits()
    return len(oa) == len(ob) and all(x.shape == y.shape and S.same_bits(x, y) for x, y in zip(oa, ob))


def same_tables(a, b):
    """all levels, all five columns, of every orbit's table, bit for bit; and the same kind of table"""
    ta, tb = a.tables(), b.tables()
    return (a.scaled == b.scaled and len(ta) == len(tb)
            and all(len(x) == len(y) and all(p.shape == q.shape and S.same_bits(p, q) for p, q in zip(x, y)) for x, y in zip(ta, tb)))


def holders(steps):
    """per step, the step whose tables the slot holds when the step's first call arrives: None before the first, otherwise the
    last step before it that reads a table"""
    out, holder = [], None
    for s in steps:
        out.append(holder)
        if s.table_bits is not None:
            holder = s
    return out


def classes(steps):
    """per step MUST_BUILD or MAY_SERVE against its holder; None for the first step (whatever ran before it holds the slot) and
    for a step that reads no table"""
    out = []
    for s, h in zip(steps, holders(steps)):
        if h is None or s.table_bits is None:
            out.append(None)
        elif not same_orbits(s, h) or not same_tables(s, h):
            out.append(MUST_BUILD)
        else:
            out.append(MAY_SERVE)
    return out


def by_name(steps):
    out = {s.what: s for s in steps}
    assert len(out) == len(steps), "two steps of one name"
    return out


# ---- Sequence S: SCALED PT's table form ---------------------------------------------------------------------------------------

_sequences = {}


def _scaled_spec(new_config, spec):
    """(cfg, n, ints) of one of tests/pt_scaled_model.py's specs"""
    name, n, scale_log2, width, height, cap = spec
    cfg = W.view(new_config(), "M" if name == "MINI" else name, scale_log2, width, height, cap)
    return cfg, n, S.centre_ints(name, n)


def sequence_s(new_config):
    """N_900 (the slot holds something else), then M_900 changed one thing at a time, MINI_861 with its cap raised and its scale
    doubled, J_900 with its scale doubled and julia_set moved by an ulp"""
    if "S" in _sequences:
        return _sequences["S"]
    steps = []
    state = {}

    def first(what, spec, extra=None):
        state["cfg"], state["n"], state["ints"] = _scaled_spec(new_config, spec)
        state["bits"] = 40
        steps.append(ScaledStep(what, state["cfg"], state["n"], state["ints"], 40, extra))

    def step(what, bits=None, ints=None, extra=None, **change):
        state["cfg"] = changed(state["cfg"], **change)
        if bits is not None:
            state["bits"] = bits
        if ints is not None:
            state["ints"] = ints
        steps.append(ScaledStep(what, state["cfg"], state["n"], state["ints"], state["bits"], extra))

    two = lambda e: math.ldexp(1.0, e)  # noqa: E731
    first("unrelated: N at 2^900", S.N_900)
    first("M at 2^900", S.M_900, "served")
    step("scale x 2", scale=(two(901), two(901)))
    step("scale x 2^-9", scale=(two(892), two(892)))
    step("back to 2^900", scale=(two(900), two(900)))
    step("scale.im negated", scale=(two(900), -two(900)))
    step("scale.re x 1.25", scale=(1.25 * two(900), -two(900)))
    step("bits 41", bits=41)
    step("bits 0", bits=0)
    step("bits -1", bits=-1)
    step("bits 40 again", bits=40)
    step("size 21 x 37", width=21, height=37)
    step("size 74 x 42", width=74, height=42)
    step("size 37 x 21", width=37, height=21)  # from twice the size: Dw equal
    step("limit", limit=1000.5)
    step("colours and exposure", extra="render", primary_color=(9, 200, 77), secondary_color=(255, 1, 128), exposure=20.0)
    step("iterations 6001", extra="rekey", iterations=6001)
    step("iterations 600", iterations=600)
    step("iterations 6000", iterations=6000)
    step("centre: last word + 1", ints=(state["ints"][0] + 1, state["ints"][1]))
    first("MINI at 2^861", S.MINI_861)
    step("MINI: cap 3300", iterations=3300)
    step("MINI: scale x 2", scale=(two(862), two(862)))
    first("J at 2^900", S.J_900, "served")
    step("J: scale x 2", scale=(two(901), two(901)))
    js = state["cfg"].julia_set
    step("J: julia_set.im + 1 ulp", julia_set=(js.re, math.nextafter(js.im, math.inf)))
    _sequences["S"] = steps
    return steps


def scale_steps_m(new_config, log2s):
    """centre M, 16 words, 37 x 21, cap 6000, bits 40 at the scales 2^e for e in log2s: the views of the teeth conditions"""
    cfg, n, ints = _scaled_spec(new_config, S.M_900)
    return [ScaledStep("M at 2^%d" % e, changed(cfg, scale=(math.ldexp(1.0, e), math.ldexp(1.0, e))), n, ints, 40) for e in log2s]


# ---- Sequence B: BLA-PT with a dd centre --------------------------------------------------------------------------------------


def sequence_b(new_config):
    """N_16 (the slot holds something else), then tests/bla_model.py's SEAHORSE changed one thing at a time"""
    if "B" in _sequences:
        return _sequences["B"]
    steps = []
    _kind, name, n, scale_log2, width, height, cap = B.N_16
    steps.append(BlaStep("unrelated: N at 2^300", W.view(new_config(), name, scale_log2, width, height, cap), n=n,
                         ints=W.centre_ints(name, n)))
    state = {"cfg": new_config(), "bits": 40}
    state["lo"] = own = P.seahorse_view(state["cfg"])
    first_cfg = state["cfg"].clone()
    steps.append(BlaStep("SEAHORSE", state["cfg"], own, extra="served"))

    def step(what, bits=None, lo=None, cfg=None, **change):
        state["cfg"] = changed(state["cfg"] if cfg is None else cfg, **change)
        if bits is not None:
            state["bits"] = bits
        if lo is not None:
            state["lo"] = lo
        steps.append(BlaStep(what, state["cfg"], state["lo"], bits=state["bits"]))

    scale, cap = first_cfg.scale.re, first_cfg.iterations
    step("pos_lo.im + 0.2 ulp", lo=(own[0], own[1] + 0.2 * math.ulp(first_cfg.pos.im)))
    step("iterations - 1", iterations=cap - 1)
    step("iterations + 1", iterations=cap)
    step("scale x 2", scale=(2.0 * scale, 2.0 * scale))
    step("scale x 1.5", scale=(3.0 * scale, 3.0 * scale))
    step("size 21 x 37", width=21, height=37)
    step("size 42 x 74", width=42, height=74)  # the same aspect doubled: D equal
    step("bits 53", bits=53)
    step("bits 24", bits=24)
    step("limit", limit=1000.5)
    julia = state["cfg"].clone()
    julia_lo = P.julia_rebase_view(julia)
    step("algo: Julia", lo=julia_lo, cfg=julia)
    js = state["cfg"].julia_set
    step("julia_set.im + 1 ulp", julia_set=(js.re, math.nextafter(js.im, math.inf)))
    step("back to the first", bits=40, lo=own, cfg=first_cfg)
    step("iterations - 1, orbit cut at the cap", iterations=cap - 1)  # this orbit runs to the cap: the cap decides its length
    step("iterations + 1, orbit cut at the cap", iterations=cap)
    _sequences["B"] = steps
    return steps


def wide_bla_steps(new_config):
    """tests/bla_model.py's M_16 and the same view at 2^301"""
    _kind, name, n, scale_log2, width, height, cap = B.M_16
    ints = W.centre_ints(name, n)
    return [BlaStep("M_16 at 2^%d" % e, W.view(new_config(), name, e, width, height, cap), n=n, ints=ints)
            for e in (scale_log2, scale_log2 + 1)]
