"""The generated views of tests/deep_random_views.py on the host models alone, without a device: conditions on the INPUTS of
tests/test_gpu_deep_random.py, so that a later edit of the generator cannot hollow the GPU tests out unnoticed, and the models
themselves against exact orbits on views nobody wrote by hand.
  - the generator is deterministic and draws what its header says; every view lies in the domains it claims;
  - over the GPU file's seeds (the counts are printed with -s): at least half of the views with cap >= 300 are resolved (>= 4
    distinct escape indices); at least a quarter of those have pixels at the cap; among the resolved views at least three each
    are Julia, have a negative axis, unequal axes, n above the minimum, zero shift, lie inside 2^440, lie past it; of the table
    runs on resolved views three quarters take skips, half have rebases, five ride a reference orbit ended by escape;
  - in the common domain SCALED PT at bits -1 is WIDE PT bit for bit, its table form is BLA-PT, and scaled DE's u 2^e is the wide
    derivative (the header's CLAIM and CLAIM 2), on every generated and edge view there;
  - the truth spot check: on eight drawn pixels and the centre pixel of every resolved view the exact orbit and derivative
    (deep_truth.View.pixel, de_scaled_truth._orbit, at P and P + 320; a pixel on which the two disagree is left out) against the
    wide, BLA and scaled models at bits -1, 40 and 53: the exact index on settled pixels, z within move + Z_FLOOR max(|z|, 1), D
    within de_scaled_truth.D_TOLERANCE where the exact D >= 2^-10 pixels; bits 24 is printed; at least 60 % of the sampled
    pixels are compared, and 30 % of each view's;
  - the edge views are resolved where they are meant to be, and one rides an orbit ended by escape within a few entries;
  - at least half of the dd-centre views that the GPU file draws lie inside the domain of each call it makes on them."""
import math
from fractions import Fraction

import numpy as np
import pytest

import bla_model as B
import de_model as D
import de_scaled_model as M
import de_scaled_truth as U
import deep_random_views as G
import deep_truth as T
import pt_scaled_model as S
import pt_wide_model as W


@pytest.fixture(scope="module")
def fr():
    import __graft_entry__ as ge

    ge.build()
    import fractal_renderer_amd

    return fractal_renderer_amd


class Run:
    """a view with its config, its orbits and the models' results, each computed once"""

    def __init__(self, fr, g):
        self.g = g
        self.cfg = g.cfg(fr.Config.new)
        self.orbits = g.orbits(self.cfg)
        self.x = self.orbits.x[0]
        self.k = self.orbits.k[0] if g.julia else None
        self._rows = {}

    def rows(self, mode, bits=-1):
        """(z, iters, ...) of a model over the whole view: "wide", "bla", "scaled" (z, iters, passes[, rebases]); "de" the scaled
        DE model (z, iters, u, ...); "de_wide" de_model on the wide orbits"""
        key = (mode, bits)
        if key not in self._rows:
            if mode == "wide":
                (z, it, _, _), reb = W.state_rows(self.cfg, self.orbits, rule=1)
                r = (z, it, None, reb)
            elif mode == "bla":
                r = B.escape_rows(self.cfg, self.x, self.k, bits)
            elif mode == "scaled":
                r = S.escape_rows(self.cfg, self.x, self.k, bits)
            elif mode == "de":
                r = M.escape_rows(self.cfg, self.x, self.k, bits)
            elif mode == "de_wide":
                r = D.pt_wide_rows(self.cfg, self.orbits)
            else:
                raise KeyError(mode)
            self._rows[key] = r
        return self._rows[key]

    @property
    def resolved(self):
        return self.g.cap >= G.RESOLVED_CAP and len(np.unique(self.rows("scaled")[1])) >= G.RESOLVED_INDICES

    @property
    def ended(self):
        return bool(self.orbits.x[1] or self.orbits.k[1])


_runs = {}


def runs(fr):
    """{(seed, k): Run} of every generated view of the GPU file's seeds"""
    if not _runs:
        for seed in G.SEEDS:
            for k, g in enumerate(G.views(seed)):
                _runs[seed, k] = Run(fr, g)
    return _runs


_edges = {}


def edges(fr):
    if not _edges:
        for name in G.EDGES:
            _edges[name] = Run(fr, G.edge(name))
    return _edges


# ---- 1. the generator -------------------------------------------------------------------------------------------------------------


def test_a_seed_gives_the_same_views_every_time():
    for seed in (0, 7, 15):
        a, b = G.views(seed), G.views(seed)
        assert [g.draw for g in a] == [g.draw for g in b] and len(a) == G.PER_SEED >= 2
        assert [g.ints for g in a] == [g.ints for g in b]
    assert G.views(0)[0].draw != G.views(1)[0].draw


def test_the_draws_are_python_numbers_inside_the_stated_ranges():
    seen = {"centre": set(), "ratio1": 0, "limit": set(), "cap": set(), "bits": set(), "n_min": 0, "constant": 0}
    count = 0
    for seed in G.SEEDS:
        for g in G.views(seed):
            d = g.draw
            count += 1
            assert all(type(v) is float for v in d.scale + (d.limit,)) and all(type(v) is int for v in d.shift + (d.n, d.cap, d.bits))
            hi, lo = max(abs(s) for s in d.scale), min(abs(s) for s in d.scale)
            f, e = math.frexp(hi)
            assert 0.5 < f < 1.0 and G.E_MIN <= e <= G.E_MAX and e == g.e, "never a power of two"
            assert any(lo == hi * r for r in G.RATIOS)
            assert W.words_for_scale(hi) <= d.n <= 16 and 1 <= d.width <= 48 and 1 <= d.height <= 40
            assert d.cap in G.CAPS and d.limit in G.LIMITS and d.bits in G.BITS
            a, b, k = d.shift
            assert (a, b, k) == (0, 0, 0) or (max(abs(a), abs(b)) <= 4 and e <= k <= e + 5)
            assert g.wide == (e <= G.E_WIDE) and g.roads[-1] == "scaled"
            assert g.julia == (d.centre == "J" or d.julia_set is not None)
            seen["centre"].add(d.centre)
            seen["ratio1"] += lo == hi
            seen["n_min"] += d.n == W.words_for_scale(hi)
            seen["constant"] += d.julia_set is not None
            for key in ("limit", "cap", "bits"):
                seen[key].add(getattr(d, key))
    assert seen["centre"] == {"M", "N", "J", "MINI", "F"} and seen["limit"] == set(G.LIMITS) and seen["bits"] == set(G.BITS)
    assert seen["cap"] == set(G.CAPS) and 0 < seen["ratio1"] < count and count // 4 <= seen["n_min"] <= 3 * count // 4
    assert seen["constant"] >= 1


def test_the_edge_views_stand_where_they_say():
    e = {name: G.edge(name) for name in G.EDGES}
    assert max(abs(s) for s in e["below_2^440"].draw.scale) == math.nextafter(2.0 ** 440, 0.0) and e["below_2^440"].wide
    assert e["e_951"].e == 951 and e["e_951"].n == 16
    lo, hi = sorted(abs(s) for s in e["ratio_2^-32"].draw.scale)
    assert lo == hi * 2.0 ** -32
    for name in ("F_e+64_n8", "F_e+64_n3"):
        assert W.frac_bits(e[name].n) == e[name].e + 64
    assert e["F_e+64_n8"].wide and e["F_e+64_n8"].e == 440
    assert e["n16_e70"].n == 16 and e["n16_e70"].e == 70 and W.words_for_scale(e["n16_e70"].draw.scale[0]) == 3
    assert e["limit_2^20"].draw.limit == e["limit_2^20_J"].draw.limit == 2.0 ** 20
    assert {(1, 1), (1, 17), (17, 1), (33, 31), (31, 33)} <= {(g.draw.width, g.draw.height) for g in e.values()}
    for name, special in (("on_a_pixel", "M"), ("on_a_pixel_J", "J")):
        g = e[name]
        ore, oim = g.v.offset(5, 3)
        f = 1 << W.frac_bits(g.n)
        cre, cim = S.centre_ints(special, g.n)
        assert (g.v.centre[0] + ore, g.v.centre[1] + oim) == (Fraction(cre, f), Fraction(cim, f)), "the special point IS pixel (5, 3)"


def test_the_edge_views_are_resolved_or_flat_as_meant(fr):
    for name, r in edges(fr).items():
        it = r.rows("scaled")[1]
        print("%s: %d distinct indices, %d pixels at the cap, orbit of %d entries%s" % (
            name, len(np.unique(it)), int((it == r.g.cap).sum()), len(r.x), ", ended by escape" if r.ended else ""))
    e = edges(fr)
    out = e["outside"]
    assert out.orbits.x[1] and len(out.x) <= 8 and out.g.cap == 3000, "a reference orbit ended by escape within a few entries"
    assert int(out.rows("scaled")[3].sum()) >= out.g.shape[0] * out.g.shape[1], "every pixel outlives the orbit and rebases at its end"
    for name in ("below_2^440", "e_951", "n16_e70", "limit_2^20", "limit_2^20_J", "on_a_pixel", "on_a_pixel_J"):
        assert e[name].resolved, name


# ---- 2. the generated set is worth running ------------------------------------------------------------------------------------------


def test_the_generated_set_meets_its_conditions(fr):
    all_runs = runs(fr)
    capped = [r for r in all_runs.values() if r.g.cap >= G.RESOLVED_CAP]
    resolved = [r for r in capped if r.resolved]
    at_cap = [r for r in resolved if (r.rows("scaled")[1] == r.g.cap).any()]
    print("views %d, with cap >= %d: %d, resolved: %d, of them with pixels at the cap: %d" % (
        len(all_runs), G.RESOLVED_CAP, len(capped), len(resolved), len(at_cap)))
    assert 2 * len(resolved) >= len(capped)
    assert 4 * len(at_cap) >= len(resolved)
    kinds = {
        "Julia": lambda g: g.julia,
        "a negative axis": lambda g: min(g.draw.scale) < 0,
        "unequal axes": lambda g: abs(g.draw.scale[0]) != abs(g.draw.scale[1]),
        "n above the minimum": lambda g: g.n > W.words_for_scale(max(abs(s) for s in g.draw.scale)),
        "zero shift": lambda g: g.draw.shift == (0, 0, 0),
        "inside 2^440": lambda g: g.wide,
        "past 2^440": lambda g: not g.wide,
    }
    for what, f in kinds.items():
        n = sum(1 for r in resolved if f(r.g))
        print("resolved and %s: %d" % (what, n))
        assert n >= 3, what
    skips = rebases = ended = 0
    for r in resolved:
        z, it, passes, reb = r.rows("scaled", r.g.table_bits)
        skips += int(passes.astype(np.uint64).sum()) < S.steps(r.cfg, it)
        rebases += bool(reb.any())
        ended += r.ended
    print("table runs on resolved views %d: with skips %d, with rebases %d, on an orbit ended by escape %d" % (
        len(resolved), skips, rebases, ended))
    assert 4 * skips >= 3 * len(resolved) and 2 * rebases >= len(resolved) and ended >= 5


# ---- 3. the common domain: the header's claims on the models ------------------------------------------------------------------------


def test_in_the_common_domain_the_scaled_models_are_the_unscaled_ones(fr):
    checked = subnormal = 0
    for r in list(runs(fr).values()) + list(edges(fr).values()):
        if not r.g.wide:
            continue
        what = r.g.describe(r.cfg)
        wide, scaled = r.rows("wide"), r.rows("scaled")
        assert np.array_equal(wide[1], scaled[1]) and S.same_bits(wide[0], scaled[0]), "CLAIM, bits -1: " + what
        bits = r.g.table_bits
        bla, table = r.rows("bla", bits), r.rows("scaled", bits)
        assert np.array_equal(bla[1], table[1]) and S.same_bits(bla[0], table[0]), "CLAIM, bits %d: %s" % (bits, what)
        de, de_wide = r.rows("de"), r.rows("de_wide")
        assert np.array_equal(de[1], de_wide[1]) and S.same_bits(de[0], de_wide[0]), "DE CLAIM 1: " + what
        checked += 1
        if de[5][2]:  # CLAIM 2 is about runs without a subnormal intermediate: u = d 2^-e of an interior pixel whose derivative dies
            subnormal += 1
            continue
        assert D.same_doubles(np.ldexp(de[2], r.g.e), de_wide[2]), "DE CLAIM 2, u 2^e is the wide derivative: " + what
        view = M.scaled_view(r.cfg)
        assert D.same_doubles(D.distance(view, *de[:3]), D.distance(r.cfg, *de_wide)), "DE CLAIM 2, the distances: " + what
    print("common-domain views checked: %d, of them with a subnormal u (CLAIM 2 does not apply): %d" % (checked, subnormal))
    assert checked >= len(G.SEEDS) and 4 * subnormal <= checked


# ---- 4. the truth spot check --------------------------------------------------------------------------------------------------------


def exact_pixel(g, x, y):
    """(iters, z, settled, move, u) of a pixel, or None where P and P + 320 disagree in any returned value"""
    v = g.v
    a, b = v.pixel(x, y), v.pixel(x, y, T.EXTRA)
    ua, ub = U.pixel(v, x, y), U.pixel(v, x, y, T.EXTRA)
    if a != b or ua != ub:
        return None
    assert ua[0] == a[0]
    return a + (ua[1],)


MODELS = [("wide", -1), ("bla", 40), ("bla", 53), ("scaled", -1), ("scaled", 40), ("scaled", 53)]


def test_the_models_follow_exact_orbits_on_sampled_pixels_of_the_generated_views(fr):
    sampled = compared = d_compared = 0
    worst_excess = {bits: (-math.inf, None) for bits in (-1, 40, 53)}
    worst_d, worst_where = {-1: 0.0, 40: 0.0, 53: 0.0}, {}
    off24 = 0
    for (seed, k), r in runs(fr).items():
        if not r.resolved:
            continue
        g = r.g
        what = g.describe(r.cfg)
        pixels = G.pixels(seed, k, g)
        view = M.scaled_view(r.cfg)
        here = 0
        for x, y in pixels:
            t = exact_pixel(g, x, y)
            if t is None or not t[2]:
                continue
            it, z, _, move, u = t
            here += 1
            for mode, bits in MODELS:
                if mode not in g.roads:
                    continue
                mz, mit = r.rows(mode, bits)[:2]
                assert int(mit[y, x]) == it, "%s bits %d, pixel (%d, %d): index %d, exact %d; %s" % (mode, bits, x, y, mit[y, x], it, what)
                err = max(abs(float(mz[y, x, 0]) - z[0]), abs(float(mz[y, x, 1]) - z[1]))
                excess = (err - move) / max(math.hypot(*z), 1.0)
                if excess > worst_excess[bits][0]:
                    worst_excess[bits] = (excess, "%s bits %d, pixel (%d, %d); %s" % (mode, bits, x, y, what))
            for mode in ("bla", "scaled"):
                if mode in g.roads:
                    off24 += int(r.rows(mode, 24)[1][y, x]) != it
            if it >= g.cap:
                continue
            one = np.array([it], dtype=np.uint32)
            exact_d = float(D.distance(view, np.array([z]), one, np.array([u]))[0])
            if not (exact_d >= U.MIN_D and math.isfinite(exact_d)):
                continue
            d_compared += 1
            for bits in (-1, 40, 53):
                mz, mit, mu = r.rows("de", bits)[:3]
                got = float(D.distance(view, mz[y:y + 1, x], one, mu[y:y + 1, x])[0])
                err = abs(got - exact_d) / exact_d
                if err > worst_d[bits]:
                    worst_d[bits], worst_where[bits] = err, "%s pixel (%d, %d)" % (g.label, x, y)
                assert err <= U.D_TOLERANCE[bits], "DE bits %d, pixel (%d, %d): D is %.3g off the exact D (relative); %s" % (
                    bits, x, y, err, what)
        print("%s: %d of %d sampled pixels compared" % (g.label, here, len(pixels)))
        assert here >= 0.3 * len(pixels), "fewer than 30 %% of the sampled pixels compared: " + what
        sampled += len(pixels)
        compared += here
    print("sampled pixels %d, compared %d (%.1f %%), with a distance %d" % (sampled, compared, 100.0 * compared / sampled, d_compared))
    for bits, (excess, where) in worst_excess.items():
        print("bits %d: largest excess %r of the floor %r at %s" % (bits, excess, T.z_floor(bits), where))
        assert excess <= T.z_floor(bits), "z is %.3g max(|z|, 1) past the exact z's own movement: %s" % (excess, where)
    # the floor of a table at 40 bits is 4 times what is measured here, rounded up to a power of two; the others stay under Z_FLOOR
    assert 0 < worst_excess[40][0] <= T.Z_EXCESS_MEASURED_40 and "seed 10 view 1" in worst_excess[40][1]
    assert T.Z_FLOOR_40 == 2.0 ** math.ceil(math.log2(4 * T.Z_EXCESS_MEASURED_40))
    print("largest relative error of D per bits: %r at %r; tolerances %r" % (worst_d, worst_where, U.D_TOLERANCE))
    print("bits 24 (printed, not asserted): off the exact index on %d model pixels" % off24)
    assert compared >= 0.6 * sampled and d_compared >= 20


# ---- 5. the dd-centre views of the GPU file -----------------------------------------------------------------------------------------


def test_half_of_the_dd_centre_views_lie_inside_each_calls_domain(fr):
    from test_gpu_deep_edges import random_config

    total, inside = 0, {"bla": 0, "de_pt": 0, "de_f64": 0}
    for seed in G.SEEDS:
        rng = np.random.default_rng(G.DD_BASE_SEED + seed)
        for _ in range(G.DD_PER_SEED):
            cfg, lo = random_config(fr, rng)
            total += 1
            for call in inside:
                inside[call] += G.dd_domain(cfg, call)
    print("dd-centre views %d, inside the domain: %r" % (total, inside))
    for call in ("bla", "de_pt"):
        assert 2 * inside[call] >= total, call
    assert inside["de_f64"] >= 3
