"""The generated and edge records of tests/shallow_random_views.py on the host models alone — no device and no library call: conditions
on the INPUTS of tests/test_gpu_shallow_random.py, so that a later edit of the generator cannot hollow the GPU tests out unnoticed.
The counts are printed (pytest -s); what the set gives today stands beside each floor.
  - the generator is deterministic, draws what its header says, and a failure message rebuilds its record;
  - floors over the 120 F64 / F32 records of the GPU file's seeds, a "counted view" having cap >= 64 and at least 64 pixels (87):
      counted views with escaped and capped pixels                        at least a third     36 of 87
      counted views with at least three distinct escape indices           at least a half      59 of 87
      views whose shading at the median-D thickness changes a byte against thickness 0
                                                                          at least a quarter   62 of 120
      cap-chain links with all three classes of de_extend_cases.classes   at least ten         37 of 367
    and over all 150 records (30 of them DD) at least six each with: scale.re < 0 (48), scale.im < 0 (50), unequal |scale| axes
    (75), smooth = 0 (46), inside = 0 (45), stable_limit = 0 (22), exposure < 0 (28), Julia (59), F32 (26), DD (30), and each size
    of the fixed list (7 to 10);
  - teeth: three deliberately wrong variants, written here on top of the models' arrays, are each seen on at least ten views:
      (a) the derivative's t taken from the position after the step    50 of the 52 DE records with orbits and cap <= 1000
      (b) D formed with max(|scale.re|, |scale.im|)                     33 of 86 DE records
      (c) the shaded byte rounded to nearest instead of truncated      42 of 86 DE records
    (a) restates the F64 step in numpy, whose products are not fused: its z and iters are asserted bit for bit against the model,
    its derivative within 1e-9 |d| (1.3e-13 is the most), and a pixel counts as seen where the variant is more than 1e-6 |d| off
    the model's; (c) restates the shading in numpy and is asserted byte for byte against the model before its rounding is changed;
    no generated record reaches a non-finite derivative (0 of 86), which is why the overflow record is in the edge list;
  - the edge records stand where they say, and the overflow record's chain passes a finite derivative whose square overflows,
    (-inf, -inf) and (NaN, NaN), with D = 0."""
import math

import numpy as np

import de_extend_cases as DX
import de_model as D
import oracle_lib as O
import shallow_random_views as G

COUNTED_CAP, COUNTED_PIXELS = 64, 64


class Run:
    """a record with the models' arrays at its last cap, each computed once"""

    def __init__(self, rec):
        self.rec, self.cfg = rec, rec.cfg
        self._it, self._de = {}, None

    def iters(self, cap=None):
        """the oracle's escape indices at a cap of the chain, at the record's precision"""
        cap = self.cfg.iterations if cap is None else cap
        if cap not in self._it:
            self._it[cap] = O.escape_rows(self.rec.cfg_at(cap), self.rec.precision, threads=D.THREADS)[1]
        return self._it[cap]

    @property
    def in_de_domain(self):
        return self.cfg.limit <= G.DE_MAX

    def de(self):
        """(z, iters, der, D) of tests/de_model.py's F64 road"""
        if self._de is None:
            z, it, der = D.f64_rows(self.cfg)
            self._de = z, it, der, D.distance(self.cfg, z, it, der)
        return self._de

    @property
    def counted(self):
        return self.cfg.iterations >= COUNTED_CAP and self.cfg.width * self.cfg.height >= COUNTED_PIXELS


_runs = []


def runs():
    """a Run of every F64 / F32 record of the GPU file's seeds"""
    if not _runs:
        _runs.extend(Run(r) for seed in G.SEEDS for r in G.records(seed))
    return _runs


def de_runs():
    return [r for r in runs() if r.rec.de]


def all_records():
    return [r for seed in G.SEEDS for r in G.records(seed) + G.dd_records(seed)]


# ---- 1. the generator -------------------------------------------------------------------------------------------------------------


def test_a_seed_gives_the_same_records_every_time():
    for seed in (0, 11, 29):
        rng_a, rng_b = (np.random.default_rng(G.BASE_SEED + seed) for _ in range(2))
        a, b = [G.draw(rng_a, fixed=seed) for _ in range(2)], [G.draw(rng_b, fixed=seed) for _ in range(2)]
        assert [r.describe() for r in a] == [r.describe() for r in b]
        assert a[0].describe().split(": ", 1)[1] == G.records(seed)[0].describe().split(": ", 1)[1]
    assert bytes(G.records(0)[0].cfg) != bytes(G.records(1)[0].cfg)


def test_the_draws_lie_inside_the_stated_ranges():
    seen = {"cap": set(), "limit": set(), "s": set(), "algo": set(), "links": set()}
    for rec in all_records():
        cfg = rec.cfg
        assert 1 <= cfg.width <= 79 and 1 <= cfg.height <= 59 and 1 <= rec.s <= 8
        assert 2 <= len(rec.chain) - 1 <= 4 and set(rec.chain) <= set(G.CAPS) and rec.chain[-1] == cfg.iterations
        assert 0 <= rec.split[0] < rec.split[1] <= cfg.height and 0 <= rec.piece < len(rec.chain) - 1
        work = G.WORK_DD if rec.precision == G.DD else G.WORK
        assert rec.s == 1 or rec.s * rec.s * cfg.width * cfg.height * max(cfg.iterations, 1) <= work
        seen["links"].add(len(rec.chain) - 1)
        if rec.precision == G.DD:
            assert G.dd_domain(cfg, rec.pos_lo) and rec.z_width == 4 and not rec.de and rec.s <= 3
            continue
        hi, lo = max(abs(cfg.scale.re), abs(cfg.scale.im)), min(abs(cfg.scale.re), abs(cfg.scale.im))
        assert any(math.frexp(v)[0] * 2.0 ** 53 % 2 == 1 for v in (abs(cfg.scale.re), abs(cfg.scale.im))), "an odd mantissa"
        assert 10.0 ** -0.5 / 2 <= hi <= 1.9e9 * 2 and (rec.precision == G.F64 or hi <= 1.9e4 * 2)
        assert cfg.limit in G.LIMITS + G.PLAIN_LIMITS and cfg.stable_limit in G.STABLE_LIMITS and cfg.exposure in G.EXPOSURES
        assert rec.de == (rec.precision == G.F64 and cfg.limit <= G.DE_MAX) and (rec.thickness is not None) == rec.de
        assert not rec.de or 0.0 < rec.thickness <= G.DE_MAX / rec.s
        assert rec.tile in G.TILES and rec.loop_mode in G.LOOP_MODES
        seen["cap"].update(rec.chain)
        seen["limit"].add(cfg.limit)
        seen["s"].add(rec.s)
        seen["algo"].add(cfg.algo)
    assert seen["cap"] == set(G.CAPS) and seen["limit"] == set(G.LIMITS + G.PLAIN_LIMITS) and seen["s"] == set(range(1, 9))
    assert seen["algo"] == {0, 1, 2} and seen["links"] == {2, 3, 4}


def test_julia_records_stand_on_the_repelling_fixed_point():
    for c in G.JULIA_CONSTANTS:
        p = G.fixed_point(c)
        assert abs(p * p + complex(*c) - p) < 1e-15 and abs(2 * p) >= 1.0, c
    n = 0
    for r in runs():
        cfg = r.cfg
        if cfg.algo != O.JULIA:
            continue
        p = G.fixed_point((cfg.julia_set.re, cfg.julia_set.im))
        assert abs(cfg.pos.re - p.real) <= 0.35 / abs(cfg.scale.re) and abs(cfg.pos.im - p.imag) <= 0.35 / abs(cfg.scale.im)
        n += 1
    assert n >= 6


def test_a_failure_message_rebuilds_its_record():
    for rec in [G.records(3)[1], G.dd_records(5)[0], G.edge("overflow"), G.edge("Ts_2^20")]:
        text = rec.describe()
        expr = text.split(": ", 1)[1]
        back = eval(expr, {"shallow_random_views": G})  # noqa: S307 - the message is this file's own
        assert bytes(back.cfg) == bytes(rec.cfg) and back.describe().split(": ", 1)[1] == expr
        assert (back.precision, back.chain, back.piece, back.split, back.s, back.thickness, back.de, back.tile, back.loop_mode, back.host,
                back.pos_lo) == (rec.precision, rec.chain, rec.piece, rec.split, rec.s, rec.thickness, rec.de, rec.tile, rec.loop_mode,
                                 rec.host, rec.pos_lo)


# ---- 2. the floors -----------------------------------------------------------------------------------------------------------------


def test_counted_views_hold_escaped_and_capped_pixels_and_several_indices():
    counted = [r for r in runs() if r.counted]
    both = [r for r in counted if (r.iters() < r.cfg.iterations).any() and (r.iters() == r.cfg.iterations).any()]
    three = [r for r in counted if len(np.unique(r.iters())) >= 3]
    print("records %d, counted (cap >= %d, >= %d pixels) %d: with escaped and capped pixels %d, with >= 3 distinct indices %d" % (
        len(runs()), COUNTED_CAP, COUNTED_PIXELS, len(counted), len(both), len(three)))
    assert len(runs()) == 120 and len(counted) >= 60
    assert 3 * len(both) >= len(counted)
    assert 2 * len(three) >= len(counted)


def shaded_pair(r, thickness):
    z, it, der, _ = r.de()
    return D.colour(r.cfg, z, it, der, thickness), D.colour(r.cfg, z, it, der, 0.0)


def test_shading_changes_a_byte_on_a_quarter_of_the_views():
    changed = 0
    for r in runs():
        if not r.in_de_domain:
            continue  # a limit past 2^20: no DE, nothing shaded
        t = r.rec.thickness if r.rec.de else G.median_thickness(r.cfg, r.rec.s)  # F32 records: the same rule on the F64 model
        assert 0.0 < t <= G.DE_MAX / r.rec.s
        shaded, plain = shaded_pair(r, t)
        changed += not np.array_equal(shaded, plain)
    print("views whose shading at the median-D thickness changes a byte against thickness 0: %d of %d" % (changed, len(runs())))
    assert 4 * changed >= len(runs())


def test_every_kind_of_record_is_drawn_at_least_six_times():
    recs = all_records()
    kinds = {
        "scale.re < 0": lambda r: r.cfg.scale.re < 0,
        "scale.im < 0": lambda r: r.cfg.scale.im < 0,
        "unequal |scale| axes": lambda r: abs(r.cfg.scale.re) != abs(r.cfg.scale.im),
        "smooth = 0": lambda r: r.cfg.smooth == 0,
        "inside = 0": lambda r: r.cfg.inside == 0,
        "stable_limit = 0": lambda r: r.cfg.stable_limit == 0.0,
        "exposure < 0": lambda r: r.cfg.exposure < 0,
        "Julia": lambda r: r.cfg.algo == O.JULIA,
        "F32": lambda r: r.precision == G.F32,
        "DD": lambda r: r.precision == G.DD,
    }
    for w, h in G.FIXED_SIZES:
        kinds["%d x %d" % (w, h)] = lambda r, w=w, h=h: (r.cfg.width, r.cfg.height) == (w, h)
    print("records in all: %d" % len(recs))
    for what, f in kinds.items():
        n = sum(1 for r in recs if f(r))
        print("  %s: %d" % (what, n))
        assert n >= 6, what


def test_ten_links_hold_all_three_classes():
    links = full = 0
    for r in runs():
        for n, m in r.rec.links():
            links += 1
            full += min(DX.classes(r.iters(m), n, m)) > 0
    print("cap-chain links %d, with pixels finished before, escaping within and still capped: %d" % (links, full))
    assert full >= 10


# ---- 3. teeth ----------------------------------------------------------------------------------------------------------------------


def numpy_f64_de(cfg, t_after):
    """DE's F64 step restated in numpy (products and sums rounded one by one: no fma) -> (z, iters, der); t_after: the WRONG
    variant (a), the derivative's t = 2 z taken from the position after the step"""
    h, w = cfg.height, cfg.width
    with np.errstate(all="ignore"):
        x, y = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
        re0 = ((x / float(h)) - ((float(w) / float(h)) / 2.0)) / cfg.scale.re + cfg.pos.re
        im0 = ((y / float(h)) - 0.5) / cfg.scale.im + cfg.pos.im
        zr, zi = np.broadcast_to(re0, (h, w)).reshape(-1).copy(), np.broadcast_to(im0[:, None], (h, w)).reshape(-1).copy()
        julia = cfg.algo == O.JULIA
        cr = np.full(h * w, cfg.julia_set.re) if julia else zr.copy()
        ci = np.full(h * w, cfg.julia_set.im) if julia else zi.copy()
        b0 = 0.0 if julia else 1.0
        dr, di = np.ones(h * w), np.zeros(h * w)
        it = np.full(h * w, cfg.iterations, dtype=np.uint32)
        act = np.arange(h * w)
        squared = cfg.limit * cfg.limit
        for i in range(cfg.iterations):
            if act.size == 0:
                break
            a, b = zr[act], zi[act]
            nr, ni = ((a * a) - (b * b)) + cr[act], ((2.0 * a) * b) + ci[act]
            tr, ti = (nr + nr, ni + ni) if t_after else (a + a, b + b)
            pr, pi = dr[act], di[act]
            zr[act], zi[act] = nr, ni
            dr[act], di[act] = tr * pr + (-ti * pi + b0), tr * pi + ti * pr
            esc = nr * nr + ni * ni > squared
            it[act[esc]] = i
            act = act[~esc]
    return np.stack([zr, zi], -1).reshape(h, w, 2), it.reshape(h, w), np.stack([dr, di], -1).reshape(h, w, 2)


def off_by(der, model):
    """per pixel: |der - model| / |model| as complex numbers where both are finite; inf where only one of them is"""
    with np.errstate(all="ignore"):
        fa, fb = np.isfinite(der).all(-1), np.isfinite(model).all(-1)
        diff = np.hypot(der[..., 0] - model[..., 0], der[..., 1] - model[..., 1]) / np.hypot(model[..., 0], model[..., 1])
    out = np.where(fa & fb, np.nan_to_num(diff, nan=0.0), 0.0)  # 0 / 0: both derivatives are 0
    out[fa != fb] = np.inf
    return out


def test_teeth_a_the_derivative_taken_from_the_position_after_the_step():
    seen = tried = 0
    worst = 0.0
    for r in de_runs():
        if r.cfg.iterations > 1000 or r.cfg.algo == O.BARNSLEY_FERN:
            continue
        tried += 1
        z, it, der, _ = r.de()
        nz, nit, nder = numpy_f64_de(r.cfg, False)
        assert np.array_equal(nit, it) and D.same_doubles(nz, z), "the numpy restatement is not the model: " + r.rec.describe()
        worst = max(worst, float(off_by(nder, der).max()))
        wz, wit, wder = numpy_f64_de(r.cfg, True)
        assert np.array_equal(wit, it) and D.same_doubles(wz, z)
        seen += bool((off_by(wder, der) > 1e-6).any())
    print("teeth (a), t from the position after the step: seen on %d of %d DE records with orbits and cap <= 1000; the restatement without fma "
          "is at most %.3g |d| off the model" % (seen, tried, worst))
    assert worst <= 1e-9
    assert seen >= 10


def test_teeth_b_the_distance_formed_with_the_larger_axis():
    seen = 0
    for r in de_runs():
        z, it, der, dist = r.de()
        wrong = r.rec.cfg_at(r.cfg.iterations)
        big = max(abs(wrong.scale.re), abs(wrong.scale.im))
        wrong.scale = O.Imaginary(big, big)  # min(|re|, |im|) of it is the max of the record's
        seen += not D.same_doubles(D.distance(wrong, z, it, der), dist)
    print("teeth (b), D with max(|scale.re|, |scale.im|): seen on %d of %d DE records" % (seen, len(de_runs())))
    assert seen >= 10


def test_teeth_c_the_shaded_byte_rounded_to_nearest():
    seen = 0
    for r in de_runs():
        z, it, der, dist = r.de()
        t = r.rec.thickness
        base = D.base_colours(r.cfg, z, it).astype(np.float64)
        with np.errstate(all="ignore"):
            s = dist / t
            mask = (it < r.cfg.iterations) & (t > 0.0) & (s < 1.0)
            scaled = base * np.where(mask, s, 1.0)[..., None]
        want = D.colour(r.cfg, z, it, der, t)
        assert np.array_equal(scaled.astype(np.uint8), want), "the numpy restatement of the shading is not the model's"
        seen += not np.array_equal(np.where(mask[..., None], np.floor(scaled + 0.5), scaled).astype(np.uint8), want)
    print("teeth (c), the shaded byte rounded to nearest: seen on %d of %d DE records" % (seen, len(de_runs())))
    assert seen >= 10


# ---- 4. the edge records -------------------------------------------------------------------------------------------------------------


def test_the_edge_records_stand_where_they_say():
    e = {name: G.edge(name) for name in G.EDGES}
    assert all(r.de and r.precision == G.F64 for r in e.values())
    assert e["limit_2^20"].cfg.limit == 2.0 ** 20
    assert e["thickness_0"].thickness == 0.0 and e["thickness_2^20"].thickness == 2.0 ** 20 and e["thickness_2^20"].s == 1
    assert e["Ts_2^20"].s > 1 and e["Ts_2^20"].thickness * e["Ts_2^20"].s == 2.0 ** 20
    assert e["caps_0_1_2"].chain == (0, 1, 2) and e["scale_re_0"].cfg.scale.re == 0.0
    assert e["stable_+inf"].cfg.stable_limit == math.inf and e["stable_-1"].cfg.stable_limit == -1.0
    assert {(r.cfg.width, r.cfg.height, r.s) for r in e.values()} >= {(65, 1, 8), (65, 1, 5), (1, 9, 8), (1, 9, 5)}
    # cap 0 is (start, 0, (1, 0)), and at limit 2 the first step already has escapes
    r = e["caps_0_1_2"]
    z, it, der = D.f64_rows(r.cfg_at(0))
    assert not it.any() and (der == [1.0, 0.0]).all() and D.same_doubles(z, O.escape_rows(r.cfg_at(0))[0])
    assert min(DX.classes(D.f64_rows(r.cfg_at(2))[1], 1, 2)) > 0
    # the overflow record: what the generated set does not reach
    r = e["overflow"]
    assert r.chain == (500, 820, 821, 1200)
    der = {cap: D.f64_rows(r.cfg_at(cap))[2] for cap in r.chain}
    with np.errstate(all="ignore"):
        dn2 = der[500][..., 0] * der[500][..., 0] + der[500][..., 1] * der[500][..., 1]
    assert np.isfinite(der[500]).all() and np.isinf(dn2).sum() == 1, "a finite derivative whose square overflows"
    assert np.isinf(der[820]).sum() == 2 and not np.isnan(der[820]).any(), "the link 820 -> 821 starts from an infinite derivative"
    assert np.isnan(der[821]).sum() == 2 and np.isnan(der[1200]).sum() == 2
    z, it, _ = D.f64_rows(r.cfg)
    assert (D.distance(r.cfg, z, it, der[1200])[np.isnan(der[1200]).any(-1)] == 0.0).all()
    # scale.re = 0: every start is +-inf or NaN on the real axis, and NaN among them
    r = e["scale_re_0"]
    z0 = O.escape_rows(r.cfg_at(0))[0]
    assert not np.isfinite(z0[..., 0]).any() and np.isnan(z0[..., 0]).any() and np.isinf(z0[..., 0]).any()
    assert D.same_doubles(D.f64_rows(r.cfg_at(0))[0], z0)
    # all or nothing in the stable class
    import view_stats_model as VS

    for name, stable in (("stable_+inf", True), ("stable_-1", False)):
        r = e[name]
        z, it = O.escape_rows(r.cfg)
        rec = VS.view_stats(z, it, r.cfg.iterations, r.cfg.stable_limit)
        assert rec["stable"] == (rec["n"] if stable else 0), name


def test_the_generated_set_reaches_no_non_finite_derivative():
    """which is why the overflow record is in the edge list"""
    n = sum(1 for r in de_runs() if not np.isfinite(r.de()[2]).all())
    print("generated DE records with a non-finite derivative: %d of %d" % (n, len(de_runs())))
