"""The views of tests/deep_ss_views.py on the host models alone, without a device: conditions on the INPUTS of
tests/test_gpu_deep_ss_random.py and tests/test_gpu_adaptive_f64_random.py, so that the GPU files cannot pass on flat images and a
later edit of the generator cannot hollow them out unnoticed.  The counts are printed with -s; DESIGN.md §3.29 records them.
  - what a view gains is deterministic and lies inside the stated ranges; every s of S_VALUES occurs; every view of EXTRA is mixed;
  - MIXED views (the view's tau gives an edge share in [0.05, 0.95] and an edge pixel has F != P): a quarter of the views; among
    them three each that are Julia, have a negative axis, unequal axes, lie inside 2^440, past it, are wider than one 32-pixel mark
    tile, have `smooth` off; every s on one of them;
  - a third of the views have F != P somewhere, a third are shaded by their thickness on cfg_s, a third have pixels finished
    before the band split N and pixels escaping after it, eight of those have capped pixels too;
  - six WRONG VARIANTS of the definitions, written on top of the models' arrays, each seen on at least five views;
  - the models of cfg_s agree where §3.25's CLAIMs say they must, and ss_adaptive_model.adaptive at -1 and 255 is the filter and
    the probe;
  - the same floors for the F64 records of tests/shallow_random_views.py that the adaptive F64 file runs."""
import numpy as np
import pytest

import bla_model as B
import de_model as D
import de_scaled_model as M
import deep_random_views as G
import deep_ss_views as V
import pt_scaled_model as S
import pt_wide_model as W
import ss_adaptive_model as A
import ss_de_model as SS
import test_gpu_deep_edges as E


@pytest.fixture(scope="module")
def views():
    return V.everything()


# ---- 1. what a view gains ------------------------------------------------------------------------------------------------------------


def test_what_a_view_gains_is_deterministic_and_in_range(views):
    assert len(views) == 3 * len(G.SEEDS) + len(V.EXTRA) + len(G.EDGES)
    assert [v.key for v in V.all_of(3)] == [(3, 0), (3, 1), (3, 2)]
    V.all_of.cache_clear()
    again = {v.key: (v.s, v.piece, v.a) for v in V.all_of(3)}
    assert again == {v.key: (v.s, v.piece, v.a) for v in views if v.key in again}
    for v in views:
        d = v.g.draw
        assert v.s in V.S_VALUES and (v.s == 2 or v.s * v.s * d.width * d.height * max(d.cap, 1) <= V.WORK), v.key
        assert 0 <= v.piece[0] < v.piece[1] <= v.h and (v.a is None) == (v.h < 3) and (v.a is None or 1 <= v.a <= v.h - 2)
        assert (v.cfg_s.width, v.cfg_s.height, v.cfg_s.iterations) == (v.s * d.width, v.s * d.height, d.cap)
        assert 0 <= v.tau <= 255 and 0.0 < v.thickness * v.s <= V.DE_MAX
        n = v.split
        it = v.plain()[1]
        assert (n is None) == (d.cap < 2 or not (it < d.cap).any()) and (n is None or 1 <= n <= d.cap - 1), v.key
    assert {V.edge(name).s for name in G.EDGES} == set(V.S_VALUES), "the edge views' fixed s cover all six values"
    assert {v.s for v in views if not isinstance(v.key, str)} == set(V.S_VALUES)
    assert all(seed >= len(G.SEEDS) and 0 <= k < G.PER_SEED for seed, k in V.EXTRA)
    for v in views:
        if v.key in V.EXTRA:
            assert v.mixed, "an added view that the models do not call mixed: %r" % (v.key,)


def test_the_colour_map_is_the_deep_edge_tests_soft_colours(views):
    for v in views[::7] + [V.edge("1x1")]:
        z, it = v.scaled()[:2]
        assert np.array_equal(v.image(), E.soft_colours(v.cfg_s, z, it)), v.key
    fern = V.config_s(views[0].cfg, 1)
    fern.algo = 1
    z, it = views[0].plain()[:2]
    assert np.array_equal(V.soft_colours(fern, z, it), E.soft_colours(fern, z, it)) and not V.soft_colours(fern, z, it).any()


def test_tau_is_the_median_of_the_neighbour_differences():
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, (12, 15, 3), dtype=np.uint8)
    for tau in (0, 17, 100, 254):
        assert np.array_equal(V.neighbour_difference(A.probe(big, 3)) > tau, A.edges(big, 3, tau))
    d = V.neighbour_difference(A.probe(big, 3))
    tau = V.median_tau(big, 3)
    assert tau in d and all(abs((d > tau).mean() - 0.5) <= abs((d > v).mean() - 0.5) for v in np.unique(d))
    assert V.median_tau(np.full((6, 6, 3), 9, dtype=np.uint8), 2) == 0 and V.median_tau(big[:3, :3], 3) == 0


# ---- 2. the conditions ----------------------------------------------------------------------------------------------------------------

KINDS = {
    "Julia": lambda v: v.g.julia,
    "a negative axis": lambda v: min(v.g.draw.scale) < 0,
    "unequal axes": lambda v: abs(v.g.draw.scale[0]) != abs(v.g.draw.scale[1]),
    "inside 2^440": lambda v: v.g.wide,
    "past 2^440": lambda v: not v.g.wide,
    "wider than 32": lambda v: v.w > 32,
    "smooth off": lambda v: not v.g.draw.look.smooth,
}


def differs_somewhere(v):
    return bool((A.np_filter(v.image(), v.s) != A.probe(v.image(), v.s)).any())


def shaded(v):
    """a byte of the supersampled DE image of cfg_s at the view's thickness differs from thickness 0"""
    z, it, u = v.de_scaled()[:3]
    cfg_v = M.scaled_view(v.cfg)
    return bool((SS.colour(cfg_v, z, it, u, v.s, v.thickness) != SS.colour(cfg_v, z, it, u, v.s, 0.0)).any())


def test_the_set_meets_its_conditions(views):
    mixed = [v for v in views if v.mixed]
    print("views %d (%d generated, %d added from seeds %s, %d edge), mixed %d" % (
        len(views), 3 * len(G.SEEDS), len(V.EXTRA), sorted({s for s, _ in V.EXTRA}), len(G.EDGES), len(mixed)))
    assert 4 * len(mixed) >= len(views)
    for what, f in KINDS.items():
        n = sum(1 for v in mixed if f(v))
        print("mixed and %s: %d" % (what, n))
        assert n >= 3, what
    by_s = {s: sum(1 for v in mixed if v.s == s) for s in V.S_VALUES}
    print("mixed views by s: %r; all views by s: %r" % (by_s, {s: sum(1 for v in views if v.s == s) for s in V.S_VALUES}))
    assert all(n >= 1 for n in by_s.values()), by_s
    differ = sum(differs_somewhere(v) for v in views)
    shade = sum(shaded(v) for v in views)
    print("F != P somewhere: %d; shaded by their thickness: %d" % (differ, shade))
    assert 3 * differ >= len(views) and 3 * shade >= len(views)
    classes = [v.split_classes() for v in views]
    both = [c for c in classes if c is not None and c[0] > 0 and c[1] > 0]
    capped = [c for c in both if c[2] > 0]
    print("band splits: %d views have one, %d with pixels finished before N and pixels escaping after it, %d of those with capped pixels" % (
        sum(c is not None for c in classes), len(both), len(capped)))
    assert 3 * len(both) >= len(views) and len(capped) >= 8
    pixels = sum(v.h * v.w for v in views)
    samples = sum(v.h * v.w * v.s * v.s for v in views)
    print("output pixels %d, samples of cfg_s %d; inside 2^440: %d views, %d pixels, %d samples" % (
        pixels, samples, sum(v.g.wide for v in views), sum(v.h * v.w for v in views if v.g.wide),
        sum(v.h * v.w * v.s * v.s for v in views if v.g.wide)))


# ---- 3. the wrong variants ------------------------------------------------------------------------------------------------------------


def variant_probe_at_0_0(v):
    """the probe taken at sample (0, 0) instead of (p, p)"""
    big, s = v.image(), v.s
    P = big[0::s, 0::s]
    e = V.neighbour_difference(P) > v.tau
    return np.where(e[..., None], A.np_filter(big, s), P), int(e.sum())


def variant_four_neighbours(v):
    big, s = v.image(), v.s
    e = V.neighbour_difference(A.probe(big, s), neighbours=4) > v.tau
    return np.where(e[..., None], A.np_filter(big, s), A.probe(big, s)), int(e.sum())


def variant_no_rounding_term(v):
    """the filter without the floor(s * s / 2) term"""
    big, s = v.image(), v.s
    sums = big.reshape(v.h, s, v.w, s, 3).astype(np.uint32).sum(axis=(1, 3))
    e = A.edges(big, s, v.tau)
    return np.where(e[..., None], (sums // (s * s)).astype(np.uint8), A.probe(big, s)), int(e.sum())


def variant_swapped_axes(v):
    """the refine pass's samples with the axes' scales swapped; the probe pass is the right one"""
    cfg = V.config_s(v.cfg, v.s)
    cfg.scale.re, cfg.scale.im = v.cfg.scale.im, v.cfg.scale.re
    z, it = S.escape_rows(cfg, v.x, v.k, -1)[:2]
    wrong = V.soft_colours(cfg, z, it)
    big, s = v.image(), v.s
    e = A.edges(big, s, v.tau)
    return np.where(e[..., None], A.np_filter(wrong, s), A.probe(big, s)), int(e.sum())


def test_wrong_variants_of_the_adaptive_definition_are_seen(views):
    variants = {"the probe at sample (0, 0)": variant_probe_at_0_0, "4 neighbours for 8": variant_four_neighbours,
                "the filter without floor(s*s/2)": variant_no_rounding_term, "the refined samples with swapped axes": variant_swapped_axes}
    for what, f in variants.items():
        seen = 0
        for v in views:
            want, count = A.adaptive(v.image(), v.s, v.tau)
            got, n = f(v)
            seen += bool(n != count or not np.array_equal(got, want))
        print("%s: seen on %d views" % (what, seen))
        assert seen >= 5, what


def test_a_neighbourhood_cut_at_the_rows_of_the_call_is_seen(views):
    seen = tried = 0
    for v in views:
        if v.three_way() is None:
            continue
        tried += 1
        big, s = v.image(), v.s
        P, F = A.probe(big, s), A.np_filter(big, s)
        whole, count = A.adaptive(big, s, v.tau)
        parts, total = [], 0
        for y0, y1 in v.three_way():
            want, n = A.adaptive(big, s, v.tau, y0, y1)
            assert np.array_equal(want, whole[y0:y1])  # the definition: pieces are slices
            e = (V.neighbour_difference(P, y0=y0, y1=y1) > v.tau)[y0:y1]
            parts.append(np.where(e[..., None], F[y0:y1], P[y0:y1]))
            total += int(e.sum())
        seen += bool(total != count or not np.array_equal(np.concatenate(parts), whole))
    print("the neighbourhood cut at the call's rows: seen on %d of %d views with a three-way split" % (seen, tried))
    assert seen >= 5


def test_a_shade_at_thickness_instead_of_thickness_times_s_is_seen(views):
    seen = 0
    for v in views:
        z, it, u = v.de_scaled()[:3]
        cfg_v = M.scaled_view(v.cfg)
        want = SS.colour(cfg_v, z, it, u, v.s, v.thickness)
        wrong = SS.box(D.colour(SS.config_s(cfg_v, v.s), z, it, u, v.thickness, 3), v.s)
        seen += bool((want != wrong).any())
    print("the shade at thickness instead of thickness * s: seen on %d views" % seen)
    assert seen >= 5


# ---- 4. the models on cfg_s -----------------------------------------------------------------------------------------------------------


def test_the_models_of_cfg_s_agree_in_the_common_domain_and_the_adaptive_model_at_its_ends(views):
    checked = 0
    for v in views:
        big, s = v.image(), v.s
        out, n = A.adaptive(big, s, -1)
        assert np.array_equal(out, A.np_filter(big, s)) and n == v.h * v.w, v.key
        out, n = A.adaptive(big, s, 255)
        assert np.array_equal(out, A.probe(big, s)) and n == 0, v.key
        if not v.g.wide:
            continue
        what = v.describe()
        (z, it, _, _), _ = W.state_rows(v.cfg_s, v.orbits, rule=1)
        scaled = v.scaled(-1)
        assert np.array_equal(it, scaled[1]) and S.same_bits(z, scaled[0]), "CLAIM, bits -1, on cfg_s: " + what
        bits = v.g.table_bits
        bla, table = B.escape_rows(v.cfg_s, v.x, v.k, bits), v.scaled(bits)
        assert np.array_equal(bla[1], table[1]) and S.same_bits(bla[0], table[0]), "CLAIM, bits %d, on cfg_s: %s" % (bits, what)
        de, de_wide = v.de_scaled(), D.pt_wide_rows(v.cfg_s, v.orbits)
        assert np.array_equal(de[1], de_wide[1]) and S.same_bits(de[0], de_wide[0]), "DE CLAIM 1 on cfg_s: " + what
        checked += 1
    print("common-domain views checked on cfg_s: %d" % checked)
    assert checked >= len(G.SEEDS)


# ---- 5. the F64 records of the adaptive F64 file ----------------------------------------------------------------------------------------

F64_KINDS = {
    "scale.re < 0": lambda c: c.scale.re < 0,
    "scale.im < 0": lambda c: c.scale.im < 0,
    "unequal axes": lambda c: abs(c.scale.re) != abs(c.scale.im),
    "Julia": lambda c: c.algo == 2,
    "smooth off": lambda c: not c.smooth,
    "stable_limit 0": lambda c: c.stable_limit == 0.0,
    "a limit other than 65536": lambda c: c.limit != 65536.0,
}


def test_the_f64_records_meet_the_same_floors():
    records = V.f64_records()
    mixed = [r for r in records if V.f64_mixed(r)[1]]
    print("F64 records %d, mixed %d, by s %r" % (len(records), len(mixed), {s: sum(1 for r in mixed if r.s == s) for s in range(1, 9)}))
    assert 4 * len(mixed) >= len(records)
    for what, f in F64_KINDS.items():
        n = sum(1 for r in mixed if f(r.cfg))
        print("mixed and %s: %d" % (what, n))
        assert n >= 3, what
    assert any(r.cfg.algo == 1 for r in records), "algo = 1 is included"
    assert {r.s for r in mixed} >= {2, 3, 4, 5, 7, 8}
