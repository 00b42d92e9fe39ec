"""The inputs of tests/ss_adaptive_de_views.py on the host models alone, without a device: conditions on the INPUTS of
tests/test_gpu_ss_adaptive_de_random.py and of the transfer-1 runs of tests/test_gpu_deep_ss_random.py and
tests/test_gpu_adaptive_f64_random.py, so that the GPU files cannot pass emptily and a later edit of a generator cannot hollow
them out unnoticed.  Every count is printed with -s; DESIGN.md §3.33 records them.
  - floors on the F64 DE records and on the wide views (WIDE PT's arrays; BLA-PT's are counted beside them): de_mixed inputs,
    per s and per kind; a near-only pixel with F != P; an escaped probe with D == 0; the byte and the sRGB filter differing at a
    refined pixel;
  - the same last floor for the plain adaptive call on every deep view and on the F64 records with orbits;
  - seven WRONG VARIANTS of the near rule, each changing the bytes or the count of adaptive_de on at least five inputs of a set;
  - the ends of the model on every input: t = -1, t = 255 with R = 0, row pieces."""
import numpy as np
import pytest

import de_model as D
import deep_ss_views as V
import ss_adaptive_de_model as M
import ss_adaptive_de_views as AV
import ss_adaptive_model as A
import ss_de_model as SD


@pytest.fixture(scope="module")
def f64():
    return AV.records()


@pytest.fixture(scope="module")
def wide():
    return AV.wide("de_wide")


@pytest.fixture(scope="module")
def wide_bla():
    return AV.wide("de_bla")


# ---- 1. the floors on the sets -----------------------------------------------------------------------------------------------------------

KINDS = {
    "scale.re < 0": lambda c: c.scale.re < 0,
    "scale.im < 0": lambda c: c.scale.im < 0,
    "unequal axes": lambda c: abs(c.scale.re) != abs(c.scale.im),
    "Julia": lambda c: c.algo == 2,
    "smooth off": lambda c: not c.smooth,
    "inside off": lambda c: not c.inside,
    "a limit other than 65536": lambda c: c.limit != 65536.0,
}


def near_only_differs(inp):
    e, n = inp.sets
    return bool(inp.orbits and (n & ~e & inp.differ).any())


def zero_distance(inp, fern=False):
    """an escaped probe with D == 0; fern: an algorithm without orbits counts as well (its arrays are zeros: iters 0 under any
    cap above 0, der 0, D = 0), though the call renders it black and never reaches the rule"""
    if not inp.orbits and not fern:
        return False
    dist, escaped = AV.probe_distance(inp.cfg, *inp.arrays, inp.s)
    return bool((escaped & (dist == 0.0)).any())


def transfers_differ(H, s, refined):
    """the byte and the sRGB box filter differ at a refined pixel"""
    return bool(((AV.srgb_filter(H, s) != SD.box(H, s)).any(axis=-1) & refined).any())


def de_transfers_differ(inp):
    if not inp.orbits or inp.s < 2:
        return False
    e, n = inp.sets
    return transfers_differ(inp.H, inp.s, e | n)


def by_s(inputs, values):
    return {s: sum(1 for i in inputs if i.s == s) for s in values}


def check_floors(name, inputs, size, mixed_floor, s_values, near_floor, srgb_floor):
    assert len(inputs) == size, (name, len(inputs))
    mixed = [i for i in inputs if i.de_mixed]
    print("%s: %d inputs, de_mixed %d, by s %r" % (name, len(inputs), len(mixed), by_s(mixed, s_values)))
    assert len(mixed) >= mixed_floor
    assert all(n >= 1 for n in by_s(mixed, s_values).values()), by_s(mixed, s_values)
    for what, f in KINDS.items():
        n = sum(1 for i in mixed if f(i.cfg))
        print("%s: de_mixed and %s: %d" % (name, what, n))
        assert n >= 3, (name, what)
    lonely = sum(near_only_differs(i) for i in inputs)
    print("%s: a near-only pixel with F != P: %d" % (name, lonely))
    assert lonely >= near_floor
    differ = [i for i in inputs if de_transfers_differ(i)]
    print("%s: the byte and the sRGB filter differ at a refined pixel: %d, by s %r" % (name, len(differ), by_s(differ, s_values)))
    assert len(differ) >= srgb_floor
    assert all(n >= 1 for s, n in by_s(differ, s_values).items() if s >= 2), by_s(differ, s_values)
    return mixed


def test_the_f64_records_meet_their_floors(f64):
    mixed = check_floors("F64 records", f64, 99, 30, range(2, 9), 20, 30)
    zero = [i for i in f64 if zero_distance(i)]
    print("F64 records: an escaped probe with D == 0: %d, %d with s > 1, %d de_mixed" % (
        len(zero), sum(i.s > 1 for i in zero), sum(i in mixed for i in zero)))
    fern = [i for i in f64 if zero_distance(i, fern=True)]
    print("F64 records: the same with the records of algo 1 counted: %d, %d with s > 1" % (len(fern), sum(i.s > 1 for i in fern)))
    assert sum(i.s > 1 for i in zero) >= 5 and sum(i in mixed for i in zero) >= 1
    for i in zero:  # the rule: an escaped probe with D = 0 is near whenever Rs > 0, and is not at R = 0
        dist, escaped = AV.probe_distance(i.cfg, *i.arrays, i.s)
        at = escaped & (dist == 0.0)
        assert i.reach > 0 and i.edge_sets()[1][at].all() and not i.edge_sets(reach=0.0)[1].any(), i.label
    print("F64 records: algo 1 %d, s = 1 %d" % (sum(not i.orbits for i in f64), sum(i.s == 1 for i in f64)))
    assert any(not i.orbits for i in f64) and any(i.s == 1 for i in f64)


def test_the_wide_views_meet_their_floors(wide, wide_bla):
    check_floors("wide views, WIDE PT", wide, 34, 10, V.S_VALUES, 6, 8)
    zero = sum(zero_distance(i) for i in wide)
    print("wide views, WIDE PT: an escaped probe with D == 0: %d" % zero)  # no floor
    # BLA-PT's arrays are another model's: its own tau and reach, counted beside WIDE PT's
    mixed = [i for i in wide_bla if i.de_mixed]
    same = sum(a.de_mixed == b.de_mixed and a.tau == b.tau and a.reach == b.reach for a, b in zip(wide, wide_bla))
    print("wide views, BLA-PT: de_mixed %d, by s %r; (de_mixed, tau, reach) are WIDE PT's on %d of %d" % (
        len(mixed), by_s(mixed, V.S_VALUES), same, len(wide)))
    assert len(mixed) >= 10 and all(n >= 1 for n in by_s(mixed, V.S_VALUES).values())


def test_every_input_is_deterministic_and_in_range(f64, wide, wide_bla):
    for i in f64 + wide + wide_bla:
        assert 0 <= i.tau <= 255 and 0.0 < i.reach * i.s <= AV.DE_MAX and 0.0 <= i.thickness * i.s <= AV.DE_MAX, i.label
        assert i.H.shape == (i.s * i.h, i.s * i.w, 3)
        text = i.describe()
        assert bytes(i.cfg).hex() in text and float(i.reach).hex() in text and i.thickness.hex() in text and "s %d" % i.s in text
        assert "tau %d" % i.tau in text
    i = f64[3]
    assert AV.median_reach(i.cfg, *i.arrays, i.s) == i.reach and V.median_tau(M.shaded(i.cfg, *i.arrays, i.s, i.thickness), i.s) == i.tau
    odd = 0
    for i in f64 + wide:  # the boundary: with an odd count the reach times s is a probe's own D
        dist, escaped = AV.probe_distance(i.cfg, *i.arrays, i.s)
        good = dist[escaped & np.isfinite(dist) & (dist > 0.0)]
        if good.size % 2 == 1 and i.reach * i.s < AV.DE_MAX:
            odd += bool(np.abs(good - i.reach * i.s).min() <= 2.0 ** -50 * i.reach * i.s)
    print("inputs whose R * s lies on or within 2^-50 of a probe's own D: %d" % odd)
    assert odd >= 10  # about half of the inputs with escaped probes have an odd number of them


# ---- 2. the plain adaptive call under the sRGB transfer ------------------------------------------------------------------------------------


def test_the_plain_adaptive_inputs_tell_the_transfers_apart():
    views = V.everything()
    differ = [v for v in views if transfers_differ(v.image(), v.s, A.edges(v.image(), v.s, v.tau))]
    print("deep views %d: the transfers differ at a refined pixel on %d, by s %r" % (len(views), len(differ), by_s(differ, V.S_VALUES)))
    assert len(views) == 65 and len(differ) >= 12 and all(n >= 1 for n in by_s(differ, V.S_VALUES).values())
    records = [r for r in V.f64_records() if r.cfg.algo in (0, 2) and r.s >= 2]
    differ = [r for r in records if transfers_differ(V.f64_image(r), r.s, A.edges(V.f64_image(r), r.s, V.median_tau(V.f64_image(r), r.s)))]
    print("F64 records with orbits and s >= 2: %d; the transfers differ at a refined pixel on %d, by s %r" % (
        len(records), len(differ), by_s(differ, range(2, 9))))
    assert len(differ) >= 35 and all(n >= 1 for n in by_s(differ, range(2, 9)).values())


# ---- 3. the wrong variants of the near rule ------------------------------------------------------------------------------------------------


def wrong_near(inp, rs=None, largest_scale=False, capped=False, le=False, left=False, at_0_0=False, zero_far=False):
    """adaptive_de with a near rule that is wrong in one way: (bytes, count)"""
    cfg, s = inp.cfg, inp.s
    z, it, der = inp.arrays
    p = 0 if at_0_0 else s // 2  # of the distance rule's probe; the colour rule keeps the right one
    cfg_s = SD.config_s(cfg, s)
    if largest_scale:  # both axes at the larger modulus: the last factor takes the max of the two
        big = max(abs(cfg.scale.re), abs(cfg.scale.im))
        cfg_s.scale.re = cfg_s.scale.im = big
    dist = D.distance(cfg_s, *(np.ascontiguousarray(a[p::s, p::s]) for a in (z, it, der)))
    rs = float(inp.reach) * float(s) if rs is None else rs
    n = (dist <= rs) if le else (dist < rs)
    if not capped:
        n &= it[p::s, p::s] < cfg.iterations
    if zero_far:
        n &= dist != 0.0
    if left:
        n = np.roll(n, 1, axis=1)  # column 0 reads the row's last probe
    H = inp.H
    P = A.probe(H, s)
    e = (V.neighbour_difference(P) > inp.tau) | n
    return np.where(e[..., None], SD.box(H, s), P), int(e.sum())


VARIANTS = {
    "Rs = R instead of R * s": lambda i: wrong_near(i, rs=float(i.reach)),
    "max of the scales for min": lambda i: wrong_near(i, largest_scale=True),
    "capped probes may be near": lambda i: wrong_near(i, capped=True),
    "D <= Rs for D < Rs": lambda i: wrong_near(i, le=True),
    "near read from the left neighbour's probe": lambda i: wrong_near(i, left=True),
    "the probe taken at sample (0, 0)": lambda i: wrong_near(i, at_0_0=True),
    "D = 0 not near": lambda i: wrong_near(i, zero_far=True),
}


def test_wrong_variants_of_the_near_rule_are_seen(f64, wide):
    for name, inputs in (("F64 records", f64), ("wide views", wide)):
        right = 0
        for i in inputs:
            if i.orbits:
                got, n = wrong_near(i)  # the variant machinery with nothing wrong is the model
                want, count = i.model(i.tau, i.reach)
                assert np.array_equal(got, want) and n == count, i.label
                right += 1
        assert right >= 30
        for what, f in VARIANTS.items():
            seen = 0
            for i in inputs:
                if not i.orbits:
                    continue
                want, count = i.model(i.tau, i.reach)
                got, n = f(i)
                seen += bool(n != count or not np.array_equal(got, want))
            print("%s: %s: seen on %d inputs" % (name, what, seen))
            if what == "D = 0 not near" and name == "wide views":
                continue  # no wide view has an escaped probe with D = 0
            assert seen >= 5, (name, what)


# ---- 4. the ends of the model --------------------------------------------------------------------------------------------------------------


def test_the_ends_of_the_model_on_every_input(f64, wide, wide_bla):
    for i in f64 + wide + wide_bla:
        if not i.orbits:
            for tau, reach in ((-1, i.reach), (i.tau, i.reach)):
                out, n = i.model(tau, reach)
                assert not out.any() and n == 0, i.label
            continue
        out, n = i.model(-1, i.reach)
        assert np.array_equal(out, SD.box(i.H, i.s)) and n == i.w * i.h, i.label
        out, n = i.model(255, 0.0)
        assert np.array_equal(out, A.probe(i.H, i.s)) and n == 0, i.label
        whole, count = i.model(i.tau, i.reach)
        fresh, n = M.adaptive_de(i.cfg, *i.arrays, i.s, i.thickness, i.tau, i.reach)  # without the kept H
        assert np.array_equal(fresh, whole) and n == count, i.label
        cuts = sorted({0, i.h // 3, (i.h + 1) // 2, i.h})
        parts = [i.model(i.tau, i.reach, a, b) for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate([q[0] for q in parts]), whole) and sum(q[1] for q in parts) == count, i.label
        rgba, n = i.model(i.tau, i.reach, channels=4)
        assert np.array_equal(rgba[..., :3], whole) and (rgba[..., 3] == 255).all() and n == count
        lin, n = i.model(i.tau, i.reach, filter=AV.srgb_filter)
        e, nr = i.sets
        assert n == count and np.array_equal(lin[~(e | nr)], whole[~(e | nr)]), i.label
