"""The inputs of tests/ss_adaptive_de_scaled_views.py on the host models alone, without a device: conditions on the INPUTS of
tests/test_gpu_ss_adaptive_de_scaled_random.py, so that the GPU file cannot pass emptily and a later edit of a generator cannot
hollow it out unnoticed.  Every count is printed with -s; DESIGN.md 3.34 records them.
  - every view of deep_ss_views.everything() is an input, at bits -1 and at its table bits: 65 each;
  - floors: at least 20 de_mixed inputs per form, at least 8 of them past 2^440, every s of 2, 3, 4, 5, 7, 8 and both algorithms
    among those; a near-only pixel with F != P past 2^440; the byte and the sRGB filter differing at a refined pixel past 2^440;
  - the scaled view is what makes the distance finite: past 2^440 the distance on the UNSCALED cfg_s is not the scaled view's;
  - the ends of the model on every input: t = -1, t = 255 with R = 0, row pieces, RGBA, the sRGB filter outside the union."""
import numpy as np
import pytest

import de_model as D
import de_scaled_model as DSM
import deep_ss_views as V
import ss_adaptive_de_model as M
import ss_adaptive_de_scaled_views as SV
import ss_adaptive_de_views as AV
import ss_adaptive_model as A
import ss_de_model as SD


@pytest.fixture(scope="module")
def plain():
    return SV.inputs(False)


@pytest.fixture(scope="module")
def table():
    return SV.inputs(True)


def by_s(inputs):
    return {s: sum(1 for i in inputs if i.s == s) for s in V.S_VALUES}


def near_only_differs(inp):
    e, n = inp.sets
    return bool(inp.orbits and (n & ~e & inp.differ).any())


def transfers_differ(inp):
    if not inp.orbits or inp.s < 2:
        return False
    e, n = inp.sets
    return bool(((AV.srgb_filter(inp.H, inp.s) != SD.box(inp.H, inp.s)).any(axis=-1) & (e | n)).any())


@pytest.mark.parametrize("form", ["plain", "table"])
def test_the_inputs_meet_their_floors(plain, table, form):
    inputs = plain if form == "plain" else table
    assert len(inputs) == 65 and len({id(i.v) for i in inputs}) == 65
    mixed = [i for i in inputs if i.de_mixed]
    deep = [i for i in mixed if SV.deep(i.v)]
    print("%s: %d inputs, de_mixed %d, past 2^440 %d, by s %r, Julia %d" % (form, len(inputs), len(mixed), len(deep), by_s(deep),
                                                                              sum(i.cfg.algo == 2 for i in deep)))
    assert len(mixed) >= 20 and len(deep) >= 8
    assert all(n >= 1 for n in by_s(deep).values()), by_s(deep)
    assert {int(i.cfg.algo) for i in deep} == {0, 2}
    lonely = sum(near_only_differs(i) for i in inputs if SV.deep(i.v))
    srgb = sum(transfers_differ(i) for i in inputs if SV.deep(i.v))
    print("%s, past 2^440: a near-only pixel with F != P on %d inputs, the transfers differ at a refined pixel on %d" % (form, lonely, srgb))
    assert lonely >= 4 and srgb >= 4
    for i in mixed:  # what the GPU file asserts before it trusts a pass
        e, n = i.sets
        count = i.model(i.tau, i.reach)[1]
        assert 0 < count < i.w * i.h and count == int((e | n).sum()), i.describe()


def test_the_table_form_takes_skips_on_refined_samples(table):
    """bits >= 0 is another loop: on the de_mixed inputs past 2^440 some sample of a refined pixel took a table skip"""
    seen = 0
    for i in table:
        if not (i.de_mixed and SV.deep(i.v)):
            continue
        skips = i.v.rows("de_scaled", i.bits)[4]
        e, n = i.sets
        per_pixel = skips.reshape(i.h, i.s, i.w, i.s).sum(axis=(1, 3))
        seen += bool((per_pixel[e | n] > 0).any())
    print("de_mixed inputs past 2^440 with a skip on a refined sample: %d" % seen)
    assert seen >= 6


def test_every_input_is_deterministic_and_in_range(plain, table):
    for i in plain + table:
        assert 0 <= i.tau <= 255 and 0.0 < i.reach * i.s <= AV.DE_MAX and 0.0 <= i.thickness * i.s <= AV.DE_MAX, i.label
        assert i.H.shape == (i.s * i.h, i.s * i.w, 3)
        assert bytes(i.cfg) == bytes(DSM.scaled_view(i.v.cfg)) and max(abs(i.cfg.scale.re), abs(i.cfg.scale.im)) < 1.0
        text = i.describe()
        assert bytes(i.v.cfg).hex() in text and float(i.reach).hex() in text and i.thickness.hex() in text and "s %d" % i.s in text
    i = plain[3]
    assert AV.median_reach(i.cfg, *i.arrays, i.s) == i.reach and V.median_tau(M.shaded(i.cfg, *i.arrays, i.s, i.thickness), i.s) == i.tau


def test_the_scaled_view_is_what_the_distance_needs(plain):
    """u = d 2^-e: on the view's own scale the last factor of D is 2^e too large, so past 2^440 every finite positive probe
    distance differs from the scaled view's — a kernel handed cfg_s's `pixels` instead of cfg_sv's is seen"""
    seen = 0
    for i in plain:
        if not (i.orbits and SV.deep(i.v)):
            continue
        zp, ip, up = AV.probes(i.s, *i.arrays)
        right = D.distance(SD.config_s(i.cfg, i.s), zp, ip, up)
        wrong = D.distance(i.v.cfg_s, zp, ip, up)
        good = (ip < i.cfg.iterations) & np.isfinite(right) & (right > 0.0)
        if good.any():
            assert (wrong[good] != right[good]).all(), i.label
            seen += 1
    assert seen >= 10


def test_the_ends_of_the_model_on_every_input(plain, table):
    for i in plain + table:
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
        cuts = sorted({0, i.h // 3, (i.h + 1) // 2, i.h})
        parts = [i.model(i.tau, i.reach, a, b) for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate([q[0] for q in parts]), whole) and sum(q[1] for q in parts) == count, i.label
        rgba, n = i.model(i.tau, i.reach, channels=4)
        assert np.array_equal(rgba[..., :3], whole) and (rgba[..., 3] == 255).all() and n == count
        lin, n = i.model(i.tau, i.reach, filter=AV.srgb_filter)
        e, nr = i.sets
        assert n == count and np.array_equal(lin[~(e | nr)], whole[~(e | nr)]), i.label
