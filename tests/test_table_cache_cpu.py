"""The argument tests/test_gpu_table_cache.py rests on, from the models alone (no device): which fields of a view decide its
skip tables, and that a table of the wrong view shows in the results.

The table slot of a context (fractal-renderer_amd/csrc/fr_bla.hip: bla_table_for) may serve its tables to a view only if they
are the tables that view would build.  tests/table_cache_steps.py walks views that differ one thing at a time and compares, in
the models, the orbits and the whole tables of each with the step before: a step where either differs MUST build.  The steps
that change SCALED PT's scale by a power of two are such steps although the orbit, Dw, bits and the kind of table — all a key
without S would hold — are bit-equal: every stored radius is proportional to S = 2^e.

The teeth: tests/pt_scaled_model.c run on one view with the tables of its neighbour (ptsm_rows_table_of) differs from the model
proper at hundreds of pixels, so a library that serves the neighbour's tables cannot pass the bit-for-bit comparison."""
import numpy as np
import pytest

import pt_scaled_model as S
import table_cache_steps as T

MB, MS = T.MUST_BUILD, T.MAY_SERVE


@pytest.fixture(scope="module")
def fr():
    import __graft_entry__ as ge

    ge.build()
    import fractal_renderer_amd

    return fractal_renderer_amd


def differing_pixels(a, b):
    """pixels whose z differs in bits"""
    return int((np.ascontiguousarray(a[0]).view(np.uint64) != np.ascontiguousarray(b[0]).view(np.uint64)).any(axis=-1).sum())


# ---- 1. the model's foreign-table entry point ---------------------------------------------------------------------------------


@pytest.mark.parametrize("spec", ["M_900", "J_900", "MINI_861", "M_300"])
def test_the_foreign_table_entry_point_with_the_views_own_table_is_the_model(fr, spec):
    v = S.view(fr.Config.new, getattr(S, spec))
    for bits in (40, 24):
        own = S.escape_rows(v.cfg, v.x, v.k, bits)
        got = S.escape_rows_table_of(v.cfg, v.cfg, v.x, v.k, bits)
        for a, b in zip(got, own):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else a.dtype),
                                                         b.view(np.uint64 if b.dtype == np.float64 else b.dtype))
    assert int(own[2].astype(np.uint64).sum()) < S.steps(v.cfg, own[1])  # the table is applied
    z, it, passes, reb = S.escape_rows_table_of(v.cfg, v.cfg, v.x, v.k, 40, 3, 9)  # rows
    want = v.model(40)
    assert S.same_bits(z, want[0][3:9]) and np.array_equal(it, want[1][3:9]) and np.array_equal(passes, want[2][3:9])


# ---- 2. which fields decide a table -------------------------------------------------------------------------------------------

CLASSES_S = {
    "unrelated: N at 2^900": None,
    "M at 2^900": MB,
    "scale x 2": MB,  # the orbit, Dw, bits and the kind are the step before's: S alone differs
    "scale x 2^-9": MB,
    "back to 2^900": MB,
    "scale.im negated": MS,  # Dw takes absolute values
    "scale.re x 1.25": MB,  # e stays, sre and with it Dw move
    "bits 41": MB,
    "bits 0": MB,  # 40 after 41
    "bits -1": None,  # no table
    "bits 40 again": MS,
    "size 21 x 37": MB,
    "size 74 x 42": MB,
    "size 37 x 21": MS,  # half the size, the same aspect: Dw equal
    "limit": MS,
    "colours and exposure": MS,
    "iterations 6001": MS,  # the orbit ended by escape: the same at every cap
    "iterations 600": MB,  # cut at the cap
    "iterations 6000": MB,
    "centre: last word + 1": MB,
    "MINI at 2^861": MB,
    "MINI: cap 3300": MB,
    "MINI: scale x 2": MB,
    "J at 2^900": MB,
    "J: scale x 2": MB,
    "J: julia_set.im + 1 ulp": MB,
}

CLASSES_B = {
    "unrelated: N at 2^300": None,
    "SEAHORSE": MB,
    "pos_lo.im + 0.2 ulp": MB,
    "iterations - 1": MS,  # this orbit ends by escape after 8350 steps
    "iterations + 1": MS,
    "scale x 2": MB,  # BLA-PT's D is the image's own: it halves
    "scale x 1.5": MB,
    "size 21 x 37": MB,
    "size 42 x 74": MS,  # the same aspect doubled: D equal
    "bits 53": MB,
    "bits 24": MB,
    "limit": MS,
    "algo: Julia": MB,
    "julia_set.im + 1 ulp": MB,
    "back to the first": MB,
    "iterations - 1, orbit cut at the cap": MB,
    "iterations + 1, orbit cut at the cap": MB,
}


def test_sequence_s_classes(fr):
    steps = T.sequence_s(fr.Config.new)
    got = dict(zip((s.what for s in steps), T.classes(steps)))
    assert got == CLASSES_S
    name = T.by_name(steps)
    # the power-of-two scale steps: everything a key without S holds is bit-equal, and the tables still differ
    for what, before in (("scale x 2", "M at 2^900"), ("scale x 2^-9", "scale x 2"), ("back to 2^900", "scale x 2^-9"),
                         ("MINI: scale x 2", "MINI: cap 3300"), ("J: scale x 2", "J at 2^900")):
        s, h = name[what], name[before]
        assert T.same_orbits(s, h) and S.same_bits(s.D(), h.D()) and s.table_bits == h.table_bits
        assert not T.same_tables(s, h)
        assert S.exponent(s.cfg) != S.exponent(h.cfg)
        for ts, th in zip(s.tables(), h.tables()):  # and in nothing but the radii
            assert all(S.same_bits(p[:, :4], q[:, :4]) for p, q in zip(ts, th))
    # the sign of a divisor moves every pixel and no table entry
    s, h = name["scale.im negated"], name["back to 2^900"]
    assert T.same_tables(s, h) and not S.same_bits(s.model()[0], h.model()[0])
    # a cap beyond an orbit that ended by escape changes nothing; a cap inside it cuts the orbit
    assert name["iterations 6001"].ended and len(name["iterations 6001"].x) == len(name["limit"].x) < 6000
    assert len(name["iterations 600"].x) == 602 and not name["iterations 600"].ended
    assert len(name["MINI: cap 3300"].x) == 3302 and len(name["MINI at 2^861"].x) == 3206
    assert name["MINI: cap 3300"].cache_triple()[2] > name["MINI at 2^861"].cache_triple()[2]
    for s in steps:  # no step degenerates to an empty table
        if s.table_bits is not None:
            assert s.cache_triple()[1] >= 5 and s.passes() < S.steps(s.cfg, s.model()[1]), s.what


def test_sequence_b_classes(fr):
    steps = T.sequence_b(fr.Config.new)
    got = dict(zip((s.what for s in steps), T.classes(steps)))
    assert got == CLASSES_B
    name = T.by_name(steps)
    s, h = name["size 42 x 74"], name["size 21 x 37"]
    assert S.same_bits(s.D(), h.D()) and s.shape != h.shape
    assert len(name["SEAHORSE"].x) == name["SEAHORSE"].cfg.iterations + 2  # cut at the cap
    wide = T.wide_bla_steps(fr.Config.new)
    # D halves, but at 2^-300 the term |B| D lies far below the rounding of every radius: the tables come out bit-equal
    assert T.classes(wide) == [None, MS] and T.same_orbits(*wide) and wide[1].D() == wide[0].D() / 2


# ---- 3. teeth: a neighbour's table shows ----------------------------------------------------------------------------------------


def test_a_stale_table_shows_in_the_model(fr):
    m892, m899, m900, m901 = T.scale_steps_m(fr.Config.new, (892, 899, 900, 901))
    assert m900.shape == (21, 37) and m900.cfg.iterations == 6000 and m900.n == 16 and m900.table_bits == 40
    for v in (m892, m899, m901):
        assert T.same_orbits(v, m900) and S.same_bits(v.D(), m900.D())
    # the first radii at 2^901 are exactly twice those at 2^900
    r900, r901 = m900.tables()[0][1][:8, 4], m901.tables()[0][1][:8, 4]
    assert (r900 > 0).all() and S.same_bits(r901, 2.0 * r900)
    floors = {}
    for v, floor in ((m901, 100), (m899, 50), (m892, 700)):
        stale = v.model_with_table_of(m900)
        floors[v.what] = n = differing_pixels(stale, v.model())
        print("%s with the table of 2^900: %d of %d pixels differ, passes %d against %d" % (
            v.what, n, v.shape[0] * v.shape[1], int(stale[2].astype(np.uint64).sum()), v.passes()))
        assert n >= floor, (v.what, n)
    stale = m901.model_with_table_of(m900)
    assert int(stale[2].astype(np.uint64).sum()) != m901.passes()  # the skips move: the pass count sees a wrong table too


# ---- 4. the library's host-only table does not go through the slot ---------------------------------------------------------------


def test_the_librarys_host_table_follows_s(fr):
    m900, m901 = T.scale_steps_m(fr.Config.new, (900, 901))
    got = {}
    for v in (m900, m901):
        want = v.tables()[0]
        got[v.what] = [fr.bla_table(v.cfg, level, bla=40, scaled=True, **v.kw(fr)) for level in range(len(want))]
        assert fr.bla_table(v.cfg, len(want), bla=40, scaled=True, **v.kw(fr)).shape == (0, 5)
        for level, (g, w) in enumerate(zip(got[v.what], want)):
            assert g.shape == w.shape and S.same_bits(g, w), (v.what, level)
    differ = 0
    for a, b in zip(got[m900.what], got[m901.what]):
        assert S.same_bits(a[:, :4], b[:, :4])
        differ += int((a[:, 4] != b[:, 4]).sum())
    assert differ > 0
