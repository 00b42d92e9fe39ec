"""RESUMABLE DE on the host (include/fractal_hip.h, fr_precision: "RESUMABLE DE"): tests/de_state_model.c against the models it
must agree with, and against itself.  No device.

CLAIM 1: z, iters and der of the PT state run are DE's (tests/de_model.c), dz and m are RESUMABLE PT's (tests/pt_state_model.c
for a dd centre, tests/pt_wide_model.c for a wide one).  CLAIM 2: a state continued from N to M on the orbits of M is the state
run at M, in all five arrays — from N = 0, over a chain, and with M = N.  The F64 road: (z, iters, der) of DE continued is DE at
the higher cap.  And the cases are what the tests chose them for: pixels finished below N, escaping in [N, M), capped at M."""
import numpy as np
import pytest

import de_extend_cases as X
import de_model as D
import de_state_model as S
import pt_state_model as PSM
import pt_wide_model as W


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", X.ALL)
def test_the_cases_are_what_they_claim(name):
    c = X.case(name)
    it = c.state(c.m)[1]
    got = X.classes(it, c.n, c.m)
    assert sum(got) == it.size
    if c.counts is not None:
        assert got == c.counts, (name, got)
    assert got[1] + got[2] > 0, "nothing would be continued"
    at_n = c.state(c.n)[1]
    assert int((at_n == c.n).sum()) == got[1] + got[2]  # the running pixels at N are the ones the extension continues


def test_the_special_cases():
    for name in ("f64-overflow", "pt-overflow"):  # the overflow is crossed inside the extension
        c = X.case(name)
        run_n, run_m = c.state(c.n)[1] == c.n, c.state(c.m)[1] == c.m
        assert run_n.sum() >= 1 and run_m.sum() == 1
        d_n, d_m = c.state(c.n)[-1][run_m], c.state(c.m)[-1][run_m]
        assert np.isfinite(d_n).all() and 1e187 < np.hypot(*d_n[0]) < 1e189
        assert not np.isfinite(d_m).all()
    c = X.case("pt-julia-rebase")  # continued pixels carry the on-K bit; at 150 every pixel is running
    st = c.state(300)
    running = st[1] == 300
    assert running.sum() == 74 and (st[3][running] & S.ON_K).all()
    assert (c.state(150)[1] == 150).all() and not (c.state(150)[3] & S.ON_K).any()
    c = X.case("pt-orbit-escapes")  # R is cut by the cap at N and ended by escape at M
    assert PSM.orbit_info(c.cfg_at(c.n))[1] is False
    last, ended = PSM.orbit_info(c.cfg_at(c.m))
    assert ended and last + 1 == 31
    c = X.case("wide-2^200-16x12")  # every pixel is at the cap at N
    assert (c.state(c.n)[1] == c.n).all()


@pytest.mark.parametrize("name", X.PT)
def test_claim_1_the_state_run_is_de_and_resumable_pt(name):
    c = X.case(name)
    for cap in sorted({0, 1, c.n, c.m}):
        z, it, dz, m, der = c.state(cap)
        wz, wit, wder = c.de_rows(cap)
        assert np.array_equal(it, wit) and D.same_doubles(z, wz) and D.same_doubles(der, wder), (name, cap)
        cfg = c.cfg_at(cap)
        if c.wide:
            pz, pit, pdz, pm = W.state_rows(cfg, c.orbits(cap))[0]
        else:
            pz, pit, pdz, pm = PSM.state_rows(cfg, c.pos_lo or (0.0, 0.0))
        assert np.array_equal(it, pit) and np.array_equal(m, pm), (name, cap)
        assert np.array_equal(bits(z), bits(pz)) and np.array_equal(bits(dz), bits(pdz)), (name, cap)
        if cap == 0:
            assert (der == [1.0, 0.0]).all() and not it.any()


@pytest.mark.parametrize("name", X.ALL)
def test_claim_2_a_continued_state_is_the_state_run(name):
    c = X.case(name)
    want = c.state(c.m)
    assert c.same(c.continued(c.state(c.n), c.n, c.m), want), "N -> M"
    assert c.same(c.continued(c.state(0), 0, c.m), want), "0 -> M"
    st = c.state(c.chain[0])
    for a, b in zip(c.chain, c.chain[1:]):
        st = c.continued(st, a, b)
        assert c.same(st, c.state(b)), (a, b)
    st = c.continued(c.state(0), 0, 1)  # a link of one step, then on to N
    assert c.same(c.continued(st, 1, c.n), c.state(c.n))
    assert c.same(c.continued(want, c.m, c.m), want), "M == N changes nothing"


@pytest.mark.parametrize("name", ["f64-mandelbrot-37x23", "pt-seahorse-pos-lo", "wide-julia"])
def test_a_row_piece_and_finished_pixels_left_alone(name):
    c = X.case(name)
    piece = tuple(a[5:15] for a in c.state(c.n))
    got = c.continued(piece, c.n, c.m, 5, 15)
    assert c.same(got, tuple(a[5:15] for a in c.state(c.m)))
    # a finished pixel is identified by its iters word alone: poison in its other arrays survives
    poisoned = [np.array(a) for a in c.state(c.n)]
    finished = poisoned[1] != c.n
    assert finished.any()
    for k, a in enumerate(poisoned):
        if k != 1:
            a[finished] = 0xA5A5A5A5 if a.dtype == np.uint32 else -1234.5
    got = c.continued(tuple(poisoned), c.n, c.m)
    for k, a in enumerate(got):
        if k != 1:
            assert np.array_equal(a[finished], poisoned[k][finished])
    running = ~finished
    for g, w in zip(got, c.state(c.m)):
        assert D.same_doubles(g[running], w[running]) if g.dtype == np.float64 else np.array_equal(g[running], w[running])


def test_an_algorithm_without_orbits():
    c = X.case("pt-mandelbrot-37x23")
    cfg = c.cfg_at(50)
    cfg.algo = 1
    st = S.pt_state_rows(cfg)
    assert all(not a.any() for a in st)
    assert S.same_state(S.pt_continue(cfg, st, 0), st)
