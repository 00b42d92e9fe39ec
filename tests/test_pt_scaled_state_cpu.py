"""RESUMABLE SCALED PT without a device (include/fractal_hip.h, fr_precision: "RESUMABLE SCALED PT").  Every check of the
definition here uses MODELS only: tests/pt_scaled_state_model.py (the paragraph restated) against tests/pt_scaled_model.py
(SCALED PT's plain loop) and tests/pt_wide_model.py (RESUMABLE PT on a wide centre), all on pt_wide_model's integer orbits.
  - claim 1: z and iters of the state run are the plain scaled loop's (bits = -1) at every cap of every chain;
  - claim 2: the state continued link by link, and in one jump, is the state run at the higher cap in all four arrays;
  - claim 3: inside WIDE PT's domain z, iters and m are pt_wide_model's state and w is ldexp(dz, e), as bits;
  - the conditions (a) .. (e) that make the chains reach what can go wrong, asserted on the model;
  - through the library, no device: the domain of the four new calls, each refusal with status 1 and a message, and the legal
    no-ops.  On the commit before the calls existed these fail for lack of the symbols.

The chains (pt_scaled_state_model.CHAINS) are pt_scaled_model's views with the cap replaced, at the caps the feature's issue
names; none of those caps had to move.  One thing did not hold as the issue expected.  Condition (b) wants a pixel of J_900
that rebases on m == end, on V and on K, "because V and K end by escape at 631 and 252 and the escape indices reach 1139".
The model counts NO such rebase on J_900 at any cap up to 5000 (every pixel has escaped by then): at limit 2 a pixel that
reaches the last entry of an orbit ended by escape without a rebase sits beside an entry with re*re + im*im > 4 and escapes
in that very step, and on K, 253 entries long, a pixel rebases on the test about every 20 steps (27 rebases at most in 1139
steps).  No cap can mend that, so J_900 stays in every other check as the issue gives it, and (b) is asserted on a fifth
chain of the same kind, J2_900: the repelling fixed point of julia_set = 1.1i at 2^900, 16 x 12, limit 65536 (the library's
default), where K ends by escape after 4 steps and V after 648.  There 49 rebases on K's end happen before cap 600 and the
centre pixel rebases on V's end at step 647."""
import ctypes as C
import math

import numpy as np
import pytest

import pt_scaled_model as S
import pt_scaled_state_model as T
import pt_wide_model as W

INVALID = 1


@pytest.fixture(scope="module")
def fr():
    import __graft_entry__ as ge

    ge.build()
    import fractal_renderer_amd

    return fractal_renderer_amd


@pytest.fixture(scope="module")
def native(fr):
    from fractal_renderer_amd import _native

    return _native


@pytest.fixture(scope="module")
def lib(native):
    return native.load()


def message(lib):
    return lib.fr_last_error().decode()


def on_k(state):
    return (state[3] & T.ON_K) != 0


def running(state, cap):
    return state[1] == cap


# ---- claims 1 and 2 on every chain ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(T.CHAINS))
def test_claim_1_z_and_iters_are_the_plain_scaled_loops_at_every_cap(fr, name):
    c = T.chain(fr.Config.new, name)
    for cap in c.caps:
        (z, it, w, m), _reb, _end = c.state(cap)
        pz, pit, _passes, _preb = c.plain(cap)
        assert np.array_equal(it, pit), (name, cap)
        assert S.same_bits(z, pz), (name, cap)
        escaped = it < cap
        assert (w[escaped] == 0).all() and (m[escaped] == 0).all(), "an escaped pixel stores w = (0, 0), m = 0"
        assert np.isfinite(z).all() and np.isfinite(w).all()
    (z, it, w, m), reb, _end = c.state(0)  # N = 0: the initial state
    o = c.orbits(0)
    julia = c.cfg(0).algo == 2
    m0 = 0 if julia else 1
    assert (it == 0).all() and (m == m0).all() and (reb == 0).all()
    sinv = math.ldexp(1.0, -S.exponent(c.cfg(0)))
    x = o.x[0][m0]
    # w Sinv is exact (a power of two, nothing subnormal), so fma(w, Sinv, X_m) is this sum
    assert S.same_bits(z[..., 0], w[..., 0] * sinv + x[0]) and S.same_bits(z[..., 1], w[..., 1] * sinv + x[1])


@pytest.mark.parametrize("name", list(T.CHAINS))
def test_claim_2_link_by_link_and_in_one_jump(fr, name):
    c = T.chain(fr.Config.new, name)
    state = c.state(c.caps[0])[0]
    for a, b in c.links():
        state, _reb, _end = T.continue_rows(c.cfg(b), c.orbits(b), state, a)
        assert T.same_state(state, c.state(b)[0]), "%s: %d -> %d" % (name, a, b)
    first, last = c.caps[0], c.caps[-1]
    jump, _reb, _end = T.continue_rows(c.cfg(last), c.orbits(last), c.state(first)[0], first)
    assert T.same_state(jump, c.state(last)[0]), "%s: %d -> %d in one jump" % (name, first, last)
    # the rebases add up as well: a run to N is a prefix of the run to M
    a, b = c.links()[-1]
    _s, reb, end = T.continue_rows(c.cfg(b), c.orbits(b), c.state(a)[0], a)
    assert np.array_equal(c.state(a)[1] + reb, c.state(b)[1]) and np.array_equal(c.state(a)[2] + end, c.state(b)[2])


def test_rows_of_the_model_are_slices_of_the_whole(fr):
    c = T.chain(fr.Config.new, "M_900")
    whole = c.state(560)[0]
    piece = T.state_rows(c.cfg(560), c.orbits(560), 5, 12)[0]
    assert T.same_state(piece, tuple(a[5:12] for a in whole))
    cont = T.continue_rows(c.cfg(600), c.orbits(600), piece, 560, 5, 12)[0]
    assert T.same_state(cont, tuple(a[5:12] for a in c.state(600)[0]))


# ---- claim 3: inside WIDE PT's domain ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("spec", [S.M_200, S.M_440, S.N_300, S.J_300], ids=["M_200", "M_440", "N_300", "J_300"])
def test_claim_3_inside_wide_pts_domain_the_state_is_wide_pts_with_w_for_dz(fr, spec):
    v = S.view(fr.Config.new, spec)
    (z, it, dz, m), reb = W.state_rows(v.cfg, v.orbits, rule=0)
    (sz, sit, sw, sm), sreb, _end = T.state_rows(v.cfg, v.orbits)
    assert np.array_equal(sit, it) and np.array_equal(sm, m) and np.array_equal(sreb, reb)
    assert S.same_bits(sz, z)
    assert S.same_bits(sw, np.ldexp(dz, S.exponent(v.cfg)))  # w = dz 2^e exactly
    assert (it == v.cfg.iterations).any() or len(np.unique(it)) > 1


# ---- the conditions on the chains ---------------------------------------------------------------------------------------------


def test_a_the_cap_dependent_rebase_is_met_and_left_out(fr):
    """(a) M at cap 300: the orbit is cut by the cap, and pixels meet m == last at the final step without having rebased: the
    plain loop rebases there, the state rule does not."""
    c = T.chain(fr.Config.new, "M_900")
    o = c.orbits(300)
    assert not o.x[1] and len(o.x[0]) - 1 == 301  # cut by the cap: last = N + 1
    (z, it, w, m), reb, end = c.state(300)
    never = running((z, it, w, m), 300) & (reb == 0)
    assert never.any() and (m[never] == 301).all()  # m == last after the final step
    preb = c.plain(300)[3]
    assert (preb[never] == reb[never] + 1).all() and (end == 0).all()


def test_b_rebases_on_the_end_of_v_and_of_k(fr):
    """(b), on J2_900 (the module's docstring says why not on J_900).  On K: a link at whose cap V is still cut by the cap, so
    that only K can supply m == end.  On V: the one-step link 647 -> 648, by a pixel that starts it on V."""
    c = T.chain(fr.Config.new, "J2_900")
    assert not c.orbits(600).x[1] and c.orbits(600).k[1] and len(c.orbits(600).k[0]) - 1 == 4
    _s, _reb, end = T.continue_rows(c.cfg(600), c.orbits(600), c.state(400)[0], 400)
    assert int(end.sum()) == 49  # on K: V is cut at this cap
    assert c.orbits(648).x[1] and len(c.orbits(648).x[0]) - 1 == 648
    before = c.state(647)[0]
    after, reb, end = T.continue_rows(c.cfg(648), c.orbits(648), before, 647)
    on_v = running(before, 647) & ~on_k(before)
    assert on_v.any() and (end[on_v] == 1).all() and on_k(after)[on_v].all() and (after[3][on_v] == T.ON_K).all()
    # and what the issue expected of J_900 does not happen there, at any cap: every pixel has escaped by 5000
    j = T.chain(fr.Config.new, "J_900")
    assert not running(j.state(5000)[0], 5000).any() and int(j.state(5000)[2].sum()) == 0


@pytest.mark.parametrize("name", list(T.CHAINS))
def test_c_a_link_begins_with_finished_and_running_pixels(fr, name):
    """(c) N_900 has no such link: the nucleus' pixels all run to every cap, which the test pins instead."""
    c = T.chain(fr.Config.new, name)
    mixed = [(a, b) for a, b in c.links() if 0 < int(running(c.state(a)[0], a).sum()) < c.shape[0] * c.shape[1]]
    if name == "N_900":
        assert not mixed and all(running(c.state(cap)[0], cap).all() for cap in c.caps)
    else:
        assert mixed, name


def test_d_a_link_begins_with_nothing_running(fr):
    c = T.chain(fr.Config.new, "M_900")
    assert (600, 6000) in c.links() and not running(c.state(600)[0], 600).any()
    cont = T.continue_rows(c.cfg(6000), c.orbits(6000), c.state(600)[0], 600)[0]
    assert T.same_state(cont, c.state(600)[0]) and T.same_state(cont, c.state(6000)[0])


def test_e_a_cut_orbit_is_continued_and_one_links_orbits_are_all_ended(fr):
    n = T.chain(fr.Config.new, "N_900")
    assert not n.orbits(1).x[1] and not n.orbits(1000).x[1]
    assert len(n.orbits(1000).x[0]) - len(n.orbits(1).x[0]) == 999  # what the cache computes for 1 -> 1000
    assert np.array_equal(n.orbits(1000).x[0][:3], n.orbits(1).x[0])  # a proper prefix
    j = T.chain(fr.Config.new, "J_900")
    for cap in (632, 800):
        o = j.orbits(cap)
        assert o.x[1] and o.k[1] and (len(o.x[0]), len(o.k[0])) == (632, 253)
    assert running(j.state(632)[0], 632).any()  # and pixels do continue on them


# ---- the library's domain, no device -----------------------------------------------------------------------------------------


def domain_view(fr, native, scale_log2=900, n=16, cap=100):
    cfg = W.view(fr.Config.new(), "M", scale_log2, 16, 12, cap)
    re, im = W.centre_ints("M", n)
    words = W.to_words(re, n), W.to_words(im, n)
    p64 = C.POINTER(C.c_uint64)
    st = native.fr_wide_centre(n, words[0].ctypes.data_as(p64), words[1].ctypes.data_as(p64))
    return cfg, st, words


class Arrays:
    def __init__(self, cfg, rows):
        npx = rows * cfg.width
        self.z, self.w = np.zeros(2 * npx + 1), np.zeros(2 * npx + 1)
        self.it, self.m = np.zeros(npx + 1, dtype=np.uint32), np.zeros(npx + 1, dtype=np.uint32)

    def ptrs(self, null=None, skew=None):
        p = {"z": self.z.ctypes.data, "it": self.it.ctypes.data, "w": self.w.ctypes.data, "m": self.m.ctypes.data}
        if null:
            p[null] = None
        if skew:
            p[skew[0]] += skew[1]
        return p["z"], p["it"], p["w"], p["m"]


def calls(lib):
    """the four calls as f(cfg, centre, y0, y1, from, z, it, w, m) -> status; the state calls ignore `from`"""
    ref = lambda cfg: None if cfg is None else C.byref(cfg)  # noqa: E731
    return {
        "state": lambda cfg, st, y0, y1, frm, *a: lib.fr_escape_rows_pt_scaled_state(ref(cfg), st, y0, y1, *a),
        "state_device": lambda cfg, st, y0, y1, frm, *a: lib.fr_escape_rows_pt_scaled_state_device(ref(cfg), st, y0, y1, *a, None),
        "extend": lambda cfg, st, y0, y1, frm, *a: lib.fr_escape_extend_pt_scaled(ref(cfg), st, y0, y1, frm, *a),
        "extend_device": lambda cfg, st, y0, y1, frm, *a: lib.fr_escape_extend_pt_scaled_device(ref(cfg), st, y0, y1, frm, *a, None),
    }


CALLS = ["state", "state_device", "extend", "extend_device"]


@pytest.mark.parametrize("call", CALLS)
def test_a_null_array_is_refused(fr, native, lib, call):
    cfg, st, _w = domain_view(fr, native)
    a = Arrays(cfg, 12)
    for null in ("z", "it", "w", "m"):
        assert calls(lib)[call](cfg, C.byref(st), 0, 12, 50, *a.ptrs(null=null)) == INVALID, null
        assert "NULL array" in message(lib) and "all four" in message(lib)


@pytest.mark.parametrize("call", CALLS)
def test_a_misaligned_array_is_refused(fr, native, lib, call):
    cfg, st, _w = domain_view(fr, native)
    a = Arrays(cfg, 12)
    for skew in (("z", 4), ("w", 4), ("it", 2), ("m", 2)):
        assert calls(lib)[call](cfg, C.byref(st), 0, 12, 50, *a.ptrs(skew=skew)) == INVALID, skew
        assert "aligned" in message(lib)


@pytest.mark.parametrize("call", ["extend", "extend_device"])
def test_a_lower_cap_is_refused(fr, native, lib, call):
    cfg, st, _w = domain_view(fr, native, cap=100)
    a = Arrays(cfg, 12)
    assert calls(lib)[call](cfg, C.byref(st), 0, 12, 101, *a.ptrs()) == INVALID
    assert "from_iterations" in message(lib)
    assert calls(lib)[call](cfg, C.byref(st), 0, 0, 101, None, None, None, None) == INVALID  # before the rows are looked at


@pytest.mark.parametrize("call", CALLS)
def test_a_scale_of_2_952_and_a_null_centre_are_refused(fr, native, lib, call):
    cfg, st, _w = domain_view(fr, native, 951)
    a = Arrays(cfg, 12)
    assert calls(lib)[call](cfg, C.byref(st), 0, 0, 100, *a.ptrs()) == 0  # 2^951 is inside
    cfg.scale.re = cfg.scale.im = math.ldexp(1.0, 952)
    assert calls(lib)[call](cfg, C.byref(st), 0, 12, 50, *a.ptrs()) == INVALID
    assert "SCALED PT" in message(lib) and "e + 64" in message(lib)
    cfg, st, _w = domain_view(fr, native)
    assert calls(lib)[call](cfg, None, 0, 12, 50, *a.ptrs()) == INVALID
    assert "SCALED PT" in message(lib) and "centre is NULL" in message(lib)
    cfg.limit = 2.0 ** 21  # SCALED PT's own rules hold for the state calls too
    assert calls(lib)[call](cfg, C.byref(st), 0, 12, 50, *a.ptrs()) == INVALID and "2^20" in message(lib)
    assert calls(lib)[call](None, C.byref(st), 0, 0, 50, *a.ptrs()) == INVALID


@pytest.mark.parametrize("call", CALLS)
def test_the_legal_no_ops_need_no_device(fr, native, lib, call):
    cfg, st, _w = domain_view(fr, native, cap=100)
    a = Arrays(cfg, 12)
    assert calls(lib)[call](cfg, C.byref(st), 5, 5, 100, None, None, None, None) == 0  # y0 == y1 needs no arrays either
    assert calls(lib)[call](cfg, C.byref(st), 12, 12, 40, *a.ptrs()) == 0
    assert calls(lib)[call](cfg, C.byref(st), 3, 2, 100, *a.ptrs()) == INVALID
    assert calls(lib)[call](cfg, C.byref(st), 0, 13, 100, *a.ptrs()) == INVALID
    if call.startswith("extend"):
        assert calls(lib)[call](cfg, C.byref(st), 0, 12, 100, *a.ptrs()) == 0  # M == N
        assert not a.z.any() and not a.it.any() and not a.w.any() and not a.m.any()
        cfg.algo = int(fr.Algo.BarnsleyFern)  # no orbits: the extension does nothing
        assert calls(lib)[call](cfg, C.byref(st), 0, 12, 50, *a.ptrs()) == 0


def test_python_scaled_needs_a_centre(fr):
    c = T.chain(fr.Config.new, "N_900")
    cfg = c.cfg(7)
    with pytest.raises(ValueError, match="scaled= needs centre="):
        fr.escape_rows_pt_state(cfg, scaled=True)
    with pytest.raises(ValueError, match="scaled= needs centre="):
        fr.extend_rows_pt(cfg, np.zeros((12, 16, 2)), np.zeros((12, 16), np.uint32), np.zeros((12, 16, 2)), np.zeros((12, 16), np.uint32),
                          1, scaled=True)
    with pytest.raises(ValueError, match="scaled= needs centre="):
        fr.escape_rows_pt_state_device(cfg, 0, 0, 0, 0, scaled=True)
    with pytest.raises(ValueError, match="scaled= needs centre="):
        fr.extend_rows_pt_device(cfg, 0, 0, 0, 0, 1, pos_lo=(0.0, 0.0), scaled=True)
    centre = fr.WideCentre(c.n, re=c.words[0], im=c.words[1])
    z, it, w, m = fr.escape_rows_pt_state(cfg, y0=4, y1=4, centre=centre, scaled=True)  # no rows: no device
    assert z.shape == (0, 16, 2) and m.shape == (0, 16)
    same = fr.extend_rows_pt(cfg, z, it, w, m, 7, y0=4, y1=4, centre=centre, scaled=True)
    assert same[0].shape == (0, 16, 2)
