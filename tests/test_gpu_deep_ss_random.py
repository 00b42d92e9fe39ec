"""The supersampled, adaptive and kept scaled-DE calls of the deep roads on the device, byte for byte and bit for bit against the
HOST MODELS of cfg_s, on the generated and edge views of tests/deep_ss_views.py: shifted centres, negative and unequal axes, drawn
colour fields with `smooth` and `inside` off, every lane mapping s = 2, 3, 4, 5, 7, 8, images wider than one mark tile.
tests/test_deep_ss_random_cpu.py asserts from the models alone that the set has teeth.  Nothing is compared against the code under
test; every device call gets guarded destinations, the smallest workspace it accepts and a canary behind it; every assertion
message carries the view (config bytes, n and centre words in hex), s and the threshold.
The roads of a view: WIDE PT with the centre and BLA-PT where the view lies inside 2^440; SCALED PT at bits -1 and at the view's
table bits everywhere.
  a. the anchor: the road's existing plain render of cfg_s is soft_colours of the road's model on cfg_s;
  b. fr_render_rows_ss_pt_device, 3 and 4 channels, the drawn row piece and an empty piece, against the box filter of the model image;
  c. fr_render_rows_ss_adaptive_device at thresholds -1, 255, 0 and the view's tau against ss_adaptive_model.adaptive with the
     refined count, and fr_render_rows_ss_adaptive_tf_device with transfer 1 at the view's tau and at -1 against the same model
     with F replaced by the sRGB filter; the three-way split; RGBA; the grid forced to 1 and 2 workgroups and d_refined NULL on one view per seed; the
     dd-centre views of test_gpu_deep_edges.random_config on PT PLAIN and BLA-PT with pos_lo at one drawn s;
  d. fr_render_rows_ss_de_device on WIDE PT and BLA-PT inside 2^440 and fr_render_rows_ss_de_pt_scaled_device everywhere, at the
     view's thickness, at 0 and for the row piece, against ss_de_model.colour over the DE models of cfg_s;
     fr_colour_de_rows_ss_device and fr_colour_rows_ss_device over the arrays the scaled escape calls write for cfg_s;
  e. fr_escape_rows_de_pt_scaled_state_device at the band split N, at min(cap, 1) and at a drawn split in all five arrays, then
     fr_escape_extend_de_pt_scaled_device to the cap; inside 2^440 the state against the wide DE state where the models agree; on
     one view per seed the kept anti-aliased chain: the state of cfg_s at N, extended, recoloured = the supersampled render.
Host forms run on the first view of a seed.  The views of a seed run in one process one after another."""
import ctypes as C

import numpy as np
import pytest

import bla_model as B
import de_model as D
import de_scaled_model as M
import de_scaled_state_model as DSS
import de_state_model as DS
import deep_random_views as G
import deep_ss_views as V
import pt_model as P
import pt_scaled_model as S
import ss_adaptive_de_views as AV
import ss_adaptive_model as A
import ss_de_model as SS
from test_gpu_de import Buf, Rows
from test_gpu_deep_edges import random_config
from test_gpu_deep_random import DeState, drawn_splits
from test_gpu_deep_truth import Road, check, fr, lib, native, torch  # noqa: F401  (fixtures and helpers)
from test_gpu_ss_adaptive import ad_device, ad_host
from test_gpu_ss_deep import BLA, PLAIN, SCALED, ss_pt_device, ss_pt_host, workspace

pytestmark = pytest.mark.gpu

PT = 3


class Case:
    """a view of deep_ss_views with the library's configs and its centre"""

    def __init__(self, fr, native, lib, v):
        self.fr, self.lib, self.v, self.g = fr, lib, v, v.g
        self._road = Road(fr, native, lib, v.g.v)  # keeps the centre alive
        self.centre = self._road.centre
        assert bytes(v.g.dress(self._road.cfg)) == bytes(v.cfg), "the oracle's default config is the library's"
        self.cfg = fr.Config.from_buffer_copy(bytes(v.cfg))
        self.cfg_s = fr.Config.from_buffer_copy(bytes(v.cfg_s))
        self.h, self.w, self.s = v.h, v.w, v.s
        self.what = v.describe()

    def roads(self):
        """(name, road, the call's bits, the model's mode, the model's bits)"""
        g = self.g
        out = []
        if g.wide:
            out.append(("WIDE PT", PLAIN, 0, "wide", -1))
            out.append(("BLA-PT, bits %d" % g.call_bits, BLA, g.call_bits, "bla", g.table_bits))
        out.append(("SCALED PT, bits -1", SCALED, -1, "scaled", -1))
        out.append(("SCALED PT, bits %d" % g.call_bits, SCALED, g.call_bits, "scaled", g.table_bits))
        return out

    def plain(self, road, bits):
        """the road's existing plain render of cfg_s (host form)"""
        cfg, lib = self.cfg_s, self.lib
        out = np.full((cfg.height, cfg.width, 3), 0x5A, dtype=np.uint8)
        tail = (0, cfg.height, 3, out.ctypes.data, out.nbytes)
        if road == PLAIN:
            check(lib.fr_render_rows_pt_wide(C.byref(cfg), self.centre, *tail))
        elif road == BLA:
            check(lib.fr_render_rows_pt_bla(C.byref(cfg), None, self.centre, bits, *tail))
        else:
            check(lib.fr_render_rows_pt_scaled(C.byref(cfg), self.centre, bits, *tail))
        return out

    def at(self, cap, s=1):
        """(the library's config, the oracle's, the orbits) of the view at another cap, of cfg_s for s > 1"""
        low = V.config_s(self.v.cfg, s, cap)
        return self.fr.Config.from_buffer_copy(bytes(low)), low, self.g.orbits(low)


_cases = {}


def case(fr, native, lib, v):
    if v.key not in _cases:
        _cases[v.key] = Case(fr, native, lib, v)
    return _cases[v.key]


def cases_of(fr, native, lib, seed):
    return [case(fr, native, lib, v) for v in V.views(seed)]


def differ(got, want):
    return int((got != want).any(axis=-1).sum()) if got.shape == want.shape else -1


# ---- a, b: the anchor and the supersampled render ------------------------------------------------------------------------------------


def check_anchor_and_ss(c, torch, host):
    v, lib, s, h = c.v, c.lib, c.s, c.h
    for name, road, bits, mode, model_bits in c.roads():
        big = v.image(model_bits, mode)
        got = c.plain(road, bits)
        assert np.array_equal(got, big), "%s: the plain render of cfg_s differs from the model at %d samples; %s" % (name, differ(got, big), c.what)
        want = {ch: A.np_filter(big, s, ch) for ch in (3, 4)}
        mn, best = workspace(lib, c.cfg, s, 0, h)
        assert 0 < mn <= best
        for ch in (3, 4):
            got = ss_pt_device(torch, lib, c.cfg, c.centre, road, bits, s, 0, h, ch, mn)
            assert np.array_equal(got, want[ch]), "%s: fr_render_rows_ss_pt_device, %d channels: %d pixels differ; %s" % (
                name, ch, differ(got, want[ch]), c.what)
        y0, y1 = v.piece
        got = ss_pt_device(torch, lib, c.cfg, c.centre, road, bits, s, y0, y1, 4, workspace(lib, c.cfg, s, y0, y1)[0])
        assert np.array_equal(got, want[4][y0:y1]), "%s: fr_render_rows_ss_pt_device, rows [%d, %d); %s" % (name, y0, y1, c.what)
        assert ss_pt_device(torch, lib, c.cfg, c.centre, road, bits, s, y0, y0, 3, 0).shape == (0, c.w, 3)  # guards and canary hold
        if host:
            got = ss_pt_host(lib, c.cfg, c.centre, road, bits, s, 0, h, 3)
            assert np.array_equal(got, want[3]), "%s: fr_render_rows_ss_pt; %s" % (name, c.what)


@pytest.mark.parametrize("seed", V.SEEDS)
def test_random_views_anchor_and_supersampled_render(fr, native, lib, torch, seed):
    for k, c in enumerate(cases_of(fr, native, lib, seed)):
        check_anchor_and_ss(c, torch, host=k == 0)


# ---- c: adaptive supersampling -------------------------------------------------------------------------------------------------------


def check_adaptive(c, torch, extras):
    """extras: the forced grids, d_refined NULL and the host form as well"""
    v, lib, s = c.v, c.lib, c.s
    for name, road, bits, mode, model_bits in c.roads():
        big = v.image(model_bits, mode)
        kw = dict(precision=PT, centre=c.centre, road=road, bits=bits)

        def run(tau, what="", **more):
            want, count = A.adaptive(big, s, tau, more.get("y0", 0), more.get("y1"), more.get("channels", 3),
                                     filter=AV.FILTERS[more.get("transfer") or 0])
            got, n = ad_device(torch, lib, c.cfg, s, tau, **more, **kw)
            assert np.array_equal(got, want) and n == count, "%s, threshold %d%s: %d pixels differ, refined %d, the model %d; %s" % (
                name, tau, what, differ(got, want), n, count, c.what)

        for tau in dict.fromkeys((-1, 255, 0, v.tau)):
            run(tau)
        for tau in dict.fromkeys((v.tau, -1)):  # the LINEAR instance of the road's refine kernel: F is the sRGB filter
            run(tau, ", transfer 1", transfer=1)
        if v.three_way() is not None:
            for y0, y1 in v.three_way():  # each piece against its slice: the bytes concatenate to the whole, the counts sum
                run(v.tau, ", rows [%d, %d)" % (y0, y1), y0=y0, y1=y1)
        run(v.tau, ", RGBA", channels=4)
        if extras:
            try:
                for groups in (1, 2):
                    check(lib.fr_debug_ss_adaptive_grid(groups))
                    for tau in dict.fromkeys((-1, v.tau)):
                        run(tau, ", %d workgroups" % groups)
            finally:
                check(lib.fr_debug_ss_adaptive_grid(0))
            want, count = A.adaptive(big, s, v.tau)
            got, _ = ad_device(torch, lib, c.cfg, s, v.tau, want_refined=False, **kw)
            assert np.array_equal(got, want), "%s, d_refined NULL; %s" % (name, c.what)
            got, n = ad_host(lib, c.cfg, s, v.tau, **kw)
            assert np.array_equal(got, want) and n == count, "%s: fr_render_rows_ss_adaptive; %s" % (name, c.what)


@pytest.mark.parametrize("seed", V.SEEDS)
def test_random_views_adaptive(fr, native, lib, torch, seed):
    for k, c in enumerate(cases_of(fr, native, lib, seed)):
        check_adaptive(c, torch, extras=k == 0)


@pytest.mark.parametrize("seed", G.SEEDS)
def test_random_dd_centre_views_adaptive(fr, native, lib, torch, seed):
    """PT PLAIN and BLA-PT with pos_lo.  H is the existing fr_render_rows_pt / fr_render_rows_pt_bla of cfg_s, itself anchored to
    pt_model / bla_model on the view of the seed with the least work"""
    rng = np.random.default_rng(G.DD_BASE_SEED + seed)
    drawn = [random_config(fr, rng) for _ in range(G.DD_PER_SEED)]  # nothing else is drawn from rng
    sizes = [V.dd_supersample(seed, k, cfg) for k, (cfg, _) in enumerate(drawn)]
    anchor = int(np.argmin([s * s * cfg.width * cfg.height * max(cfg.iterations, 1) for s, (cfg, _) in zip(sizes, drawn)]))
    for k, (cfg, lo) in enumerate(drawn):
        s = sizes[k]
        what = "config %s, pos_lo %s %s, seed %d, s %d" % (bytes(cfg).hex(), float(lo[0]).hex(), float(lo[1]).hex(), seed, s)
        cfg_s = cfg.clone()
        cfg_s.width, cfg_s.height = s * cfg.width, s * cfg.height
        plo = C.byref(native.Imaginary(*lo))
        bits = (0, 24, 40, 53)[(cfg.width + cfg.height) % 4]
        orbits = cfg.algo in (0, 2)
        pt = np.full((cfg_s.height, cfg_s.width, 3), 0x5A, dtype=np.uint8)
        check(lib.fr_render_rows_pt(C.byref(cfg_s), plo, 0, cfg_s.height, 3, pt.ctypes.data, pt.nbytes))
        bla = np.full_like(pt, 0x5A)
        check(lib.fr_render_rows_pt_bla(C.byref(cfg_s), plo, None, bits, 0, cfg_s.height, 3, bla.ctypes.data, bla.nbytes))
        if k == anchor:
            z, it = P.escape_rows(cfg_s, lo)
            assert np.array_equal(pt, V.soft_colours(cfg_s, z, it)), "fr_render_rows_pt of cfg_s against pt_model; " + what
            if orbits:
                x = P.reference_orbit(cfg_s, lo, 0)
                kk = P.reference_orbit(cfg_s, lo, 1) if cfg.algo == 2 else None
                z, it = B.escape_rows(cfg_s, x, kk, bits or 40)[:2]
            assert np.array_equal(bla, V.soft_colours(cfg_s, z, it)), "fr_render_rows_pt_bla of cfg_s against bla_model; " + what
        for name, road, rbits, big in (("PT", PLAIN, 0, pt), ("BLA-PT, bits %d" % bits, BLA, bits, bla)):
            for tau in dict.fromkeys((-1, 255, V.median_tau(big, s))):
                want, count = A.adaptive(big, s, tau, escape_algo=orbits)
                got, n = ad_device(torch, lib, cfg, s, tau, precision=PT, pos_lo=plo, road=road, bits=rbits)
                assert np.array_equal(got, want) and n == count, "%s, threshold %d: %d pixels differ, refined %d, the yardstick %d; %s" % (
                    name, tau, differ(got, want), n, count, what)


# ---- d: supersampled DE --------------------------------------------------------------------------------------------------------------


def ss_de_device(torch, lib, c, road, bits, thickness, y0, y1, channels):
    """fr_render_rows_ss_de_device (WIDE PT, BLA-PT) or fr_render_rows_ss_de_pt_scaled_device with the smallest workspace"""
    need = channels * c.w * (y1 - y0)
    work_len = c.fr.ss_de_workspace_bytes(c.cfg, c.s, y0, y1)[0]
    work, out = Buf(torch, work_len), Buf(torch, need)
    if road == SCALED:
        check(lib.fr_render_rows_ss_de_pt_scaled_device(C.byref(c.cfg), c.centre, bits, thickness, c.s, y0, y1, channels, out.ptr, need,
                                                        work.ptr, work_len, None))
    else:
        check(lib.fr_render_rows_ss_de_device(C.byref(c.cfg), PT, None, c.centre, road, bits, thickness, c.s, y0, y1, channels, out.ptr, need,
                                              work.ptr, work_len, None))
    got = out.get(np.uint8, (y1 - y0, c.w, channels))
    work.get(np.uint8)  # its guards
    return got


def check_ss_de(c, torch, host):
    v, g, lib, s, h, w = c.v, c.g, c.lib, c.s, c.h, c.w
    thick = v.thickness
    cfg_v = M.scaled_view(v.cfg)
    lib_view = c.fr.de_scaled_view(c.cfg)
    assert bytes(lib_view) == bytes(cfg_v), "fr_de_scaled_view; " + c.what
    roads = []
    if g.wide:
        assert g.draw.limit <= 2.0 ** 20
        roads.append(("WIDE PT", PLAIN, 0, "de_wide", -1, v.cfg))
        roads.append(("BLA-PT, bits %d" % g.call_bits, BLA, g.call_bits, "de_bla", g.table_bits, v.cfg))
    roads.append(("SCALED PT, bits -1", SCALED, -1, "de_scaled", -1, cfg_v))
    roads.append(("SCALED PT, bits %d" % g.call_bits, SCALED, g.call_bits, "de_scaled", g.table_bits, cfg_v))
    y0, y1 = v.piece
    for name, road, bits, mode, model_bits, mcfg in roads:
        z, it, der = v.rows(mode, model_bits)[:3]
        for t in (thick, 0.0):
            want = SS.colour(mcfg, z, it, der, s, t, 3)
            got = ss_de_device(torch, lib, c, road, bits, t, 0, h, 3)
            assert np.array_equal(got, want), "%s: the supersampled DE render at thickness %r: %d pixels differ; %s" % (
                name, t, differ(got, want), c.what)
        want = SS.colour(mcfg, z, it, der, s, thick, 4)
        got = ss_de_device(torch, lib, c, road, bits, thick, y0, y1, 4)
        assert np.array_equal(got, want[y0:y1]), "%s: the supersampled DE render of rows [%d, %d), RGBA; %s" % (name, y0, y1, c.what)
        if host:
            got = np.full((h, w, 4), 0x5A, dtype=np.uint8)
            if road == SCALED:
                check(lib.fr_render_rows_ss_de_pt_scaled(C.byref(c.cfg), c.centre, bits, thick, s, 0, h, 4, got.ctypes.data, got.nbytes))
            else:
                check(lib.fr_render_rows_ss_de(C.byref(c.cfg), PT, None, c.centre, road, bits, thick, s, 0, h, 4, got.ctypes.data, got.nbytes))
            assert np.array_equal(got, want), "%s: the host form of the supersampled DE render; %s" % (name, c.what)
        if road != SCALED:
            continue
        # the kept arrays of cfg_s, recoloured: with the derivative, and without
        r = Rows(torch, s * h, s * w)
        check(lib.fr_escape_rows_de_pt_scaled_device(C.byref(c.cfg_s), c.centre, bits, 0, s * h, r.z.ptr, r.it.ptr, r.der.ptr, None))
        kept = r.get()
        assert np.array_equal(kept[1], it) and S.same_bits(kept[0], z) and D.same_doubles(kept[2], der), (
            "fr_escape_rows_de_pt_scaled_device on cfg_s, bits %d; %s" % (bits, c.what))
        big = v.image(model_bits, "scaled")
        pz, pit = Buf(torch, 16 * r.n), Buf(torch, 4 * r.n)
        check(lib.fr_escape_rows_pt_scaled_device(C.byref(c.cfg_s), c.centre, bits, 0, s * h, pz.ptr, pit.ptr, None))
        sz, sit = v.rows("scaled", model_bits)[:2]
        assert np.array_equal(pit.get(np.uint32, sit.shape), sit) and S.same_bits(pz.get(np.float64, sz.shape), sz), (
            "fr_escape_rows_pt_scaled_device on cfg_s, bits %d; %s" % (bits, c.what))
        for ch in (3, 4):
            need = ch * w * h
            out = Buf(torch, need)
            check(lib.fr_colour_de_rows_ss_device(C.byref(lib_view), r.z.ptr, r.it.ptr, r.der.ptr, w, h, s, thick, ch, out.ptr, need, None))
            want = SS.colour(cfg_v, z, it, der, s, thick, ch)
            got = out.get(np.uint8, (h, w, ch))
            assert np.array_equal(got, want), "fr_colour_de_rows_ss_device, bits %d, %d channels: %d pixels differ; %s" % (
                bits, ch, differ(got, want), c.what)
            out = Buf(torch, need)
            check(lib.fr_colour_rows_ss_device(C.byref(c.cfg), pz.ptr, 2, pit.ptr, w, h, s, ch, out.ptr, need, None))
            want = A.np_filter(big, s, ch)
            got = out.get(np.uint8, (h, w, ch))
            assert np.array_equal(got, want), "fr_colour_rows_ss_device, bits %d, %d channels: %d pixels differ; %s" % (
                bits, ch, differ(got, want), c.what)


@pytest.mark.parametrize("seed", V.SEEDS)
def test_random_views_supersampled_de(fr, native, lib, torch, seed):
    for k, c in enumerate(cases_of(fr, native, lib, seed)):
        check_ss_de(c, torch, host=k == 0)


# ---- e: the kept scaled DE view ----------------------------------------------------------------------------------------------------------


def same_as_wide(scaled, wide, e):
    """a scaled DE state against the wide DE state: w = dz 2^e and der = u 2^e, both exactly"""
    return DS.same_state((scaled[0], scaled[1], scaled[2], scaled[3], np.ldexp(scaled[4], e)),
                         (wide[0], wide[1], np.ldexp(wide[2], e), wide[3], wide[4]))


def check_kept_de(c, torch, splits):
    """-> the number of splits at which the state was also compared with the wide DE state"""
    v, g, lib, h = c.v, c.g, c.lib, c.h
    whole = DSS.state_rows(v.cfg, v.orbits)
    e = S.exponent(v.cfg)
    compared = 0
    for n in splits:
        low, low_model, low_orbits = c.at(n)
        st = DeState(torch, g.shape)
        check(lib.fr_escape_rows_de_pt_scaled_state_device(C.byref(low), c.centre, 0, h, *st.ptrs, None))
        got, want = st.read(), DSS.state_rows(low_model, low_orbits)
        assert DSS.same_state(got, want), "the scaled DE state at %d; %s" % (n, c.what)
        if g.wide:
            model_wide = DS.pt_wide_state_rows(low_model, low_orbits)
            if same_as_wide(want, model_wide, e):  # the models decide where the claim applies (no subnormal u or w)
                wide = DeState(torch, g.shape)
                check(lib.fr_escape_rows_de_pt_state_device(C.byref(low), None, c.centre, 0, h, *wide.ptrs, None))
                assert same_as_wide(got, wide.read(), e), "the scaled DE state at %d against the wide DE state; %s" % (n, c.what)
                compared += 1
        check(lib.fr_escape_extend_de_pt_scaled_device(C.byref(c.cfg), c.centre, 0, h, n, *st.ptrs, None))
        assert DSS.same_state(st.read(), whole), "the scaled DE state extended %d -> %d; %s" % (n, g.cap, c.what)
    return compared


def check_kept_chain(c, torch):
    """§3.27's kept anti-aliased view: the state of cfg_s at N, extended to the cap, recoloured = the supersampled render"""
    v, lib, s, h, w = c.v, c.lib, c.s, c.h, c.w
    n = v.split if v.split is not None else min(c.g.cap, 1)
    low = c.at(n, s)[0]
    st = DeState(torch, (s * h, s * w))
    check(lib.fr_escape_rows_de_pt_scaled_state_device(C.byref(low), c.centre, 0, s * h, *st.ptrs, None))
    check(lib.fr_escape_extend_de_pt_scaled_device(C.byref(c.cfg_s), c.centre, 0, s * h, n, *st.ptrs, None))
    got = st.read()
    z, it, u = v.rows("de_scaled", -1)[:3]
    assert np.array_equal(got[1], it) and S.same_bits(got[0], z) and D.same_doubles(got[4], u), (
        "the state of cfg_s extended %d -> %d against the DE model of cfg_s; %s" % (n, c.g.cap, c.what))
    need = 3 * w * h
    out = Buf(torch, need)
    view = c.fr.de_scaled_view(c.cfg)
    check(lib.fr_colour_de_rows_ss_device(C.byref(view), st.ptrs[0], st.ptrs[1], st.ptrs[4], w, h, s, v.thickness, 3, out.ptr, need, None))
    want = SS.colour(M.scaled_view(v.cfg), z, it, u, s, v.thickness, 3)
    got = out.get(np.uint8, (h, w, 3))
    assert np.array_equal(got, want), "the kept anti-aliased view recoloured: %d pixels differ; %s" % (differ(got, want), c.what)


def splits_of(v, drawn):
    return sorted(set(drawn) | ({v.split} if v.split is not None else set()))


@pytest.mark.parametrize("seed", V.SEEDS)
def test_random_views_kept_scaled_de(fr, native, lib, torch, seed):
    rng = np.random.default_rng([G.BASE_SEED + seed, 9])
    cases = cases_of(fr, native, lib, seed)
    compared = 0
    for c in cases:
        compared += check_kept_de(c, torch, splits_of(c.v, drawn_splits(rng, c.g.cap)))
    print("seed %d: %d splits compared with the wide DE state" % (seed, compared))
    with_split = [c for c in cases if c.v.split is not None]
    check_kept_chain((with_split or cases)[0], torch)


# ---- the edge views -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(G.EDGES))
def test_edge_views(fr, native, lib, torch, name):
    c = case(fr, native, lib, V.edge(name))
    check_anchor_and_ss(c, torch, host=True)
    check_adaptive(c, torch, extras=True)
    check_ss_de(c, torch, host=True)
    check_kept_de(c, torch, splits_of(c.v, {c.g.cap // 3, min(c.g.cap, 1)}))
    check_kept_chain(c, torch)
