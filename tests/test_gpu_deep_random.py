"""The wide-centre deep roads on the device against their host models BIT FOR BIT, on the generated and edge views of
tests/deep_random_views.py: shifted centres, scales whose mantissa is not 1, negative and unequal axes, spare centre words,
reference orbits ended by escape, every limit and cap of the generator, sizes from 1 x 1 to 48 x 40.  tests/test_deep_random_cpu.py
asserts that this set is worth running and that the models follow exact orbits on it.  The models run on pt_wide_model's
Python-integer orbits; every assertion message carries the view (config bytes, n and centre words in hex).
  - escape rows: fr_escape_rows_pt_wide, fr_escape_rows_pt_bla(_device) with the centre, fr_escape_rows_pt_scaled(_device) without
    and with a table; the pass counts of fr_debug_bla_count and fr_debug_pt_scaled_count; device forms on every view, host forms on
    the first view of a seed;
  - fr_debug_reference_orbit_wide against the integers' orbit, its end by escape included;
  - RGB and RGBA renders of each road against the oracle's soft-log2 colour map over the model's arrays, with drawn colour fields;
  - WIDE PT's and SCALED PT's state at a drawn cap N, at min(cap, 1) and at the view's band split (tests/deep_ss_views.py), and its
    extension to the cap, in all four arrays;
  - DE: fr_escape_rows_de_pt_wide, fr_escape_rows_de_pt_bla and the wide DE state with its extension inside 2^440;
    fr_escape_rows_de_pt_scaled without and with a table everywhere, then fr_distance_rows_device and fr_colour_de_rows_device on
    fr_de_scaled_view's config with a drawn thickness;
  - a drawn row piece [y0, y1), y0 == y1 included, of one road per view against the slice of the whole;
  - the edge views through all of it with fixed choices;
  - the dd-centre views of test_gpu_deep_edges.random_config on BLA-PT's pos_lo form, fr_escape_rows_de (PT; F64 where the scale
    permits) and fr_escape_rows_de_pt_bla, against bla_model, de_model and de_bla_model on pt_model's orbits.
The views of a seed run in one process one after another, and nothing resets the context between them: the orbit cache and the
table slot serve, continue and rebuild across unrelated views."""
import ctypes as C

import numpy as np
import pytest

import bla_model as B
import de_bla_model as DB
import de_model as D
import de_scaled_model as M
import de_state_model as DS
import deep_random_views as G
import deep_ss_views as V
import pt_model as P
import pt_scaled_model as S
import pt_scaled_state_model as R
import pt_wide_model as W
from test_gpu_de import Buf, Rows
from test_gpu_deep_edges import random_config, soft_colours
from test_gpu_deep_truth import Road, State, check, fr, lib, native, torch  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

THICKNESSES = (0.0, 0.5, 1.0, None)  # None: 2^20 / height


class Case:
    """a generated view with its calls (test_gpu_deep_truth.Road), its orbits and its models, each computed once"""

    def __init__(self, fr, native, lib, g):
        self.fr, self.native, self.lib, self.g = fr, native, lib, g
        self.road = Road(fr, native, lib, g.v)
        g.dress(self.road.cfg)
        self.cfg, self.centre = self.road.cfg, self.road.centre
        self.orbits = g.orbits(self.cfg)
        self.x, self.k = self.orbits.x[0], (self.orbits.k[0] if g.julia else None)
        self.what = g.describe(self.cfg)
        self.h, self.w = g.shape
        self._models = {}

    def at(self, cap):
        """(config, orbits) of the view at another cap"""
        cfg = self.g.cfg(self.fr.Config.new, cap)
        return cfg, self.g.orbits(cfg)

    def model(self, mode, bits=-1):
        key = (mode, bits)
        if key not in self._models:
            cfg, x, k = self.cfg, self.x, self.k
            if mode == "wide":
                (z, it, _, _), _ = W.state_rows(cfg, self.orbits, rule=1)
                r = (z, it)
            elif mode == "bla":
                r = B.escape_rows(cfg, x, k, bits)
            elif mode == "scaled":
                r = S.escape_rows(cfg, x, k, bits)
            elif mode == "de_wide":
                r = D.pt_wide_rows(cfg, self.orbits)
            elif mode == "de_bla":
                r = DB.escape_rows(cfg, x, k, bits)
            elif mode == "de_scaled":
                r = M.escape_rows(cfg, x, k, bits)
            else:
                raise KeyError(mode)
            self._models[key] = r
        return self._models[key]


_cases = {}


def case(fr, native, lib, key):
    """the Case of (seed, k) or of an edge view's name, made once per process"""
    if key not in _cases:
        g = G.edge(key) if isinstance(key, str) else G.views(key[0])[key[1]]
        _cases[key] = Case(fr, native, lib, g)
    return _cases[key]


def cases_of(fr, native, lib, seed):
    return [case(fr, native, lib, (seed, k)) for k in range(G.PER_SEED)]


def same(a, b):
    return S.same_bits(a, b)


def assert_rows(got, want, c, what):
    assert got[1].shape == want[1].shape, "%s: shape; %s" % (what, c.what)
    assert np.array_equal(got[1], want[1]), "%s: escape indices differ at %d pixels; %s" % (what, int((got[1] != want[1]).sum()), c.what)
    assert same(got[0], want[0]), "%s: z differs; %s" % (what, c.what)


def assert_de(got, want, c, what):
    assert_rows(got, want, c, what)
    assert D.same_doubles(got[2], want[2]), "%s: der differs; %s" % (what, c.what)


# ---- escape rows and pass counts --------------------------------------------------------------------------------------------------


def check_escape_rows(c, torch, host):
    g, road, lib = c.g, c.road, c.lib
    cfg, h = C.byref(c.cfg), c.h
    a, b = C.c_uint64(0), C.c_uint64(0)
    if g.wide:
        assert_rows(road.rows("wide"), c.model("wide"), c, "fr_escape_rows_pt_wide")
        want = c.model("bla", g.table_bits)
        assert_rows(road.rows("bla", g.call_bits, True, torch), want, c, "fr_escape_rows_pt_bla_device, bits %d" % g.call_bits)
        if host:
            assert_rows(road.rows("bla", g.call_bits), want, c, "fr_escape_rows_pt_bla, bits %d" % g.call_bits)
        check(lib.fr_debug_bla_count(cfg, None, c.centre, g.call_bits, 0, h, C.byref(a), C.byref(b)))
        assert (a.value, b.value) == (int(want[2].astype(np.uint64).sum()), B.steps(c.cfg, want[1])), "fr_debug_bla_count; " + c.what
    for bits, model_bits in ((-1, -1), (g.call_bits, g.table_bits)):
        want = c.model("scaled", model_bits)
        assert_rows(road.rows("scaled", bits, True, torch), want, c, "fr_escape_rows_pt_scaled_device, bits %d" % bits)
        if host:
            assert_rows(road.rows("scaled", bits), want, c, "fr_escape_rows_pt_scaled, bits %d" % bits)
        check(lib.fr_debug_pt_scaled_count(cfg, c.centre, bits, 0, h, C.byref(a), C.byref(b)))
        assert (a.value, b.value) == (int(want[2].astype(np.uint64).sum()), S.steps(c.cfg, want[1])), (
            "fr_debug_pt_scaled_count, bits %d; %s" % (bits, c.what))


def check_orbit(c):
    """the library's orbit is the integers', entry for entry; an orbit ended by escape ends at the same entry.  The call's domain
    is WIDE PT's and an orbit does not depend on the scale, so a view past 2^440 asks with a scale of 2^50."""
    cfg = c.fr.Config.from_buffer_copy(bytes(c.cfg))
    if not c.g.wide:
        cfg.scale.re = cfg.scale.im = 2.0 ** 50
    for which, (want, ended, _) in ((0, c.orbits.x), (1, c.orbits.k)):
        if which == 1 and not c.g.julia:
            continue
        n = C.c_uint32()
        check(c.lib.fr_debug_reference_orbit_wide(C.byref(cfg), c.centre, which, None, 0, C.byref(n)))
        assert n.value == len(want), "orbit %d has %d entries, the integers' %d; %s" % (which, n.value, len(want), c.what)
        got = np.full((n.value, 2), np.nan)
        check(c.lib.fr_debug_reference_orbit_wide(C.byref(cfg), c.centre, which, got.ctypes.data, n.value, C.byref(n)))
        assert same(got, want), "orbit %d differs; %s" % (which, c.what)
        last = len(want) - 1  # the model's own flag is what the entries say: the last one is past 2 and was tested (k >= kmin)
        assert bool(ended) == (last >= (1 if c.g.julia else 2) and float(want[-1, 0] ** 2 + want[-1, 1] ** 2) > 4.0), c.what


@pytest.mark.parametrize("seed", G.SEEDS)
def test_random_views_escape_rows_counts_and_orbits(fr, native, lib, torch, seed):
    for k, c in enumerate(cases_of(fr, native, lib, seed)):
        check_escape_rows(c, torch, host=k == 0)
        check_orbit(c)


# ---- renders ---------------------------------------------------------------------------------------------------------------------


def check_renders(c):
    g, lib, cfg, h, w = c.g, c.lib, C.byref(c.cfg), c.h, c.w
    roads = []
    if g.wide:
        roads.append(("fr_render_rows_pt_wide", c.model("wide"),
                      lambda ch, out: lib.fr_render_rows_pt_wide(cfg, c.centre, 0, h, ch, out.ctypes.data, out.nbytes)))
        roads.append(("fr_render_rows_pt_bla", c.model("bla", g.table_bits),
                      lambda ch, out: lib.fr_render_rows_pt_bla(cfg, None, c.centre, g.call_bits, 0, h, ch, out.ctypes.data, out.nbytes)))
    roads.append(("fr_render_rows_pt_scaled, plain", c.model("scaled", -1),
                  lambda ch, out: lib.fr_render_rows_pt_scaled(cfg, c.centre, -1, 0, h, ch, out.ctypes.data, out.nbytes)))
    roads.append(("fr_render_rows_pt_scaled, table", c.model("scaled", g.table_bits),
                  lambda ch, out: lib.fr_render_rows_pt_scaled(cfg, c.centre, g.call_bits, 0, h, ch, out.ctypes.data, out.nbytes)))
    for name, want, call in roads:
        for channels in (3, 4):
            out = np.full((h, w, channels), 0x5A, dtype=np.uint8)
            check(call(channels, out))
            colours = soft_colours(c.cfg, want[0], want[1], rgba=channels == 4)
            assert np.array_equal(out, colours), "%s, %d channels: %d pixels differ; %s" % (
                name, channels, int((out != colours).any(-1).sum()), c.what)


@pytest.mark.parametrize("seed", G.SEEDS)
def test_random_views_renders(fr, native, lib, seed):
    for c in cases_of(fr, native, lib, seed):
        check_renders(c)


# ---- state and extension ------------------------------------------------------------------------------------------------------------


def check_states(c, torch, splits):
    lib, h, w = c.lib, c.h, c.w
    kinds = [("SCALED PT", lib.fr_escape_rows_pt_scaled_state_device, lib.fr_escape_extend_pt_scaled_device,
              lambda cfg, orbits: R.state_rows(cfg, orbits)[0])]
    if c.g.wide:
        kinds.append(("WIDE PT", lib.fr_escape_rows_pt_wide_state_device, lib.fr_escape_extend_pt_wide_device,
                      lambda cfg, orbits: W.state_rows(cfg, orbits, rule=0)[0]))
    for name, render, extend, model in kinds:
        whole = model(c.cfg, c.orbits)
        for n in splits:
            low, low_orbits = c.at(n)
            st = State(torch, h * w)
            check(render(C.byref(low), c.centre, 0, h, *st.ptrs, None))
            assert W.same_state(st.read(c.g.shape), model(low, low_orbits)), "%s: the state at %d; %s" % (name, n, c.what)
            check(extend(C.byref(c.cfg), c.centre, 0, h, n, *st.ptrs, None))
            assert W.same_state(st.read(c.g.shape), whole), "%s: the state extended %d -> %d; %s" % (name, n, c.g.cap, c.what)


def drawn_splits(rng, cap):
    return sorted({int(rng.integers(0, cap)) if cap > 0 else 0, min(cap, 1)})


def with_band_split(splits, v):
    """the splits and the view's band split N of tests/deep_ss_views.py (the median escaped index + 1): where a view has one, pixels
    finished before N stand beside pixels escaping after it on a third of the views, which a drawn split almost never gives"""
    return sorted(set(splits) | ({v.split} if v.split is not None else set()))


@pytest.mark.parametrize("seed", G.SEEDS)
def test_random_views_state_and_extension(fr, native, lib, torch, seed):
    rng = np.random.default_rng([G.BASE_SEED + seed, 1])
    for k, c in enumerate(cases_of(fr, native, lib, seed)):
        check_states(c, torch, with_band_split(drawn_splits(rng, c.g.cap), V.all_of(seed)[k]))


# ---- distance estimation -------------------------------------------------------------------------------------------------------------


class DeState:
    """(z, iters, dz, m, der) of `npx` pixels in guarded device memory"""

    def __init__(self, torch, shape):
        n = shape[0] * shape[1]
        self.shape = shape
        self.bufs = [Buf(torch, s * n) for s in (16, 4, 16, 4, 16)]
        self.ptrs = [b.ptr for b in self.bufs]

    def read(self):
        types = (np.float64, np.uint32, np.float64, np.uint32, np.float64)
        return tuple(b.get(t, self.shape + ((2,) if t is np.float64 else ())) for b, t in zip(self.bufs, types))


def check_de(c, torch, splits, thickness):
    g, lib, cfg, h, w = c.g, c.lib, C.byref(c.cfg), c.h, c.w
    if g.wide:
        r = Rows(torch, h, w)
        check(lib.fr_escape_rows_de_pt_wide_device(cfg, c.centre, 0, h, r.z.ptr, r.it.ptr, r.der.ptr, None))
        assert_de(r.get(), c.model("de_wide"), c, "fr_escape_rows_de_pt_wide_device")
        r = Rows(torch, h, w)
        check(lib.fr_escape_rows_de_pt_bla_device(cfg, None, c.centre, g.call_bits, 0, h, r.z.ptr, r.it.ptr, r.der.ptr, None))
        assert_de(r.get(), c.model("de_bla", g.table_bits), c, "fr_escape_rows_de_pt_bla_device, bits %d" % g.call_bits)
        whole = DS.pt_wide_state_rows(c.cfg, c.orbits)
        for n in splits:
            low, low_orbits = c.at(n)
            st = DeState(torch, g.shape)
            check(lib.fr_escape_rows_de_pt_state_device(C.byref(low), None, c.centre, 0, h, *st.ptrs, None))
            assert DS.same_state(st.read(), DS.pt_wide_state_rows(low, low_orbits)), "the DE state at %d; %s" % (n, c.what)
            check(lib.fr_escape_extend_de_pt_device(cfg, None, c.centre, 0, h, n, *st.ptrs, None))
            assert DS.same_state(st.read(), whole), "the DE state extended %d -> %d; %s" % (n, g.cap, c.what)
    view = c.fr.de_scaled_view(c.cfg)
    assert bytes(view) == bytes(M.scaled_view(c.cfg)), "fr_de_scaled_view; " + c.what
    t = 2.0 ** 20 / h if thickness is None else thickness
    for bits, model_bits in ((-1, -1), (g.call_bits, g.table_bits)):
        want = c.model("de_scaled", model_bits)
        r = Rows(torch, h, w)
        check(lib.fr_escape_rows_de_pt_scaled_device(cfg, c.centre, bits, 0, h, r.z.ptr, r.it.ptr, r.der.ptr, None))
        assert_de(r.get(), want, c, "fr_escape_rows_de_pt_scaled_device, bits %d" % bits)
        dist = Buf(torch, 8 * r.n)
        check(lib.fr_distance_rows_device(C.byref(view), r.z.ptr, r.it.ptr, r.der.ptr, r.n, dist.ptr, None))
        assert D.same_doubles(dist.get(np.float64, r.shape), D.distance(view, *want[:3])), "fr_distance_rows_device, bits %d; %s" % (bits, c.what)
        for channels in (3, 4):
            out = Buf(torch, channels * r.n)
            check(lib.fr_colour_de_rows_device(C.byref(view), r.z.ptr, r.it.ptr, r.der.ptr, r.n, t, channels, out.ptr, None))
            colours = D.colour(view, *want[:3], t, channels)
            got = out.get(np.uint8, r.shape + (channels,))
            assert np.array_equal(got, colours), "fr_colour_de_rows_device, bits %d, thickness %r, %d channels: %d pixels differ; %s" % (
                bits, t, channels, int((got != colours).any(-1).sum()), c.what)


@pytest.mark.parametrize("seed", G.SEEDS)
def test_random_views_distance_estimation(fr, native, lib, torch, seed):
    rng = np.random.default_rng([G.BASE_SEED + seed, 2])
    for k, c in enumerate(cases_of(fr, native, lib, seed)):
        splits = with_band_split(drawn_splits(rng, c.g.cap), V.all_of(seed)[k])
        check_de(c, torch, splits, THICKNESSES[int(rng.integers(len(THICKNESSES)))])


# ---- a row piece ---------------------------------------------------------------------------------------------------------------------


def check_row_piece(c, torch, mode, y0, y1):
    bits = {"wide": -1, "bla": c.g.call_bits, "scaled": -1, "table": c.g.call_bits}[mode]
    model_bits = {"wide": -1, "bla": c.g.table_bits, "scaled": -1, "table": c.g.table_bits}[mode]
    call = "scaled" if mode == "table" else mode
    want = c.model(call, model_bits)
    got = c.road.rows(call, bits, call != "wide", torch, y0, y1)
    assert_rows(got, (want[0][y0:y1], want[1][y0:y1]), c, "rows [%d, %d) of %s, bits %d" % (y0, y1, call, bits))


@pytest.mark.parametrize("seed", G.SEEDS)
def test_random_views_row_pieces(fr, native, lib, torch, seed):
    rng = np.random.default_rng([G.BASE_SEED + seed, 3])
    for c in cases_of(fr, native, lib, seed):
        modes = (("wide", "bla") if c.g.wide else ()) + ("scaled", "table")
        mode = modes[int(rng.integers(len(modes)))]
        y0 = int(rng.integers(0, c.h + 1))
        y1 = int(rng.integers(y0, c.h + 1))
        check_row_piece(c, torch, mode, y0, y1)
        check_row_piece(c, torch, mode, y0, y0)


# ---- the edge views ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(G.EDGES))
def test_edge_views(fr, native, lib, torch, name):
    c = case(fr, native, lib, name)
    splits = with_band_split({c.g.cap // 3, min(c.g.cap, 1)}, V.edge(name))
    check_escape_rows(c, torch, host=True)
    check_orbit(c)
    check_renders(c)
    check_states(c, torch, splits)
    check_de(c, torch, splits, 1.0)
    for mode in (("wide", "bla") if c.g.wide else ()) + ("scaled", "table"):
        check_row_piece(c, torch, mode, c.h // 3, c.h - c.h // 3)
        check_row_piece(c, torch, mode, c.h // 2, c.h // 2)


# ---- dd-centre views: BLA-PT and DE ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("seed", G.SEEDS)
def test_random_dd_centre_views_on_bla_pt_and_de(fr, native, lib, seed):
    rng = np.random.default_rng(G.DD_BASE_SEED + seed)
    for _ in range(G.DD_PER_SEED):
        cfg, lo = random_config(fr, rng)  # the draws of tests/test_deep_random_cpu.py: nothing else is drawn from rng
        what = "config %s, pos_lo %s %s, seed %d" % (bytes(cfg).hex(), float(lo[0]).hex(), float(lo[1]).hex(), seed)
        h, w = cfg.height, cfg.width
        bits = (0, 24, 40, 53)[(cfg.width + cfg.height) % 4]
        model_bits = bits or 40
        c_lo = native.Imaginary(*lo)
        orbits = cfg.algo in (0, 2)
        x = P.reference_orbit(cfg, lo, 0) if orbits else None
        k = P.reference_orbit(cfg, lo, 1) if cfg.algo == 2 else None

        def arrays():
            return np.full((h, w, 2), np.nan), np.full((h, w), 0xFFFFFFFF, dtype=np.uint32), np.full((h, w, 2), np.nan)

        assert G.dd_domain(cfg, "bla")
        z, it, _ = arrays()
        check(lib.fr_escape_rows_pt_bla(C.byref(cfg), C.byref(c_lo), None, bits, 0, h, z.ctypes.data, it.ctypes.data))
        if orbits:
            want = B.escape_rows(cfg, x, k, model_bits)
            assert np.array_equal(it, want[1]) and same(z, want[0]), "fr_escape_rows_pt_bla, bits %d; %s" % (bits, what)
        else:
            assert not z.any() and not it.any(), "an algorithm without orbits writes zeros; " + what
        if G.dd_domain(cfg, "de_pt"):
            z, it, der = arrays()
            check(lib.fr_escape_rows_de(C.byref(cfg), 3, C.byref(c_lo), 0, h, z.ctypes.data, it.ctypes.data, der.ctypes.data))
            want = D.pt_rows(cfg, lo)
            assert np.array_equal(it, want[1]) and same(z, want[0]) and D.same_doubles(der, want[2]), "fr_escape_rows_de, PT; " + what
            z, it, der = arrays()
            check(lib.fr_escape_rows_de_pt_bla(C.byref(cfg), C.byref(c_lo), None, bits, 0, h, z.ctypes.data, it.ctypes.data, der.ctypes.data))
            want = DB.escape_rows(cfg, x, k, model_bits)
            assert np.array_equal(it, want[1]) and same(z, want[0]) and D.same_doubles(der, want[2]), (
                "fr_escape_rows_de_pt_bla, bits %d; %s" % (bits, what))
        if G.dd_domain(cfg, "de_f64"):
            z, it, der = arrays()
            check(lib.fr_escape_rows_de(C.byref(cfg), 0, None, 0, h, z.ctypes.data, it.ctypes.data, der.ctypes.data))
            want = D.f64_rows(cfg)
            assert np.array_equal(it, want[1]) and same(z, want[0]) and D.same_doubles(der, want[2]), "fr_escape_rows_de, F64; " + what
