"""The table slot of a context (Ctx::bla_table; fractal-renderer_amd/csrc/fr_bla.hip: bla_table_for) under a changing view.

The kernels of BLA-PT and SCALED PT read more than their arguments: they read the tables the context's cache hands them.  Here
sequences of views run on one thread through the primary context, each view differing from the one before in one thing
(tests/table_cache_steps.py), and at every step
  - the road's host form — fr_escape_rows_pt_scaled, fr_escape_rows_pt_bla — is the model's (z, iters) bit for bit, on every
    third step the device form into guarded buffers too;
  - the pass count (fr_debug_pt_scaled_count, fr_debug_bla_count) is the model's: tables with wrong radii move the skips even
    where no escape index moves;
  - fr_debug_bla_cache after the step's first call: where the models' orbits or tables differ from the step before
    (must_build, computed in tests/table_cache_steps.py from the models alone and asserted in tests/test_table_cache_cpu.py)
    the table was built and has the model's bits, levels and entries; where they do not, the flag is free.  Three calls must be
    served, as include/fractal_hip.h promises: a row piece, the repeat of a call, the DE call after the plain call.
A sequence records every step that fails and goes on, so one run shows all of them."""
import ctypes as C

import numpy as np
import pytest

import bla_model as B
import de_bla_model as DB
import de_model as D
import de_scaled_model as DS
import pt_scaled_model as S
import table_cache_steps as T
from test_gpu_deep_edges import soft_colours

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def fr():
    import fractal_renderer_amd

    assert fractal_renderer_amd.device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    fractal_renderer_amd.init(0)
    assert fractal_renderer_amd.device_name().startswith("gfx950")
    return fractal_renderer_amd


@pytest.fixture(scope="module")
def native(fr):
    from fractal_renderer_amd import _native

    return _native


@pytest.fixture(scope="module")
def lib(native):
    return native.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def check(rc):
    from fractal_renderer_amd import _native

    _native.check(rc)


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the calls of a step, SCALED PT's or BLA-PT's ---------------------------------------------------------------------------


def host_rows(lib, native, s, y0=0, y1=None):
    """the road's host form over rows [y0, y1)"""
    y1 = s.cfg.height if y1 is None else y1
    z = np.full((y1 - y0, s.cfg.width, 2), np.nan)
    it = np.full((y1 - y0, s.cfg.width), 0xFFFFFFFF, dtype=np.uint32)
    if s.scaled:
        st = s.centre(native)
        check(lib.fr_escape_rows_pt_scaled(C.byref(s.cfg), C.byref(st), s.bits, y0, y1, z.ctypes.data, it.ctypes.data))
    else:
        lo, centre, _keep = s.args(native)
        check(lib.fr_escape_rows_pt_bla(C.byref(s.cfg), lo, centre, s.bits, y0, y1, z.ctypes.data, it.ctypes.data))
    return z, it


def device_rows(lib, native, torch, s):
    """the road's device form over the whole image into guarded buffers"""
    h, w = s.shape
    npx = h * w
    zb = torch.full((GUARD + 16 * npx + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ib = torch.full((GUARD + 4 * npx + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    if s.scaled:
        st = s.centre(native)
        check(lib.fr_escape_rows_pt_scaled_device(C.byref(s.cfg), C.byref(st), s.bits, 0, h, zb.data_ptr() + GUARD, ib.data_ptr() + GUARD,
                                                  None))
    else:
        lo, centre, _keep = s.args(native)
        check(lib.fr_escape_rows_pt_bla_device(C.byref(s.cfg), lo, centre, s.bits, 0, h, zb.data_ptr() + GUARD, ib.data_ptr() + GUARD,
                                               None))
    torch.cuda.synchronize()
    zh, ih = zb.cpu().numpy(), ib.cpu().numpy()
    for a, n in ((zh, 16 * npx), (ih, 4 * npx)):
        assert (a[:GUARD] == 0xA5).all() and (a[GUARD + n:] == 0xA5).all(), "%s: a write outside the array" % s.what
    return (zh[GUARD:GUARD + 16 * npx].copy().view(np.float64).reshape(h, w, 2),
            ih[GUARD:GUARD + 4 * npx].copy().view(np.uint32).reshape(h, w))


def counts(fr, s):
    """(passes, nominal iterations) summed on the device"""
    if s.scaled:
        return fr.pt_scaled_count(s.cfg, bla=None if s.bits < 0 else s.bits, **s.kw(fr))
    return fr.bla_count(s.cfg, bla=s.bits, **s.kw(fr))


def rows_differ(got, want, y0=0, y1=None):
    """'' if (z, iters) are the model's over rows [y0, y1), else what differs"""
    wz, wit = want[0][y0:y1], want[1][y0:y1]
    out = []
    if not np.array_equal(got[1], wit):
        out.append("escape indices differ at %d pixels" % int((got[1] != wit).sum()))
    if not np.array_equal(bits_of(got[0]), bits_of(wz)):
        out.append("z differs at %d of %d pixels" % (int((bits_of(got[0]) != bits_of(wz)).any(axis=-1).sum()), wit.size))
    return ", ".join(out)


def render_differs(lib, native, s):
    """fr_render_rows_pt_scaled against the colour map over the model's rows"""
    h, w = s.shape
    st = s.centre(native)
    want = soft_colours(s.cfg, s.model()[0], s.model()[1])
    if len(np.unique(want.reshape(-1, 3), axis=0)) <= 3:
        return "the colour map over the model's rows is a flat image: the render is not tested"
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    check(lib.fr_render_rows_pt_scaled(C.byref(s.cfg), C.byref(st), s.bits, 0, h, 3, rgb.ctypes.data, rgb.nbytes))
    n = int((rgb != want).any(axis=-1).sum())
    return "the render differs from the colour map over the model's rows at %d pixels" % n if n else ""


def walk(fr, native, lib, torch, steps):
    """run the steps in order; -> the failures, one line per failed check"""
    failures = []
    classes = T.classes(steps)
    for index, (s, cls) in enumerate(zip(steps, classes)):
        bad = []
        want = s.model()
        before = fr.bla_cache()
        got = host_rows(lib, native, s)  # the first call of the step: the slot hits or misses here
        cache = fr.bla_cache()
        orbit_cache = fr.pt_orbit_cache()
        bad.append(rows_differ(got, want))
        if s.table_bits is None:
            if cache != before:
                bad.append("a call without a table changed the slot: %r -> %r" % (before, cache))
        else:
            if cache[:3] != s.cache_triple():
                bad.append("the slot holds (bits, levels, entries) = %r, the model's tables have %r" % (cache[:3], s.cache_triple()))
            if cls == T.MUST_BUILD and cache[3] != 1:
                bad.append("the tables were served where the model's differ from the step before")
        if s.extra == "rekey" and orbit_cache[3] != 0:
            bad.append("an orbit ended by escape was computed again for a higher cap")
        passes, nominal = counts(fr, s)
        if (passes, nominal) != (s.passes(), S.steps(s.cfg, want[1])):
            bad.append("passes and steps %r, the model's %r" % ((passes, nominal), (s.passes(), S.steps(s.cfg, want[1]))))
        if index % 3 == 2:
            d = rows_differ(device_rows(lib, native, torch, s), want)
            bad.append(d and "device form: " + d)
        if s.extra == "render":
            bad.append(render_differs(lib, native, s))
        if s.extra == "served":  # the repeat of the call and a row piece: include/fractal_hip.h promises both the slot's tables
            bad.append(rows_differ(host_rows(lib, native, s), want) and "the repeat differs")
            if fr.bla_cache()[3] != 0:
                bad.append("the repeat of a call built its tables again")
            y0, y1 = 5, min(12, s.cfg.height)
            bad.append(rows_differ(host_rows(lib, native, s, y0, y1), want, y0, y1) and "the row piece differs")
            if fr.bla_cache()[3] != 0:
                bad.append("a row piece built its tables again")
        failures += ["%s (%s): %s" % (s.what, cls, b) for b in bad if b]
    return failures


# ---- Sequence S ------------------------------------------------------------------------------------------------------------------


def test_sequence_s_scaled_pt(fr, native, lib, torch):
    steps = T.sequence_s(fr.Config.new)
    failures = walk(fr, native, lib, torch, steps)
    assert not failures, "\n" + "\n".join(failures)


def test_de_on_scaled_pt_shares_the_slot_with_the_plain_call(fr, native, lib):
    name = T.by_name(T.sequence_s(fr.Config.new))
    other, m900, m901 = name["unrelated: N at 2^900"], name["M at 2^900"], name["scale x 2"]
    assert T.classes([m900, m901])[1] == T.MUST_BUILD

    def de_rows(s):
        st = s.centre(native)
        z, der = np.full(s.shape + (2,), np.nan), np.full(s.shape + (2,), np.nan)
        it = np.full(s.shape, 0xFFFFFFFF, dtype=np.uint32)
        check(lib.fr_escape_rows_de_pt_scaled(C.byref(s.cfg), C.byref(st), 40, 0, s.shape[0], z.ctypes.data, it.ctypes.data, der.ctypes.data))
        return z, it, der

    def assert_de(s, what):
        z, it, der = de_rows(s)
        wz, wit, wder = DS.model(s, 40)[:3]
        assert not rows_differ((z, it), s.model()), what
        assert not rows_differ((z, it), (wz, wit)), what
        assert D.same_doubles(der, wder), what + ": der differs"

    host_rows(lib, native, other)
    assert not rows_differ(host_rows(lib, native, m900), m900.model())  # 1. the plain call builds
    assert fr.bla_cache() == m900.cache_triple() + (1,)
    assert_de(m900, "2. the DE call on the same view and bits")
    assert fr.bla_cache() == m900.cache_triple() + (0,)  # served
    assert_de(m901, "3. the DE call at 2^901")
    assert fr.bla_cache() == m901.cache_triple() + (1,)  # S differs: built
    assert not rows_differ(host_rows(lib, native, m901), m901.model()), "4. the plain call at 2^901"
    assert counts(fr, m901)[0] == m901.passes()


# ---- Sequence B ------------------------------------------------------------------------------------------------------------------


def test_sequence_b_bla_pt_on_a_dd_centre(fr, native, lib, torch):
    steps = T.sequence_b(fr.Config.new)
    failures = walk(fr, native, lib, torch, steps)
    assert not failures, "\n" + "\n".join(failures)


def test_bla_pt_on_a_wide_centre_de_and_the_supersampled_form(fr, native, lib, torch):
    new = fr.Config.new
    m300, m301 = wide = T.wide_bla_steps(new)
    other = T.sequence_b(new)[0]
    failures = walk(fr, native, lib, torch, [other] + wide)
    assert not failures, "\n" + "\n".join(failures)
    # DE ON BLA-PT after the plain call on one view: served, and the model's derivative
    assert not rows_differ(host_rows(lib, native, m301), m301.model())
    z, it, der = fr.escape_rows_de(m301.cfg, precision=fr.Precision.PT, bla=40, **m301.kw(fr))
    assert fr.bla_cache() == m301.cache_triple() + (0,)
    wz, wit, wder = DB.model(m301, 40)[:3]
    assert not rows_differ((z, it), (wz, wit)) and not rows_differ((z, it), m301.model())
    assert D.same_doubles(der, wder), "der differs"
    # the supersampled form renders the rows of cfg_s, twice the size: D is equal, the orbit is the same, the bits are
    cfg = T.changed(m301.cfg, exposure=20.0)  # the default exposure leaves this view nearly black
    big = T.BlaStep("M_16 at 2^301, supersampled", T.changed(cfg, width=2 * cfg.width, height=2 * cfg.height), n=m301.n, ints=m301.ints)
    assert T.classes([m301, big])[1] == T.MAY_SERVE and B.same_bits(big.D(), m301.D())
    want = fr.box_filter(soft_colours(big.cfg, big.model()[0], big.model()[1]), 2)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 5
    assert np.array_equal(fr.get_image_ss_pt(cfg, 2, bla=40, **m301.kw(fr)), want)
    assert fr.bla_cache()[:3] == big.cache_triple()
    assert not rows_differ(host_rows(lib, native, m301), m301.model())  # and back
