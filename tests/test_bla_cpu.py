"""BLA-PT without a device (include/fractal_hip.h, fr_precision: "BLA-PT"):
  - fr_debug_bla_table against tests/bla_model.py bit for bit at every level — the seahorse dd view, the Misiurewicz centre
    at n = 6 and scale 2^300, the Julia fixed point with both tables — and the shape of a table: n_k halve, r2 never grows
    up the levels for a fixed first step;
  - the accuracy statement: the MODEL against the PT models, at 40 bits and limit = 2 (the conditions of the issue that
    introduced BLA-PT; the counts the model gave are in DESIGN.md, "BLA-PT");
  - the edges where BLA-PT must be PT bit for bit: caps 0, 1, 2, an orbit of 31 entries met again and again, and a skip that
    never overshoots the cap;
  - the argument errors, each with a message and before any device work (on a box without a device anything that touched one
    would answer FR_ERR_NO_DEVICE instead), and the calls that need none."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bla_model as B
import pt_wide_model as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def lib_level(lib, native, v, which, level, bits=0, cap=None):
    lo, centre, _keep = v.args(native)
    n = C.c_uint32(12345)
    assert lib.fr_debug_bla_table(C.byref(v.cfg), lo, centre, bits, which, level, None, 0, C.byref(n)) == 0, message(lib)
    cap = n.value if cap is None else cap
    out = np.full((cap + 1, 5), np.nan)
    assert lib.fr_debug_bla_table(C.byref(v.cfg), lo, centre, bits, which, level, out.ctypes.data, cap, C.byref(n)) == 0
    assert np.isnan(out[min(cap, n.value):]).all(), "a write past min(len, cap) entries"
    return out[:min(cap, n.value)], n.value


# ---- the table ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("spec,which,bits", [
    (B.SEAHORSE, 0, 0), (B.M_16, 0, 0), (B.J_64, 0, 0), (B.J_64, 1, 0), (B.M_16, 0, 24), (B.M_16, 0, 53),
], ids=["seahorse", "M", "J-V", "J-K", "M-24", "M-53"])
def test_the_librarys_table_is_the_models(fr, native, lib, spec, which, bits):
    v = B.view(fr.Config.new, *spec)
    orbit = v.k if which else v.x
    want = B.table(v.cfg, orbit, bits or B.DEFAULT_BITS)
    n0 = len(orbit) - 2
    assert n0 >= 100 and len(want) == n0.bit_length()
    applied = 0
    for k, w in enumerate(want):
        assert len(w) == n0 >> k  # n_k halve as defined
        got, n = lib_level(lib, native, v, which, k, bits)
        assert n == len(w), "level %d" % k
        assert B.same_bits(got[:, 4], w[:, 4]), "r2 of level %d" % k
        live = w[:, 4] > 0
        applied += int(live.sum()) if k else 0
        assert B.same_bits(got[live, :4], w[live, :4]), "A, B of level %d" % k
        assert np.isfinite(w[live, :4]).all()
        if k:  # r never grows from an entry's first child to the entry
            assert (w[:, 4] <= want[k - 1][0:2 * len(w):2, 4]).all()
    assert applied > 0, "a table nobody could apply"
    assert want[-1].shape == (1, 5)
    for past in (len(want), len(want) + 1, 40, 0xFFFFFFFF):
        assert lib_level(lib, native, v, which, past, bits)[1] == 0
    got, n = lib_level(lib, native, v, which, 1, bits, cap=3)  # a short buffer takes min(len, cap) entries
    assert n == n0 >> 1 and B.same_bits(got[:, 4], want[1][:3, 4])


def test_level_zero_is_the_orbit_doubled(fr, native, lib):
    v = B.view(fr.Config.new, *B.M_16)
    got, _ = lib_level(lib, native, v, 0, 0)
    assert B.same_bits(got[:, 0:2], 2.0 * v.x[1:-1]) and (got[:, 2] == 1.0).all() and (got[:, 3] == 0.0).all()
    j = B.view(fr.Config.new, *B.J_64)
    got, _ = lib_level(lib, native, j, 1, 0)
    assert B.same_bits(got[:, 0:2], 2.0 * j.k[1:-1]) and (got[:, 2:4] == 0.0).all()  # b0 = 0 for Julia


def test_python_bla_table(fr):
    v = B.view(fr.Config.new, *B.M_16)
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    want = B.table(v.cfg, v.x)
    assert B.same_bits(fr.bla_table(v.cfg, 2, centre=centre)[:, 4], want[2][:, 4])
    assert fr.bla_table(v.cfg, len(want), centre=centre).shape == (0, 5)
    s = B.view(fr.Config.new, *B.SEAHORSE)
    assert B.same_bits(fr.bla_table(s.cfg, 3, pos_lo=s.pos_lo, bla=40)[:, 4], B.table(s.cfg, s.x)[3][:, 4])
    assert len(fr.bla_cache()) == 4  # answers without a device


# ---- the accuracy statement: the model against PT -----------------------------------------------------------------------


@pytest.mark.parametrize("spec", [B.M_64, B.M_16], ids=["64x48", "16x12"])
def test_misiurewicz_views_keep_every_escape_index_at_a_third_of_the_passes(fr, spec):
    v = B.view(fr.Config.new, *spec)
    z, it, passes = v.model()
    pt_steps = B.steps(v.cfg, v.pt[1])
    print("M %dx%d: PT iterations %d, BLA passes %d, ratio %.2f, indices equal %d / %d" % (
        v.shape[1], v.shape[0], pt_steps, int(passes.sum()), pt_steps / passes.sum(), int((it == v.pt[1]).sum()), it.size))
    assert np.array_equal(it, v.pt[1])
    assert int(passes.sum()) < pt_steps / 3
    assert len(np.unique(it)) > 5 and (it < v.cfg.iterations).all()


def test_the_nucleus_view_is_pt_bit_for_bit(fr):
    v = B.view(fr.Config.new, *B.N_64)
    z, it, passes = v.model()
    print("N: PT iterations %d, BLA passes %d" % (B.steps(v.cfg, v.pt[1]), int(passes.sum())))
    assert (it == 3000).all() and np.array_equal(it, v.pt[1]) and B.same_bits(z, v.pt[0])
    assert int(passes.sum()) < B.steps(v.cfg, v.pt[1])  # and it did skip


@pytest.mark.parametrize("spec", [B.J_64, B.SEAHORSE], ids=["J", "seahorse"])
def test_chaotic_views_differ_on_at_most_two_per_cent(fr, spec):
    v = B.view(fr.Config.new, *spec)
    z, it, passes = v.model()
    differ = int((it != v.pt[1]).sum())
    pt_steps = B.steps(v.cfg, v.pt[1])
    print("%s: PT iterations %d, BLA passes %d, ratio %.2f, indices differ %d / %d" % (
        spec[1], pt_steps, int(passes.sum()), pt_steps / passes.sum(), differ, it.size))
    assert differ <= 0.02 * it.size
    assert int(passes.sum()) < pt_steps


# ---- edges: BLA-PT is PT ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cap", [0, 1, 2])
def test_tiny_caps_are_pt(fr, cap):
    """an empty table (caps 0 and 1: at most one plain step), or at cap 2 a single skip of two whose dz' is absorbed in z"""
    m = B.view(fr.Config.new, "wide", "M", 6, 300, 16, 12, cap)
    j = B.view(fr.Config.new, "wide", "J", 6, 300, 16, 12, cap)
    s = B.view(fr.Config.new, "dd", "seahorse_view", {"iterations": cap})
    for v in (m, j, s):
        z, it, passes = v.model()
        assert np.array_equal(it, v.pt[1]) and B.same_bits(z, v.pt[0]), cap
        if cap < 2:
            assert (passes == cap).all()


def test_an_orbit_of_31_entries_met_again_and_again(fr):
    v = B.view(fr.Config.new, *B.EARLY)
    assert len(v.x) == 31
    z, it, passes = v.model()
    assert np.array_equal(it, v.pt[1]) and B.same_bits(z, v.pt[0])
    assert (it == v.cfg.iterations).sum() > it.size // 2  # the pixels that go round the orbit to the cap


@pytest.mark.parametrize("cap", [2999, 3000, 3001])
def test_a_skip_never_overshoots_the_cap(fr, cap):
    v = B.view(fr.Config.new, "wide", "N", 6, 300, 16, 12, cap)
    z, it, passes = v.model()
    assert (it == cap).all() and np.array_equal(it, v.pt[1]) and B.same_bits(z, v.pt[0])
    assert int(passes.sum()) < cap * it.size


# ---- argument errors and no-ops, without a device ----------------------------------------------------------------------------


def calls(lib, cfg, lo, centre, bits, channels=3):
    h, w = cfg.height, cfg.width
    rgb = np.zeros((h, w, 4), dtype=np.uint8)
    z = np.zeros((h, w, 2))
    it = np.zeros((h, w), dtype=np.uint32)
    a, b, n = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    return {
        "fr_render_rows_pt_bla": lambda: lib.fr_render_rows_pt_bla(C.byref(cfg), lo, centre, bits, 0, h, channels, rgb.ctypes.data, rgb.nbytes),
        "fr_render_rows_pt_bla_device": lambda: lib.fr_render_rows_pt_bla_device(C.byref(cfg), lo, centre, bits, 0, h, channels, 4096,
                                                                                  rgb.nbytes, None),
        "fr_escape_rows_pt_bla": lambda: lib.fr_escape_rows_pt_bla(C.byref(cfg), lo, centre, bits, 0, h, z.ctypes.data, it.ctypes.data),
        "fr_escape_rows_pt_bla_device": lambda: lib.fr_escape_rows_pt_bla_device(C.byref(cfg), lo, centre, bits, 0, h, 4096, 4096, None),
        "fr_debug_bla_table": lambda: lib.fr_debug_bla_table(C.byref(cfg), lo, centre, bits, 0, 1, None, 0, C.byref(n)),
        "fr_debug_bla_count": lambda: lib.fr_debug_bla_count(C.byref(cfg), lo, centre, bits, 0, h, C.byref(a), C.byref(b)),
    }


def refused(lib, cfg, lo, centre, bits, word, channels=3, only=None):
    for name, call in calls(lib, cfg, lo, centre, bits, channels).items():
        if only is None or name in only:
            assert call() == INVALID, name
            assert word in message(lib), (name, message(lib))


def test_argument_errors_need_no_device(fr, native, lib):
    v = B.view(fr.Config.new, *B.M_16)
    _, centre, _keep = v.args(native)
    s = B.view(fr.Config.new, *B.SEAHORSE)
    lo, _, _keep2 = s.args(native)
    for bits in (23, 54, -1, 1):
        refused(lib, v.cfg, None, centre, bits, "bits")
        refused(lib, s.cfg, lo, None, bits, "bits")
    refused(lib, v.cfg, lo, centre, 0, "pos_lo must be NULL")  # both centres
    refused(lib, v.cfg, None, centre, 0, "channels", channels=5, only=("fr_render_rows_pt_bla", "fr_render_rows_pt_bla_device"))
    # a centre too coarse for its scale: n = 2 at 2^300 (WIDE PT's refusal, with its message)
    w2 = W.to_words(W.centre_ints("M", 2)[0], 2), W.to_words(W.centre_ints("M", 2)[1], 2)
    p64 = C.POINTER(C.c_uint64)
    coarse = native.fr_wide_centre(2, w2[0].ctypes.data_as(p64), w2[1].ctypes.data_as(p64))
    for name, call in calls(lib, v.cfg, None, C.byref(coarse), 0).items():
        assert call() == INVALID and "scale" in message(lib), (name, message(lib))
    # PT's domain on the dd road: iterations past FR_PT_MAX_ITERATIONS
    big = fr.Config.from_buffer_copy(bytes(s.cfg))
    big.iterations = (1 << 24) + 1
    refused(lib, big, lo, None, 0, "FR_PT_MAX_ITERATIONS")
    # rows
    assert lib.fr_escape_rows_pt_bla(C.byref(v.cfg), None, centre, 0, 5, 4, None, None) == INVALID and "y0 > y1" in message(lib)
    assert lib.fr_render_rows_pt_bla(C.byref(v.cfg), None, centre, 0, 0, 13, 3, None, 0) == INVALID and "height" in message(lib)
    assert lib.fr_render_rows_pt_bla(None, None, None, 0, 0, 0, 3, None, 0) == INVALID
    n = C.c_uint32(0)
    assert lib.fr_debug_bla_table(C.byref(v.cfg), None, centre, 0, 1, 0, None, 0, C.byref(n)) == INVALID and "which" in message(lib)
    assert lib.fr_debug_bla_table(C.byref(v.cfg), None, centre, 0, 0, 0, None, 0, None) == INVALID
    assert lib.fr_debug_bla_cache(None) == INVALID


def test_calls_without_rows_need_no_device(fr, native, lib):
    v = B.view(fr.Config.new, *B.M_16)
    _, centre, _keep = v.args(native)
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert lib.fr_render_rows_pt_bla(C.byref(v.cfg), None, centre, 0, 3, 3, 3, None, 0) == 0
    assert lib.fr_render_rows_pt_bla_device(C.byref(v.cfg), None, centre, 40, 3, 3, 4, None, 0, None) == 0
    assert lib.fr_escape_rows_pt_bla(C.byref(v.cfg), None, centre, 24, 12, 12, None, None) == 0
    assert lib.fr_escape_rows_pt_bla_device(C.byref(v.cfg), None, centre, 53, 0, 0, None, None, None) == 0
    assert lib.fr_debug_bla_count(C.byref(v.cfg), None, centre, 0, 2, 2, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    out = (C.c_uint32 * 4)(9, 9, 9, 9)
    assert lib.fr_debug_bla_cache(out) == 0 and tuple(out) != (9, 9, 9, 9)


def test_python_refusals(fr):
    v = B.view(fr.Config.new, *B.M_16)
    centre = fr.WideCentre(v.n, re=v.words[0], im=v.words[1])
    with pytest.raises(ValueError):
        fr.get_image(v.cfg, fr.Precision.F64, bla=0)
    with pytest.raises(ValueError):
        fr.get_image(v.cfg, fr.Precision.PT, centre=centre, bla=23)
    with pytest.raises(ValueError):
        fr.get_image_rows(v.cfg, 0, 4, fr.Precision.PT, centre=centre, bla=0, supersample=2)
    with pytest.raises(ValueError):
        fr.escape_rows(v.cfg, precision=fr.Precision.PT, centre=centre, pos_lo=(0.0, 0.0), bla=0)
    assert fr.BLA_DEFAULT_BITS == 40


# ---- the header ------------------------------------------------------------------------------------------------------------


def test_the_header_states_the_definition_and_keeps_the_abi(fr, native, lib):
    text = open(os.path.join(ROOT, "include", "fractal_hip.h")).read()
    assert "#define FR_BLA_DEFAULT_BITS 40" in text and re.search(r"#define FR_ABI_VERSION 3\b", text)
    assert lib.fr_abi_version() == 3
    for phrase in ("BLA-PT", "q = (ry - sqrt(Bx.re*Bx.re + Bx.im*Bx.im) * D) / sqrt(Ax.re*Ax.re + Ax.im*Ax.im)",
                   "i + 2^k <= iterations", "r2 == 0 is never applied", "Escapes inside a skipped block are not looked for"):
        assert phrase in text, phrase
    for name in ("fr_render_rows_pt_bla", "fr_render_rows_pt_bla_device", "fr_escape_rows_pt_bla", "fr_escape_rows_pt_bla_device",
                 "fr_debug_bla_table", "fr_debug_bla_count", "fr_debug_bla_cache"):
        assert re.search(r"\bint %s\(" % name, text) and name in native.PROTOTYPES
