"""Statistics of a kept view (include/fractal_hip.h, "statistics of a kept view": fr_view_stats(_device), fr_stats_percentile,
fr_auto_exposure) without a device: every refusal comes before any device work — it is checked on a box that has none —
with its message; n == 0 through the host form needs no device; the two host helpers against tests/view_stats_model.py on
hand-made records; the record's layout."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import view_stats_model as M

INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def refused(lib, rc, message):
    assert rc == INVALID, (rc, lib.fr_last_error())
    assert lib.fr_last_error().decode() == message


# ---- layout -----------------------------------------------------------------------------------------------------


def test_the_record_is_8248_bytes_with_the_headers_offsets(native):
    st = native.fr_view_stats
    assert C.sizeof(st) == 8248 == M.SIZEOF
    offsets = {f: getattr(st, f).offset for f, _ in st._fields_}
    assert offsets == dict(n=0, stable=8, capped=16, escaped=24, sum_iters=32, min_iters=40, max_iters=44, shift=48, reserved=52, hist=56)
    assert native.FR_STATS_BINS == M.BINS == len(st().hist)
    header = open(os.path.join(ROOT, "include", "fractal_hip.h")).read()
    assert re.search(r"#define FR_STATS_BINS (\d+)", header).group(1) == "1024"
    body = re.search(r"struct fr_view_stats \{(.*?)\};", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\w+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f for f, _ in st._fields_]  # the header's fields in the header's order


# ---- fr_view_stats / fr_view_stats_device: the domain -------------------------------------------------------------

Z_WIDTH = "z_width must be 2 (re, im) or 4 (re.hi, re.lo, im.hi, im.lo)"
TOO_MANY = "n > 2^40: one call covers one array of at most 2^40 pixels"
NAN_LIMIT = "stable_limit is NaN: the classes are not defined"
NULL_ARRAY = "NULL array: the statistics need both z and iters"
ALIGN = "z must be 8-byte aligned and iters 4-byte aligned"


def device_call(lib, cfg, z=0x1000, zw=2, it=0x2000, n=16, stats=0x3000):
    """argument checks only: the pointers are never dereferenced before the checks have passed"""
    return lib.fr_view_stats_device(C.byref(cfg) if cfg is not None else None, z, zw, it, n, stats, None)


def host_call(lib, native, cfg, z=0x1000, zw=2, it=0x2000, n=16, stats=True):
    out = native.fr_view_stats()
    return lib.fr_view_stats(C.byref(cfg) if cfg is not None else None, z, zw, it, n, C.byref(out) if stats else None)


def test_every_refusal_of_the_two_reductions_comes_with_its_message(fr, native, lib):
    cfg = fr.Config.new()
    nan = fr.Config.new()
    nan.stable_limit = math.nan
    for call in (lambda *a, **k: device_call(lib, *a, **k), lambda *a, **k: host_call(lib, native, *a, **k)):
        refused(lib, call(None), "cfg is NULL")
        for zw in (0, 1, 3, 5, -2):
            refused(lib, call(cfg, zw=zw), Z_WIDTH)
        refused(lib, call(cfg, n=(1 << 40) + 1), TOO_MANY)
        refused(lib, call(nan), NAN_LIMIT)
        refused(lib, call(nan, n=0, z=None, it=None), NAN_LIMIT)  # the config is checked for an empty array too
        refused(lib, call(cfg, z=None), NULL_ARRAY)
        refused(lib, call(cfg, it=None), NULL_ARRAY)
        refused(lib, call(cfg, z=0x1004), ALIGN)
        refused(lib, call(cfg, it=0x2002), ALIGN)
    refused(lib, device_call(lib, cfg, stats=None), "d_stats is NULL")
    refused(lib, device_call(lib, cfg, n=0, z=None, it=None, stats=None), "d_stats is NULL")
    refused(lib, device_call(lib, cfg, stats=0x3004), "d_stats must be 8-byte aligned")
    refused(lib, host_call(lib, native, cfg, stats=False), "out is NULL")
    refused(lib, host_call(lib, native, cfg, n=0, z=None, it=None, stats=False), "out is NULL")


def test_an_empty_array_through_the_host_form_needs_no_device(fr, native, lib):
    cfg = fr.Config.new()
    for inf in (math.inf, -math.inf, 2.0):
        cfg.stable_limit = inf  # an infinite limit is in the domain: only NaN is refused
        out = native.fr_view_stats()
        C.memset(C.byref(out), 0xFF, C.sizeof(out))
        assert lib.fr_view_stats(C.byref(cfg), None, 2, None, 0, C.byref(out)) == 0
        assert bytes(out) == bytes(8248)
    st = fr.view_stats(cfg, np.empty((0, 4, 2)), np.empty((0, 4), dtype=np.uint32))
    assert isinstance(st, fr.ViewStats) and bytes(st) == bytes(8248)
    assert fr.stats_percentile(st, 0.99) == 0 and fr.auto_exposure(cfg, st) == cfg.exposure
    with pytest.raises(ValueError):
        fr.view_stats(cfg, np.zeros((4, 3)), np.zeros(4, dtype=np.uint32))
    with pytest.raises(ValueError):
        fr.view_stats(cfg, np.zeros((4, 2)), np.zeros(5, dtype=np.uint32))


# ---- fr_stats_percentile / fr_auto_exposure against the model ------------------------------------------------------


def record(min_iters, max_iters, bins, **other):
    """a self-consistent record with class E spread as `bins` = {bin: count}"""
    rec = dict(n=0, stable=0, capped=0, escaped=sum(bins.values()), sum_iters=0, min_iters=min_iters, max_iters=max_iters,
               shift=M.shift_of(min_iters, max_iters), reserved=0, hist=[0] * M.BINS)
    for b, c in bins.items():
        rec["hist"][b] = c
    rec["n"] = rec["escaped"]
    rec.update(other)
    return rec


RNG = np.random.default_rng(20260)
RECORDS = {
    "empty": record(0, 0, {}, n=5, stable=3, capped=2),
    "one_pixel": record(7, 7, {0: 1}),
    "one_pixel_at_zero": record(0, 0, {0: 1}),  # q = max(0, 1): the exposure divides by 1
    "shift0_full": record(10, 10 + 1023, {b: int(c) for b, c in enumerate(RNG.integers(0, 50, size=1024))} | {0: 3, 1023: 2}),
    "shift0_200_singles": record(100, 299, {b: 1 for b in range(200)}),
    "shift1": record(3, 3 + 1024, {0: 5, 17: 9, 512: 1}),
    "shift22_from_zero": record(0, 2 ** 32 - 2, {0: 4, 511: 2, 1023: 3}),
    "shift22_edge_past_2p32": record(5, 2 ** 32 - 2, {0: 1, 1023: 1}),  # 5 + (1024 << 22) - 1 > 2^32: clamped to max_iters
    "huge_counts": record(50, 60, {0: 2 ** 40, 10: 2 ** 39 + 1}),
}
PS = [0.0, 1.0, 0.5, math.nextafter(0.5, 1.0), math.nextafter(0.5, 0.0), 0.99, 0.07, 0.29, 0.57, 1e-300, 5e-324,
      math.nextafter(1.0, 0.0), 0.995, 1.0 / 3.0]


def test_the_ps_land_on_and_just_beside_an_integer():
    """the cases the issue asks for exist in PS x RECORDS: p * escaped exactly k, and one ulp to either side of it"""
    assert 0.5 * 200.0 == 100.0 and math.ceil(math.nextafter(0.5, 1.0) * 200.0) == 101
    assert math.ceil(math.nextafter(0.5, 0.0) * 200.0) == 100
    assert 0.07 * 100.0 != 7.0 and 0.29 * 100.0 != 29.0  # f64 products that miss the integer the decimals suggest
    assert M.percentile(RECORDS["shift0_200_singles"], 0.5) == 199 and M.percentile(RECORDS["shift0_200_singles"], math.nextafter(0.5, 1.0)) == 200
    assert M.percentile(RECORDS["shift22_edge_past_2p32"], 1.0) == 2 ** 32 - 2
    assert M.percentile(RECORDS["shift22_from_zero"], 0.0) == (1 << 22) - 1


@pytest.mark.parametrize("name", list(RECORDS))
def test_percentile_and_exposure_are_the_models(fr, native, lib, name):
    rec = RECORDS[name]
    st = M.to_struct(rec, fr.ViewStats)
    assert M.from_struct(st) == rec
    cfg = fr.Config.new()
    for iterations, exposure in ((50, 2.0), (3000, 5.0), (0, 2.0), (2 ** 32 - 1, 0.25)):
        cfg.iterations, cfg.exposure = iterations, exposure
        for p in PS:
            got, want = C.c_uint32(12345), M.percentile(rec, p)
            assert lib.fr_stats_percentile(C.byref(st), p, C.byref(got)) == 0, lib.fr_last_error()
            assert got.value == want == fr.stats_percentile(st, p), (name, p)
            e = C.c_double(-1.0)
            assert lib.fr_auto_exposure(C.byref(cfg), C.byref(st), p, C.byref(e)) == 0, lib.fr_last_error()
            want_e = M.auto_exposure(iterations, exposure, rec, p)
            assert e.value.hex() == want_e.hex() == fr.auto_exposure(cfg, st, p).hex(), (name, p, iterations)
    cfg.iterations, cfg.exposure = 3000, 2.0
    assert fr.auto_exposure(cfg, st) == M.auto_exposure(3000, 2.0, rec, 0.99)  # the presentation default


P_DOMAIN = "p must be finite and within [0, 1]"


def test_the_helpers_refuse_a_bad_p_a_null_and_an_inconsistent_record(fr, native, lib):
    cfg = fr.Config.new()
    good = M.to_struct(RECORDS["shift1"], native.fr_view_stats)
    q, e = C.c_uint32(0), C.c_double(0.0)
    for p in (math.nan, math.inf, -math.inf, -1e-300, math.nextafter(1.0, 2.0), 2.0):
        refused(lib, lib.fr_stats_percentile(C.byref(good), p, C.byref(q)), P_DOMAIN)
        refused(lib, lib.fr_auto_exposure(C.byref(cfg), C.byref(good), p, C.byref(e)), P_DOMAIN)
    refused(lib, lib.fr_stats_percentile(None, 0.5, C.byref(q)), "the statistics record is NULL")
    refused(lib, lib.fr_stats_percentile(C.byref(good), 0.5, None), "iters_out is NULL")
    refused(lib, lib.fr_auto_exposure(None, C.byref(good), 0.5, C.byref(e)), "cfg is NULL")
    refused(lib, lib.fr_auto_exposure(C.byref(cfg), None, 0.5, C.byref(e)), "the statistics record is NULL")
    refused(lib, lib.fr_auto_exposure(C.byref(cfg), C.byref(good), 0.5, None), "exposure_out is NULL")
    bad = {
        "inconsistent statistics record: shift >= 32": dict(shift=32),
        "inconsistent statistics record: min_iters > max_iters": dict(min_iters=2000),
        "inconsistent statistics record: the histogram holds fewer pixels than `escaped`": dict(escaped=16),
    }
    for message, change in bad.items():
        st = M.to_struct(dict(RECORDS["shift1"], **change), native.fr_view_stats)
        refused(lib, lib.fr_stats_percentile(C.byref(st), 1.0, C.byref(q)), message)
        refused(lib, lib.fr_auto_exposure(C.byref(cfg), C.byref(st), 1.0, C.byref(e)), message)
    with pytest.raises(fr.FractalHipError, match="within"):
        fr.stats_percentile(good, 1.5)
    # an empty class E is consistent only as the all-zero range; the refusals above come first
    st = M.to_struct(dict(RECORDS["empty"], shift=40), native.fr_view_stats)
    refused(lib, lib.fr_stats_percentile(C.byref(st), 0.5, C.byref(q)), "inconsistent statistics record: shift >= 32")


# ---- the model against the header's own words ---------------------------------------------------------------------


def test_the_model_on_a_case_worked_by_hand():
    """cfg: iterations 10, stable_limit 2.  Six pixels: dist 2 (S: not above the limit), NaN (S), 4.25 at it 10 (C), at it
    11 (C), at it 9 (E), 1e300-ish at it 3 (E)."""
    z = np.array([[1.0, 1.0], [math.nan, 0.0], [2.0, 0.5], [2.0, 0.5], [0.5, -2.0], [1e150, 1e150]])
    it = np.array([0, 5, 10, 11, 9, 3], dtype=np.uint32)
    rec = M.view_stats(z, it, 10, 2.0)
    assert (rec["n"], rec["stable"], rec["capped"], rec["escaped"]) == (6, 2, 2, 2)
    assert (rec["sum_iters"], rec["min_iters"], rec["max_iters"], rec["shift"]) == (12, 3, 9, 0)
    assert rec["hist"][0] == 1 and rec["hist"][6] == 1 and sum(rec["hist"]) == 2
    assert M.percentile(rec, 0.5) == 3 and M.percentile(rec, 0.51) == 9
    assert M.auto_exposure(10, 2.0, rec, 1.0) == 10.0 / 9.0
    assert [M.shift_of(0, r) for r in (0, 1023, 1024, 2047, 2048, 2 ** 24 - 1, 2 ** 32 - 2)] == [0, 0, 1, 1, 2, 14, 22]
    wide = np.array([[1.0, 9.0, 1.0, 9.0]])  # z_width 4: the low parts (9) would make it E if they were read
    assert M.view_stats(wide, np.array([1], dtype=np.uint32), 10, 2.0)["stable"] == 1
