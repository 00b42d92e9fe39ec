"""ADAPTIVE SUPERSAMPLING on the F64 road under every kernel selector, byte for byte, no tolerance anywhere.  The F64 probe is
the only caller of the RGB render kernels over a strided pixel map (x_stride = s, block_rows = 1), and it takes its kernel from
fr_set_tile and fr_set_loop_mode; every other adaptive test runs with the defaults.
  a. every F64 record of tests/shallow_random_views.py (generated and edge, algo 1 included) through
     fr_render_rows_ss_adaptive_device at the record's own s, tile and loop_mode, at thresholds -1, 255 and the record's tau
     (deep_ss_views.median_tau of the host model's image of cfg_s), with the refined count, and for the record's row piece; at the
     record's tau and at -1 also with transfer 1, against the model with F replaced by the sRGB filter.  H is
     the HOST MODEL's image: the oracle's F64 rows of cfg_s through its colour map with the software log2; the device's plain
     render of cfg_s under the same selectors is asserted to equal it before it is used.  tests/test_deep_ss_random_cpu.py holds the
     conditions on these records;
  b. the selector sweep on the seahorse and the Julia view of tests/test_gpu_ss_adaptive.py at 65 x 33 — the smallest size that
     crosses a mark tile and a 64-pixel strip in x and four mark tiles in y — and 37 x 29, s in {2, 3, 5}, threshold 8: every
     fr_set_tile of TILES, every fr_set_loop_mode of LOOP_MODES, fr_set_palette(0) with `smooth` off and fr_set_colour_filter in
     {0, 1, 2} give the bytes and the count of the default run, which the model asserts once."""
import numpy as np
import pytest

import deep_ss_views as V
import oracle_lib as O
import shallow_random_views as R
import ss_adaptive_de_views as AV
import ss_adaptive_model as A
from test_gpu_shallow_random import Selectors
from test_gpu_ss_adaptive import ad_device, check, f64_cfg, fr, lib, native, scaled_up, torch  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

TILES = (0, 1, 2, 4, 8, 9, 10, 11, 12, 13, 14, 15, 16, 808, 1604, 3202, 6401)
LOOP_MODES = (-1, 0, 2, 4, 5)
SWEEP_VIEWS = ("seahorse", "julia")
SWEEP_SIZES = ((65, 33), (37, 29))
SWEEP_S = (2, 3, 5)
SWEEP_TAU = 8


# ---- a. the generated F64 records -----------------------------------------------------------------------------------------------------


def adaptive_record(fr, lib, torch, rec):
    what = rec.describe()
    s, final = rec.s, rec.chain[-1]
    orbits = rec.cfg.algo in (0, 2)
    big = V.f64_image(rec)
    tau = V.median_tau(big, s)
    cfg = rec.cfg_at(final, config=fr.Config)
    cfg_s = rec.cfg_at(final, s, config=fr.Config)
    with Selectors(lib, rec):
        plain = fr.get_image(cfg_s)
        assert np.array_equal(plain, big), "the plain render of cfg_s under tile %d, loop mode %d differs from the model at %d samples; %s" % (
            rec.tile, rec.loop_mode, int((plain != big).any(axis=-1).sum()), what)
        for t in dict.fromkeys((-1, 255, tau)):
            want, count = A.adaptive(big, s, t, escape_algo=orbits)
            got, n = ad_device(torch, lib, cfg, s, t)
            assert np.array_equal(got, want) and n == count, "threshold %d: %d pixels differ, refined %d, the model %d; %s" % (
                t, int((got != want).any(axis=-1).sum()), n, count, what)
        for t in dict.fromkeys((tau, -1)):  # the LINEAR instance of ss_refine_f64_kernel: F is the sRGB filter
            want, count = A.adaptive(big, s, t, escape_algo=orbits, filter=AV.srgb_filter)
            got, n = ad_device(torch, lib, cfg, s, t, transfer=1)
            assert np.array_equal(got, want) and n == count, "threshold %d, transfer 1: %d pixels differ, refined %d, the model %d; %s" % (
                t, int((got != want).any(axis=-1).sum()), n, count, what)
        y0, y1 = rec.split
        want, count = A.adaptive(big, s, tau, y0, y1, escape_algo=orbits)
        got, n = ad_device(torch, lib, cfg, s, tau, y0, y1)
        assert np.array_equal(got, want) and n == count, "threshold %d, rows [%d, %d): %d pixels differ, refined %d, the model %d; %s" % (
            tau, y0, y1, int((got != want).any(axis=-1).sum()), n, count, what)


@pytest.mark.parametrize("seed", R.SEEDS)
def test_generated_f64_records(fr, lib, torch, seed):
    for rec in R.records(seed):
        if rec.precision == R.F64:
            adaptive_record(fr, lib, torch, rec)


@pytest.mark.parametrize("name", list(R.EDGES))
def test_edge_f64_records(fr, lib, torch, name):
    adaptive_record(fr, lib, torch, R.edge(name))


# ---- b. the selector sweep ---------------------------------------------------------------------------------------------------------------

_defaults = {}


def default_run(fr, lib, torch, view, size, s, smooth=True):
    """(cfg, bytes, count) of the default run, asserted once against the model on the oracle's image of cfg_s"""
    key = (view, size, s, smooth)
    if key not in _defaults:
        cfg = f64_cfg(fr, view, *size)
        cfg.smooth = int(smooth)
        ocfg = O.Config.from_buffer_copy(bytes(scaled_up(cfg, s)))
        z, it = O.escape_rows(ocfg, O.F64, threads=16)
        big = V.soft_colours(ocfg, z, it)
        want, count = A.adaptive(big, s, SWEEP_TAU)
        share = count / float(size[0] * size[1])
        print("%s %dx%d s=%d smooth=%d: edge share %.3f" % (view, size[0], size[1], s, smooth, share))
        assert 0.05 <= share <= 0.95, (view, size, s, share)
        got, n = ad_device(torch, lib, cfg, s, SWEEP_TAU)
        assert np.array_equal(got, want) and n == count, (view, size, s, smooth, int((got != want).any(axis=-1).sum()), n, count)
        got.setflags(write=False)
        _defaults[key] = (cfg, got, n)
    return _defaults[key]


def sweep(fr, lib, torch, view, setter, values, restore, smooth=True):
    try:
        for size in SWEEP_SIZES:
            for s in SWEEP_S:
                cfg, want, count = default_run(fr, lib, torch, view, size, s, smooth)
                for value in values:
                    check(setter(value))
                    got, n = ad_device(torch, lib, cfg, s, SWEEP_TAU)
                    assert np.array_equal(got, want) and n == count, "%s(%d), %s %dx%d, s %d: %d pixels differ, refined %d, the default run %d" % (
                        setter.__name__, value, view, size[0], size[1], s, int((got != want).any(axis=-1).sum()), n, count)
                check(setter(restore))
    finally:
        setter(restore)


@pytest.mark.parametrize("view", SWEEP_VIEWS)
def test_every_tile_gives_the_default_runs_bytes(fr, lib, torch, view):
    sweep(fr, lib, torch, view, lib.fr_set_tile, TILES, 0)


@pytest.mark.parametrize("view", SWEEP_VIEWS)
def test_every_loop_mode_gives_the_default_runs_bytes(fr, lib, torch, view):
    sweep(fr, lib, torch, view, lib.fr_set_loop_mode, LOOP_MODES, -1)


@pytest.mark.parametrize("view", SWEEP_VIEWS)
def test_palette_off_and_every_colour_filter_give_the_default_runs_bytes(fr, lib, torch, view):
    sweep(fr, lib, torch, view, lib.fr_set_palette, (0,), 1, smooth=False)
    sweep(fr, lib, torch, view, lib.fr_set_colour_filter, (0, 1, 2), 1)
