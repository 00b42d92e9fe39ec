"""Speculative blocks that grow while a tile stays quiet (fr_kernels.hip: FR_SC_SPEC_BODY) against the CPU oracle.

The four-iteration scaled loop's unchecked blocks start at 16 iterations and double after every block that passes its end
test, up to fr_kparams::loop_spec_max (default 128); a tile that has thrown a block away stays at 16.  Whatever the longest
block, a lane that escapes inside one must be reported with the exact index and position recursive() returns
(calc/src/lib.rs:245-257).  fr_debug_set_spec_maxlen switches the longest block between renders of one process: every case
runs with 16 (the blocks of before), 32, 128 and 1024, in both precisions, through every kernel that calls
orbit_scaled_run<T, 4> (strips of 7 / 1 / 4 tiles, the refilling kernel, the 4-wave kernel; the escape-index and position
output of the strips), and is compared bit for bit with the oracle AND with the same render without speculation
(loop_mode 5)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import fr, oracle_image, same_f64, to_fr  # noqa: F401  (fixture + helpers)

SEAHORSE = dict(pos=(-0.7436447860, 0.1318252536), scale=(500.0, 500.0))
ELEPHANT = dict(pos=(0.2925, 0.0149), scale=(60.0, 60.0))
MAXLENS = (16, 32, 128, 1024)
TILES = (0, 1, 4, 8, 9, 808)  # the kernels that run orbit_scaled_run<T, 4, false>


def check(fr, ocfg, mode=-1, tiles=(0,), precisions=("f64", "f32"), maxlens=MAXLENS):
    from fractal_renderer_amd import _native

    lib = _native.load()
    cfg = to_fr(fr, ocfg)
    try:
        for pn in precisions:
            op, fp = (O.F64, fr.Precision.F64) if pn == "f64" else (O.F32, fr.Precision.F32)
            wz, wit = O.escape_rows(ocfg, op)
            wimg = oracle_image(ocfg, op)
            # the same render without speculation
            _native.check(lib.fr_debug_set_spec_maxlen(0))
            _native.check(lib.fr_set_loop_mode(5))
            pz, pit = fr.escape_rows(cfg, precision=fp)
            plain = {tile: fr.get_image_rows(cfg, 0, cfg.height, fp, opts=fr.RenderOpts(tile=tile, loop_mode=5)) for tile in tiles}
            _native.check(lib.fr_set_loop_mode(mode))
            for maxlen in maxlens:
                _native.check(lib.fr_debug_set_spec_maxlen(maxlen))
                z, it = fr.escape_rows(cfg, precision=fp)
                assert np.array_equal(it, wit) and np.array_equal(it, pit), (pn, maxlen, "escape indices")
                assert same_f64(z, wz) and same_f64(z, pz), (pn, maxlen, "final positions")
                for tile in tiles:
                    got = fr.get_image_rows(cfg, 0, cfg.height, fp, opts=fr.RenderOpts(tile=tile, loop_mode=mode))
                    assert np.array_equal(got, wimg), (pn, maxlen, tile, "against the oracle")
                    assert np.array_equal(got, plain[tile]), (pn, maxlen, tile, "against loop_mode 5")
    finally:
        lib.fr_set_loop_mode(-1)
        lib.fr_debug_set_spec_maxlen(0)


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["seahorse", "elephant", "default"])
def test_late_escapes_inside_long_blocks(fr, view):
    """Orbits that leave after hundreds of quiet iterations, i.e. inside a block of 64, 128 or more: the rollback from a
    long block, then blocks of 16 for the rest of the tile."""
    kw = dict(seahorse=SEAHORSE, elephant=ELEPHANT, default={})[view]
    check(fr, O.cli_config(328, 200, iterations=3000 if view != "default" else 700, **kw), tiles=TILES)


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [32, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1037])
def test_every_cap_remainder_around_the_block_sums(fr, iterations):
    """An interior tile's blocks end at 16, 32, 64, 128, 256, ... iterations (+ the cap's remainder modulo 4, which runs
    first): caps on, one under and one over every such sum — the next block is halved until it fits, and with fewer than 16
    left the wave finishes in blocks of four.  The default view has whole tiles inside the set."""
    check(fr, O.cli_config(200, 120, iterations=iterations), tiles=(0, 9))
    check(fr, O.cli_config(200, 120, iterations=iterations, **SEAHORSE), tiles=(0,))


@pytest.mark.gpu
def test_overflow_to_nan_inside_a_long_block(fr):
    """limit 2^400: an orbit past it goes through +inf to NaN and stays there for the rest of a long block; the end test is
    `NOT (T >= dist)`, true for NaN.  (f64 only: (f32)limit^2 is +inf and nothing escapes.)"""
    check(fr, O.cli_config(160, 96, iterations=600, limit=2.0 ** 400), tiles=(0, 9), precisions=("f64",))
    check(fr, O.cli_config(160, 96, iterations=300, limit=2.0 ** 400, scale=(1e-3, 1e-3), pos=(0.0, 0.0)), tiles=(0,), precisions=("f64",))


@pytest.mark.gpu
def test_rollbacks_without_an_escape_keep_the_tile_at_sixteen(fr):
    """limit 1000 forced through the 4-iteration loop: T = 0.9 — lanes wander above T all the time, blocks are thrown away
    without any escape, and the tile goes on in blocks of 16 whatever the longest block allowed."""
    check(fr, O.cli_config(200, 120, iterations=400, limit=1000.0), mode=4, tiles=(0, 9, 808))


def test_the_plan_carries_the_longest_block_where_speculation_is_on():
    """Host arithmetic only (no device): the default is 128 wherever spec_quiet is non-zero and 0 wherever it is 0; what
    fr_debug_set_spec_maxlen asks for is brought down to 16 * 2^k."""
    import fractal_renderer_amd as fr
    from fractal_renderer_amd import _native

    lib = _native.load()

    def plan(ocfg, precision=0, mode=-1):
        cfg = fr.Config.from_buffer_copy(bytes(ocfg))
        lm, t, sq, ml = C.c_uint32(), C.c_double(), C.c_uint32(), C.c_uint32()
        try:
            _native.check(lib.fr_set_loop_mode(mode))
            _native.check(lib.fr_debug_loop_plan(C.byref(cfg), precision, C.byref(lm), C.byref(t), C.byref(sq)))
            _native.check(lib.fr_debug_spec_maxlen(C.byref(cfg), precision, C.byref(ml)))
        finally:
            lib.fr_set_loop_mode(-1)
        return lm.value, sq.value, ml.value

    c2 = O.cli_config(16384, 16384, iterations=1024)
    try:
        for prec in (0, 1):
            assert plan(c2, prec) == (4, 16, 128)
            assert plan(c2, prec, mode=5) == (4, 0, 0)  # automatic without speculation
        assert plan(O.cli_config(750, 500, iterations=200, limit=3.99)) == (0, 0, 0)  # limit^2 < 16
        assert plan(O.cli_config(750, 500, iterations=200, limit=2.0 ** 501)) == (0, 0, 0)
        assert plan(O.cli_config(320, 200, iterations=300, pos=(float("nan"), 0.0))) == (0, 0, 0)
        assert plan(O.cli_config(100, 100, O.BARNSLEY_FERN)) == (0, 0, 0)
        assert plan(O.cli_config(320, 200, iterations=300, limit=1000.0), mode=4) == (4, 16, 128)
        for asked, want in ((16, 16), (1, 16), (17, 16), (32, 32), (100, 64), (128, 128), (1024, 1024), (1 << 20, 0x8000), (0, 128)):
            _native.check(lib.fr_debug_set_spec_maxlen(asked))
            assert plan(c2) == (4, 16, want), (asked, want)
            assert plan(c2, mode=5) == (4, 0, 0)
    finally:
        lib.fr_debug_set_spec_maxlen(0)
    assert lib.fr_debug_spec_maxlen(None, 0, None) != 0
