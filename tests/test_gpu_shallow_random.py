"""The calls on top of the FR_PRECISION_F64, FR_PRECISION_F32 and FR_PRECISION_DD roads on the generated and edge records of
tests/shallow_random_views.py, bit for bit against the host models; a NaN equals any NaN, nothing else has a tolerance.
tests/test_shallow_random_cpu.py holds the conditions on the records themselves.  Guard bytes lie on both sides of every device
array and are checked at every read; every failure message carries the record (shallow_random_views.replay rebuilds it).

The kept view (F64, F32, DD; kernels escape_strip_kernel / escape_dd_kernel, escape_extend_kernel<T>, escape_extend_dd_kernel,
colour_rows_kernel, colour_filter_kernel<S>, view_stats_*): fr_escape_rows_device at the chain's first cap; fr_escape_extend_device
link by link, one link first on the row piece alone (the rows outside it stay as they were), against the oracle or
tests/dd_model.py at every cap; one jump from the first cap to the last from a fresh copy; on the final arrays
fr_colour_rows_device (RGB at byte offsets 0 .. 3, RGBA), fr_colour_rows_ss_device over the device's render of cfg_s,
fr_view_stats_device, fr_stats_percentile and fr_auto_exposure; the host forms on one record in four.

F64 DE (escape_de_kernel, escape_extend_de_kernel, distance_rows_kernel, colour_de_rows_kernel, colour_de_filter_kernel<S>):
fr_escape_rows_de_device against tests/de_model.py, its z and iters against fr_escape_rows_device's; fr_escape_extend_de_device
along the chain with the row piece against tests/de_state_model.py; fr_distance_rows_device; fr_colour_de_rows_device at the
record's thickness and at 0; fr_colour_de_rows_ss_device over the DE arrays of cfg_s; fr_render_rows_ss_de_device for the whole
image (smallest workspace) and the row piece; the host forms on one record in four."""
import ctypes as C

import numpy as np
import pytest

import dd_model as DM
import de_model as D
import de_state_model as S
import extend_cases as X
import oracle_lib as O
import shallow_random_views as G
import ss_de_model as SS
import view_stats_model as VS
from test_gpu_de import Buf, check

pytestmark = pytest.mark.gpu

PERCENTILES = (0.0, 0.5, 0.99, 1.0)


@pytest.fixture(scope="module")
def fr():
    import fractal_renderer_amd

    assert fractal_renderer_amd.device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    fractal_renderer_amd.init(0)
    assert fractal_renderer_amd.device_name().startswith("gfx950")
    return fractal_renderer_amd


@pytest.fixture(scope="module")
def lib(fr):
    from fractal_renderer_amd import _native

    return _native.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


# ---- the models ----------------------------------------------------------------------------------------------------------------------


def model_rows(rec, cap, s=1):
    """(z float64 [rows, width, z_width], iters) of the record's road at a cap, of cfg_s for s > 1"""
    cfg = rec.cfg_at(cap, s)
    if rec.precision == G.DD:
        return DM.escape_rows(cfg, rec.pos_lo)
    return O.escape_rows(cfg, rec.precision, threads=DM.THREADS)  # the oracle's default is a thread per processor


def hi_parts(z):
    return z if z.shape[-1] == 2 else np.ascontiguousarray(z[..., 0::2])


def soft_colours(cfg, z, it, channels=3):
    """the oracle's colour map in soft-log2 mode over the positions the colour map reads; an algorithm without orbits is black"""
    rgb = D.base_colours(cfg, hi_parts(z), it)
    if channels == 3:
        return rgb
    out = np.full(rgb.shape[:-1] + (4,), 255, dtype=np.uint8)
    out[..., :3] = rgb
    return out


def same_rows(got, want):
    return bool(np.array_equal(got[1], want[1])) and X.same_f64(got[0], want[0])


# ---- device memory -------------------------------------------------------------------------------------------------------------------


class Kept:
    """(z, iters[, der]) of rows x width pixels in guarded device arrays"""

    def __init__(self, torch, rows, width, zw=2, der=False):
        self.shape, self.n, self.zw, self.width = (rows, width), rows * width, zw, width
        self.z, self.it = Buf(torch, 8 * zw * self.n), Buf(torch, 4 * self.n)
        self.der = Buf(torch, 16 * self.n) if der else None

    def ptrs(self, y0=0):
        """the arrays' pointers at row y0: (z, iters) or (z, iters, der)"""
        k = y0 * self.width
        p = (self.z.ptr + 8 * self.zw * k, self.it.ptr + 4 * k)
        return p + (self.der.ptr + 16 * k,) if self.der else p

    def get(self):
        out = (self.z.get(np.float64, self.shape + (self.zw,)), self.it.get(np.uint32, self.shape))
        return out + (self.der.get(np.float64, self.shape + (2,)),) if self.der else out

    def put(self, arrays):
        for b, a in zip((self.z, self.it, self.der), arrays):
            b.put(a)
        return self


def output(torch, need, off, call):
    """the `need` bytes a call writes `off` bytes behind an 8-byte boundary; the guards around them are checked"""
    b = Buf(torch, need + off)
    call(b.ptr + off)
    return b.get(np.uint8, offset=off)


def lo_arg(rec):
    from fractal_renderer_amd import _native

    return None if rec.pos_lo is None else C.byref(_native.Imaginary(*rec.pos_lo))


def pieces(rec):
    """the row piece of the record and what lies around it"""
    (y0, y1), h = rec.split, rec.cfg.height
    return (y0, y1), [(0, y0), (y1, h)]


class Selectors:
    """the drawn fr_set_tile and fr_set_loop_mode for the time of a chain; the defaults afterwards, whatever happens"""

    def __init__(self, lib, rec):
        self.lib, self.rec = lib, rec

    def __enter__(self):
        if self.rec.precision != G.DD:
            check(self.lib.fr_set_tile(self.rec.tile))
            check(self.lib.fr_set_loop_mode(self.rec.loop_mode))

    def __exit__(self, *exc):
        self.lib.fr_set_tile(0)
        self.lib.fr_set_loop_mode(-1)
        return False


# ---- the kept view ---------------------------------------------------------------------------------------------------------------------


def kept_view(fr, lib, torch, rec):
    what = rec.describe()
    h, w = rec.shape
    n, zw, prec, final = h * w, rec.z_width, rec.precision, rec.chain[-1]
    with Selectors(lib, rec):
        # the render at N0
        cfg = rec.cfg_at(rec.chain[0], config=fr.Config)
        kept = Kept(torch, h, w, zw)
        check(lib.fr_escape_rows_device(C.byref(cfg), prec, lo_arg(rec), 0, h, zw, *kept.ptrs(), None, None))
        first = kept.get()
        assert same_rows(first, model_rows(rec, rec.chain[0])), "fr_escape_rows_device at cap %d; %s" % (rec.chain[0], what)

        def extend(k, frm, y0, y1):
            check(lib.fr_escape_extend_device(C.byref(cfg), prec, lo_arg(rec), y0, y1, frm, zw, *k.ptrs(y0), None, None))

        # the chain, one link first on the row piece alone
        for link, (a, b) in enumerate(rec.links()):
            cfg.iterations = b
            want = model_rows(rec, b)
            if link == rec.piece:
                (y0, y1), rest = pieces(rec)
                before = kept.get()
                extend(kept, a, y0, y1)
                mixed = tuple(np.array(x) for x in before)
                for m, x in zip(mixed, want):
                    m[y0:y1] = x[y0:y1]
                got = kept.get()
                assert np.array_equal(got[1], mixed[1]) and X.same_f64(got[0], mixed[0]), (
                    "link %d -> %d on rows [%d, %d): the piece is not the model's or the rows outside it changed; %s" % (a, b, y0, y1, what))
                for r0, r1 in rest:
                    extend(kept, a, r0, r1)
            else:
                extend(kept, a, 0, h)
            assert same_rows(kept.get(), want), "fr_escape_extend_device %d -> %d; %s" % (a, b, what)
        last = kept.get()
        jump = Kept(torch, h, w, zw).put(first)
        extend(jump, rec.chain[0], 0, h)
        assert same_rows(jump.get(), last), "one jump %d -> %d against the chain; %s" % (rec.chain[0], final, what)
        if rec.host:
            hz, hit = np.array(first[0]), np.array(first[1])
            check(lib.fr_escape_extend(C.byref(cfg), prec, lo_arg(rec), 0, h, rec.chain[0], zw, hz.ctypes.data, hit.ctypes.data))
            assert same_rows((hz, hit), last), "fr_escape_extend %d -> %d; %s" % (rec.chain[0], final, what)

        # colours, the filtered colours of cfg_s, statistics
        z, it = last
        for channels, offsets in ((3, (0, 1, 2, 3)), (4, (0,))):
            want = soft_colours(cfg, z, it, channels)
            for off in offsets:
                got = output(torch, channels * n, off, lambda p: check(lib.fr_colour_rows_device(
                    C.byref(cfg), kept.z.ptr, zw, kept.it.ptr, n, channels, p, channels * n, None)))
                assert np.array_equal(got.reshape(h, w, channels), want), "fr_colour_rows_device, %d channels at byte offset %d; %s" % (
                    channels, off, what)
        s = rec.s
        cfg_s = rec.cfg_at(final, s, config=fr.Config)
        big = Kept(torch, s * h, s * w, zw)
        check(lib.fr_escape_rows_device(C.byref(cfg_s), prec, lo_arg(rec), 0, s * h, zw, *big.ptrs(), None, None))
        zs, its = big.get()
        assert same_rows((zs, its), model_rows(rec, final, s)), "fr_escape_rows_device of cfg_s, s = %d; %s" % (s, what)
        samples = soft_colours(cfg_s, zs, its)
        for channels in (3, 4):
            got = output(torch, channels * n, 0, lambda p: check(lib.fr_colour_rows_ss_device(
                C.byref(cfg), big.z.ptr, zw, big.it.ptr, w, h, s, channels, p, channels * n, None)))
            assert np.array_equal(got.reshape(h, w, channels), SS.box(samples, s, channels)), (
                "fr_colour_rows_ss_device, s = %d, %d channels; %s" % (s, channels, what))
    want = VS.view_stats(z.reshape(-1, zw), it, cfg.iterations, cfg.stable_limit)
    raw = output(torch, VS.SIZEOF, 0, lambda p: check(lib.fr_view_stats_device(C.byref(cfg), kept.z.ptr, zw, kept.it.ptr, n, p, None)))
    stats = fr.ViewStats.from_bytes(raw.tobytes())
    got = VS.from_struct(stats)
    assert not VS.diff(got, want), "fr_view_stats_device: fields %s differ; %s" % (VS.diff(got, want)[:4], what)
    if rec.host:
        host = VS.from_struct(fr.view_stats(cfg, z, it))
        assert not VS.diff(host, want), "fr_view_stats: fields %s differ; %s" % (VS.diff(host, want)[:4], what)
    for p in PERCENTILES:
        assert fr.stats_percentile(stats, p) == VS.percentile(want, p), "fr_stats_percentile(%g); %s" % (p, what)
        got_e, want_e = fr.auto_exposure(cfg, stats, p), VS.auto_exposure(cfg.iterations, cfg.exposure, want, p)
        assert got_e == want_e, "fr_auto_exposure(%g): %r, the model %r; %s" % (p, got_e, want_e, what)


# ---- F64 DE ----------------------------------------------------------------------------------------------------------------------------


def assert_state(got, want, message):
    assert np.array_equal(got[1], want[1]), "%s: escape indices differ at %d pixels" % (message, int((got[1] != want[1]).sum()))
    assert D.same_doubles(got[0], want[0]), message + ": z differs"
    assert D.same_doubles(got[2], want[2]), message + ": der differs"


def f64_de(fr, lib, torch, rec):
    what = rec.describe()
    assert rec.de and rec.precision == G.F64
    h, w = rec.shape
    n, final, s, T = h * w, rec.chain[-1], rec.s, rec.thickness
    with Selectors(lib, rec):
        # the DE render at N0; z and iters are fr_escape_rows_device's
        cfg = rec.cfg_at(rec.chain[0], config=fr.Config)
        kept = Kept(torch, h, w, der=True)
        check(lib.fr_escape_rows_de_device(C.byref(cfg), G.F64, None, 0, h, *kept.ptrs(), None))
        first = kept.get()
        state = D.f64_rows(rec.cfg_at(rec.chain[0]))
        assert_state(first, state, "fr_escape_rows_de_device at cap %d; %s" % (rec.chain[0], what))
        plain = Kept(torch, h, w)
        check(lib.fr_escape_rows_device(C.byref(cfg), G.F64, None, 0, h, 2, *plain.ptrs(), None, None))
        assert same_rows(first[:2], plain.get()), "z and iters of fr_escape_rows_de_device against fr_escape_rows_device; %s" % what

        def extend(k, frm, y0, y1):
            check(lib.fr_escape_extend_de_device(C.byref(cfg), G.F64, y0, y1, frm, *k.ptrs(y0), None))

        # the chain against the model's continuation of its own state
        for link, (a, b) in enumerate(rec.links()):
            cfg.iterations = b
            mcfg = rec.cfg_at(b)
            if link == rec.piece:
                (y0, y1), rest = pieces(rec)
                part = S.f64_continue(mcfg, tuple(x[y0:y1] for x in state), a, y0, y1)
                mixed = tuple(np.array(x) for x in state)
                for m, x in zip(mixed, part):
                    m[y0:y1] = x
                extend(kept, a, y0, y1)
                assert_state(kept.get(), mixed, "fr_escape_extend_de_device %d -> %d on rows [%d, %d), the rows outside them as they were; %s" % (
                    a, b, y0, y1, what))
                for r0, r1 in rest:
                    extend(kept, a, r0, r1)
            else:
                extend(kept, a, 0, h)
            state = S.f64_continue(mcfg, state, a)
            assert_state(kept.get(), state, "fr_escape_extend_de_device %d -> %d; %s" % (a, b, what))
        z, it, der = last = kept.get()
        assert_state(last, D.f64_rows(rec.cfg), "the extended arrays against the DE render at cap %d; %s" % (final, what))
        mcfg = rec.cfg

        # the distance, the shaded colours
        dist = output(torch, 8 * n, 0, lambda p: check(lib.fr_distance_rows_device(C.byref(cfg), *kept.ptrs(), n, p, None))).view(np.float64)
        assert D.same_doubles(dist.reshape(h, w), D.distance(mcfg, z, it, der)), "fr_distance_rows_device; %s" % what
        for thickness in (T, 0.0):
            for channels in (3, 4):
                got = output(torch, channels * n, 0, lambda p: check(lib.fr_colour_de_rows_device(
                    C.byref(cfg), *kept.ptrs(), n, thickness, channels, p, None)))
                assert np.array_equal(got.reshape(h, w, channels), D.colour(mcfg, z, it, der, thickness, channels)), (
                    "fr_colour_de_rows_device, thickness %r, %d channels; %s" % (thickness, channels, what))

        # the fused recolour over the DE arrays of cfg_s
        cfg_s = rec.cfg_at(final, s, config=fr.Config)
        big = Kept(torch, s * h, s * w, der=True)
        check(lib.fr_escape_rows_de_device(C.byref(cfg_s), G.F64, None, 0, s * h, *big.ptrs(), None))
        zs, its, ders = samples = big.get()
        assert_state(samples, D.f64_rows(rec.cfg_at(final, s)), "fr_escape_rows_de_device of cfg_s, s = %d; %s" % (s, what))
        want = {ch: SS.colour(mcfg, zs, its, ders, s, T, ch) for ch in (3, 4)}
        for channels in (3, 4):
            got = output(torch, channels * n, 0, lambda p: check(lib.fr_colour_de_rows_ss_device(
                C.byref(cfg), *big.ptrs(), w, h, s, T, channels, p, channels * n, None)))
            assert np.array_equal(got.reshape(h, w, channels), want[channels]), "fr_colour_de_rows_ss_device, s = %d, %d channels; %s" % (
                s, channels, what)

        # the banded render of the whole image with the smallest workspace, and of the row piece with the largest
        (y0, y1), _ = pieces(rec)
        for (r0, r1), which, channels in (((0, h), 0, 3), ((0, h), 0, 4), ((y0, y1), 1, 3)):
            work_len = fr.ss_de_workspace_bytes(cfg, s, r0, r1)[which]
            work = Buf(torch, work_len)
            need = channels * w * (r1 - r0)
            got = output(torch, need, 0, lambda p: check(lib.fr_render_rows_ss_de_device(
                C.byref(cfg), G.F64, None, None, 0, 0, T, s, r0, r1, channels, p, need, work.ptr, work_len, None)))
            work.get(np.uint8)  # its guards
            assert np.array_equal(got.reshape(r1 - r0, w, channels), want[channels][r0:r1]), (
                "fr_render_rows_ss_de_device, rows [%d, %d), s = %d, %d channels, a workspace of %d bytes; %s" % (r0, r1, s, channels, work_len, what))

        # the host forms give the device forms' bytes
        if rec.host:
            cfg.iterations = rec.chain[0]
            host = tuple(np.empty_like(x) for x in first)
            check(lib.fr_escape_rows_de(C.byref(cfg), G.F64, None, 0, h, *(x.ctypes.data for x in host)))
            assert_state(host, first, "fr_escape_rows_de at cap %d; %s" % (rec.chain[0], what))
            cfg.iterations = final
            check(lib.fr_escape_extend_de(C.byref(cfg), G.F64, 0, h, rec.chain[0], *(x.ctypes.data for x in host)))
            assert_state(host, last, "fr_escape_extend_de %d -> %d; %s" % (rec.chain[0], final, what))
            hd = np.empty((h, w), dtype=np.float64)
            check(lib.fr_distance_rows(C.byref(cfg), *(x.ctypes.data for x in host), n, hd.ctypes.data))
            assert D.same_doubles(hd, dist.reshape(h, w)), "fr_distance_rows; %s" % what
            rgb = np.empty((h, w, 3), dtype=np.uint8)
            check(lib.fr_colour_de_rgb8(C.byref(cfg), *(x.ctypes.data for x in host), n, T, rgb.ctypes.data, rgb.nbytes))
            assert np.array_equal(rgb, D.colour(mcfg, z, it, der, T, 3)), "fr_colour_de_rgb8; %s" % what


# ---- the tests -------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("seed", G.SEEDS)
def test_kept_view_of_generated_records(fr, lib, torch, seed):
    """the F64 and F32 records of a seed and its DD record through the kept-view chain"""
    for rec in G.records(seed) + G.dd_records(seed):
        kept_view(fr, lib, torch, rec)


@pytest.mark.parametrize("seed", G.SEEDS)
def test_f64_de_of_generated_records(fr, lib, torch, seed):
    """the records of a seed inside DE's domain through the F64 DE chain"""
    for rec in G.records(seed):
        if rec.de:
            f64_de(fr, lib, torch, rec)


@pytest.mark.parametrize("name", list(G.EDGES))
def test_kept_view_of_edge_records(fr, lib, torch, name):
    kept_view(fr, lib, torch, G.edge(name))


@pytest.mark.parametrize("name", list(G.EDGES))
def test_f64_de_of_edge_records(fr, lib, torch, name):
    f64_de(fr, lib, torch, G.edge(name))
