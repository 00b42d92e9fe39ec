"""ADAPTIVE SUPERSAMPLED DE on the device (fr_render_rows_ss_adaptive_de(_tf)(_device): ss_mark_de_kernel and the three
ss_refine_de_{f64,pt,bla}_kernel templates, byte and LINEAR instances), byte for byte and count for count against
ss_adaptive_de_model.adaptive_de over the HOST MODEL arrays of cfg_s, on the generated inputs of tests/ss_adaptive_de_views.py:
shifted centres, negative and unequal axes, drawn colour fields with `smooth` and `inside` off, limits other than 65536, every
lane mapping s = 2 .. 8, images wider than the 32 x 8 mark tile, a reach that sits on a probe's own distance.
tests/test_ss_adaptive_de_random_cpu.py asserts from the models alone that the sets have teeth.  Nothing is compared against the
code under test, except the dd-centre views, whose arrays are the road's existing fr_escape_rows_de* call of cfg_s, anchored to
de_model.pt_rows / de_bla_model on the view of a seed with the least work.  Every device call gets a guarded destination, the
smallest workspace between guards and a guarded d_refined (test_gpu_ss_adaptive_de.ad_device); every assertion message carries the
input's describe(); a de_mixed input asserts on the model that it cannot pass emptily.
  a. the F64 DE records: (tau_de, reach), (255, reach), (tau_de, 0) and (-1, reach), the whole image and the record's row piece,
     transfers 0 and 1; RGBA and the host form on one record in four; algo 1 is black; s = 1 is the DE render coloured at T;
  b. the wide views on WIDE PT and BLA-PT at (tau_de, reach): the whole image, the row piece and the three-way split, both
     transfers; on the first view of a seed and on the edge views the grid forced to 1 and 2 workgroups, d_refined NULL, the host
     form and the host form forced into row pieces;
  c. the dd-centre views of test_gpu_deep_edges.random_config on PT PLAIN and BLA-PT with pos_lo;
  d. profiling: the kernel that fr_last_kernel_name reports at each s of 4, 5, 7, 8 on the deep roads, and transfer 1 on all
     seven refine kernels in their Mandelbrot and Julia instances, each on an input the models call refined.
The inputs of a seed run in one process one after another."""
import ctypes as C

import numpy as np
import pytest

import de_bla_model as DB
import de_model as D
import deep_random_views as G
import deep_ss_views as V
import pt_model as P
import shallow_random_views as R
import ss_adaptive_de_model as M
import ss_adaptive_de_views as AV
import ss_adaptive_model as A
import test_gpu_ss_adaptive as PLAIN_CALL
from test_gpu_deep_edges import random_config
from test_gpu_deep_ss_random import case, differ
from test_gpu_deep_truth import check, fr, lib, native, torch  # noqa: F401  (fixtures and helpers)
from test_gpu_ss_adaptive_de import ad_device, ad_host

pytestmark = pytest.mark.gpu

F64, PT = 0, 3
PLAIN, BLA, SCALED = 0, 1, 2
REFUSAL = r"distance estimation: limit must be <= 2\^20"


def run(torch, lib, cfg, kw, inp, tau, reach, transfer, what, host=False, **more):
    """one call against the model: bytes and count"""
    want, count = inp.model(tau, reach, more.get("y0", 0), more.get("y1"), more.get("channels", 3), filter=AV.FILTERS[transfer])
    if host:
        got, n = ad_host(lib, cfg, kw, inp.s, inp.thickness, tau, reach, transfer=transfer, **more)
    else:
        got, n = ad_device(torch, lib, cfg, kw, inp.s, inp.thickness, tau, reach, transfer=transfer, **more)
    if more.get("want_refined", True) is False:
        n = count
    assert np.array_equal(got, want) and n == count, "%s, t %d, R %r, transfer %d: %d pixels differ, refined %d, the model %d; %s" % (
        what, tau, reach, transfer, differ(got, want), n, count, inp.describe())
    return count


def not_empty(inp):
    """a de_mixed input cannot pass emptily: by the model, 0 < refined < width * rows and a pixel that only `near` marks"""
    if inp.de_mixed:
        e, n = inp.sets
        count = inp.model(inp.tau, inp.reach)[1]
        assert 0 < count < inp.w * inp.h and (n & ~e).any(), inp.describe()


# ---- a. the F64 DE records ------------------------------------------------------------------------------------------------------------


def check_record(fr, lib, torch, inp):
    rec = inp.rec
    cfg = rec.cfg_at(rec.chain[-1], config=fr.Config)
    kw = {}
    not_empty(inp)
    y0, y1 = rec.split
    for transfer in (0, 1):
        for tau, reach in dict.fromkeys(((inp.tau, inp.reach), (255, inp.reach), (inp.tau, 0.0), (-1, inp.reach))):
            count = run(torch, lib, cfg, kw, inp, tau, reach, transfer, "the whole image")
            run(torch, lib, cfg, kw, inp, tau, reach, transfer, "rows [%d, %d)" % (y0, y1), y0=y0, y1=y1)
            if not inp.orbits:
                assert count == 0 and not inp.model(tau, reach)[0].any()
            elif rec.s == 1:  # the DE render coloured at T, whatever t and R
                plain = D.colour(rec.cfg, *inp.arrays, inp.thickness, 3)
                assert np.array_equal(inp.model(tau, reach, filter=AV.FILTERS[transfer])[0], plain), inp.describe()
    if rec.host:
        for transfer in (0, 1):
            run(torch, lib, cfg, kw, inp, inp.tau, inp.reach, transfer, "RGBA", channels=4)
            run(torch, lib, cfg, kw, inp, inp.tau, inp.reach, transfer, "the host form", host=True)
            run(torch, lib, cfg, kw, inp, inp.tau, inp.reach, transfer, "the host form, RGBA, rows [%d, %d)" % (y0, y1), host=True,
                channels=4, y0=y0, y1=y1)


@pytest.mark.parametrize("seed", R.SEEDS)
def test_generated_f64_de_records(fr, lib, torch, seed):
    for inp in AV.records_of(seed):
        check_record(fr, lib, torch, inp)


@pytest.mark.parametrize("name", list(R.EDGES))
def test_edge_f64_de_records(fr, lib, torch, name):
    assert R.edge(name).de
    check_record(fr, lib, torch, AV.of_record(R.edge(name)))


# ---- b. the wide views ------------------------------------------------------------------------------------------------------------------


def roads_of(c):
    """(the input, the five leading arguments of the C call) of WIDE PT and of BLA-PT, modelled at the view's table bits"""
    return [(AV.of_view(c.v, "de_wide"), dict(c_call=(PT, None, c.centre, PLAIN, 0))),
            (AV.of_view(c.v, "de_bla"), dict(c_call=(PT, None, c.centre, BLA, c.g.call_bits)))]


def check_wide(c, torch, extras):
    """extras: the forced grids, d_refined NULL, the host form and the host form in row pieces as well"""
    v, lib = c.v, c.lib
    for inp, kw in roads_of(c):
        not_empty(inp)
        tau, reach = inp.tau, inp.reach
        for transfer in (0, 1):
            run(torch, lib, c.cfg, kw, inp, tau, reach, transfer, "the whole image")
            y0, y1 = v.piece
            run(torch, lib, c.cfg, kw, inp, tau, reach, transfer, "rows [%d, %d)" % (y0, y1), y0=y0, y1=y1)
            if v.three_way() is not None:  # each piece against its slice: the bytes concatenate to the whole, the counts sum
                for y0, y1 in v.three_way():
                    run(torch, lib, c.cfg, kw, inp, tau, reach, transfer, "rows [%d, %d)" % (y0, y1), y0=y0, y1=y1)
        if not extras:
            continue
        try:
            for groups in (1, 2):
                check(lib.fr_debug_ss_adaptive_grid(groups))
                for transfer in (0, 1):
                    run(torch, lib, c.cfg, kw, inp, tau, reach, transfer, "%d workgroups" % groups)
        finally:
            check(lib.fr_debug_ss_adaptive_grid(0))
        run(torch, lib, c.cfg, kw, inp, tau, reach, 1, "d_refined NULL", want_refined=False)
        for transfer in (0, 1):
            run(torch, lib, c.cfg, kw, inp, tau, reach, transfer, "the host form", host=True)
        if c.h >= 3:  # pieces of n rows with a neighbour row on either side fit the cap, the whole image does not
            n = max(1, c.h // 4)
            cap = M.workspace_bytes(c.w, c.h, 1, 1 + n)
            assert cap % 8 == 0 and M.workspace_bytes(c.w, c.h, 0, c.h) > cap
            try:
                check(lib.fr_debug_ss_host_work_cap(cap))
                run(torch, lib, c.cfg, kw, inp, tau, reach, 1, "the host form in pieces of at most %d rows" % n, host=True, channels=4)
            finally:
                check(lib.fr_debug_ss_host_work_cap(0))


@pytest.mark.parametrize("seed", V.SEEDS)
def test_random_wide_views(fr, native, lib, torch, seed):
    first = True
    for v in V.views(seed):
        if v.g.wide:
            check_wide(case(fr, native, lib, v), torch, extras=first)
            first = False


WIDE_EDGES = [name for name, d in G.EDGES.items() if max(abs(d.scale[0]), abs(d.scale[1])) < 2.0 ** G.E_WIDE]  # inside 2^440


@pytest.mark.parametrize("name", WIDE_EDGES)
def test_edge_wide_views(fr, native, lib, torch, name):
    assert [n for n in G.EDGES if V.edge(n).g.wide] == WIDE_EDGES
    check_wide(case(fr, native, lib, V.edge(name)), torch, extras=True)


# ---- c. the dd-centre views -------------------------------------------------------------------------------------------------------------


class Arrays:
    """a dd-centre view with the arrays of cfg_s that a road's existing DE call gave, as an input of ss_adaptive_de_views"""

    def __init__(self, cfg, s, arrays, what):
        ocfg = V.O.Config.from_buffer_copy(bytes(cfg))
        reach = AV.median_reach(ocfg, *arrays, s)
        self.inp = AV.Input(what, ocfg, s, reach, lambda: arrays, lambda: what)  # the thickness is the reach: the same rule


@pytest.mark.parametrize("seed", G.SEEDS)
def test_random_dd_centre_views(fr, native, lib, torch, seed):
    """PT PLAIN and BLA-PT with pos_lo.  The arrays of cfg_s are the existing fr_escape_rows_de (PT) and fr_escape_rows_de_pt_bla,
    themselves compared with de_model.pt_rows / de_bla_model on the view of the seed, among those inside DE's domain, with the
    least work.  A view with a limit above 2^20 is refused by name."""
    rng = np.random.default_rng(G.DD_BASE_SEED + seed)
    drawn = [random_config(fr, rng) for _ in range(G.DD_PER_SEED)]  # nothing else is drawn from rng
    sizes = [V.dd_supersample(seed, k, cfg) for k, (cfg, _) in enumerate(drawn)]
    inside = [k for k, (cfg, _) in enumerate(drawn) if G.dd_domain(cfg, "de_pt")]
    work = {k: sizes[k] ** 2 * drawn[k][0].width * drawn[k][0].height * max(drawn[k][0].iterations, 1) for k in inside}
    anchor = min(work, key=work.get) if work else None
    for k, (cfg, lo) in enumerate(drawn):
        s = sizes[k]
        what = "config %s, pos_lo %s %s, seed %d, s %d" % (bytes(cfg).hex(), float(lo[0]).hex(), float(lo[1]).hex(), seed, s)
        c_lo = native.Imaginary(*lo)
        plo = C.byref(c_lo)
        bits = (0, 24, 40, 53)[(cfg.width + cfg.height) % 4]
        calls = (("PT", dict(c_call=(PT, plo, None, PLAIN, 0))), ("BLA-PT, bits %d" % bits, dict(c_call=(PT, plo, None, BLA, bits))))
        if k not in inside:
            for name, kw in calls:
                with pytest.raises(native.FractalHipError, match=REFUSAL):
                    ad_device(torch, lib, cfg, kw, s, 1.0, 8, 1.0)
            continue
        cfg_s = cfg.clone()
        cfg_s.width, cfg_s.height = s * cfg.width, s * cfg.height
        shape = (cfg_s.height, cfg_s.width)

        def arrays():
            return np.full(shape + (2,), np.nan), np.full(shape, 0xFFFFFFFF, dtype=np.uint32), np.full(shape + (2,), np.nan)

        pt, bla = arrays(), arrays()
        check(lib.fr_escape_rows_de(C.byref(cfg_s), PT, plo, 0, shape[0], *(a.ctypes.data for a in pt)))
        check(lib.fr_escape_rows_de_pt_bla(C.byref(cfg_s), plo, None, bits, 0, shape[0], *(a.ctypes.data for a in bla)))
        if k == anchor:
            want = D.pt_rows(cfg_s, lo)
            assert np.array_equal(pt[1], want[1]) and D.same_doubles(pt[0], want[0]) and D.same_doubles(pt[2], want[2]), (
                "fr_escape_rows_de of cfg_s against de_model.pt_rows; " + what)
            if cfg.algo in (0, 2):
                x = P.reference_orbit(cfg_s, lo, 0)
                kk = P.reference_orbit(cfg_s, lo, 1) if cfg.algo == 2 else None
                want = DB.escape_rows(cfg_s, x, kk, bits or 40)
                assert np.array_equal(bla[1], want[1]) and D.same_doubles(bla[0], want[0]) and D.same_doubles(bla[2], want[2]), (
                    "fr_escape_rows_de_pt_bla of cfg_s against de_bla_model; " + what)
        for (name, kw), got in zip(calls, (pt, bla)):
            inp = Arrays(cfg, s, got, "%s, %s" % (name, what)).inp
            for tau, reach, transfer in ((inp.tau, inp.reach, 0), (inp.tau, inp.reach, 1), (-1, inp.reach, 0), (255, inp.reach, 0)):
                run(torch, lib, cfg, kw, inp, tau, reach, transfer, name)


# ---- d. the kernels by name --------------------------------------------------------------------------------------------------------------


def last_kernel(lib):
    ms, name = C.c_float(), C.create_string_buffer(160)
    check(lib.fr_last_kernel_ms(C.byref(ms)))
    check(lib.fr_last_kernel_name(name, len(name)))
    return name.value.decode(), ms.value


def refined_wide(mode, julia=None, s=None):
    """the first wide input of a road that the model refines without refining everything, of an instance and an s if given"""
    for inp in AV.wide(mode):
        count = inp.model(inp.tau, inp.reach)[1]
        if inp.orbits and 0 < count < inp.w * inp.h and (julia is None or inp.v.g.julia == julia) and (s is None or inp.s == s):
            return inp
    raise AssertionError("no wide input on %s with julia %r, s %r" % (mode, julia, s))


def test_the_deep_refine_kernels_run_at_every_narrow_lane_mapping(fr, native, lib, torch):
    """ppw = 4, 2, 1, 1: with profiling on, the last kernel of the call is the road's refine kernel at each s of 4, 5, 7 and 8"""
    check(lib.fr_set_profiling(1))
    try:
        for s in (4, 5, 7, 8):
            for mode, k, kernel in (("de_wide", 0, "ss_refine_de_pt_kernel"), ("de_bla", 1, "ss_refine_de_bla_kernel")):
                inp = refined_wide(mode, s=s)
                c = case(fr, native, lib, inp.v)
                run(torch, lib, c.cfg, roads_of(c)[k][1], inp, inp.tau, inp.reach, 0, kernel)
                name, ms = last_kernel(lib)
                assert name == kernel and ms > 0, (s, name, ms, inp.describe())
    finally:
        check(lib.fr_set_profiling(0))


def plain_inputs(fr, native, lib, julia):
    """(kernel, s, run) of the plain adaptive call's four refine kernels on the first input of an instance where the byte and the
    sRGB filter differ at a refined pixel: an F64 record, and a deep view on WIDE PT, BLA-PT and SCALED PT"""
    out = []
    for rec in V.f64_records():
        big = V.f64_image(rec)
        if rec.s < 2 or rec.cfg.algo != (2 if julia else 0):
            continue
        tau = V.median_tau(big, rec.s)
        e = A.edges(big, rec.s, tau)
        if (e & (AV.srgb_filter(big, rec.s) != A.np_filter(big, rec.s)).any(axis=-1)).any():
            cfg = rec.cfg_at(rec.chain[-1], config=fr.Config)
            out.append(("ss_refine_f64_kernel", rec.s, big, tau, cfg, dict(), rec.describe()))
            break
    roads = (("ss_refine_pt_kernel", PLAIN, "wide", lambda g: (0, -1)), ("ss_refine_bla_kernel", BLA, "bla", lambda g: (g.call_bits, g.table_bits)),
             ("ss_refine_scaled_kernel", SCALED, "scaled", lambda g: (-1, -1)))
    for kernel, road, mode, bits_of in roads:
        for v in V.everything():
            if v.g.julia != julia or (road != SCALED and not v.g.wide):
                continue
            bits, model_bits = bits_of(v.g)
            big = v.image(model_bits, mode)
            if (A.edges(big, v.s, v.tau) & (AV.srgb_filter(big, v.s) != A.np_filter(big, v.s)).any(axis=-1)).any():
                c = case(fr, native, lib, v)
                out.append((kernel, c.s, big, v.tau, c.cfg, dict(precision=PT, centre=c.centre, road=road, bits=bits), c.what))
                break
    return out


@pytest.mark.parametrize("julia", [False, True], ids=["mandelbrot", "julia"])
def test_transfer_1_reaches_all_seven_refine_kernels(fr, native, lib, torch, julia):
    """the LINEAR instance of every refine kernel, in this instance of the algorithm: each on a generated input that the host model
    refines somewhere, compared with the model, and named by fr_last_kernel_name.  What ran is asserted from the roads, the s values
    and the algos of the inputs."""
    ran = []
    check(lib.fr_set_profiling(1))
    try:
        for kernel, s, big, tau, cfg, kw, what in plain_inputs(fr, native, lib, julia):
            want, count = A.adaptive(big, s, tau, filter=AV.srgb_filter)
            assert count > 0 and not np.array_equal(want, A.adaptive(big, s, tau)[0]), what
            got, n = PLAIN_CALL.ad_device(torch, lib, cfg, s, tau, transfer=1, **kw)
            assert np.array_equal(got, want) and n == count, "%s, transfer 1: %d pixels differ, refined %d, the model %d; %s" % (
                kernel, differ(got, want), n, count, what)
            assert last_kernel(lib)[0] == kernel, (kernel, last_kernel(lib), what)
            ran.append((kernel, kw.get("precision", F64), kw.get("road", PLAIN), int(cfg.algo), s))
        records = [i for i in AV.records() if i.orbits and i.s >= 2 and (i.cfg.algo == 2) == julia and 0 < i.model(i.tau, i.reach)[1]]
        inp = records[0]
        cfg = inp.rec.cfg_at(inp.rec.chain[-1], config=fr.Config)
        run(torch, lib, cfg, {}, inp, inp.tau, inp.reach, 1, "ss_refine_de_f64_kernel")
        assert last_kernel(lib)[0] == "ss_refine_de_f64_kernel", inp.describe()
        ran.append(("ss_refine_de_f64_kernel", F64, PLAIN, int(cfg.algo), inp.s))
        for mode, k, kernel in (("de_wide", 0, "ss_refine_de_pt_kernel"), ("de_bla", 1, "ss_refine_de_bla_kernel")):
            inp = refined_wide(mode, julia=julia)
            c = case(fr, native, lib, inp.v)
            run(torch, lib, c.cfg, roads_of(c)[k][1], inp, inp.tau, inp.reach, 1, kernel)
            assert last_kernel(lib)[0] == kernel, inp.describe()
            ran.append((kernel, PT, (PLAIN, BLA)[k], int(c.cfg.algo), inp.s))
    finally:
        check(lib.fr_set_profiling(0))
    print("transfer 1 ran on: %r" % (ran,))
    assert len(ran) == 7 and all(algo == (2 if julia else 0) and s >= 2 for _, _, _, algo, s in ran)
    assert sorted((p, r) for _, p, r, _, _ in ran) == sorted([(F64, PLAIN), (PT, PLAIN), (PT, BLA), (PT, SCALED), (F64, PLAIN), (PT, PLAIN),
                                                              (PT, BLA)])
