"""The host-buffer render roads (fractal-renderer_amd/csrc/fr_host.hip, copy_out_kernel, the host sink of fr_multi.hip):
band seams, misaligned caller buffers, bytes outside the request, fallbacks.

Every frame lands in  guard | payload | guard  (host_road_driver.Guarded) at an offset of 0, 1, 8 or 4095 bytes from a
page boundary, in written memory or in a never-touched mmap, and is compared byte for byte with the CPU oracle; the guards
must come back intact.  The shapes are those of host_road_cases.py, whose mirror of the geometry says which road, bands,
heads and tails each one hits (checked without a GPU by test_host_road_shapes_cpu.py).  What the library reads from the
environment once per process runs in child processes (host_road_driver.py), one at a time, each with its own timeout.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import host_road_cases as H
import host_road_driver as D
import oracle_lib as O

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_road_driver.py")
OFFSETS = (0, 1, 4095)


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


def variants(name):
    """the (off, mem, prec, slack) of a case: the whole cross product, except for the 108 MB image"""
    if name == "pin_road_108mb":
        return [dict(off=1, mem="fresh", prec="f64"), dict(off=4095, mem="resident", prec="f32")]
    v = [dict(off=off, mem=mem, prec=prec) for prec in ("f64", "f32") for off in OFFSETS for mem in ("resident", "fresh")]
    return v + [dict(off=8, mem="resident", prec="f64", slack=4096), dict(off=8, mem="fresh", prec="f32", slack=4096)]


def failures(reports):
    return [json.dumps(r) for r in reports if not r["ok"]]


# ---- in-process, default environment -------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(H.CASES))
def test_every_case_at_every_offset_fresh_and_resident(fr, name):
    reports = []
    for prec in ("f64", "f32"):
        want = D.expected_bytes(name, prec)
        for v in variants(name):
            if v["prec"] == prec:
                reports.append(D.run_spec(fr, H.make_spec(name, **v), want))
    assert len(reports) == len(variants(name))
    assert not failures(reports), "\n".join(failures(reports))


@pytest.mark.parametrize("name", ["head8_1031", "four_engine_bands", "stage_max_plus_row"])
def test_the_same_buffer_rendered_into_twice(fr, name):
    """a fresh mmap: the first call faults it in, the second finds it resident"""
    want = D.expected_bytes(name, "f64")
    g = H.case_geometry(name, 1)
    buf = D.Guarded(g["need"], 1, fresh=True)
    for k in range(2):
        scratch = D.Guarded(g["need"], 1)  # another view in between: the staging buffer does not hold this frame
        assert D.render(fr, name, "f64", scratch.out, scratch.out_len, poison=True) == 0
        assert scratch.guards_intact() is None, scratch.guards_intact()
        if k:
            buf.refill()
        assert D.render(fr, name, "f64", buf.out, buf.out_len) == 0
        assert not D.check(buf, want, g), (k, D.check(buf, want, g))


@pytest.mark.parametrize("name", ["head8_1031", "stage_max_plus_row"])
def test_a_buffer_pinned_by_the_caller_rendered_into_at_base_plus_one(fr, lib, name):
    """fr_pin_host_buffer over the WHOLE allocation, the payload one byte past a page boundary inside it: the staged
    road never registers anything; the pin road finds every chunk registered already"""
    from fractal_renderer_amd import _native

    want = D.expected_bytes(name, "f64")
    g = H.case_geometry(name, 1)
    assert g["road"] == ("staged" if name == "head8_1031" else "pin")
    buf = D.Guarded(g["need"], 1, fresh=False)
    _native.check(lib.fr_pin_host_buffer(C.c_void_p(buf.base), buf.total))
    try:
        for _ in range(2):
            buf.refill()
            assert D.render(fr, name, "f64", buf.out, buf.out_len) == 0
            assert not D.check(buf, want, g), D.check(buf, want, g)
    finally:
        _native.check(lib.fr_unpin_host_buffer(C.c_void_p(buf.base)))


def _deep_frame(fr, lib, which):
    """(render(out, out_len) -> status, expected bytes, need) of a DD (RGB) or PT (RGBA) host render of about 400 x 300,
    the expected bytes from the host models, built the way test_gpu_dd.py and test_gpu_pt.py build them"""
    import dd_model
    import pt_model

    cfg = fr.Config.new()
    dd_model.deep_view(cfg, False, 401, 299, 400)
    ocfg = O.Config.from_buffer_copy(bytes(cfg))
    O.set_log2_mode(O.LOG2_LIBM)
    if which == "dd":
        z4, it = dd_model.escape_rows(cfg, (0.0, 0.0))
        want = O.colour_rows(ocfg, np.ascontiguousarray(z4[..., 0::2]), it).reshape(-1)
        return (lambda out, n: lib.fr_render_rows_rgb8(C.byref(cfg), 2, 0, cfg.height, C.c_void_p(out), n)), want, want.size
    lo = (0.0, 0.0)
    z, it = pt_model.escape_rows(cfg, lo)
    assert len(np.unique(it)) > 8  # a resolved image, not a flat block
    rgb = O.colour_rows(ocfg, np.ascontiguousarray(z), it)
    want = np.full(rgb.shape[:2] + (4,), 255, dtype=np.uint8)
    want[..., :3] = rgb
    want = want.reshape(-1)
    c_lo = fr.Imaginary(*lo)
    return (lambda out, n: lib.fr_render_rows_pt(C.byref(cfg), C.byref(c_lo), 0, cfg.height, 4, C.c_void_p(out), n)), want, want.size


def test_a_sequence_of_different_frames_in_one_process(fr, lib):
    """flags, sequence numbers, counters and events are reused from frame to frame: four copy-engine bands, two kernel
    bands, one band under 1 MiB, RGBA, the mixed frame, a DD and a PT frame (the deep road), then the first again"""
    names = ["four_engine_bands", "head8_1031", "tiny_one_band", "rgba_1080p", "mixed_engine_kernel"]
    want = {n: D.expected_bytes(n, "f64") for n in names}
    deep = {w: _deep_frame(fr, lib, w) for w in ("dd", "pt")}
    bad = []
    for rnd in range(2):
        for step in names + ["dd", "pt", names[0]]:
            if step in deep:
                call, exp, need = deep[step]
                buf = D.Guarded(need, 1, fresh=bool(rnd))
                g = H.geometry(401, 299, 3 if step == "dd" else 4, 1, deep=True)
                assert g["need"] == need
                rc = call(buf.out, buf.out_len)
            else:
                g = H.case_geometry(step, 1)
                exp = want[step]
                buf = D.Guarded(g["need"], 1, fresh=bool(rnd))
                rc = D.render(fr, step, "f64", buf.out, buf.out_len)
            assert rc == 0, (rnd, step, rc, lib.fr_last_error())
            problems = D.check(buf, exp, g)
            if problems:
                bad.append((rnd, step, problems))
    assert not bad, bad


def test_two_threads_on_multi_band_frames(fr):
    """the render thread and the screenshot thread (src/gui.rs:56-60, 322-326) at multi-band sizes: one RGB frame whose
    second band starts 8 bytes past a 16-byte boundary, one RGBA frame, five frames each, every frame against the oracle"""
    names = ["head8_1031", "rgba_1080p"]
    want = [D.expected_bytes(n, "f64") for n in names]
    errs = []

    def work(i):
        try:
            g = H.case_geometry(names[i], 1)
            for k in range(5):
                buf = D.Guarded(g["need"], 1, fresh=bool(k & 1))
                rc = D.render(fr, names[i], "f64", buf.out, buf.out_len)
                problems = D.check(buf, want[i], g) if rc == 0 else {"status": rc}
                if problems:
                    errs.append((names[i], k, problems))
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    ts = [threading.Thread(target=work, args=(i,)) for i in (0, 1)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs


MULTI_SHAPES = {"over_64_mib": (4801, 4803), "gui_sized": (1031, 1031)}


@pytest.mark.parametrize("shape", sorted(MULTI_SHAPES))
def test_multi_device_host_sink_into_a_misaligned_buffer(fr, lib, shape):
    """fr_render_rgb8_multi pins the caller's buffer in page-aligned chunks too: payload at offsets 1 and 4095"""
    w, h = MULTI_SHAPES[shape]
    case = dict(width=w, height=h, bpp=3, view="mandelbrot", y0=0, y1=h)
    ocfg = H.oracle_config(O, case)
    O.set_log2_mode(O.LOG2_SOFT)
    try:
        want = O.get_image(ocfg, O.F64, threads=D.ORACLE_THREADS).reshape(-1)
    finally:
        O.set_log2_mode(O.LOG2_LIBM)
    cfg = fr.Config.from_buffer_copy(bytes(ocfg))
    need = 3 * w * h
    assert (need > H.K_CHUNK) == (shape == "over_64_mib")
    bad = []
    fr.init_devices([0, 0, 0])
    try:
        for off, fresh, block_rows in ((1, True, 0), (4095, False, 8), (4095, True, 64), (1, False, 0)):
            g = H.geometry(w, h, 3, off, staging=False)
            g["chunks"] = H.chunk_bounds(off, need)  # the host sink always pins in chunks
            buf = D.Guarded(need, off, fresh)
            rc = lib.fr_render_rgb8_multi(C.byref(cfg), 0, block_rows, C.c_void_p(buf.out), buf.out_len)
            assert rc == 0, (off, fresh, rc, lib.fr_last_error())
            problems = D.check(buf, want, g)
            if problems:
                bad.append((off, fresh, block_rows, problems))
    finally:
        fr.init_devices([0])
    assert not bad, bad


def test_errors_leave_the_buffer_alone(fr, lib):
    from fractal_renderer_amd import _native

    for name in ("head8_1031", "rgba_1080p", "stage_max_plus_row"):
        g = H.case_geometry(name, 1)
        buf = D.Guarded(g["need"], 1, fresh=False)
        rc = D.render(fr, name, "f64", buf.out, g["need"] - 1)
        assert rc == _native.FR_ERR_BUFFER_TOO_SMALL, (name, rc)
        assert buf.guards_intact() is None and buf.payload_untouched(), name
    case = H.CASES["head8_1031"]
    cfg = fr.Config.from_buffer_copy(bytes(H.oracle_config(O, case)))
    for y in (0, 7, case["height"]):
        assert lib.fr_render_rows_rgb8(C.byref(cfg), 0, y, y, None, 0) == _native.FR_OK
        assert lib.fr_render_rows_rgba8(C.byref(cfg), 1, y, y, None, 0) == _native.FR_OK


# ---- child processes: what the library reads from the environment once ---------------------------------------------


def run_child(specs, env, timeout=600):
    """one fresh process of the driver; returns (reports by spec, stderr).  Fails the test when the child fails, times
    out or reports a mismatch — the caller starts no further child then.  A child that was killed by a signal or ran
    into its timeout ends the whole session: nothing more is started on a GPU that may have faulted."""
    full = {k: v for k, v in os.environ.items() if not k.startswith("FR_")}
    full.update(env)
    try:
        r = subprocess.run([sys.executable, DRIVER] + specs, env=full, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        pytest.exit("host_road_driver.py %s with %s did not finish in %d s: %s" % (specs, env, timeout, (e.stderr or b"")[-2000:]), 1)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit("host_road_driver.py %s with %s died with status %d:\n%s\n%s" % (specs, env, r.returncode, r.stdout[-1500:],
                                                                                 r.stderr[-3000:]), 1)
    reports = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(reports) == len(specs) and not failures(reports), (
        env, r.returncode, "\n".join(failures(reports)), r.stdout[-1500:], r.stderr[-3000:])
    return dict(zip(specs, reports)), r.stderr


def trace_lines(stderr):
    return [ln for ln in stderr.splitlines() if ln.startswith("[fr_host]")]


def test_without_the_staging_buffer(fr):
    """FR_HOST_STAGING=0 — also what a process gets when the 40 MiB staging allocation fails: one kernel and one plain
    copy under 16 MiB (with y0 = 3), the chunked-pin road with 16 MiB chunks from 16 to 40 MiB"""
    plain, pin = "rows_1031", "four_engine_bands"
    assert plain in H.cases_of_class("plain copy under 16 MiB with y0 = 3")
    assert pin in H.cases_of_class("pin road between 16 and 40 MiB, 16 MiB chunks")
    specs = [H.make_spec(plain, off=0), H.make_spec(plain, off=1, mem="fresh", prec="f32"),
             H.make_spec(pin, off=1, mem="fresh"), H.make_spec(pin, off=1, mem="resident", prec="f32"),
             H.make_spec(pin, off=4095, mem="fresh", prec="f32"), H.make_spec(pin, off=4095, mem="resident")]
    reports, stderr = run_child(specs, {"FR_HOST_STAGING": "0", "FR_TRACE": "1"})
    assert [reports[s]["road"] for s in specs] == ["plain"] * 2 + ["pin"] * 4
    lines = trace_lines(stderr)
    assert not [ln for ln in lines if "staged" in ln], lines
    need = H.case_geometry(pin)["need"]
    assert len([ln for ln in lines if ln.startswith("[fr_host] %d bytes: kernels enqueued" % need)]) == 4, lines
    assert not [ln for ln in lines if " %d bytes" % H.case_geometry(plain)["need"] in ln], lines


@pytest.mark.parametrize("env", [{"FR_COPY_THREADS": "1", "FR_TOUCH_THREADS": "1"}, {"FR_COPY_THREADS": "16"}],
                         ids=["copy1_touch1", "copy16"])
def test_copy_and_touch_thread_counts(fr, env):
    """the piece arithmetic of `spread` with no helper and with fifteen, and the single-thread first touch"""
    specs = []
    for name in ("head8_1031", "four_kernel_bands", "four_engine_bands"):
        specs += [H.make_spec(name, off=1, mem="fresh"), H.make_spec(name, off=4095, mem="resident", prec="f32", slack=4096)]
    run_child(specs, env)


def test_nothing_behind_the_end_of_the_buffer_is_touched(fr):
    """touch_range and prefault write every page of the caller's buffer back to itself: a touch one page too far changes
    no byte, so no guard pattern sees it.  Here the payload ends at a page boundary and the page behind it is
    inaccessible (mem=fenced, in a child: a stray touch ends the process): the single-threaded first touch of a small
    frame, the pooled one of a 4K frame, the pin road's background toucher and its rounded-out registration."""
    specs = [H.make_spec(n, mem="fenced", prec=p) for n, p in (("one_band_prefault", "f64"), ("head8_1031", "f32"),
                                                               ("four_engine_bands", "f64"), ("stage_max_plus_row", "f32"))]
    reports, _ = run_child(specs, {})
    assert [reports[s]["road"] for s in specs] == ["staged"] * 3 + ["pin"]


def test_the_trace_says_which_road_ran(fr):
    """FR_TRACE=1: the road and the band count the library reports are the mirror's — this ties the table to what ran"""
    staged = ["head8_1031", "four_kernel_bands", "mixed_engine_kernel", "tiny_one_band"]
    pin = ["stage_max_plus_row"]
    specs = [H.make_spec(n, off=1, mem="fresh") for n in staged + pin]
    reports, stderr = run_child(specs, {"FR_TRACE": "1"})
    lines = trace_lines(stderr)
    for n in staged:
        g = H.case_geometry(n, 1)
        assert g["road"] == "staged"
        # the poison frame and the frame itself
        hits = [ln for ln in lines if ln.startswith("[fr_host] staged %d bytes in %d bands:" % (g["need"], len(g["bands"])))]
        assert len(hits) == 2, (n, lines)
    for n in pin:
        g = H.case_geometry(n, 1)
        assert g["road"] == "pin"
        assert len([ln for ln in lines if ln.startswith("[fr_host] %d bytes: kernels enqueued" % g["need"])]) == 1, (n, lines)
        kernels = [ln for ln in lines if ln.startswith("[fr_host]   band kernels done at (ms):")]
        assert len(kernels) == 1 and len(kernels[0].split(":")[1].split()) == len(g["bands"]), (n, lines)
