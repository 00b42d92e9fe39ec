"""BLA-PT (40 bits) against PT on the device, same view, alternating: kernel times from profiling events (fr_set_profiling around
the kernel of a device-pointer render), median and min-max spread of --reps renders each after a warm-up, one process per
view; beside them the pass counts of fr_debug_bla_count, so that the time ratio can be read against the pass ratio, and the
host time of building and uploading a view's table (the first BLA call of a view whose orbit PT has cached already, minus the
second call, which is served).

Views, both 1920 x 1080, limit 2:
  M         the Misiurewicz point (root of c^3 + 2c^2 + 2c + 2 near -0.228 + 1.115i) as a wide centre of n = 8 words, scale
            2^420, cap 5000;
  seahorse  -0.743643887037158704752191506114774 + 0.131825904205311970493132056385139i split into pos + pos_lo, scale 10^20,
            20000 iterations (an orbit of 20 002 entries);
and, for the table's host time alone, the period-3 nucleus at scale 10^20 with iterations = 2^22 - 2 (an orbit of 2^22 entries
cut by the cap) on 16 x 1 pixels.

GATE (M only; the exit code is 1 if it fails): BLA-PT's median is below PT's median by more than the larger of the two min-max
spreads.  The seahorse numbers are reported without a gate.

    python3 tools/bla_throughput.py [--reps 7] [--out profiles/bla_throughput.txt]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

VIEWS = ("M", "seahorse", "table22")
SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")


def make_view(fr, name):
    """-> (cfg, pos_lo or None, WideCentre or None)"""
    import pt_wide_orbit as WO

    cfg = fr.Config.new()
    cfg.limit = 2.0
    if name == "M":
        cfg.width, cfg.height, cfg.iterations = 1920, 1080, 5000
        cfg.scale.re = cfg.scale.im = 2.0 ** 420
        re, im = WO.newton([1, 2, 2, 2], -0.22815549, 1.11514251)
        return cfg, None, WO.wide_centre(re, im, 8)
    if name == "seahorse":
        cfg.width, cfg.height, cfg.iterations = 1920, 1080, 20000
        (cfg.pos.re, lo_re), (cfg.pos.im, lo_im) = fr.split_dd(SEAHORSE[0]), fr.split_dd(SEAHORSE[1])
        cfg.scale.re = cfg.scale.im = 1e20
        return cfg, (lo_re, lo_im), None
    cfg.width, cfg.height, cfg.iterations = 16, 1, (1 << 22) - 2
    re, _ = WO.newton([1, 2, 1, 1], -1.75487767, 0)
    cfg.pos.re, lo_re = fr.split_dd(re)
    cfg.pos.im = 0.0
    cfg.scale.re = cfg.scale.im = 1e20
    return cfg, (lo_re, 0.0), None


def child(name, reps):
    import torch  # first: the library binds to the HIP runtime torch carries

    import fractal_renderer_amd as fr
    from fractal_renderer_amd import _native

    fr.init(0)
    lib = _native.load()
    cfg, pos_lo, centre = make_view(fr, name)
    lo = C.byref(_native.Imaginary(*pos_lo)) if pos_lo is not None else None
    st = centre.c_struct() if centre is not None else None
    ce = C.byref(st) if st is not None else None
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n = cfg.width * cfg.height * 3
    buf = torch.empty(n, dtype=torch.uint8, device=dev)

    def pt():
        if ce is not None:
            return lib.fr_render_rows_pt_wide_device(C.byref(cfg), ce, 0, cfg.height, 3, buf.data_ptr(), n, stream.cuda_stream)
        return lib.fr_render_rows_pt_device(C.byref(cfg), lo, 0, cfg.height, 3, buf.data_ptr(), n, stream.cuda_stream)

    def bla():
        return lib.fr_render_rows_pt_bla_device(C.byref(cfg), lo, ce, 40, 0, cfg.height, 3, buf.data_ptr(), n, stream.cuda_stream)

    def wall(call):
        stream.synchronize()
        t = time.perf_counter()
        _native.check(call())
        stream.synchronize()
        return (time.perf_counter() - t) * 1e3

    rec = {"view": name, "width": cfg.width, "height": cfg.height, "iterations": cfg.iterations, "device": fr.device_name(),
           "build": fr.build_id()}
    rec["pt_first_call_ms"] = round(wall(pt), 3)  # the orbit, on the host, and its upload
    rec["pt_second_call_ms"] = round(wall(pt), 3)
    first = wall(bla)  # the orbit is cached: its download, the table, the upload, the kernel
    second = wall(bla)  # served
    cache = fr.bla_cache()
    rec.update(bla_first_call_ms=round(first, 3), bla_second_call_ms=round(second, 3), table_host_ms=round(first - second, 3),
               orbit_entries=fr.pt_orbit_cache()[1], table_levels=cache[1], table_entries=cache[2])
    if name != "table22":
        passes, steps = fr.bla_count(cfg, pos_lo=pos_lo, centre=centre, bla=40)
        rec.update(bla_passes=passes, pt_iterations=steps, pass_ratio=round(steps / passes, 3))
        ms = C.c_float()
        times = {"bla": [], "pt": []}
        kname = C.create_string_buffer(160)
        _native.check(lib.fr_set_profiling(1))
        try:
            for k in range(reps + 1):  # alternating; the first pair is a warm-up
                for which, call in (("bla", bla), ("pt", pt)):
                    _native.check(call())
                    _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
                    if k:
                        times[which].append(ms.value)
                    if which == "bla":
                        _native.check(lib.fr_last_kernel_name(kname, len(kname)))
        finally:
            _native.check(lib.fr_set_profiling(0))
        for which in ("bla", "pt"):
            t = times[which]
            rec[which + "_ms_median"] = round(statistics.median(t), 4)
            rec[which + "_ms_spread"] = round(max(t) - min(t), 4)
            rec[which + "_ms_all"] = [round(x, 4) for x in t]
        rec["kernel"] = kname.value.decode()
        rec["time_ratio_pt_over_bla"] = round(rec["pt_ms_median"] / rec["bla_ms_median"], 3)
        # what a pass costs against a PT iteration: (BLA time / passes) / (PT time / iterations)
        rec["pass_cost_in_pt_iterations"] = round(rec["pass_ratio"] / rec["time_ratio_pt_over_bla"], 3)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    ap.add_argument("--view", choices=VIEWS, default=None, help="measure this view in this process (what the parent starts)")
    args = ap.parse_args()
    if args.view:
        child(args.view, args.reps)
        return 0
    lines = ["# tools/bla_throughput.py: BLA-PT (40 bits) against PT, alternating, %d timed renders each (median, min-max spread), "
             "one process per view" % args.reps]
    recs = {}
    for name in VIEWS:  # one after another: a fresh process per view, never two at a time
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--view", name, "--reps", str(args.reps)], capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            return 2  # nothing more is started after a failure
        line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
        recs[name] = json.loads(line)
        lines.append(line)
    for name in ("M", "seahorse"):
        r = recs[name]
        lines.append("# %-8s PT %8.3f ms (spread %.3f)  BLA-PT %8.3f ms (spread %.3f)  PT / BLA-PT = %.2f  passes %d for %d iterations "
                     "(%.2fx fewer)  one pass costs %.2f PT iterations" % (
                         name, r["pt_ms_median"], r["pt_ms_spread"], r["bla_ms_median"], r["bla_ms_spread"], r["time_ratio_pt_over_bla"],
                         r["bla_passes"], r["pt_iterations"], r["pass_ratio"], r["pass_cost_in_pt_iterations"]))
    for name in VIEWS:
        r = recs[name]
        lines.append("# %-8s table: %d orbit entries, %d levels, %d table entries; first BLA call %.3f ms, served call %.3f ms: build "
                     "and upload %.3f ms on the host" % (name, r["orbit_entries"], r["table_levels"], r["table_entries"],
                                                         r["bla_first_call_ms"], r["bla_second_call_ms"], r["table_host_ms"]))
    m = recs["M"]
    margin = max(m["bla_ms_spread"], m["pt_ms_spread"])
    ok = m["bla_ms_median"] < m["pt_ms_median"] - margin
    lines.append("# GATE (M): BLA-PT median %.4f ms %s PT median %.4f ms - max spread %.4f ms: %s" % (
        m["bla_ms_median"], "<" if ok else ">=", m["pt_ms_median"], margin, "PASS" if ok else "FAIL"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
