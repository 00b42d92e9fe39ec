"""SCALED PT against the roads it extends, on the device: kernel times from profiling events (fr_set_profiling around the kernel
of a device-pointer render), median with min-max of --reps renders each after a warm-up round, the roads of a view
alternating, one process per view.

Views, both 1920 x 1080 on the Misiurewicz point (root of c^3 + 2c^2 + 2c + 2 near -0.228 + 1.115i), limit 2:
  M440  scale 2^440, n = 9 words, cap 5000: the edge of WIDE PT's domain, where all four roads run —
        escape_pt_scaled_kernel against escape_pt_kernel, escape_bla_scaled_kernel against escape_bla_kernel (40 bits);
  M900  scale 2^900, n = 16 words, cap 6000: past the edge only the scaled kernels run, so their times stand alone, beside the
        pass counts of fr_debug_pt_scaled_count.

No gate: what a scaled step costs is a number to write down, not a condition.

    python3 tools/pt_scaled_throughput.py [--reps 7] [--out profiles/pt_scaled_throughput.txt]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

VIEWS = {"M440": (440, 9, 5000), "M900": (900, 16, 6000)}


def child(name, reps):
    import torch  # first: the library binds to the HIP runtime torch carries

    import fractal_renderer_amd as fr
    import pt_wide_orbit as WO
    from fractal_renderer_amd import _native

    fr.init(0)
    lib = _native.load()
    scale_log2, words, cap = VIEWS[name]
    cfg = fr.Config.new()
    cfg.limit = 2.0
    cfg.width, cfg.height, cfg.iterations = 1920, 1080, cap
    cfg.scale.re = cfg.scale.im = 2.0 ** scale_log2
    centre = WO.wide_centre(*WO.newton([1, 2, 2, 2], -0.22815549, 1.11514251), words)
    st = centre.c_struct()
    ce = C.byref(st)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n = cfg.width * cfg.height * 3
    buf = torch.empty(n, dtype=torch.uint8, device=dev)
    tail = (0, cfg.height, 3, buf.data_ptr(), n, stream.cuda_stream)
    roads = {
        "pt_scaled": lambda: lib.fr_render_rows_pt_scaled_device(C.byref(cfg), ce, -1, *tail),
        "bla_scaled": lambda: lib.fr_render_rows_pt_scaled_device(C.byref(cfg), ce, 40, *tail),
    }
    if name == "M440":
        roads["pt"] = lambda: lib.fr_render_rows_pt_wide_device(C.byref(cfg), ce, *tail)
        roads["bla"] = lambda: lib.fr_render_rows_pt_bla_device(C.byref(cfg), None, ce, 40, *tail)
    rec = {"view": name, "width": cfg.width, "height": cfg.height, "iterations": cfg.iterations, "scale_log2": scale_log2,
           "device": fr.device_name(), "build": fr.build_id()}
    passes, steps = fr.pt_scaled_count(cfg, centre, bla=40)
    rec.update(bla_scaled_passes=passes, iterations_total=steps, pass_ratio=round(steps / passes, 3),
               orbit_entries=fr.pt_orbit_cache()[1])
    ms = C.c_float()
    kname = C.create_string_buffer(160)
    times = {k: [] for k in roads}
    names = {}
    _native.check(lib.fr_set_profiling(1))
    try:
        for k in range(reps + 1):  # alternating; the first round is a warm-up
            for which in sorted(roads):
                if which.startswith("bla"):  # the two kinds of table share one slot: build this one outside the timed call,
                    _native.check(roads[which]())  # whose events then bracket the kernel alone
                _native.check(roads[which]())
                _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
                if k:
                    times[which].append(ms.value)
                _native.check(lib.fr_last_kernel_name(kname, len(kname)))
                names[which] = kname.value.decode()
    finally:
        _native.check(lib.fr_set_profiling(0))
    for which, t in times.items():
        rec[which + "_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4),
                              "kernel": names[which]}
    if name == "M440":
        rec["pt_scaled_over_pt"] = round(rec["pt_scaled_ms"]["median"] / rec["pt_ms"]["median"], 3)
        rec["bla_scaled_over_bla"] = round(rec["bla_scaled_ms"]["median"] / rec["bla_ms"]["median"], 3)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    ap.add_argument("--view", choices=sorted(VIEWS), default=None, help="measure this view in this process (what the parent starts)")
    args = ap.parse_args()
    if args.view:
        child(args.view, args.reps)
        return 0
    lines = ["# tools/pt_scaled_throughput.py: SCALED PT against WIDE PT and BLA-PT (40 bits), alternating, %d timed renders each "
             "(median, min - max), one process per view" % args.reps]
    for name in sorted(VIEWS):  # one after another: a fresh process per view, never two at a time
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--view", name, "--reps", str(args.reps)], capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            return 2  # nothing more is started after a failure
        line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
        rec = json.loads(line)
        lines.append(line)
        for which in ("pt", "pt_scaled", "bla", "bla_scaled"):
            if which + "_ms" in rec:
                t = rec[which + "_ms"]
                lines.append("# %-5s %-24s %9.3f ms (%.3f - %.3f)" % (name, t["kernel"], t["median"], t["min"], t["max"]))
        if name == "M440":
            lines.append("# M440  escape_pt_scaled_kernel / escape_pt_kernel = %.3f   escape_bla_scaled_kernel / escape_bla_kernel = %.3f" % (
                rec["pt_scaled_over_pt"], rec["bla_scaled_over_bla"]))
        lines.append("# %-5s %d passes of the scaled BLA loop for %d iterations (%.2fx fewer); orbit of %d entries" % (
            name, rec["bla_scaled_passes"], rec["iterations_total"], rec["pass_ratio"], rec["orbit_entries"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
