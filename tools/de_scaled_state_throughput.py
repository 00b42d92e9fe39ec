"""What RESUMABLE SCALED DE and SUPERSAMPLED SCALED DE cost on the device (include/fractal_hip.h, the sections of those names;
csrc/fr_de_scaled.hip, csrc/fr_ss_de.hip), on the deep views of tools/de_scaled_throughput.py: M440 (2^440, the edge of WIDE PT's
domain) and M900 (2^900), both 1920 x 1080 on the Misiurewicz point, limit 2.  Three things per view:
  1. what keeping the state costs: escape_pt_scaled_de_state_kernel (fr_escape_rows_de_pt_scaled_state_device) beside
     escape_pt_scaled_de_kernel (fr_escape_rows_de_pt_scaled_device, bits = -1) at the same cap, alternating;
  2. an extension N -> M (fr_escape_extend_de_pt_scaled_device, escape_extend_pt_scaled_de_kernel) beside the fresh DE render at M,
     for N = M / 2 and N = 0.9 M, with the share of pixels running at N and the extension's share of the render's pixel-iterations:
     at M = the view's cap, and at M = the cap under which 90 % of the view's escape indices lie, where pixels are still running
     (at the caps of these two views every pixel has escaped long before M / 2).  The state at N is rendered once; before every
     timed extension it is copied back into the working arrays, outside the events;
  3. the supersampled scaled DE render (fr_render_rows_ss_de_pt_scaled_device, T = 1) beside the unshaded supersampled render of the
     same road (fr_render_rows_ss_pt_device with FR_PT_ROAD_SCALED), at s = 2 and 4, bits = -1 and 40, each with its largest
     workspace; the times are the spans from the first band's kernel to the last filter.
Kernel time is fr_set_profiling's events: median with min - max of --reps calls after a warm-up round.  One process per view, one
after another, each under a time limit of its own; nothing more is started after a failure — from a shell the same is
    timeout -k 10 300 python3 tools/de_scaled_state_throughput.py --view M440 && \\
    timeout -k 10 300 python3 tools/de_scaled_state_throughput.py --view M900
No gate: these are numbers to write down.

    python3 tools/de_scaled_state_throughput.py [--reps 5] [--out profiles/de_scaled_state_throughput.txt]"""
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

import pt_scaled_throughput as PS  # noqa: E402  (the views; it imports nothing of the device)

BITS = 40
THICKNESS = 1.0
CHILD_TIMEOUT = 300  # seconds for one view


def summary(times):
    return {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}


def child(name, reps):
    import torch  # first: the library binds to the HIP runtime torch carries

    import fractal_renderer_amd as fr
    import pt_wide_orbit as WO
    from fractal_renderer_amd import _native

    fr.init(0)
    lib = _native.load()
    scale_log2, words, cap = PS.VIEWS[name]
    cfg = fr.Config.new()
    cfg.limit = 2.0
    cfg.width, cfg.height, cfg.iterations = 1920, 1080, cap
    cfg.scale.re = cfg.scale.im = 2.0 ** scale_log2
    centre = WO.wide_centre(*WO.newton([1, 2, 2, 2], -0.22815549, 1.11514251), words)
    st = centre.c_struct()
    ce = C.byref(st)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    n = cfg.width * cfg.height
    ms, kname = C.c_float(), C.create_string_buffer(160)

    def timed(call, before=None):
        """-> (times of `reps` calls after one warm-up call, the kernel's name)"""
        times = []
        for rep in range(reps + 1):
            if before:
                before()
                stream.synchronize()
            _native.check(call())
            _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
            if rep:
                times.append(ms.value)
        _native.check(lib.fr_last_kernel_name(kname, len(kname)))
        return times, kname.value.decode()

    def alternating(calls):
        """-> {name: (times, kernel)}: the calls alternate within every repetition, the first round is a warm-up"""
        times, names = {k: [] for k in calls}, {}
        for rep in range(reps + 1):
            for which, call in calls.items():
                _native.check(call())
                _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
                if rep:
                    times[which].append(ms.value)
                else:
                    _native.check(lib.fr_last_kernel_name(kname, len(kname)))
                    names[which] = kname.value.decode()
        return {k: (times[k], names[k]) for k in calls}

    def arrays():
        return [torch.empty(2 * n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty(2 * n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty(2 * n, dtype=torch.float64, device=dev)]

    def steps_of(it, cap_):  # the nominal pixel-iterations of a result: escape index + 1, or the cap
        return int(torch.clamp(it.to(torch.int64) + 1, max=cap_).sum())

    rec = {"view": name, "width": cfg.width, "height": cfg.height, "iterations": cap, "scale_log2": scale_log2, "device": fr.device_name(),
           "build": fr.build_id(), "reps": reps}
    work = arrays()
    ptrs = [t.data_ptr() for t in work]
    z, it, _w, _m, der = ptrs
    _native.check(lib.fr_set_profiling(1))
    try:
        with torch.cuda.stream(stream):
            # 1. the state render beside the DE render, the same cap
            r = alternating({
                "de": lambda: lib.fr_escape_rows_de_pt_scaled_device(C.byref(cfg), ce, -1, 0, cfg.height, z, it, der, s),
                "state": lambda: lib.fr_escape_rows_de_pt_scaled_state_device(C.byref(cfg), ce, 0, cfg.height, *ptrs, s),
            })
            stream.synchronize()
            steps_m = steps_of(work[1], cap)
            rec["pixel_iterations"] = steps_m
            for k, (t, kn) in r.items():
                rec[k + "_ms"] = dict(summary(t), kernel=kn)
            rec["state_over_de"] = round(rec["state_ms"]["median"] / rec["de_ms"]["median"], 3)
            # 2. extensions N -> M beside the fresh DE render at M: at the view's cap, and at the cap that 90 % of the pixels' escape
            # indices lie under, where pixels are still running
            def extensions(m_cap, fresh_ms, steps_top):
                rows = []
                top = cfg.clone()
                top.iterations = m_cap
                for frac in (0.5, 0.9):
                    n_cap = int(m_cap * frac)
                    low = cfg.clone()
                    low.iterations = n_cap
                    kept = arrays()
                    _native.check(lib.fr_escape_rows_de_pt_scaled_state_device(C.byref(low), ce, 0, cfg.height, *(t.data_ptr() for t in kept), s))
                    stream.synchronize()
                    running = int((kept[1] == n_cap).sum())
                    steps_n = steps_of(kept[1], n_cap)

                    def restore():
                        for a, b in zip(work, kept):
                            a.copy_(b)

                    t, kn = timed(lambda: lib.fr_escape_extend_de_pt_scaled_device(C.byref(top), ce, 0, cfg.height, n_cap, *ptrs, s), restore)
                    stream.synchronize()
                    assert steps_of(work[1], m_cap) == steps_top, "the extended view is not the view at the new cap"
                    e = dict(summary(t), kernel=kn, running_pixels=running, running_share=round(running / n, 6))
                    e["from"], e["to"] = n_cap, m_cap
                    e["steps_share"] = round((steps_top - steps_n) / steps_top, 6)
                    e["fresh_ms"] = fresh_ms
                    e["extension_over_fresh"] = round(e["median"] / fresh_ms, 3)
                    rows.append(e)
                    del kept
                return rows

            rec["extensions"] = extensions(cap, rec["de_ms"]["median"], steps_m)
            p90 = int(torch.quantile(work[1].to(torch.float64)[::7], 0.9)) + 1  # a sample of the pixels: the cap is a round figure
            short = cfg.clone()
            short.iterations = p90
            t, kn = timed(lambda: lib.fr_escape_rows_de_pt_scaled_device(C.byref(short), ce, -1, 0, cfg.height, z, it, der, s))
            stream.synchronize()
            rec["p90_cap"] = p90
            rec["p90_de_ms"] = dict(summary(t), kernel=kn)
            rec["extensions"] += extensions(p90, rec["p90_de_ms"]["median"], steps_of(work[1], p90))
            # 3. the supersampled renders, largest workspace each
            rec["supersampled"] = []
            out = torch.empty(3 * n, dtype=torch.uint8, device=dev)
            for ss in (2, 4):
                de_best = fr.ss_de_workspace_bytes(cfg, ss)[1]
                pt_best = fr.ss_workspace_bytes(cfg, ss)[1]
                wk = torch.empty(max(de_best, pt_best), dtype=torch.uint8, device=dev)
                for bits in (-1, BITS):
                    r = alternating({
                        "ss_pt": lambda: lib.fr_render_rows_ss_pt_device(C.byref(cfg), None, ce, _native.FR_PT_ROAD_SCALED, bits, ss, 0,
                                                                         cfg.height, 3, out.data_ptr(), out.numel(), wk.data_ptr(), pt_best, s),
                        "ss_de": lambda: lib.fr_render_rows_ss_de_pt_scaled_device(C.byref(cfg), ce, bits, THICKNESS, ss, 0, cfg.height, 3,
                                                                                   out.data_ptr(), out.numel(), wk.data_ptr(), de_best, s),
                    })
                    stream.synchronize()
                    e = {"supersample": ss, "bits": bits, "de_workspace_bytes": de_best, "pt_workspace_bytes": pt_best}
                    for k, (t, kn) in r.items():
                        e[k + "_ms"] = dict(summary(t), kernel=kn)
                    e["ss_de_over_ss_pt"] = round(e["ss_de_ms"]["median"] / e["ss_pt_ms"]["median"], 3)
                    rec["supersampled"].append(e)
                del wk
    finally:
        _native.check(lib.fr_set_profiling(0))
    print(json.dumps(rec), flush=True)


def report(rec):
    name = rec["view"]
    d, t = rec["de_ms"], rec["state_ms"]
    lines = ["# %-5s %-34s %9.3f ms (%.3f - %.3f)" % (name, d["kernel"], d["median"], d["min"], d["max"]),
             "# %-5s %-34s %9.3f ms (%.3f - %.3f)   state / DE render = %.3f" % (name, t["kernel"], t["median"], t["min"], t["max"],
                                                                                 rec["state_over_de"])]
    for e in rec["extensions"]:
        lines.append("# %-5s extension %5d -> %5d  %9.3f ms (%.3f - %.3f)   running %.3f %% (%d pixels), steps %.3f %%, fresh DE render at %d "
                     "%.3f ms, extension / fresh = %.3f"
                     % (name, e["from"], e["to"], e["median"], e["min"], e["max"], 100 * e["running_share"], e["running_pixels"],
                        100 * e["steps_share"], e["to"], e["fresh_ms"], e["extension_over_fresh"]))
    for e in rec["supersampled"]:
        a, b = e["ss_pt_ms"], e["ss_de_ms"]
        lines.append("# %-5s s = %d, bits %2d: %s %9.3f ms (%.3f - %.3f), scaled DE %s %9.3f ms (%.3f - %.3f)   DE / unshaded = %.3f"
                     % (name, e["supersample"], e["bits"], a["kernel"], a["median"], a["min"], a["max"], b["kernel"], b["median"], b["min"],
                        b["max"], e["ss_de_over_ss_pt"]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    ap.add_argument("--view", choices=sorted(PS.VIEWS), default=None, help="measure this view in this process (what the parent starts)")
    args = ap.parse_args()
    if args.view:
        child(args.view, args.reps)
        return 0
    lines = ["# tools/de_scaled_state_throughput.py: RESUMABLE SCALED DE and SUPERSAMPLED SCALED DE, kernel times from profiling events, "
             "%d timed calls each after a warm-up (median, min - max), one process per view" % args.reps]
    for name in sorted(PS.VIEWS):  # one after another: a fresh process per view under its own time limit, never two at a time
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--view", name, "--reps", str(args.reps)], capture_output=True,
                               text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.stderr.write("%s: no result within %d s\n" % (name, CHILD_TIMEOUT))
            return 2
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            return 2  # nothing more is started after a failure
        line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
        lines.append(line)
        lines += report(json.loads(line))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
