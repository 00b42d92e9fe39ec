"""What the statistics of a kept view cost beside the recolour they serve.

On a kept F64 view (default Mandelbrot, 1024 iterations, smooth on) at 1920 x 1080 and 3840 x 2160, and on an array of the
same sizes in which every pixel escaped at ONE index (the bad case for a histogram: every add hits one bin), two variants
over the SAME device arrays:
  stats   fr_view_stats_device: a memset and the pair of launches (view_stats_range_kernel, view_stats_hist_kernel)
  colour  fr_colour_rows_device, RGBA: the recolour of the same view — the yardstick, a kernel this tool's subject does not touch
Device events on a stream of the tool's own around --inner back-to-back calls (one call is tens of microseconds: a window of
one would time the event pair), divided by --inner; one warm-up round, then --reps rounds with the variants ALTERNATING;
median with min - max.  The record is checked against the arrays first (class counts by torch).

The GB/s column is bytes the algorithm reads over the time of a call.  It is NOT an HBM rate: a window is --inner calls over
the same 41 MB / 166 MB arrays, which stay in the 256 MiB Infinity Cache between calls and between the alternating variants,
so "bound by HBM" is neither confirmed nor refuted by it.  The gate is relative and both variants get the same treatment.

GATE per row: stats <= 2 x colour (median) + the colour's own spread (max - min): the statistics read the view twice where the
colour map reads it once, and write nothing of size.

    python3 tools/view_stats_throughput.py [--reps 7] [--inner 20] [--out profiles/view_stats_throughput.txt]
Exit status 1 when a gate fails."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("1080p", 1920, 1080), ("2160p", 3840, 2160)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    args = ap.parse_args()
    if args.reps < 5 or args.inner < 1:
        ap.error("--reps must be at least 5 and --inner at least 1")

    import torch  # first: the library binds to the HIP runtime torch carries

    import fractal_renderer_amd as fr
    from fractal_renderer_amd import _native

    fr.init(0)
    lib = _native.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.inner):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.inner

    recs = []
    for label, width, height in SIZES:
        n = width * height
        view = fr.Config.new()
        view.width, view.height, view.iterations = width, height, 1024
        z = torch.empty(2 * n, dtype=torch.float64, device=dev)
        it = torch.empty(n, dtype=torch.int32, device=dev)
        _native.check(lib.fr_escape_rows_device(C.byref(view), 0, None, 0, height, 2, z.data_ptr(), it.data_ptr(), st, None))
        one = fr.Config.new()
        one.width, one.height, one.iterations = width, height, 3000
        z1 = torch.tensor([0.0, -2.5], dtype=torch.float64, device=dev).repeat(n)
        it1 = torch.full((n,), 137, dtype=torch.int32, device=dev)
        stream.synchronize()
        torch.cuda.synchronize()
        rgba = torch.empty(4 * n, dtype=torch.uint8, device=dev)
        d_stats = torch.full((C.sizeof(_native.fr_view_stats),), 0xFF, dtype=torch.uint8, device=dev)
        for case, cfg, dz, di in (("view_" + label, view, z, it), ("one_bin_" + label, one, z1, it1)):
            def stats():
                _native.check(lib.fr_view_stats_device(C.byref(cfg), dz.data_ptr(), 2, di.data_ptr(), n, d_stats.data_ptr(), st))

            def colour():
                _native.check(lib.fr_colour_rows_device(C.byref(cfg), dz.data_ptr(), 2, di.data_ptr(), n, 4, rgba.data_ptr(), rgba.numel(), st))

            stats()
            stream.synchronize()
            rec = fr.ViewStats.from_bytes(d_stats.cpu().numpy().tobytes())
            zz = dz.view(n, 2)
            outside = (zz[:, 0] * zz[:, 0] + zz[:, 1] * zz[:, 1]) > cfg.stable_limit
            escaped = int((outside & (di < cfg.iterations)).sum())
            assert (rec.n, rec.stable, rec.escaped) == (n, n - int(outside.sum()), escaped) and sum(rec.hist) == escaped, "a wrong record"
            times = {"stats": [], "colour": []}
            for r in range(args.reps + 1):  # the first round warms up
                for name, fn in (("stats", stats), ("colour", colour)):
                    ms = timed(fn)
                    if r:
                        times[name].append(ms)
            for name, ts in times.items():
                passes = 2 if name == "stats" else 1
                out = {"case": case, "variant": name, "ms_median": round(statistics.median(ts), 5), "ms_min": round(min(ts), 5),
                       "ms_max": round(max(ts), 5), "runs": len(ts), "inner": args.inner, "bytes_read": passes * 20 * n,
                       "bytes_written": 4 * n if name == "colour" else C.sizeof(_native.fr_view_stats), "escaped": escaped,
                       "shift": rec.shift}
                out["read_GBps"] = round(out["bytes_read"] / 1e9 / (out["ms_median"] * 1e-3), 1)
                recs.append(out)
                print(json.dumps(out), flush=True)
        del z, it, z1, it1, rgba

    lines = ["# tools/view_stats_throughput.py on %s, build %s, %d timed runs per variant of %d back-to-back calls each (ms per call: "
             "median, min, max; variants alternate)" % (fr.device_name(), fr.build_id(), args.reps, args.inner)]
    lines += [json.dumps(r) for r in recs]
    lines.append("# %-18s %-8s %10s %10s %10s %12s" % ("case", "variant", "median ms", "min", "max", "read GB/s*"))
    for r in recs:
        lines.append("# %-18s %-8s %10.4f %10.4f %10.4f %12.1f" % (r["case"], r["variant"], r["ms_median"], r["ms_min"], r["ms_max"], r["read_GBps"]))
    lines.append("# * algorithmic bytes read / time of a call; the arrays stay in the Infinity Cache between calls: not an HBM rate")
    failed = False
    by = {(r["case"], r["variant"]): r for r in recs}
    for case in dict.fromkeys(r["case"] for r in recs):
        a, b = by[(case, "stats")], by[(case, "colour")]
        bound = 2.0 * b["ms_median"] + (b["ms_max"] - b["ms_min"])
        ok = a["ms_median"] <= bound
        failed = failed or not ok
        lines.append("# gate %s: stats %.4f ms <= 2 x colour %.4f + its spread %.4f = %.4f ms (ratio %.2f) -> %s"
                     % (case, a["ms_median"], b["ms_median"], b["ms_max"] - b["ms_min"], bound, a["ms_median"] / b["ms_median"],
                        "PASS" if ok else "FAIL"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
