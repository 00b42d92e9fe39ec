"""Supersampled rendering on the device: what the box filter and the banding cost beside the render they follow.

One child process per case, each with a warm-up round; inside a case the variants ALTERNATE (variant 1, 2, ..., 1, 2, ...)
so that a drift of the machine hits all of them alike; medians of --reps (at least 5) timed runs; device events around the
work on a stream of the tool's own (host clock for the host road).  Cases ("Supersampling"):
  a  default view, 1024 iterations, F64, output 8192^2 at s = 2 (C2's 16384^2 samples, 805 MB):
       ss_best   fr_render_rows_ss_device with best_bytes (one band)
       plain     fr_render_rows_rgb8_device of cfg_s into a full 805 MB buffer: the yardstick
       filter    fr_box_filter_rgb8_device over that buffer
       d2d       hipMemcpyDtoDAsync of the same 805 MB
       ss_64MiB  fr_render_rows_ss_device with a 64 MiB workspace (reported only)
     GATES: ss_best <= 1.10 x plain (end to end), filter <= 1.5 x d2d.
  b  1920 x 1080 at s = 2 and s = 4, F64 (report only: launch tails dominate at this size)
  c  PT seahorse view, 1920 x 1080, s = 2 (report only)
  d  the host road of (a), fr_render_rows_ss, against fr_render_rgb8 of cfg_s (report only)

    python3 tools/ss_throughput.py [--reps 7] [--out profiles/ss_throughput.txt] [--cases abcd]
Exit status 1 when a gate fails."""
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

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")


def hip_runtime():
    """the HIP runtime this process already has loaded (the one torch carries)"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def child(case, reps):
    import numpy as np
    import torch

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
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def run(variants):
        """[(name, fn)] -> {name: [ms, ...]}: one warm-up round, then `reps` rounds, the variants alternating"""
        times = {n: [] for n, _ in variants}
        for r in range(reps + 1):
            for n, fn in variants:
                ms = timed(fn)
                if r:
                    times[n].append(ms)
        return times

    def report(label, times, extra=None):
        for n, ts in times.items():
            rec = {"case": label, "variant": n, "ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
                   "ms_max": round(max(ts), 4), "runs": len(ts)}
            rec.update(extra or {})
            print(json.dumps(rec), flush=True)

    def ss_variants(cfg, s, precision=0, lo=None, with_copy=False, with_small=False):
        cfg_s = cfg.clone()
        cfg_s.width, cfg_s.height = cfg.width * s, cfg.height * s
        mn, best = fr.ss_workspace_bytes(cfg, s)
        big = torch.empty(3 * cfg_s.width * cfg_s.height, dtype=torch.uint8, device=dev)
        work = big  # the workspace of ss_best and the plain render's buffer are never in use at the same time
        out = torch.empty(3 * cfg.width * cfg.height, dtype=torch.uint8, device=dev)
        plo = C.byref(_native.Imaginary(*lo)) if lo is not None else None
        assert best == big.numel(), (best, big.numel())

        def ss(work_len):
            _native.check(lib.fr_render_rows_ss_device(C.byref(cfg), precision, plo, s, 0, cfg.height, 3, out.data_ptr(),
                                                       out.numel(), work.data_ptr(), work_len, st, None))

        def plain():
            if precision == 3:
                _native.check(lib.fr_render_rows_pt_device(C.byref(cfg_s), plo, 0, cfg_s.height, 3, big.data_ptr(), big.numel(), st))
            else:
                _native.check(lib.fr_render_rows_rgb8_device(C.byref(cfg_s), precision, 0, cfg_s.height, big.data_ptr(),
                                                             big.numel(), st))

        def filt():
            _native.check(lib.fr_box_filter_rgb8_device(big.data_ptr(), cfg.width, cfg.height, s, 3, out.data_ptr(), out.numel(), st))

        v = [("ss_best", lambda: ss(best)), ("plain", plain), ("filter", filt)]
        if with_copy:
            hip = hip_runtime()
            hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            copy = torch.empty_like(big)

            def d2d():
                rc = hip.hipMemcpyDtoDAsync(copy.data_ptr(), big.data_ptr(), big.numel(), st)
                assert rc == 0, rc

            v.append(("d2d", d2d))
        if with_small:
            v.append(("ss_64MiB", lambda: ss(64 << 20)))
        return v, {"src_bytes": big.numel(), "out_bytes": out.numel()}

    if case == "a":
        cfg = fr.Config.new()
        cfg.width, cfg.height, cfg.iterations = 8192, 8192, 1024
        v, extra = ss_variants(cfg, 2, with_copy=True, with_small=True)
        report("a_default_8192sq_s2_f64", run(v), extra)
    elif case == "b":
        for s in (2, 4):
            cfg = fr.Config.new()
            cfg.width, cfg.height, cfg.iterations = 1920, 1080, 1024
            v, extra = ss_variants(cfg, s)
            report("b_default_1080p_s%d_f64" % s, run(v), extra)
    elif case == "c":
        cfg = fr.Config.new()
        cfg.width, cfg.height, cfg.iterations = 1920, 1080, 20000
        cfg.limit = 2.0
        (cfg.pos.re, lo_re), (cfg.pos.im, lo_im) = fr.split_dd(SEAHORSE[0]), fr.split_dd(SEAHORSE[1])
        cfg.scale.re = cfg.scale.im = 1e20
        v, extra = ss_variants(cfg, 2, precision=3, lo=(lo_re, lo_im))
        report("c_pt_seahorse_1080p_s2", run(v), extra)
    elif case == "d":
        cfg = fr.Config.new()
        cfg.width, cfg.height, cfg.iterations = 8192, 8192, 1024
        cfg_s = cfg.clone()
        cfg_s.width, cfg_s.height = 16384, 16384
        small = np.empty((cfg.height, cfg.width, 3), dtype=np.uint8)
        large = np.empty((cfg_s.height, cfg_s.width, 3), dtype=np.uint8)
        times = {"host_ss": [], "host_plain": []}
        for r in range(reps + 1):
            t = time.perf_counter()
            _native.check(lib.fr_render_rows_ss(C.byref(cfg), 0, None, 2, 0, cfg.height, 3, small.ctypes.data, small.nbytes, None))
            a = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            _native.check(lib.fr_render_rgb8(C.byref(cfg_s), large.ctypes.data, large.nbytes))
            b = (time.perf_counter() - t) * 1e3
            if r:
                times["host_ss"].append(a)
                times["host_plain"].append(b)
        report("d_host_road_of_a", times, {"src_bytes": large.nbytes, "out_bytes": small.nbytes, "clock": "host"})
    print(json.dumps({"case": case, "device": fr.device_name(), "build": fr.build_id()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.child:
        child(args.child, args.reps)
        return 0
    lines, recs = [], []
    for case in args.cases:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(args.reps)],
                           capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("case %s failed with exit status %d" % (case, p.returncode))
        for ln in p.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(ln)
                recs.append(json.loads(ln))
    head = [r for r in recs if "device" in r]
    out = ["# tools/ss_throughput.py on %s, build %s, %d timed runs per variant (median; variants alternate)"
           % (head[0]["device"], head[0]["build"], args.reps)]
    out += lines
    out.append("# %-28s %-10s %10s %10s %10s" % ("case", "variant", "median ms", "min", "max"))
    med = {}
    for r in recs:
        if "variant" in r:
            med[(r["case"], r["variant"])] = r
            out.append("# %-28s %-10s %10.3f %10.3f %10.3f" % (r["case"], r["variant"], r["ms_median"], r["ms_min"], r["ms_max"]))
    failed = False
    a = "a_default_8192sq_s2_f64"
    if (a, "plain") in med:
        ss, plain, filt, d2d = (med[(a, k)] for k in ("ss_best", "plain", "filter", "d2d"))
        e2e = ss["ms_median"] / plain["ms_median"]
        spread = (plain["ms_max"] - plain["ms_min"]) / plain["ms_median"]
        fr_ = filt["ms_median"] / d2d["ms_median"]
        gb = filt["src_bytes"] / 1e9
        out.append("# gate end to end: ss_best / plain = %.4f (<= 1.10); spread of the yardstick (max - min) / median = %.4f -> %s"
                   % (e2e, spread, "PASS" if e2e <= 1.10 else "FAIL"))
        out.append("# gate filter: filter / d2d = %.4f (<= 1.5); filter reads %.0f GB/s of source, the copy moves %.0f GB/s -> %s"
                   % (fr_, gb / (filt["ms_median"] * 1e-3), gb / (d2d["ms_median"] * 1e-3), "PASS" if fr_ <= 1.5 else "FAIL"))
        failed = e2e > 1.10 or fr_ > 1.5
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
