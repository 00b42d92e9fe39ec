"""Adaptive supersampling beside the supersampled render it shortens: 1920 x 1080, s = 4, threshold 8.

One child process per case, each with a warm-up pair; inside a case the two calls ALTERNATE so that a drift of the machine hits
both alike; medians of --reps (at least 5) timed runs with min - max; device events around the work on a stream of the tool's
own.  Cases:
  f64   the default Mandelbrot view at cap 1024 on the F64 road
          adaptive  fr_render_rows_ss_adaptive_device
          full      fr_render_rows_ss_device with best_bytes (one band): the parent's unchanged call
          probe     the adaptive call at threshold 255: the probe pass and ss_mark_kernel alone, no refine launch — where
                    the time of `adaptive` goes (not part of the pair's ratio)
  bla   a BLA-PT deep view with structure at every scale: the Julia set of -0.8 + 0.156i at its repelling fixed point
        (1 + sqrt(1 - 4 J)) / 2, scale 2^200, n = 5, cap 3000, limit 2
          adaptive  fr_render_rows_ss_adaptive_device with FR_PT_ROAD_BLA
          full      fr_render_rows_ss_pt_device with FR_PT_ROAD_BLA and best_bytes
          probe     as above
  flat  a BLA-PT deep view without edges: the Misiurewicz point of profiles/pt_wide_orbit.txt at the same scale and cap — the
        refined share is 0 and the adaptive call is its probe pass: the floor of the ratio
The refined share (edge pixels / pixels) stands beside each pair, with the ratio adaptive / full and its distance from
1 / s^2 + share: the probe costs one sample of every pixel, the refine pass s^2 of the edge pixels.

    python3 tools/ss_adaptive_throughput.py [--reps 7] [--out profiles/ss_adaptive_throughput.txt] [--cases f64,bla,flat]"""
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

CASES = ["f64", "bla", "flat"]
S, TAU = 4, 8


def child(case, reps):
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
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    cfg = fr.Config.new()
    cfg.width, cfg.height = 1920, 1080
    ce, precision, road = None, 0, 0
    if case == "f64":
        cfg.iterations = 1024
    else:
        import pt_wide_orbit as WO

        cfg.limit = 2.0
        cfg.iterations = 3000
        cfg.scale.re = cfg.scale.im = 2.0 ** 200
        if case == "bla":
            import cmath
            from fractions import Fraction

            cfg.algo = 2
            cfg.julia_set.re, cfg.julia_set.im = -0.8, 0.156
            a, b = Fraction(cfg.julia_set.re), Fraction(cfg.julia_set.im)  # the f64 values, exactly
            c0 = (1 + cmath.sqrt(1 - 4 * complex(cfg.julia_set.re, cfg.julia_set.im))) / 2
            # z^2 - z + J = 0 times its conjugate: a real quartic with the fixed point among its roots
            cst = WO.wide_centre(*WO.newton([1, -2, 1 + 2 * a, -2 * a, a * a + b * b], c0.real, c0.imag), 5).c_struct()
        else:
            cst = WO.wide_centre(*WO.newton([1, 2, 2, 2], -0.22815549, 1.11514251), 5).c_struct()
        ce, precision, road = C.byref(cst), 3, 1
    _mn, best = fr.ss_workspace_bytes(cfg, S)
    work = torch.empty(max(best, fr.ss_adaptive_workspace_bytes(cfg, S)), dtype=torch.uint8, device=dev)
    assert work.data_ptr() % 8 == 0
    out_a = torch.empty(3 * cfg.width * cfg.height, dtype=torch.uint8, device=dev)
    out_f = torch.empty_like(out_a)
    refined = torch.zeros(1, dtype=torch.int64, device=dev)

    out_p = torch.empty_like(out_a)

    def adaptive(tau=TAU, out=out_a, count=refined):
        _native.check(lib.fr_render_rows_ss_adaptive_device(C.byref(cfg), precision, None, ce, road, 0, S, tau, 0, cfg.height, 3, out.data_ptr(),
                                                            out.numel(), work.data_ptr(), work.numel(), count.data_ptr() if count is not None else None,
                                                            st))

    def probe():
        adaptive(255, out_p, None)

    def full():
        if case == "f64":
            _native.check(lib.fr_render_rows_ss_device(C.byref(cfg), 0, None, S, 0, cfg.height, 3, out_f.data_ptr(), out_f.numel(),
                                                       work.data_ptr(), best, st, None))
        else:
            _native.check(lib.fr_render_rows_ss_pt_device(C.byref(cfg), None, ce, road, 0, S, 0, cfg.height, 3, out_f.data_ptr(), out_f.numel(),
                                                          work.data_ptr(), best, st))

    times = {"adaptive": [], "full": [], "probe": []}
    for r in range(reps + 1):  # the first round warms up
        for name, fn in (("adaptive", adaptive), ("full", full), ("probe", probe)):
            ms = timed(fn)
            if r:
                times[name].append(ms)
    stream.synchronize()
    npx = cfg.width * cfg.height
    share = int(refined.item()) / npx
    differ = int((out_a != out_f).sum().item())
    for name, ts in times.items():
        print(json.dumps({"case": case, "variant": name, "ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
                          "ms_max": round(max(ts), 4), "runs": len(ts), "refined_share": round(share, 4),
                          "bytes_differing_from_full": differ}), flush=True)
    print(json.dumps({"case": case, "device": fr.device_name(), "build": fr.build_id()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.child:
        child(args.child, args.reps)
        return 0
    lines, recs = [], []
    for case in args.cases.split(","):  # one after another: a fresh process per case, never two at a time
        if case not in CASES:
            ap.error("unknown case " + case)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(args.reps)],
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("case %s failed with exit status %d" % (case, p.returncode))  # nothing more is started after a failure
        for ln in p.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(ln)
                recs.append(json.loads(ln))
    head = [r for r in recs if "device" in r]
    out = ["# tools/ss_adaptive_throughput.py on %s, build %s: 1920 x 1080, s = %d, threshold %d, %d timed runs per variant "
           "(median; the two calls alternate)" % (head[0]["device"], head[0]["build"], S, TAU, args.reps)]
    out += lines
    out.append("# %-6s %-10s %10s %10s %10s" % ("case", "variant", "median ms", "min", "max"))
    med = {}
    for r in recs:
        if "variant" in r:
            med[(r["case"], r["variant"])] = r
            out.append("# %-6s %-10s %10.3f %10.3f %10.3f" % (r["case"], r["variant"], r["ms_median"], r["ms_min"], r["ms_max"]))
    for case in args.cases.split(","):
        a, f = med[(case, "adaptive")], med[(case, "full")]
        ratio, share = a["ms_median"] / f["ms_median"], a["refined_share"]
        model = 1.0 / (S * S) + share
        out.append("# %s: refined share %.4f; adaptive / full = %.4f; 1 / s^2 + share = %.4f; ratio - model = %+.4f; spread of full "
                   "(max - min) / median = %.4f; probe pass and mark alone = %.4f of full"
                   % (case, share, ratio, model, ratio - model, (f["ms_max"] - f["ms_min"]) / f["ms_median"],
                      med[(case, "probe")]["ms_median"] / f["ms_median"]))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
