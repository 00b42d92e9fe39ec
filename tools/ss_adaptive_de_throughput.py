"""Adaptive supersampled DE beside the supersampled DE render it shortens: 1920 x 1080, T = 1, threshold 8,
s in {2, 4}, reach in {0, 2}.

One child process per (case, s), each under its own time limit and with a warm-up round; inside a child the calls ALTERNATE so
that a drift of the machine hits all alike; medians of --reps (at least 5) timed runs with min - max; device events around the
work on a stream of the tool's own.  Cases:
  f64       the default Mandelbrot view at cap 1024 on the F64 road
  pt-wide   a deep view with structure at every scale on plain PT with a wide centre: the Julia set of -0.8 + 0.156i at its
            repelling fixed point (1 + sqrt(1 - 4 J)) / 2, scale 2^200, n = 5, cap 3000, limit 2 (tools/ss_adaptive_throughput.py's)
  bla-wide  the same view on BLA-PT
  scaled-plain  the same Julia view at scale 2^900, n = 16 — it has the same structure at every scale — on SCALED PT's plain
            loop (bits -1) through fr_render_rows_ss_adaptive_de_pt_scaled_device
  scaled-bla    the same on SCALED PT's table form (bits 0)
Variants, per (case, s):
  full      fr_render_rows_ss_de_device (scaled-*: fr_render_rows_ss_de_pt_scaled_device) with best_bytes: the existing call, the
            baseline
  r0, r2    fr_render_rows_ss_adaptive_de_device (scaled-*: its _pt_scaled sibling) at reach 0 and 2, with their refined shares
  all       the same call at threshold -1 (every pixel refined: full's bytes, by the slower way)
  probe     the same call at threshold 255, reach 0: the DE probe, its colours and ss_mark_de_kernel alone, no refine launch
  plain     fr_render_rows_ss_adaptive_device (unshaded, threshold 8), for scale
The expectation beside each ratio is 1 / s^2 + share: the probe costs one sample of every pixel, the refine pass s^2 of the
edge pixels; the probe's colours and the mark pass come on top.

    python3 tools/ss_adaptive_de_throughput.py [--reps 7] [--out profiles/ss_adaptive_de_throughput.txt] [--cases f64,pt-wide,bla-wide,scaled-plain,scaled-bla]"""
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

CASES = ["f64", "pt-wide", "bla-wide", "scaled-plain", "scaled-bla"]
SS = [2, 4]
T, TAU = 1.0, 8
CHILD_LIMIT = 300  # seconds, per (case, s)


def child(case, s, reps):
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
    scaled = case.startswith("scaled-")
    words, bits = (16, -1 if case == "scaled-plain" else 0) if scaled else (5, 0)
    if case == "f64":
        cfg.iterations = 1024
    else:
        import cmath
        from fractions import Fraction

        import pt_wide_orbit as WO

        cfg.limit = 2.0
        cfg.iterations = 3000
        cfg.scale.re = cfg.scale.im = 2.0 ** (900 if scaled else 200)
        cfg.algo = 2
        cfg.julia_set.re, cfg.julia_set.im = -0.8, 0.156
        a, b = Fraction(cfg.julia_set.re), Fraction(cfg.julia_set.im)  # the f64 values, exactly
        c0 = (1 + cmath.sqrt(1 - 4 * complex(cfg.julia_set.re, cfg.julia_set.im))) / 2
        # z^2 - z + J = 0 times its conjugate: a real quartic with the fixed point among its roots
        cst = WO.wide_centre(*WO.newton([1, -2, 1 + 2 * a, -2 * a, a * a + b * b], c0.real, c0.imag), words).c_struct()
        ce, precision, road = C.byref(cst), 3, 2 if scaled else 1 if case == "bla-wide" else 0
    _mn, best = fr.ss_de_workspace_bytes(cfg, s)
    need = max(best, fr.ss_adaptive_de_workspace_bytes(cfg, s), fr.ss_adaptive_workspace_bytes(cfg, s))
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    assert work.data_ptr() % 8 == 0
    nbytes = 3 * cfg.width * cfg.height
    outs = {k: torch.empty(nbytes, dtype=torch.uint8, device=dev) for k in ("full", "r0", "r2", "all", "probe", "plain")}
    counts = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in ("r0", "r2", "all", "probe", "plain")}

    def adaptive_de(key, tau, reach):
        def run_scaled():
            _native.check(lib.fr_render_rows_ss_adaptive_de_pt_scaled_device(C.byref(cfg), ce, bits, T, s, tau, reach, 0, cfg.height, 3,
                                                                             outs[key].data_ptr(), nbytes, work.data_ptr(), work.numel(),
                                                                             counts[key].data_ptr(), st))

        def run():
            _native.check(lib.fr_render_rows_ss_adaptive_de_device(C.byref(cfg), precision, None, ce, road, 0, T, s, tau, reach, 0, cfg.height, 3,
                                                                   outs[key].data_ptr(), nbytes, work.data_ptr(), work.numel(),
                                                                   counts[key].data_ptr(), st))
        return run_scaled if scaled else run

    def full():
        if scaled:
            _native.check(lib.fr_render_rows_ss_de_pt_scaled_device(C.byref(cfg), ce, bits, T, s, 0, cfg.height, 3, outs["full"].data_ptr(), nbytes,
                                                                    work.data_ptr(), best, st))
            return
        _native.check(lib.fr_render_rows_ss_de_device(C.byref(cfg), precision, None, ce, road, 0, T, s, 0, cfg.height, 3, outs["full"].data_ptr(),
                                                      nbytes, work.data_ptr(), best, st))

    def plain():
        _native.check(lib.fr_render_rows_ss_adaptive_device(C.byref(cfg), precision, None, ce, road, bits, s, TAU, 0, cfg.height, 3,
                                                            outs["plain"].data_ptr(), nbytes, work.data_ptr(), work.numel(),
                                                            counts["plain"].data_ptr(), st))

    variants = (("full", full), ("r0", adaptive_de("r0", TAU, 0.0)), ("r2", adaptive_de("r2", TAU, 2.0)), ("all", adaptive_de("all", -1, 0.0)),
                ("probe", adaptive_de("probe", 255, 0.0)), ("plain", plain))
    times = {name: [] for name, _ in variants}
    for r in range(reps + 1):  # the first round warms up
        for name, fn in variants:
            ms = timed(fn)
            if r:
                times[name].append(ms)
    stream.synchronize()
    npx = cfg.width * cfg.height
    assert torch.equal(outs["all"], outs["full"]), "threshold -1 must give the supersampled DE render's bytes"
    for name, ts in times.items():
        rec = {"case": case, "s": s, "variant": name, "ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
               "ms_max": round(max(ts), 4), "runs": len(ts)}
        if name in counts:
            rec["refined_share"] = round(int(counts[name].item()) / npx, 4)
        if name in ("r0", "r2"):  # output pixels further than the threshold from the full supersampled DE image, in some channel
            d = (outs[name].view(-1, 3).to(torch.int16) - outs["full"].view(-1, 3).to(torch.int16)).abs().amax(dim=1)
            rec["pixels_off_by_more_than_threshold"] = int((d > TAU).sum().item())
        print(json.dumps(rec), flush=True)
    print(json.dumps({"case": case, "s": s, "device": fr.device_name(), "build": fr.build_id()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--s", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.child:
        child(args.child, args.s, args.reps)
        return 0
    lines, recs = [], []
    for case in args.cases.split(","):  # one after another: a fresh process per step, never two at a time
        if case not in CASES:
            ap.error("unknown case " + case)
        for s in SS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--s", str(s), "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=CHILD_LIMIT)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("case %s s=%d failed with exit status %d" % (case, s, p.returncode))  # nothing more is started after a failure
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    lines.append(ln)
                    recs.append(json.loads(ln))
    head = [r for r in recs if "device" in r]
    out = ["# tools/ss_adaptive_de_throughput.py on %s, build %s: 1920 x 1080, T = %g, threshold %d, %d timed runs per variant "
           "(median; the calls alternate)" % (head[0]["device"], head[0]["build"], T, TAU, args.reps)]
    out += lines
    out.append("# %-9s %2s %-8s %10s %10s %10s %8s" % ("case", "s", "variant", "median ms", "min", "max", "share"))
    med = {}
    for r in recs:
        if "variant" in r:
            med[(r["case"], r["s"], r["variant"])] = r
            out.append("# %-9s %2d %-8s %10.3f %10.3f %10.3f %8s" % (r["case"], r["s"], r["variant"], r["ms_median"], r["ms_min"], r["ms_max"],
                                                                    "%.4f" % r["refined_share"] if "refined_share" in r else ""))
    for case in args.cases.split(","):
        for s in SS:
            f = med[(case, s, "full")]
            for v in ("r0", "r2"):
                a = med[(case, s, v)]
                ratio, share = a["ms_median"] / f["ms_median"], a["refined_share"]
                model = 1.0 / (s * s) + share
                out.append("# %s s=%d %s: refined share %.4f; adaptive DE / full = %.4f; 1 / s^2 + share = %.4f; ratio - model = %+.4f; "
                           "%d pixels off by more than the threshold" % (case, s, v, share, ratio, model, ratio - model,
                                                                         a["pixels_off_by_more_than_threshold"]))
            out.append("# %s s=%d: threshold -1 / full = %.4f; probe, colours and mark alone = %.4f of full; unshaded adaptive / full = %.4f "
                       "(share %.4f); spread of full (max - min) / median = %.4f"
                       % (case, s, med[(case, s, "all")]["ms_median"] / f["ms_median"], med[(case, s, "probe")]["ms_median"] / f["ms_median"],
                          med[(case, s, "plain")]["ms_median"] / f["ms_median"], med[(case, s, "plain")]["refined_share"],
                          (f["ms_max"] - f["ms_min"]) / f["ms_median"]))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
