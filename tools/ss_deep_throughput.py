"""Anti-aliased deep views on the device: what the supersampled form of a deep road costs beside the road's plain render of
cfg_s, and the fused recolour of a kept anti-aliased view beside the two calls it replaces.

One child process per case, each with a warm-up round; inside a case the variants ALTERNATE so that a drift of the machine
hits all of them alike; medians of --reps (at least 5) timed runs with min - max; device events around the work on a stream of
the tool's own.  Cases:
  a  deep supersampled render, 1920 x 1080 at s = 2, limit 2, on the Misiurewicz point of profiles/pt_wide_orbit.txt:
       a200  scale 2^200, n = 5, cap 3000, WIDE PT (FR_PT_ROAD_PLAIN with the centre)
       a900  scale 2^900, n = 16, cap 6000, SCALED PT with bits = -1 and bits = 40
     variants  ss_best  fr_render_rows_ss_pt_device with best_bytes (one band)
               plain    the road's plain device call of cfg_s into a full-size buffer: the yardstick
     GATE: ss_best <= 1.10 x plain per road (DESIGN.md §3.8's end-to-end gate).
  b  fused recolour, default view, 1024 iterations, smooth on, F64 results of cfg_s kept on the device, RGBA and RGB output:
       b1080  1920 x 1080 at s = 2 and s = 4;   b2160  3840 x 2160 at s = 2 and s = 4
     variants  fused        fr_colour_rows_ss_device
               composition  fr_colour_rows_device into a 3 s^2 bytes-per-pixel scratch, then fr_box_filter_rgb8_device
     GATE: fused <= 1.10 x composition per size, s and format; the composition's own spread is printed beside it.

    python3 tools/ss_deep_throughput.py [--reps 7] [--out profiles/ss_deep_throughput.txt] [--cases a200,a900,b1080,b2160]
Exit status 1 when a gate fails."""
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

CASES = ["a200", "a900", "b1080", "b2160"]
DEEP = {"a200": (200, 5, 3000, [(0, 0)]), "a900": (900, 16, 6000, [(2, -1), (2, 40)])}  # log2 scale, words, cap, [(road, bits)]
ROAD_NAMES = {(0, 0): "wide", (2, -1): "scaled", (2, 40): "scaled_bla40"}


def child(case, reps):
    import torch  # first: the library binds to the HIP runtime torch carries

    import fractal_renderer_amd as fr
    import pt_wide_orbit as WO
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

    if case in DEEP:
        log2, words, cap, roads = DEEP[case]
        s = 2
        cfg = fr.Config.new()
        cfg.limit = 2.0
        cfg.width, cfg.height, cfg.iterations = 1920, 1080, cap
        cfg.scale.re = cfg.scale.im = 2.0 ** log2
        cfg_s = cfg.clone()
        cfg_s.width, cfg_s.height = s * cfg.width, s * cfg.height
        centre = WO.wide_centre(*WO.newton([1, 2, 2, 2], -0.22815549, 1.11514251), words)
        cst = centre.c_struct()
        ce = C.byref(cst)
        mn, best = fr.ss_workspace_bytes(cfg, s)
        big = torch.empty(3 * cfg_s.width * cfg_s.height, dtype=torch.uint8, device=dev)
        assert best == big.numel(), (best, big.numel())  # the workspace and the plain render's buffer are never in use together
        out = torch.empty(3 * cfg.width * cfg.height, dtype=torch.uint8, device=dev)
        for road, bits in roads:
            def ss():
                _native.check(lib.fr_render_rows_ss_pt_device(C.byref(cfg), None, ce, road, bits, s, 0, cfg.height, 3, out.data_ptr(),
                                                              out.numel(), big.data_ptr(), best, st))

            def plain():
                tail = (0, cfg_s.height, 3, big.data_ptr(), big.numel(), st)
                if road == 0:
                    _native.check(lib.fr_render_rows_pt_wide_device(C.byref(cfg_s), ce, *tail))
                else:
                    _native.check(lib.fr_render_rows_pt_scaled_device(C.byref(cfg_s), ce, bits, *tail))

            times = run([("ss_best", ss), ("plain", plain)])
            report("%s_%s_1080p_s%d" % (case, ROAD_NAMES[(road, bits)], s), times,
                   {"src_bytes": big.numel(), "out_bytes": out.numel(), "orbit_entries": fr.pt_orbit_cache()[1]})
    else:
        width, height = (1920, 1080) if case == "b1080" else (3840, 2160)
        for s in (2, 4):
            cfg = fr.Config.new()
            cfg.width, cfg.height, cfg.iterations = width, height, 1024
            cfg_s = cfg.clone()
            cfg_s.width, cfg_s.height = s * width, s * height
            n = cfg_s.width * cfg_s.height
            z = torch.empty(2 * n, dtype=torch.float64, device=dev)
            it = torch.empty(n, dtype=torch.int32, device=dev)
            _native.check(lib.fr_escape_rows_device(C.byref(cfg_s), 0, None, 0, cfg_s.height, 2, z.data_ptr(), it.data_ptr(), st, None))
            stream.synchronize()
            scratch = torch.empty(3 * n, dtype=torch.uint8, device=dev)
            for channels in (4, 3):
                got = torch.empty(channels * width * height, dtype=torch.uint8, device=dev)
                want = torch.empty_like(got)

                def fused():
                    _native.check(lib.fr_colour_rows_ss_device(C.byref(cfg), z.data_ptr(), 2, it.data_ptr(), width, height, s, channels,
                                                               got.data_ptr(), got.numel(), st))

                def composition():
                    _native.check(lib.fr_colour_rows_device(C.byref(cfg), z.data_ptr(), 2, it.data_ptr(), n, 3, scratch.data_ptr(),
                                                            scratch.numel(), st))
                    _native.check(lib.fr_box_filter_rgb8_device(scratch.data_ptr(), width, height, s, channels, want.data_ptr(),
                                                                want.numel(), st))

                times = run([("fused", fused), ("composition", composition)])
                stream.synchronize()
                assert torch.equal(got, want), "the fused recolour and the composition differ"
                report("%s_s%d_%s" % (case, s, "rgba" if channels == 4 else "rgb"), times,
                       {"sample_bytes": 20 * n, "scratch_bytes": scratch.numel(), "out_bytes": got.numel()})
            del z, it, scratch
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
                           capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("case %s failed with exit status %d" % (case, p.returncode))  # nothing more is started after a failure
        for ln in p.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(ln)
                recs.append(json.loads(ln))
    head = [r for r in recs if "device" in r]
    out = ["# tools/ss_deep_throughput.py on %s, build %s, %d timed runs per variant (median; variants alternate)"
           % (head[0]["device"], head[0]["build"], args.reps)]
    out += lines
    out.append("# %-30s %-12s %10s %10s %10s" % ("case", "variant", "median ms", "min", "max"))
    med, order = {}, []
    for r in recs:
        if "variant" in r:
            med[(r["case"], r["variant"])] = r
            if r["case"] not in order:
                order.append(r["case"])
            out.append("# %-30s %-12s %10.3f %10.3f %10.3f" % (r["case"], r["variant"], r["ms_median"], r["ms_min"], r["ms_max"]))
    failed = False
    for label in order:
        new, old = ("ss_best", "plain") if label.startswith("a") else ("fused", "composition")
        a, b = med[(label, new)], med[(label, old)]
        ratio = a["ms_median"] / b["ms_median"]
        spread = (b["ms_max"] - b["ms_min"]) / b["ms_median"]
        note = ""
        if new == "fused":
            note = "; fused reads %.0f GB/s of samples" % (a["sample_bytes"] / 1e9 / (a["ms_median"] * 1e-3))
        ok = ratio <= 1.10
        failed = failed or not ok
        out.append("# gate %s: %s / %s = %.4f (<= 1.10); spread of the yardstick (max - min) / median = %.4f%s -> %s"
                   % (label, new, old, ratio, spread, note, "PASS" if ok else "FAIL"))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
