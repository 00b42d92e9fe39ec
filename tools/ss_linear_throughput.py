"""Linear-light supersampling (include/fractal_hip.h, "LINEAR-LIGHT SUPERSAMPLING"): what the linear form of the reduction costs
beside the byte form, and whether the byte form still costs what it did.

One child process per case, each with a warm-up round; inside a case the variants ALTERNATE so that a drift of the machine hits
all of them alike; medians of --reps (at least 5) timed runs; device events around the work on a stream of the tool's own.
--tree ROOT runs the byte variants of ANOTHER checkout (one that may lack the _tf calls, e.g. the parent commit, built) through
the same code: the byte form against the parent is the two files side by side.  Cases (3.8's (a) and (b)):
  a  default view, 1024 iterations, F64, output 8192^2 at s = 2 (16384^2 samples, 805 MB), best_bytes:
       plain           fr_render_rows_rgb8_device of cfg_s: the yardstick, its spread (max - min) / median is reported
       ss_bytes        fr_render_rows_ss_device              ss_linear      fr_render_rows_ss_tf_device, transfer 1
       filter_bytes    fr_box_filter_rgb8_device             filter_linear  fr_box_filter_rgb8_tf_device, transfer 1
       d2d             hipMemcpyDtoDAsync of the same 805 MB
  b  1920 x 1080 at s = 2 and s = 4: plain, ss_bytes, ss_linear, filter_bytes, filter_linear
  k  the kept recolour at 1080p, s = 4: fr_colour_rows_ss_device against fr_colour_rows_ss_tf_device, transfer 1
  d  the adaptive call at 1080p, s = 4, threshold 8: fr_render_rows_ss_adaptive_device against its _tf form, transfer 1

    python3 tools/ss_linear_throughput.py [--reps 7] [--out profiles/ss_linear_throughput.txt] [--cases abkd] [--tree ROOT]
No gate: the numbers are reported, with the ratios DESIGN.md 3.31 discusses."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hip_runtime():
    """the HIP runtime this process already has loaded (the one torch carries)"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def child(case, reps, tree):
    import torch

    sys.path.insert(0, tree)
    import fractal_renderer_amd as fr
    from fractal_renderer_amd import _native

    fr.init(0)
    lib = _native.load()
    has_tf = hasattr(lib, "fr_render_rows_ss_tf_device")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    check = _native.check

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def run(label, variants, extra=None):
        times = {n: [] for n, _ in variants}
        for r in range(reps + 1):
            for n, fn in variants:
                ms = timed(fn)
                if r:
                    times[n].append(ms)
        for n, ts in times.items():
            rec = {"case": label, "variant": n, "ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
                   "ms_max": round(max(ts), 4), "runs": len(ts)}
            rec.update(extra or {})
            print(json.dumps(rec), flush=True)

    def view(width, height):
        cfg = fr.Config.new()
        cfg.width, cfg.height, cfg.iterations = width, height, 1024
        return cfg

    def scaled_up(cfg, s):
        big = cfg.clone()
        big.width, big.height = cfg.width * s, cfg.height * s
        return big

    def ss_case(label, cfg, s, with_copy):
        cfg_s = scaled_up(cfg, s)
        _, best = fr.ss_workspace_bytes(cfg, s)
        big = torch.empty(3 * cfg_s.width * cfg_s.height, dtype=torch.uint8, device=dev)
        out = torch.empty(3 * cfg.width * cfg.height, dtype=torch.uint8, device=dev)
        assert best == big.numel()
        p, need = C.byref(cfg), out.numel()
        v = [("plain", lambda: check(lib.fr_render_rows_rgb8_device(C.byref(cfg_s), 0, 0, cfg_s.height, big.data_ptr(), big.numel(), st))),
             ("ss_bytes", lambda: check(lib.fr_render_rows_ss_device(p, 0, None, s, 0, cfg.height, 3, out.data_ptr(), need, big.data_ptr(),
                                                                     best, st, None)))]
        if has_tf:
            v.append(("ss_linear", lambda: check(lib.fr_render_rows_ss_tf_device(p, 0, None, s, 1, 0, cfg.height, 3, out.data_ptr(), need,
                                                                                 big.data_ptr(), best, st, None))))
        # the filters read what the last render left in `big`: the same image for every variant
        v.append(("filter_bytes", lambda: check(lib.fr_box_filter_rgb8_device(big.data_ptr(), cfg.width, cfg.height, s, 3, out.data_ptr(), need, st))))
        if has_tf:
            v.append(("filter_linear", lambda: check(lib.fr_box_filter_rgb8_tf_device(big.data_ptr(), cfg.width, cfg.height, s, 1, 3,
                                                                                      out.data_ptr(), need, st))))
        if with_copy:
            hip = hip_runtime()
            hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            copy = torch.empty_like(big)

            def d2d():
                rc = hip.hipMemcpyDtoDAsync(copy.data_ptr(), big.data_ptr(), big.numel(), st)
                assert rc == 0, rc

            v.append(("d2d", d2d))
        run(label, v, {"src_bytes": big.numel(), "out_bytes": need})

    if case == "a":
        ss_case("a_default_8192sq_s2", view(8192, 8192), 2, True)
    elif case == "b":
        for s in (2, 4):
            ss_case("b_default_1080p_s%d" % s, view(1920, 1080), s, False)
    elif case == "k":
        cfg, s = view(1920, 1080), 4
        cfg_s = scaled_up(cfg, s)
        n = cfg_s.width * cfg_s.height
        z = torch.empty(2 * n, dtype=torch.float64, device=dev)
        it = torch.empty(n, dtype=torch.int32, device=dev)
        out = torch.empty(4 * cfg.width * cfg.height, dtype=torch.uint8, device=dev)
        fr.escape_rows_device(cfg_s, z.data_ptr(), it.data_ptr(), stream=st)
        stream.synchronize()
        p = C.byref(cfg)
        v = [("kept_bytes", lambda: check(lib.fr_colour_rows_ss_device(p, z.data_ptr(), 2, it.data_ptr(), cfg.width, cfg.height, s, 4,
                                                                       out.data_ptr(), out.numel(), st)))]
        if has_tf:
            v.append(("kept_linear", lambda: check(lib.fr_colour_rows_ss_tf_device(p, z.data_ptr(), 2, it.data_ptr(), cfg.width, cfg.height, s, 1,
                                                                                   4, out.data_ptr(), out.numel(), st))))
        run("k_kept_1080p_s4", v, {"src_bytes": 20 * n, "out_bytes": out.numel()})
    elif case == "d":
        cfg, s = view(1920, 1080), 4
        work_len = fr.ss_adaptive_workspace_bytes(cfg, s)
        work = torch.empty(work_len, dtype=torch.uint8, device=dev)
        out = torch.empty(3 * cfg.width * cfg.height, dtype=torch.uint8, device=dev)
        refined = torch.zeros(1, dtype=torch.int64, device=dev)
        p = C.byref(cfg)
        v = [("adaptive_bytes", lambda: check(lib.fr_render_rows_ss_adaptive_device(p, 0, None, None, 0, 0, s, 8, 0, cfg.height, 3, out.data_ptr(),
                                                                                    out.numel(), work.data_ptr(), work_len,
                                                                                    refined.data_ptr(), st)))]
        if has_tf:
            v.append(("adaptive_linear", lambda: check(lib.fr_render_rows_ss_adaptive_tf_device(p, 0, None, None, 0, 0, s, 1, 8, 0, cfg.height, 3,
                                                                                                out.data_ptr(), out.numel(), work.data_ptr(),
                                                                                                work_len, refined.data_ptr(), st))))
        run("d_adaptive_1080p_s4_t8", v, {"out_bytes": out.numel()})
        stream.synchronize()
        print(json.dumps({"case": "d_adaptive_1080p_s4_t8", "refined": int(refined.item()), "pixels": cfg.width * cfg.height}), flush=True)
    print(json.dumps({"case": case, "device": fr.device_name(), "build": fr.build_id(), "has_tf": has_tf}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    ap.add_argument("--cases", default="abkd")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose built library runs (default: this one)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    tree = os.path.abspath(args.tree)
    if args.child:
        child(args.child, args.reps, tree)
        return 0
    lines, recs = [], []
    for case in args.cases:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(args.reps), "--tree", tree],
                           capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("case %s failed with exit status %d" % (case, p.returncode))
        for ln in p.stdout.splitlines():
            if ln.startswith("{"):
                lines.append(ln)
                recs.append(json.loads(ln))
    head = [r for r in recs if "device" in r]
    out = ["# tools/ss_linear_throughput.py on %s, build %s (%s the _tf calls), %d timed runs per variant (median; variants alternate)"
           % (head[0]["device"], head[0]["build"], "with" if head[0]["has_tf"] else "WITHOUT", args.reps)]
    out += lines
    out.append("# %-26s %-16s %10s %10s %10s" % ("case", "variant", "median ms", "min", "max"))
    med = {}
    for r in recs:
        if "variant" in r:
            med[(r["case"], r["variant"])] = r
            out.append("# %-26s %-16s %10.3f %10.3f %10.3f" % (r["case"], r["variant"], r["ms_median"], r["ms_min"], r["ms_max"]))
    for case in sorted({c for c, _ in med}):
        m = {v: med[(c, v)] for c, v in med if c == case}
        if "plain" in m:
            pl = m["plain"]
            out.append("# %s: yardstick spread (max - min) / median of plain = %.4f; filter_bytes / ss_bytes = %.4f"
                       % (case, (pl["ms_max"] - pl["ms_min"]) / pl["ms_median"], m["filter_bytes"]["ms_median"] / m["ss_bytes"]["ms_median"]))
        for lin, byt in (("ss_linear", "ss_bytes"), ("filter_linear", "filter_bytes"), ("kept_linear", "kept_bytes"),
                         ("adaptive_linear", "adaptive_bytes")):
            if lin in m:
                out.append("# %s: %s / %s = %.4f" % (case, lin, byt, m[lin]["ms_median"] / m[byt]["ms_median"]))
        if "d2d" in m:
            for f in ("filter_bytes", "filter_linear"):
                if f in m:
                    out.append("# %s: %s / d2d = %.4f" % (case, f, m[f]["ms_median"] / m["d2d"]["ms_median"]))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
