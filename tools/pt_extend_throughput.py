"""What raising the cap of a deep view costs with its PT state kept on the device, against rendering it again.

The seahorse view (pos + pos_lo, scale 10^20) at 1920 x 1080 in FR_PRECISION_PT, links 10 000 -> 20 000 and 19 000 -> 20 000.
Per link, in ONE process, every shape warmed up first, the variants ALTERNATING inside the same run (one of each per round,
--reps rounds), device events around each call, median per variant and the spread (max - min) of its repeats:
  (i)   raw(M)       fr_escape_rows_device in PT at the new cap M: escape_pt_kernel, the existing road;
  (ii)  state(M)     fr_escape_rows_pt_state_device at M: the same loop storing 40 instead of 20 bytes per pixel;
  (iii) extend N->M  fr_escape_extend_pt_device over arrays that hold cap N (restored from a device copy before every
                     repeat, outside the timed span).
The orbit is in the context's cache for all three (the warm-up put it there), so these are kernel times.
The extension's time is set by its longest orbit, not by its work: `longest_continued_steps` is the most steps one pixel runs
in the link and `extend_ns_per_step_of_longest_orbit` the extension's time divided by it (the render's time over M beside it).
Work: executed pixel-iterations S(N), S(M) from the stored escape indices of this very view (fr_count_iterations takes no
pos_lo), S(M) - S(N) being exactly what the extension executes; pixel-iterations/s of each variant.
Host orbit time, separately: wall time of a call over 8 rows that has to make the orbit for cap M — fresh (another view was
cached: M + 2 entries) against continued (cap N was cached: M - N entries, a device-to-device copy of the rest) — with the
entry counts from fr_debug_pt_orbit_cache; the call returns once its kernel is enqueued, so this is host time.

    python3 tools/pt_extend_throughput.py [--reps 7] [--out profiles/pt_extend_throughput.txt]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: the library binds to the HIP runtime torch carries)

import fractal_renderer_amd as fr  # noqa: E402
from fractal_renderer_amd import _native  # noqa: E402

SEAHORSE_RE = "-0.743643887037158704752191506114774"
SEAHORSE_IM = "0.131825904205311970493132056385139"
LINKS = ((10000, 20000), (19000, 20000))


def seahorse(width=1920, height=1080):
    (re, re_lo), (im, im_lo) = fr.split_dd(SEAHORSE_RE), fr.split_dd(SEAHORSE_IM)
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.limit, cfg.exposure = width, height, 2.0, 5.0
    cfg.pos.re, cfg.pos.im = re, im
    cfg.scale.re = cfg.scale.im = 1e20
    assert Fraction(re) + Fraction(re_lo) != Fraction(re)
    return cfg, _native.Imaginary(re_lo, im_lo)


def executed(it, cap):
    """sum of executed iterations from escape indices on the device: i + 1 for an escape at i, cap on exhaustion"""
    it = it.to(torch.int64)
    return int(torch.where(it < cap, it + 1, torch.full_like(it, cap)).sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    args = ap.parse_args()
    assert args.reps >= 5, "median of at least 5"
    fr.init(0)
    lib = _native.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cfg, lo = seahorse()
    plo = C.byref(lo)
    npx = cfg.width * cfg.height
    lines = ["# tools/pt_extend_throughput.py on %s, build %s, seahorse view %d x %d, %d alternating rounds per link (median; "
             "spread = max - min)" % (fr.device_name(), fr.build_id(), cfg.width, cfg.height, args.reps)]

    def arrays():
        return (torch.empty(npx * 2, dtype=torch.float64, device=dev), torch.empty(npx, dtype=torch.int32, device=dev),
                torch.empty(npx * 2, dtype=torch.float64, device=dev), torch.empty(npx, dtype=torch.int32, device=dev))

    def ptrs(a):
        return [t.data_ptr() for t in a]

    def state(c, a, rows=None):
        _native.check(lib.fr_escape_rows_pt_state_device(C.byref(c), plo, 0, rows or c.height, *ptrs(a), h))

    def extend(c, a, n, rows=None):
        _native.check(lib.fr_escape_extend_pt_device(C.byref(c), plo, 0, rows or c.height, n, *ptrs(a), h))

    def raw(c, a):
        _native.check(lib.fr_escape_rows_device(C.byref(c), int(fr.Precision.PT), plo, 0, c.height, 2, a[0].data_ptr(), a[1].data_ptr(), h, None))

    def cache():
        out = (C.c_uint32 * 4)()
        _native.check(lib.fr_debug_pt_orbit_cache(out))
        return tuple(out)

    def forget():
        other = fr.Config.new()
        other.width = other.height = 8
        other.iterations = 3
        other.pos.re = 0.125
        fr.escape_rows(other, precision=fr.Precision.PT)

    table = []
    for n_cap, m_cap in LINKS:
        c_n, c_m = cfg.clone(), cfg.clone()
        c_n.iterations, c_m.iterations = n_cap, m_cap
        work, at_n, at_m, raw_m = arrays(), arrays(), arrays(), arrays()

        def restore():
            for a, b in zip(work, at_n):
                a.copy_(b)

        # host time of making the orbit for cap M, on 8 rows
        host = {"fresh": [], "continued": []}
        entries = {}
        with torch.cuda.stream(stream):
            for rnd in range(args.reps + 1):
                for kind in ("fresh", "continued"):
                    forget()
                    if kind == "continued":
                        state(c_n, work, 8)
                    stream.synchronize()
                    t0 = time.perf_counter()
                    if kind == "continued":
                        extend(c_m, work, n_cap, 8)
                    else:
                        state(c_m, work, 8)
                    t1 = time.perf_counter()
                    stream.synchronize()
                    entries[kind] = cache()
                    if rnd:
                        host[kind].append((t1 - t0) * 1e3)
            forget()
            state(c_n, at_n)
            state(c_m, at_m)
            raw(c_m, raw_m)
            restore()
            extend(c_m, work, n_cap)
            stream.synchronize()
            same = all(bool(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b))
                       for a, b in zip(work, at_m))
            same_raw = bool(torch.equal(raw_m[1], at_m[1])) and bool(torch.equal(raw_m[0].view(torch.int64), at_m[0].view(torch.int64)))
            variants = [("raw(M)", lambda: raw(c_m, raw_m), None), ("state(M)", lambda: state(c_m, at_m), None),
                        ("extend N->M", lambda: extend(c_m, work, n_cap), restore)]
            times = {name: [] for name, _, _ in variants}
            for rnd in range(args.reps + 1):  # round 0 warms every shape up
                for name, fn, before in variants:
                    if before:
                        before()
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if rnd:
                        times[name].append(e0.elapsed_time(e1))
        s_n, s_m = executed(at_n[1], n_cap), executed(at_m[1], m_cap)
        run_mask = at_n[1] == n_cap
        running = int(run_mask.sum().item())
        it_m = at_m[1][run_mask].to(torch.int64)
        longest = int(torch.where(it_m < m_cap, it_m + 1, torch.full_like(it_m, m_cap)).max().item()) - n_cap if running else 0
        rec = {"view": "seahorse_1080p", "precision": "PT", "from": n_cap, "to": m_cap, "extended_equals_state": same,
               "state_z_iters_equal_raw": same_raw, "pixels_running_at_N": running, "longest_continued_steps": longest, "pixel_iterations_M": s_m,
               "pixel_iterations_extension": s_m - s_n}
        for name, _, _ in variants:
            t = times[name]
            rec[name] = {"ms_median": round(statistics.median(t), 4), "ms_spread": round(max(t) - min(t), 4), "ms_all": [round(x, 4) for x in t]}
        for kind in ("fresh", "continued"):
            t = host[kind]
            rec["orbit_host_" + kind] = {"ms_median": round(statistics.median(t), 4), "ms_spread": round(max(t) - min(t), 4),
                                         "entries_computed": entries[kind][3], "entries": entries[kind][1]}
        t_raw, t_state, t_ext = (rec[k]["ms_median"] for k in ("raw(M)", "state(M)", "extend N->M"))
        rec["raw_rate"] = float("%.4g" % (s_m / (t_raw * 1e-3)))
        rec["state_rate"] = float("%.4g" % (s_m / (t_state * 1e-3)))
        rec["extend_rate"] = float("%.4g" % ((s_m - s_n) / (t_ext * 1e-3)))
        rec["state_over_raw_time"] = round(t_state / t_raw, 4)
        rec["extend_ns_per_step_of_longest_orbit"] = round(t_ext * 1e6 / longest, 1) if longest else 0.0
        rec["raw_ns_per_step_of_longest_orbit"] = round(t_raw * 1e6 / m_cap, 1)
        rec["extend_rate_over_raw_rate"] = round(rec["extend_rate"] / rec["raw_rate"], 4)
        lines.append(json.dumps(rec))
        table.append(rec)
        del work, at_n, at_m, raw_m
    lines.append("# %-16s %9s %9s %9s %8s %14s %14s %10s %10s %8s %11s %11s" % (
        "link", "raw ms", "state ms", "extend ms", "(ii)/(i)", "S(M)", "S(M)-S(N)", "raw it/s", "ext it/s", "ext/raw", "orbit fresh", "orbit cont."))
    for r in table:
        lines.append("# %-16s %9.3f %9.3f %9.3f %8.3f %14d %14d %10.3g %10.3g %8.3f %8.3f ms %8.3f ms" % (
            "%d -> %d" % (r["from"], r["to"]), r["raw(M)"]["ms_median"], r["state(M)"]["ms_median"], r["extend N->M"]["ms_median"],
            r["state_over_raw_time"], r["pixel_iterations_M"], r["pixel_iterations_extension"], r["raw_rate"], r["extend_rate"],
            r["extend_rate_over_raw_rate"], r["orbit_host_fresh"]["ms_median"], r["orbit_host_continued"]["ms_median"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
