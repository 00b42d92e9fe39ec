"""What raising the cap of a view past 2^440 costs with its SCALED PT state kept on the device, against rendering it again
(include/fractal_hip.h, "RESUMABLE SCALED PT").

Views, both 1920 x 1080, n = 16 words, limit 2, the centres of tests/pt_scaled_model.py:
  M     the Misiurewicz point at 2^900: every pixel escapes between steps ~550 and ~570, so the links 280 -> 560 (M = 2N) and
        448 -> 560 (M = 1.25N) continue EVERY pixel;
  MINI  the period-267 minibrot at 2^861, about a sixth of whose pixels sit at the cap: links 3204 -> 6408 and 3204 -> 4005.
One process per view.  Per link, every shape warmed up first, the variants ALTERNATING (one of each per round, --reps rounds),
kernel times from the library's profiling events (fr_set_profiling / fr_last_kernel_ms), median and min - max:
  (i)   plain(M)     fr_escape_rows_pt_scaled_device, bits = -1, at the new cap M: escape_pt_scaled_kernel, the road that exists
                     without the state; state(M), fr_escape_rows_pt_scaled_state_device at M, is the same loop storing 40
                     instead of 20 bytes per pixel: state / plain is what keeping the state costs;
  (ii)  extend N->M  fr_escape_extend_pt_scaled_device over arrays that hold cap N (restored from a device copy before every
                     repeat, outside the timed span), against plain(M).  `share_beyond_N` is the share of plain(M)'s executed
                     pixel-iterations that lie beyond step N — what the extension executes — and `extend_over_plain` the
                     measured ratio of the kernel times beside it;
  (iii) the host side of the same two roads: wall time of a call over 8 rows that has to make the orbit for cap M — fresh
                     (another view was cached) against continued (cap N was cached) — with the entries computed from
                     fr_debug_pt_orbit_cache; the call returns once its kernel is enqueued, so this is host time.
No gate: the numbers are written down, not judged.

    python3 tools/pt_scaled_extend_throughput.py [--reps 5] [--out profiles/pt_scaled_extend_throughput.txt]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

VIEWS = {"M": ("M", 900, ((280, 560), (448, 560))), "MINI": ("MINI", 861, ((3204, 6408), (3204, 4005)))}
WORDS = 16


def child(name, reps):
    import torch  # first: the library binds to the HIP runtime torch carries

    import fractal_renderer_amd as fr
    import pt_scaled_model as S
    import pt_wide_model as W
    from fractal_renderer_amd import _native

    fr.init(0)
    lib = _native.load()
    centre_name, scale_log2, links = VIEWS[name]
    cfg = fr.Config.new()
    cfg.limit = 2.0
    cfg.width, cfg.height = 1920, 1080
    cfg.scale.re = cfg.scale.im = 2.0 ** scale_log2
    ints = S.centre_ints(centre_name, WORDS)
    centre = fr.WideCentre(WORDS, re=W.to_words(ints[0], WORDS), im=W.to_words(ints[1], WORDS))
    st = centre.c_struct()
    ce = C.byref(st)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    h = stream.cuda_stream
    npx = cfg.width * cfg.height

    def arrays():
        return (torch.empty(npx * 2, dtype=torch.float64, device=dev), torch.empty(npx, dtype=torch.int32, device=dev),
                torch.empty(npx * 2, dtype=torch.float64, device=dev), torch.empty(npx, dtype=torch.int32, device=dev))

    def ptrs(a):
        return [t.data_ptr() for t in a]

    def at(cap):
        c = cfg.clone()
        c.iterations = cap
        return c

    def state(c, a, rows=None):
        _native.check(lib.fr_escape_rows_pt_scaled_state_device(C.byref(c), ce, 0, rows or c.height, *ptrs(a), h))

    def extend(c, a, n, rows=None):
        _native.check(lib.fr_escape_extend_pt_scaled_device(C.byref(c), ce, 0, rows or c.height, n, *ptrs(a), h))

    def plain(c, a):
        _native.check(lib.fr_escape_rows_pt_scaled_device(C.byref(c), ce, -1, 0, c.height, a[0].data_ptr(), a[1].data_ptr(), h))

    def forget():
        other = fr.Config.new()
        other.width = other.height = 8
        other.iterations = 3
        other.pos.re = 0.125
        fr.escape_rows(other, precision=fr.Precision.PT)

    def executed(it, cap):
        it = it.to(torch.int64)
        return int(torch.where(it < cap, it + 1, torch.full_like(it, cap)).sum().item())

    def same(a, b):
        return all(bool(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y))
                   for x, y in zip(a, b))

    ms = C.c_float()
    kname = C.create_string_buffer(160)
    for n_cap, m_cap in links:
        c_n, c_m = at(n_cap), at(m_cap)
        work, at_n, at_m, plain_m = arrays(), arrays(), arrays(), arrays()

        def restore():
            for a, b in zip(work, at_n):
                a.copy_(b)

        host = {"fresh": [], "continued": []}
        entries = {}
        with torch.cuda.stream(stream):
            for rnd in range(reps + 1):  # (iii): round 0 warms up
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
                    entries[kind] = fr.pt_orbit_cache()
                    if rnd:
                        host[kind].append((t1 - t0) * 1e3)
            forget()
            state(c_n, at_n)
            state(c_m, at_m)
            plain(c_m, plain_m)
            restore()
            extend(c_m, work, n_cap)
            stream.synchronize()
            rec = {"view": name, "scale_log2": scale_log2, "width": cfg.width, "height": cfg.height, "from": n_cap, "to": m_cap,
                   "device": fr.device_name(), "build": fr.build_id(), "extended_equals_state": same(work, at_m),
                   "state_z_iters_equal_plain": same(plain_m[:2], at_m[:2])}
            variants = [("plain(M)", lambda: plain(c_m, plain_m), None), ("state(M)", lambda: state(c_m, at_m), None),
                        ("extend N->M", lambda: extend(c_m, work, n_cap), restore)]
            times = {v[0]: [] for v in variants}
            names = {}
            _native.check(lib.fr_set_profiling(1))
            try:
                for rnd in range(reps + 1):  # alternating; round 0 warms every shape up
                    for label, fn, before in variants:
                        if before:
                            before()
                            stream.synchronize()
                        fn()
                        _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
                        _native.check(lib.fr_last_kernel_name(kname, len(kname)))
                        names[label] = kname.value.decode()
                        if rnd:
                            times[label].append(ms.value)
            finally:
                _native.check(lib.fr_set_profiling(0))
        s_n, s_m = executed(at_n[1], n_cap), executed(at_m[1], m_cap)
        rec.update(pixels_running_at_N=int((at_n[1] == n_cap).sum().item()), pixels=npx, pixels_at_cap_M=int((at_m[1] == m_cap).sum().item()),
                   pixel_iterations_M=s_m, pixel_iterations_extension=s_m - s_n, share_beyond_N=round((s_m - s_n) / s_m, 4))
        for label, t in times.items():
            rec[label] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                          "kernel": names[label]}
        for kind in ("fresh", "continued"):
            t = host[kind]
            rec["orbit_host_" + kind] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                                         "entries_computed": entries[kind][3], "entries": entries[kind][1]}
        rec["state_over_plain"] = round(rec["state(M)"]["ms_median"] / rec["plain(M)"]["ms_median"], 4)
        rec["extend_over_plain"] = round(rec["extend N->M"]["ms_median"] / rec["plain(M)"]["ms_median"], 4)
        print(json.dumps(rec), flush=True)
        del work, at_n, at_m, plain_m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    ap.add_argument("--view", choices=sorted(VIEWS), default=None, help="measure this view in this process (what the parent starts)")
    args = ap.parse_args()
    assert args.reps >= 5, "median of at least 5"
    if args.view:
        child(args.view, args.reps)
        return 0
    lines = ["# tools/pt_scaled_extend_throughput.py: the scaled state render and its extension against the plain scaled render "
             "(bits = -1) at the new cap, alternating, %d timed rounds after a warm-up (median, min - max), one process per view"
             % args.reps]
    table = []
    for name in sorted(VIEWS):  # one after another: a fresh process per view, never two at a time
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--view", name, "--reps", str(args.reps)], capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            return 2  # nothing more is started after a failure
        for line in (x for x in r.stdout.splitlines() if x.startswith("{")):
            lines.append(line)
            table.append(json.loads(line))
    lines.append("# %-5s %-14s %9s %9s %9s %8s %8s %9s %12s %12s" % (
        "view", "link", "plain ms", "state ms", "extend ms", "(i) s/p", "(ii) e/p", "share>N", "orbit fresh", "orbit cont."))
    for r in table:
        lines.append("# %-5s %-14s %9.3f %9.3f %9.3f %8.3f %8.3f %9.3f %9.3f ms %9.3f ms" % (
            r["view"], "%d -> %d" % (r["from"], r["to"]), r["plain(M)"]["ms_median"], r["state(M)"]["ms_median"],
            r["extend N->M"]["ms_median"], r["state_over_plain"], r["extend_over_plain"], r["share_beyond_N"],
            r["orbit_host_fresh"]["ms_median"], r["orbit_host_continued"]["ms_median"]))
        lines.append("#       %d of %d pixels running at N, %d at the cap M; the orbit: %d entries computed fresh, %d continued" % (
            r["pixels_running_at_N"], r["pixels"], r["pixels_at_cap_M"], r["orbit_host_fresh"]["entries_computed"],
            r["orbit_host_continued"]["entries_computed"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
