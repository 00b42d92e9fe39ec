"""What an iterations change and a recolour cost with the view kept on the device, against rendering again.

Per view, in ONE process, every shape warmed up first, the variants ALTERNATING inside the same run (one of each per
round, --reps rounds), device events around each call, median per variant and the spread (max - min) of its repeats:
  (i)   raw(M)      fr_escape_rows_device at the new cap M: the existing render road, what an iterations change cost before;
  (ii)  extend N->M fr_escape_extend_device over arrays that hold cap N (restored from a device copy before every repeat,
                    outside the timed span);
  (iii) colour      fr_colour_rows_device RGBA over the arrays at cap M, beside fr_render_rows_rgba8_device at M and beside
                    fr_colour_rgb8_device (RGB; F64 / F32 only: it takes two doubles per pixel).
Work from fr_count_iterations: S(M) and S(M) - S(N) — exactly what the extension executes — and the pixel-iterations/s
of (i) and (ii).  For DD, S comes from the escape indices of the same view (pos_lo included).

Views: the default CLI Mandelbrot view at 3840 x 2160, 1024 -> 2048, F64 and F32; the Julia set of c = -0.8 + 0.156i at
3840 x 2160, 1024 -> 4096, F64 and F32; the deep view (centre (0, 1), scale 10^18) at 1920 x 1080 in DD, 3000 -> 6000.

    python3 tools/extend_throughput.py [--reps 7] [--out profiles/extend_throughput.txt]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: the library binds to the HIP runtime torch carries)

import fractal_renderer_amd as fr  # noqa: E402
from fractal_renderer_amd import _native  # noqa: E402

P = fr.Precision


def cli_view(algo, width, height):
    cfg = fr.Config.new(algo)
    cfg.width, cfg.height, cfg.exposure = width, height, 5.0
    if algo == fr.Algo.Julia:
        cfg.julia_set.re, cfg.julia_set.im = -0.8, 0.156
    else:
        cfg.pos.re = -0.6
    return cfg


def views():
    out = []
    for prec in (P.F64, P.F32):
        out.append(("default_2160p", cli_view(fr.Algo.Mandelbrot, 3840, 2160), prec, 1024, 2048))
    for prec in (P.F64, P.F32):
        out.append(("julia_2160p", cli_view(fr.Algo.Julia, 3840, 2160), prec, 1024, 4096))
    d = fr.Config.new()
    d.width, d.height, d.limit, d.exposure = 1920, 1080, 65536.0, 5.0
    d.pos.re, d.pos.im = 0.0, 1.0
    d.scale.re = d.scale.im = 1e18
    out.append(("deep_1080p", d, P.DD, 3000, 6000))
    return out


def executed(cfg, prec, cap):
    c = cfg.clone()
    c.iterations = cap
    if prec != P.DD:
        return fr.count_iterations(c, precision=prec)[0]
    _, it = fr.escape_rows(c, precision=prec)
    it = it.astype(np.uint64)
    return int(np.where(it < cap, it + 1, cap).sum())


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
    lines = ["# tools/extend_throughput.py on %s, build %s, %d alternating rounds per view (median; spread = max - min)"
             % (fr.device_name(), fr.build_id(), args.reps)]
    table = []
    for vname, cfg, prec, n_cap, m_cap in views():
        zw = 4 if prec == P.DD else 2
        npx = cfg.width * cfg.height
        z = torch.empty(npx * zw, dtype=torch.float64, device=dev)
        it = torch.empty(npx, dtype=torch.int32, device=dev)
        z_n, it_n = torch.empty_like(z), torch.empty_like(it)
        z_m, it_m = torch.empty_like(z), torch.empty_like(it)
        rgba = torch.empty(npx * 4, dtype=torch.uint8, device=dev)
        c_n, c_m = cfg.clone(), cfg.clone()
        c_n.iterations, c_m.iterations = n_cap, m_cap

        def raw(c, zz, ii):
            _native.check(lib.fr_escape_rows_device(C.byref(c), int(prec), None, 0, c.height, zw, zz.data_ptr(), ii.data_ptr(), h, None))

        def restore():
            z.copy_(z_n)
            it.copy_(it_n)

        def ext():
            _native.check(lib.fr_escape_extend_device(C.byref(c_m), int(prec), None, 0, c_m.height, n_cap, zw, z.data_ptr(),
                                                      it.data_ptr(), h, None))

        def colour_rows():
            _native.check(lib.fr_colour_rows_device(C.byref(c_m), z_m.data_ptr(), zw, it_m.data_ptr(), npx, 4, rgba.data_ptr(),
                                                    rgba.numel(), h))

        def colour_old():
            _native.check(lib.fr_colour_rgb8_device(C.byref(c_m), z_m.data_ptr(), it_m.data_ptr(), npx, rgba.data_ptr(), rgba.numel(), h))

        def render_rgba():
            if prec == P.DD:
                _native.check(lib.fr_render_rows_dd_device(C.byref(c_m), None, 0, c_m.height, 4, rgba.data_ptr(), rgba.numel(), h))
            else:
                _native.check(lib.fr_render_rows_rgba8_device(C.byref(c_m), int(prec), 0, c_m.height, rgba.data_ptr(), rgba.numel(), h))

        variants = [("raw(M)", lambda: raw(c_m, z_m, it_m), None), ("extend N->M", ext, restore), ("colour_rows RGBA", colour_rows, None),
                    ("render RGBA(M)", render_rgba, None)]
        if prec != P.DD:
            variants.append(("colour_rgb8 (old)", colour_old, None))
        with torch.cuda.stream(stream):
            raw(c_n, z_n, it_n)
            raw(c_m, z_m, it_m)
            restore()
            ext()
            stream.synchronize()
            same = bool(torch.equal(it, it_m)) and bool(torch.equal(z.view(torch.int64), z_m.view(torch.int64)))
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
        s_n, s_m = executed(cfg, prec, n_cap), executed(cfg, prec, m_cap)
        rec = {"view": vname, "precision": prec.name, "width": cfg.width, "height": cfg.height, "from": n_cap, "to": m_cap,
               "extended_equals_raw": same, "pixel_iterations_M": s_m, "pixel_iterations_extension": s_m - s_n}
        for name, _, _ in variants:
            t = times[name]
            rec[name] = {"ms_median": round(statistics.median(t), 4), "ms_spread": round(max(t) - min(t), 4),
                         "ms_all": [round(x, 4) for x in t]}
        t_raw, t_ext = rec["raw(M)"]["ms_median"], rec["extend N->M"]["ms_median"]
        rec["raw_rate"] = float("%.4g" % (s_m / (t_raw * 1e-3)))
        rec["extend_rate"] = float("%.4g" % ((s_m - s_n) / (t_ext * 1e-3))) if s_m > s_n else 0.0
        rec["extend_wins_by_more_than_raw_spread"] = bool(t_raw - t_ext > rec["raw(M)"]["ms_spread"])
        lines.append(json.dumps(rec))
        table.append((vname, prec.name, rec))
        del z, it, z_n, it_n, z_m, it_m, rgba
    lines.append("# %-14s %-4s %9s %9s %7s %13s %13s %10s %10s %9s %9s %9s" % (
        "view", "prec", "raw ms", "extend ms", "ratio", "S(M)", "S(M)-S(N)", "raw it/s", "ext it/s", "colour ms", "render ms", "old col"))
    for vname, pname, r in table:
        lines.append("# %-14s %-4s %9.3f %9.3f %7.2f %13d %13d %10.3g %10.3g %9.3f %9.3f %9s" % (
            vname, pname, r["raw(M)"]["ms_median"], r["extend N->M"]["ms_median"],
            r["raw(M)"]["ms_median"] / r["extend N->M"]["ms_median"], r["pixel_iterations_M"], r["pixel_iterations_extension"],
            r["raw_rate"], r["extend_rate"], r["colour_rows RGBA"]["ms_median"], r["render RGBA(M)"]["ms_median"],
            "%.3f" % r["colour_rgb8 (old)"]["ms_median"] if "colour_rgb8 (old)" in r else "-"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
