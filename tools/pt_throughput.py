"""FR_PRECISION_PT against DD and F64 on the device: kernel time (fr_set_profiling events around the render kernel of a
device-pointer render, median of --reps), exact pixel-iterations per view (from the escape indices of the same view,
pos_lo included), the rates and their ratios, and the host time of the reference orbit (fr_debug_reference_orbit).

Views: the default view (Config::new) at 4096^2 with 1024 iterations; the two deep views of tools/dd_throughput.py
(centre (0, 1), scale 10^18, 3000 iterations) at 1920 x 1080; the seahorse-valley view at 1920 x 1080 (centre
-0.743643887037158704752191506114774 + 0.131825904205311970493132056385139i split into pos + pos_lo, scale 10^20,
20000 iterations, limit 2).  F64 computes the deep views wrongly (flat blocks); its numbers there are only the cost
of the f64 loop.

    python3 tools/pt_throughput.py [--reps 5] [--out profiles/pt_throughput.txt]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: the library binds to the HIP runtime torch carries)

import fractal_renderer_amd as fr  # noqa: E402
from fractal_renderer_amd import _native  # noqa: E402

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")


def views():
    d = fr.Config.new()
    d.width, d.height, d.iterations = 4096, 4096, 1024
    out = [("default_4096sq_1024it", d, (0.0, 0.0))]
    for name, algo in (("deep_mandelbrot_1080p", fr.Algo.Mandelbrot), ("deep_julia_1080p", fr.Algo.Julia)):
        c = fr.Config.new(algo)
        c.width, c.height, c.iterations = 1920, 1080, 3000
        c.limit = 65536.0
        c.pos.re, c.pos.im = 0.0, 1.0
        c.scale.re = c.scale.im = 1e18
        c.julia_set.re, c.julia_set.im = 0.0, 1.0
        out.append((name, c, (0.0, 0.0)))
    s = fr.Config.new()
    s.width, s.height, s.iterations = 1920, 1080, 20000
    s.limit = 2.0
    (s.pos.re, lo_re), (s.pos.im, lo_im) = fr.split_dd(SEAHORSE[0]), fr.split_dd(SEAHORSE[1])
    s.scale.re = s.scale.im = 1e20
    out.append(("seahorse_1080p_20000it", s, (lo_re, lo_im)))
    return out


def render(lib, cfg, precision, lo, buf, stream):
    n = buf.numel()
    if precision == fr.Precision.F64:
        return lib.fr_render_rows_rgb8_device(C.byref(cfg), 0, 0, cfg.height, buf.data_ptr(), n, stream.cuda_stream)
    f = lib.fr_render_rows_pt_device if precision == fr.Precision.PT else lib.fr_render_rows_dd_device
    return f(C.byref(cfg), C.byref(_native.Imaginary(*lo)), 0, cfg.height, 3, buf.data_ptr(), n, stream.cuda_stream)


def measure(lib, cfg, precision, lo, reps, buf, stream):
    name = C.create_string_buffer(160)
    ms = C.c_float()
    times = []
    _native.check(lib.fr_set_profiling(1))
    try:
        for _ in range(reps + 1):  # the first is a warm-up (code object load; PT: the view's reference orbit)
            _native.check(render(lib, cfg, precision, lo, buf, stream))
            _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
            times.append(ms.value)
        _native.check(lib.fr_last_kernel_name(name, len(name)))
    finally:
        _native.check(lib.fr_set_profiling(0))
    return times[1:], name.value.decode()


def pixel_iterations(cfg, precision, lo):
    if precision == fr.Precision.F64:
        return fr.count_iterations(cfg, precision=precision)[0]
    _, it = fr.escape_rows(cfg, precision=precision, pos_lo=lo)
    it = it.astype(np.uint64)
    return int(np.where(it < cfg.iterations, it + 1, cfg.iterations).sum())


def orbit_ms(lib, cfg, lo):
    n = C.c_uint32()
    t = time.perf_counter()
    _native.check(lib.fr_debug_reference_orbit(C.byref(cfg), C.byref(_native.Imaginary(*lo)), 0, None, 0, C.byref(n)))
    return (time.perf_counter() - t) * 1e3, n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    args = ap.parse_args()
    fr.init(0)
    lib = _native.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    lines = ["# tools/pt_throughput.py on %s, build %s, %d timed renders per row (median)" % (fr.device_name(), fr.build_id(),
                                                                                            args.reps)]
    rows = []
    for vname, cfg, lo in views():
        buf = torch.empty(cfg.width * cfg.height * 3, dtype=torch.uint8, device=dev)
        hms, entries = orbit_ms(lib, cfg, lo)
        lines.append("# %s: reference orbit on the host %.3f ms, %d entries (%.3f ms per 10^4 entries)"
                     % (vname, hms, entries, hms * 1e4 / max(entries, 1)))
        rates = {}
        for prec in (fr.Precision.F64, fr.Precision.DD, fr.Precision.PT):
            total = pixel_iterations(cfg, prec, lo)
            times, kname = measure(lib, cfg, prec, lo, args.reps, buf, stream)
            med = statistics.median(times)
            rate = total / (med * 1e-3)
            rates[prec] = rate
            rec = {"view": vname, "precision": prec.name, "width": cfg.width, "height": cfg.height,
                   "iterations": cfg.iterations, "pixel_iterations": total, "kernel_ms_median": round(med, 4),
                   "kernel_ms_all": [round(t, 4) for t in times], "pixel_iterations_per_s": float("%.4g" % rate),
                   "kernel": kname}
            lines.append(json.dumps(rec))
            rows.append((vname, prec.name, med, total, rate, kname))
        lines.append("# %s: PT / DD pixel-iteration rate = %.2f, PT / F64 = %.4f" % (
            vname, rates[fr.Precision.PT] / rates[fr.Precision.DD], rates[fr.Precision.PT] / rates[fr.Precision.F64]))
    lines.append("# %-24s %-4s %12s %16s %14s  %s" % ("view", "prec", "kernel ms", "pixel-its", "pixel-its/s", "kernel"))
    for vname, pname, med, total, rate, kname in rows:
        lines.append("# %-24s %-4s %12.3f %16d %14.4g  %s" % (vname, pname, med, total, rate, kname))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
