"""FR_PRECISION_DD against F64 on the device: kernel time (fr_set_profiling events around the render kernel of a
device-pointer render) and exact pixel-iterations (fr_count_iterations) per view, and the rate ratio.

Views: the default view (Config::new) at 4096^2 with 1024 iterations; the deep Mandelbrot view (centre (0, 1), the
Misiurewicz point c = i, scale 10^18) and the deep Julia view (c = i, centre (0, 1)) at 1920 x 1080 with limit 65536 and
3000 iterations — F64 computes those wrongly (flat blocks), its numbers there are only the cost of the f64 loop.

    python3 tools/dd_throughput.py [--reps 5] [--out profiles/dd_throughput.txt]

Prints one JSON line per (view, precision) and a summary table."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: the library binds to the HIP runtime torch carries)

import fractal_renderer_amd as fr  # noqa: E402
from fractal_renderer_amd import _native  # noqa: E402


def views():
    d = fr.Config.new()
    d.width, d.height, d.iterations = 4096, 4096, 1024
    out = [("default_4096sq_1024it", d)]
    for name, algo in (("deep_mandelbrot_1080p", fr.Algo.Mandelbrot), ("deep_julia_1080p", fr.Algo.Julia)):
        c = fr.Config.new(algo)
        c.width, c.height, c.iterations = 1920, 1080, 3000
        c.limit = 65536.0
        c.pos.re, c.pos.im = 0.0, 1.0
        c.scale.re = c.scale.im = 1e18
        c.julia_set.re, c.julia_set.im = 0.0, 1.0
        out.append((name, c))
    return out


def measure(lib, cfg, precision, reps, buf, stream):
    name = C.create_string_buffer(160)
    ms = C.c_float()
    times = []
    _native.check(lib.fr_set_profiling(1))
    try:
        for _ in range(reps + 1):  # the first is a warm-up (code object load, first-launch work of the view)
            _native.check(lib.fr_render_rows_rgb8_device(C.byref(cfg), int(precision), 0, cfg.height, buf.data_ptr(),
                                                         buf.numel(), stream.cuda_stream))
            _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
            times.append(ms.value)
        _native.check(lib.fr_last_kernel_name(name, len(name)))
    finally:
        _native.check(lib.fr_set_profiling(0))
    return times[1:], name.value.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    args = ap.parse_args()
    fr.init(0)
    lib = _native.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    lines = ["# tools/dd_throughput.py on %s, build %s, %d timed renders per row (median)" % (fr.device_name(), fr.build_id(),
                                                                                            args.reps)]
    rows = []
    for vname, cfg in views():
        buf = torch.empty(cfg.width * cfg.height * 3, dtype=torch.uint8, device=dev)
        rates = {}
        for prec in (fr.Precision.F64, fr.Precision.DD):
            total, npx = fr.count_iterations(cfg, precision=prec)
            times, kname = measure(lib, cfg, prec, args.reps, buf, stream)
            med = statistics.median(times)
            rate = total / (med * 1e-3)
            rates[prec] = rate
            rec = {"view": vname, "precision": prec.name, "width": cfg.width, "height": cfg.height,
                   "iterations": cfg.iterations, "pixel_iterations": total, "kernel_ms_median": round(med, 4),
                   "kernel_ms_all": [round(t, 4) for t in times], "pixel_iterations_per_s": float("%.4g" % rate),
                   "kernel": kname}
            lines.append(json.dumps(rec))
            rows.append((vname, prec.name, med, total, rate, kname))
        lines.append("# %s: DD / F64 pixel-iteration rate = %.4f (1/%.1f)" % (vname, rates[fr.Precision.DD] / rates[fr.Precision.F64],
                                                                          rates[fr.Precision.F64] / rates[fr.Precision.DD]))
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
