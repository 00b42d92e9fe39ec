"""What the derivative costs on BLA-PT, and what a DE user gains from the table: escape_bla_de_kernel (fr_escape_rows_de_pt_bla_device;
csrc/fr_de_bla.hip) beside escape_bla_kernel (fr_escape_rows_pt_bla_device, the same loop without the derivative) and
escape_pt_de_kernel (fr_escape_rows_de_device, PT: the derivative without the table), from the same build in the same process, on
the deep views of tools/pt_throughput.py (deep_mandelbrot_1080p, deep_julia_1080p, seahorse_1080p_20000it), 40 bits.

Kernel time is fr_set_profiling's events around the render kernel, as tools/de_throughput.py takes it: median of --reps renders
after a warm-up, the three kernels alternating within every repetition so that a drift of the machine meets all three alike.
Beside the times: the nominal pixel-iterations (exact, from the escape indices of the BLA render) and the passes of
fr_debug_bla_count, so that the times can be read per pass.  Two ratios per view:
    de_bla_over_bla     escape_bla_de_kernel / escape_bla_kernel      what the derivative costs
    pt_de_over_de_bla   escape_pt_de_kernel / escape_bla_de_kernel    what a DE user gains
--view NAME runs one view, so that a job can give each its own time limit; --out appends.

    python3 tools/de_bla_throughput.py [--view NAME] [--reps 5] [--out profiles/de_bla_throughput.txt]"""
import argparse
import ctypes as C
import importlib.util
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

DEEP = ("deep_mandelbrot_1080p", "deep_julia_1080p", "seahorse_1080p_20000it")
BITS = 40


def pt_views():
    spec = importlib.util.spec_from_file_location("pt_throughput", os.path.join(ROOT, "tools", "pt_throughput.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return [v for v in mod.views() if v[0] in DEEP]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--view", default=None)
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    args = ap.parse_args()
    fr.init(0)
    lib = _native.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    lines = ["# tools/de_bla_throughput.py on %s, build %s, %d bits, %d timed renders per kernel (median), alternating"
             % (fr.device_name(), fr.build_id(), BITS, args.reps)]
    for vname, cfg, lo in pt_views():
        if args.view and vname != args.view:
            continue
        n = cfg.width * cfg.height
        z = torch.empty(2 * n, dtype=torch.float64, device=dev)
        der = torch.empty(2 * n, dtype=torch.float64, device=dev)
        it = torch.empty(n, dtype=torch.int32, device=dev)
        plo = C.byref(_native.Imaginary(*lo))
        calls = {
            "bla": lambda: lib.fr_escape_rows_pt_bla_device(C.byref(cfg), plo, None, BITS, 0, cfg.height, z.data_ptr(), it.data_ptr(), s),
            "de_bla": lambda: lib.fr_escape_rows_de_pt_bla_device(C.byref(cfg), plo, None, BITS, 0, cfg.height, z.data_ptr(), it.data_ptr(),
                                                                  der.data_ptr(), s),
            "pt_de": lambda: lib.fr_escape_rows_de_device(C.byref(cfg), 3, plo, 0, cfg.height, z.data_ptr(), it.data_ptr(), der.data_ptr(), s),
        }
        ms, times, names = C.c_float(), {k: [] for k in calls}, {}
        _native.check(lib.fr_set_profiling(1))
        try:
            for rep in range(args.reps + 1):  # the first round is a warm-up (code object load, the view's orbit and table)
                for which, call in calls.items():
                    _native.check(call())
                    _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
                    if rep:
                        times[which].append(ms.value)
                    else:
                        name = C.create_string_buffer(160)
                        _native.check(lib.fr_last_kernel_name(name, len(name)))
                        names[which] = name.value.decode()
        finally:
            _native.check(lib.fr_set_profiling(0))
        _native.check(calls["bla"]())
        stream.synchronize()
        iters = it.cpu().numpy().view(np.uint32).astype(np.uint64)
        total = int(np.where(iters < cfg.iterations, iters + 1, cfg.iterations).sum())
        passes, steps = fr.bla_count(cfg, pos_lo=lo, bla=BITS)
        assert steps == total
        med = {k: statistics.median(t) for k, t in times.items()}
        rec = {"view": vname, "width": cfg.width, "height": cfg.height, "iterations": cfg.iterations, "bits": BITS,
               "pixel_iterations": total, "bla_passes": passes, "iterations_per_pass": round(total / passes, 3)}
        for k in calls:
            rec[k + "_kernel"] = names[k]
            rec[k + "_ms_median"] = round(med[k], 4)
            rec[k + "_ms_all"] = [round(t, 4) for t in times[k]]
        rec["bla_ns_per_pass"] = float("%.4g" % (med["bla"] * 1e6 / passes))
        rec["de_bla_ns_per_pass"] = float("%.4g" % (med["de_bla"] * 1e6 / passes))
        rec["pt_de_ns_per_pixel_iteration"] = float("%.4g" % (med["pt_de"] * 1e6 / total))
        rec["de_bla_over_bla"] = round(med["de_bla"] / med["bla"], 3)
        rec["pt_de_over_de_bla"] = round(med["pt_de"] / med["de_bla"], 3)
        lines.append(json.dumps(rec))
        lines.append("# %s: escape_bla_de_kernel / escape_bla_kernel = %.2f (what the derivative costs); escape_pt_de_kernel / "
                     "escape_bla_de_kernel = %.2f (what a DE user gains); %.2f iterations per pass"
                     % (vname, rec["de_bla_over_bla"], rec["pt_de_over_de_bla"], rec["iterations_per_pass"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
