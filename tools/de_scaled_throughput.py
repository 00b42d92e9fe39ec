"""What the scaled derivative costs on SCALED PT: escape_pt_scaled_de_kernel and escape_bla_scaled_de_kernel
(fr_escape_rows_de_pt_scaled_device, bits -1 and 40; csrc/fr_de_scaled.hip) beside their siblings' escape mode, escape_pt_scaled_kernel
and escape_bla_scaled_kernel (fr_escape_rows_pt_scaled_device, the same loops without the derivative), from the same build in the
same process, on the deep views of tools/pt_scaled_throughput.py: M440 (2^440, the edge of WIDE PT's domain) and M900 (2^900), both
1920 x 1080 on the Misiurewicz point.

Kernel time is fr_set_profiling's events around the render kernel: median of --reps renders after a warm-up round, the four kernels
alternating within every repetition so that a drift of the machine meets all four alike.  The two table kernels share one cached
table (same view, bits and kind), so no timed call builds one.  Beside the times: the nominal pixel-iterations and the passes of
fr_debug_pt_scaled_count, so that the times can be read per pass.  Two ratios per view:
    pt_scaled_de_over_pt_scaled     escape_pt_scaled_de_kernel / escape_pt_scaled_kernel
    bla_scaled_de_over_bla_scaled   escape_bla_scaled_de_kernel / escape_bla_scaled_kernel
No gate: what the derivative costs is a number to write down.  --view NAME runs one view; --out appends.

    python3 tools/de_scaled_throughput.py [--view M440|M900] [--reps 5] [--out profiles/de_scaled_throughput.txt]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402,F401  (first: the library binds to the HIP runtime torch carries)

import fractal_renderer_amd as fr  # noqa: E402
import pt_scaled_throughput as PS  # noqa: E402  (the views)
import pt_wide_orbit as WO  # noqa: E402
from fractal_renderer_amd import _native  # noqa: E402

BITS = 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--view", choices=sorted(PS.VIEWS), default=None)
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    args = ap.parse_args()
    fr.init(0)
    lib = _native.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    lines = ["# tools/de_scaled_throughput.py on %s, build %s, %d bits, %d timed renders per kernel (median), alternating"
             % (fr.device_name(), fr.build_id(), BITS, args.reps)]
    for vname in sorted(PS.VIEWS):
        if args.view and vname != args.view:
            continue
        scale_log2, words, cap = PS.VIEWS[vname]
        cfg = fr.Config.new()
        cfg.limit = 2.0
        cfg.width, cfg.height, cfg.iterations = 1920, 1080, cap
        cfg.scale.re = cfg.scale.im = 2.0 ** scale_log2
        centre = WO.wide_centre(*WO.newton([1, 2, 2, 2], -0.22815549, 1.11514251), words)
        st = centre.c_struct()
        ce = C.byref(st)
        n = cfg.width * cfg.height
        z = torch.empty(2 * n, dtype=torch.float64, device=dev)
        der = torch.empty(2 * n, dtype=torch.float64, device=dev)
        it = torch.empty(n, dtype=torch.int32, device=dev)
        head = (C.byref(cfg), ce)
        rows = (0, cfg.height, z.data_ptr(), it.data_ptr())
        calls = {
            "pt_scaled": lambda: lib.fr_escape_rows_pt_scaled_device(*head, -1, *rows, s),
            "pt_scaled_de": lambda: lib.fr_escape_rows_de_pt_scaled_device(*head, -1, *rows, der.data_ptr(), s),
            "bla_scaled": lambda: lib.fr_escape_rows_pt_scaled_device(*head, BITS, *rows, s),
            "bla_scaled_de": lambda: lib.fr_escape_rows_de_pt_scaled_device(*head, BITS, *rows, der.data_ptr(), s),
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
        stream.synchronize()
        passes, steps = fr.pt_scaled_count(cfg, centre, bla=BITS)
        med = {k: statistics.median(t) for k, t in times.items()}
        rec = {"view": vname, "width": cfg.width, "height": cfg.height, "iterations": cfg.iterations, "scale_log2": scale_log2,
               "bits": BITS, "pixel_iterations": steps, "bla_scaled_passes": passes, "iterations_per_pass": round(steps / passes, 3)}
        for k in calls:
            rec[k + "_kernel"] = names[k]
            rec[k + "_ms_median"] = round(med[k], 4)
            rec[k + "_ms_all"] = [round(t, 4) for t in times[k]]
        rec["pt_scaled_de_ns_per_pixel_iteration"] = float("%.4g" % (med["pt_scaled_de"] * 1e6 / steps))
        rec["bla_scaled_de_ns_per_pass"] = float("%.4g" % (med["bla_scaled_de"] * 1e6 / passes))
        rec["pt_scaled_de_over_pt_scaled"] = round(med["pt_scaled_de"] / med["pt_scaled"], 3)
        rec["bla_scaled_de_over_bla_scaled"] = round(med["bla_scaled_de"] / med["bla_scaled"], 3)
        lines.append(json.dumps(rec))
        lines.append("# %s: escape_pt_scaled_de_kernel / escape_pt_scaled_kernel = %.2f; escape_bla_scaled_de_kernel / "
                     "escape_bla_scaled_kernel = %.2f; %.2f iterations per pass"
                     % (vname, rec["pt_scaled_de_over_pt_scaled"], rec["bla_scaled_de_over_bla_scaled"], rec["iterations_per_pass"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
