"""What the orbit's derivative costs: the DE renders (fr_escape_rows_de_device; csrc/fr_de.hip) beside the unchanged escape
renders of the same build (fr_escape_rows_device, F64 and PT) on the views of tools/pt_throughput.py, and the shaded recolour
beside the plain one.

Kernel time is fr_set_profiling's events around the render kernel, median of --reps after a warm-up; pixel-iterations are exact,
from the escape indices of the same render; ns per pixel-iteration is their quotient.  The recolours (which record no profiling
events) are timed with stream events around 20 launches.  --view NAME runs one view, so that a job can give each its own time
limit; --out appends.

    python3 tools/de_throughput.py [--view NAME] [--reps 5] [--out profiles/de_throughput.txt]"""
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


def pt_views():
    spec = importlib.util.spec_from_file_location("pt_throughput", os.path.join(ROOT, "tools", "pt_throughput.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.views()


def kernel_ms(lib, call, reps):
    ms, times = C.c_float(), []
    _native.check(lib.fr_set_profiling(1))
    try:
        for _ in range(reps + 1):  # the first is a warm-up (code object load; PT: the view's reference orbit)
            _native.check(call())
            _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
            times.append(ms.value)
        name = C.create_string_buffer(160)
        _native.check(lib.fr_last_kernel_name(name, len(name)))
    finally:
        _native.check(lib.fr_set_profiling(0))
    return times[1:], name.value.decode()


def stream_ms(stream, call, launches=20):
    _native.check(call())
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(launches):
        _native.check(call())
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


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
    lines = ["# tools/de_throughput.py on %s, build %s, %d timed renders per row (median)" % (fr.device_name(), fr.build_id(), args.reps)]
    for vname, cfg, lo in pt_views():
        if args.view and vname != args.view:
            continue
        n = cfg.width * cfg.height
        z = torch.empty(2 * n, dtype=torch.float64, device=dev)
        der = torch.empty(2 * n, dtype=torch.float64, device=dev)
        it = torch.empty(n, dtype=torch.int32, device=dev)
        rgba = torch.empty(4 * n, dtype=torch.uint8, device=dev)
        dist = torch.empty(n, dtype=torch.float64, device=dev)
        plo = C.byref(_native.Imaginary(*lo))
        ratio = {}
        for road, precision in (("F64", 0), ("PT", 3)):
            p_lo = plo if precision == 3 else None
            plain, pk = kernel_ms(lib, lambda: lib.fr_escape_rows_device(C.byref(cfg), precision, p_lo, 0, cfg.height, 2, z.data_ptr(),
                                                                         it.data_ptr(), s, None), args.reps)
            de, dk = kernel_ms(lib, lambda: lib.fr_escape_rows_de_device(C.byref(cfg), precision, p_lo, 0, cfg.height, z.data_ptr(),
                                                                         it.data_ptr(), der.data_ptr(), s), args.reps)
            stream.synchronize()
            iters = it.cpu().numpy().view(np.uint32).astype(np.uint64)
            total = int(np.where(iters < cfg.iterations, iters + 1, cfg.iterations).sum())
            mp, md = statistics.median(plain), statistics.median(de)
            ratio[road] = md / mp
            lines.append(json.dumps({"view": vname, "road": road, "width": cfg.width, "height": cfg.height, "iterations": cfg.iterations,
                                     "pixel_iterations": total, "plain_kernel": pk, "plain_ms_median": round(mp, 4),
                                     "plain_ms_all": [round(t, 4) for t in plain], "de_kernel": dk, "de_ms_median": round(md, 4),
                                     "de_ms_all": [round(t, 4) for t in de], "de_over_plain": round(md / mp, 3),
                                     "plain_ns_per_pixel_iteration": float("%.4g" % (mp * 1e6 / total)),
                                     "de_ns_per_pixel_iteration": float("%.4g" % (md * 1e6 / total))}))
        # the recolours over the arrays the PT DE render left
        plain_ms = stream_ms(stream, lambda: lib.fr_colour_rows_device(C.byref(cfg), z.data_ptr(), 2, it.data_ptr(), n, 4, rgba.data_ptr(),
                                                                        4 * n, s))
        shade_ms = stream_ms(stream, lambda: lib.fr_colour_de_rows_device(C.byref(cfg), z.data_ptr(), it.data_ptr(), der.data_ptr(), n, 2.0, 4,
                                                                          rgba.data_ptr(), s))
        dist_ms = stream_ms(stream, lambda: lib.fr_distance_rows_device(C.byref(cfg), z.data_ptr(), it.data_ptr(), der.data_ptr(), n,
                                                                        dist.data_ptr(), s))
        lines.append(json.dumps({"view": vname, "recolour_rgba_ms": round(plain_ms, 4), "shaded_recolour_rgba_ms": round(shade_ms, 4),
                                 "distance_rows_ms": round(dist_ms, 4)}))
        lines.append("# %s: DE / plain kernel time F64 %.2f, PT %.2f; shaded / plain recolour %.2f" % (vname, ratio["F64"], ratio["PT"],
                                                                                                     shade_ms / plain_ms))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
