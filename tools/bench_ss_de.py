#!/usr/bin/env python3
"""SUPERSAMPLED DE on one MI355X (include/fractal_hip.h, "SUPERSAMPLED DE"), timed with HIP events on a stream
of its own.  The default view at 1920 x 1080 output pixels, thickness 1.5, s in {2, 4, 8}:

  recolour   over the kept DE arrays of cfg_s in device memory (36 bytes per sample), RGBA and RGB:
     fused        fr_colour_de_rows_ss_device (colour_de_filter_kernel<s>), with the bytes/s it achieves counted at 36 B per
                  sample read plus the output written;
     composition  fr_colour_de_rows_device into an RGB image of cfg_s + fr_box_filter_rgb8_device: the calls the library had
                  before, the yardstick; not run at s = 8, where the arrays alone are 4.8 GB and the RGB image another 0.4;
     the two are compared byte for byte after the timing.
  render     fr_render_rows_ss_de_device with best_bytes against fr_render_rows_ss_device of the same view (s in {2, 4}): what
             the derivative and the 12 times wider band cost.

One JSON line per (case, variant): median, minimum and maximum of --reps runs after one warm-up round, the variants alternating.
No pass/fail: the figures are for DESIGN.md."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH, HEIGHT, CAP, THICKNESS = 1920, 1080, 1024, 1.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--factors", default="2,4,8")
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    args = ap.parse_args()

    import torch  # first: the library binds to the HIP runtime torch carries

    import fractal_renderer_amd as fr
    from fractal_renderer_amd import _native

    fr.init(0)
    lib = _native.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def run(variants):
        times = {n: [] for n, _ in variants}
        for r in range(args.reps + 1):
            for n, fn in variants:
                ms = timed(fn)
                if r:
                    times[n].append(ms)
        return times

    def report(case, times, extra):
        for n, ts in times.items():
            rec = {"case": case, "variant": n, "ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
                   "ms_max": round(max(ts), 4), "runs": len(ts)}
            rec.update(extra.get(n, {}))
            emit(rec)

    try:
        clock = {"sclk_mhz": torch.cuda.clock_rate()}
    except Exception:  # an older torch, or no management library: the figures stand without it
        clock = {}
    emit({"device": fr.device_name(), "build": fr.build_id(), **clock})

    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = WIDTH, HEIGHT, CAP
    for s in (int(f) for f in args.factors.split(",")):
        cfg_s = cfg.clone()
        cfg_s.width, cfg_s.height = s * WIDTH, s * HEIGHT
        n = cfg_s.width * cfg_s.height
        z = torch.empty(2 * n, dtype=torch.float64, device=dev)
        der = torch.empty(2 * n, dtype=torch.float64, device=dev)
        it = torch.empty(n, dtype=torch.int32, device=dev)
        _native.check(lib.fr_escape_rows_de_device(C.byref(cfg_s), 0, None, 0, cfg_s.height, z.data_ptr(), it.data_ptr(), der.data_ptr(), st))
        stream.synchronize()
        scratch = torch.empty(3 * n, dtype=torch.uint8, device=dev) if s < 8 else None
        for channels in (4, 3):
            got = torch.empty(channels * WIDTH * HEIGHT, dtype=torch.uint8, device=dev)
            want = torch.empty_like(got)

            def fused():
                _native.check(lib.fr_colour_de_rows_ss_device(C.byref(cfg), z.data_ptr(), it.data_ptr(), der.data_ptr(), WIDTH, HEIGHT, s,
                                                              THICKNESS, channels, got.data_ptr(), got.numel(), st))

            def composition():
                _native.check(lib.fr_colour_de_rows_device(C.byref(cfg_s), z.data_ptr(), it.data_ptr(), der.data_ptr(), n, THICKNESS * s, 3,
                                                           scratch.data_ptr(), st))
                _native.check(lib.fr_box_filter_rgb8_device(scratch.data_ptr(), WIDTH, HEIGHT, s, channels, want.data_ptr(), want.numel(), st))

            times = run([("fused", fused)] + ([("composition", composition)] if scratch is not None else []))
            stream.synchronize()
            if scratch is not None:
                assert torch.equal(got, want), "the fused recolour and the composition differ"
            moved = 36 * n + got.numel()
            report("recolour_1080p_s%d_%s" % (s, "rgba" if channels == 4 else "rgb"), times,
                   {"fused": {"bytes": moved, "gb_per_s": round(moved / statistics.median(times["fused"]) / 1e6, 1)},
                    "composition": {"scratch_bytes": 3 * n}})
        del z, der, it, scratch
        if s == 8:
            continue
        _, best = fr.ss_workspace_bytes(cfg, s)
        _, best_de = fr.ss_de_workspace_bytes(cfg, s)
        work = torch.empty(max(best, best_de), dtype=torch.uint8, device=dev)
        out = torch.empty(3 * WIDTH * HEIGHT, dtype=torch.uint8, device=dev)

        def ss_de():
            _native.check(lib.fr_render_rows_ss_de_device(C.byref(cfg), 0, None, None, 0, 0, THICKNESS, s, 0, HEIGHT, 3, out.data_ptr(),
                                                          out.numel(), work.data_ptr(), best_de, st))

        def ss():
            _native.check(lib.fr_render_rows_ss_device(C.byref(cfg), 0, None, s, 0, HEIGHT, 3, out.data_ptr(), out.numel(), work.data_ptr(),
                                                       best, st, None))

        report("render_1080p_s%d" % s, run([("ss_de", ss_de), ("ss", ss)]), {"ss_de": {"work_bytes": best_de}, "ss": {"work_bytes": best}})
        del work, out
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
