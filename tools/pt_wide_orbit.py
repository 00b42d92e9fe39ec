"""What WIDE PT's reference orbit costs on the host, and what a deep view then costs on the device.

Host, one thread, no device needed: fr_debug_reference_orbit_wide on the period-3 nucleus (the real root of c^3 + 2c^2 + c + 1,
whose orbit never escapes: cut by the cap) with iterations = 10^5 - 2, i.e. 10^5 entries, at n = 2, 4, 8 and 16 words; beside
it fr_debug_reference_orbit, the dd orbit of the same centre split into pos + pos_lo (profiles/pt_throughput.txt has 0.2 -
0.33 ms per 10^4 entries for it).  Median of --reps calls each, all in one process, alternating.
Device (skipped with --host-only or without one): the Misiurewicz view (root of c^3 + 2c^2 + 2c + 2 near -0.228 + 1.115i,
scale 2^200, n = 5, cap 3000, limit 2) at 1920 x 1080 through escape_pt_kernel: the first call's host time (orbit + upload)
and the kernel time of the following renders (device events, median).

    python3 tools/pt_wide_orbit.py [--reps 5] [--host-only] [--out profiles/pt_wide_orbit.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

try:
    import torch  # noqa: F401  (first: the library binds to the HIP runtime torch carries)
except ImportError:
    torch = None

import numpy as np  # noqa: E402

import fractal_renderer_amd as fr  # noqa: E402
from fractal_renderer_amd import _native  # noqa: E402

BITS = 1100
ENTRIES = 100000


def _trunc(x):
    return Fraction(int(x * (1 << BITS)), 1 << BITS)


def newton(coeffs, re, im):
    """a root of the real polynomial `coeffs` (highest power first) near re + i im, to ~BITS bits, as two Fractions"""
    re, im = Fraction(re), Fraction(im)
    for _ in range(10):  # quadratic from 8 digits: 27, 54, ... bits
        fr_, fi, dr, di = Fraction(0), Fraction(0), Fraction(0), Fraction(0)
        for c in coeffs:  # Horner on f and f'
            dr, di = dr * re - di * im + fr_, dr * im + di * re + fi
            fr_, fi = fr_ * re - fi * im + c, fr_ * im + fi * re
        den = dr * dr + di * di
        re, im = _trunc(re - (fr_ * dr + fi * di) / den), _trunc(im - (fi * dr - fr_ * di) / den)
    return re, im


def wide_centre(re, im, n):
    f = 64 * n - 8
    c = fr.WideCentre(n)
    for v, w in ((re, c.re), (im, c.im)):
        i = (v.numerator << f) // v.denominator  # floor
        for k in range(n):
            w[k] = (i >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    args = ap.parse_args()
    lib = _native.load()
    lines = ["# tools/pt_wide_orbit.py, build %s: host reference orbits, one thread, %d entries cut by the cap, median of %d calls"
             % (fr.build_id(), ENTRIES, args.reps)]

    nucleus = newton([1, 2, 1, 1], -1.75487767, 0)
    cfg = fr.Config.new()
    cfg.iterations, cfg.limit = ENTRIES - 2, 2.0
    cfg.scale.re = cfg.scale.im = 1.0
    out = np.empty((ENTRIES, 2), dtype=np.float64)
    ln = C.c_uint32(0)
    hi, lo = fr.split_dd(nucleus[0])
    cfg.pos.re, cfg.pos.im = hi, 0.0
    pos_lo = _native.Imaginary(lo, 0.0)
    centres = {n: wide_centre(nucleus[0], nucleus[1], n) for n in (2, 4, 8, 16)}
    structs = {n: c.c_struct() for n, c in centres.items()}
    times = {k: [] for k in ["dd", 2, 4, 8, 16]}
    for rep in range(args.reps + 1):  # the first round warms up
        for key in times:
            t0 = time.perf_counter()
            if key == "dd":
                rc = lib.fr_debug_reference_orbit(C.byref(cfg), C.byref(pos_lo), 0, out.ctypes.data, len(out), C.byref(ln))
            else:
                rc = lib.fr_debug_reference_orbit_wide(C.byref(cfg), C.byref(structs[key]), 0, out.ctypes.data, len(out), C.byref(ln))
            dt = time.perf_counter() - t0
            _native.check(rc)
            assert ln.value == ENTRIES, (key, ln.value)
            if rep:
                times[key].append(dt)
    dd_us = statistics.median(times["dd"]) / ENTRIES * 1e6
    lines.append("# orbit            bits  us/entry  ms per 10^4 entries   x dd   all (ms per call)")
    for key in times:
        us = statistics.median(times[key]) / ENTRIES * 1e6
        lines.append("  %-15s %5s  %8.4f  %19.3f  %5.1f   %s" % (
            "dd (pos+pos_lo)" if key == "dd" else "wide n = %d" % key, "~106" if key == "dd" else 64 * key - 8, us, us * 10, us / dd_us,
            " ".join("%.2f" % (t * 1e3) for t in times[key])))

    if not args.host_only and torch is not None and fr.device_count() > 0:
        fr.init(0)
        mis = newton([1, 2, 2, 2], -0.22815549, 1.11514251)
        view = fr.Config.new()
        view.width, view.height, view.iterations, view.limit, view.exposure = 1920, 1080, 3000, 2.0, 5.0
        view.scale.re = view.scale.im = 2.0 ** 200
        centre = wide_centre(mis[0], mis[1], 5)
        st = centre.c_struct()
        npx = view.width * view.height
        buf = torch.empty(3 * npx, dtype=torch.uint8, device="cuda:0")
        _native.check(lib.fr_set_profiling(1))
        ms = C.c_float(0.0)
        name = C.create_string_buffer(128)
        first, kernel = None, []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _native.check(lib.fr_render_rows_pt_wide_device(C.byref(view), C.byref(st), 0, view.height, 3, buf.data_ptr(), 3 * npx, None))
            host = time.perf_counter() - t0
            _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
            if rep == 0:
                first = host
                cache = fr.pt_orbit_cache()
            else:
                kernel.append(ms.value)
        _native.check(lib.fr_last_kernel_name(name, len(name)))
        _native.check(lib.fr_set_profiling(0))
        z = np.empty((8, view.width, 2))
        it = np.empty((8, view.width), dtype=np.uint32)
        _native.check(lib.fr_escape_rows_pt_wide(C.byref(view), C.byref(st), 536, 544, z.ctypes.data, it.ctypes.data))
        colours = len(np.unique(buf.cpu().numpy().reshape(-1, 3), axis=0))
        lines.append("# Misiurewicz view, scale 2^200, n = 5, 1920 x 1080, cap 3000 on %s: orbit of %d entries (%d computed by the "
                     "first call)" % (fr.device_name(), cache[1], cache[3]))
        lines.append("  first call, host side (orbit, upload, launch): %.3f ms" % (first * 1e3))
        lines.append("  %s: median %.4f ms of %s; rows 536..543 escape at %d..%d, %d distinct colours in the image" % (
            name.value.decode(), statistics.median(kernel), " ".join("%.4f" % k for k in kernel), int(it.min()), int(it.max()), colours))
    else:
        lines.append("# no device (or --host-only): the 1080p render was not measured")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
