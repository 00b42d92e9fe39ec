"""Views, cap chain and pixel classes shared by tests/test_extend_cpu.py and tests/test_gpu_extend.py (raising the iteration
cap of stored results: include/fractal_hip.h, fr_escape_extend_device).  Everything here comes from the CPU oracle; a
reference is computed once per (view, precision, cap, limit) and handed out read-only."""
import functools

import numpy as np

import oracle_lib as O

F64, F32, DD, PT = 0, 1, 2, 3
W, H = 67, 45  # odd, no multiple of 8: edge tiles in both directions
CHAIN = [0, 1, 5, 37, 38, 200, 333]


def view_cfg(name, iterations, width=W, height=H, limit=None):
    """(a) "mandelbrot": the default CLI Mandelbrot view; (b) "julia": Julia with c = -0.8 + 0.156i"""
    if name == "mandelbrot":
        cfg = O.cli_config(width, height)
    else:
        cfg = O.cli_config(width, height, algo=O.JULIA, julia_set=(-0.8, 0.156))
    cfg.iterations = iterations
    if limit is not None:
        cfg.limit = limit
    return cfg


@functools.lru_cache(maxsize=None)
def reference(name, precision, iterations, width=W, height=H, limit=None):
    """oracle.escape_rows of the whole view at one cap: (z float64 [h, w, 2], iters uint32 [h, w]), read-only"""
    z, it = O.escape_rows(view_cfg(name, iterations, width, height, limit), precision)
    z.flags.writeable = False
    it.flags.writeable = False
    return z, it


def classes(it_n, it_m, n, m):
    """The pixel classes of the link n -> m from the results at both caps: (finished before, escapes within, still running
    after, escapes on the first resumed step, escapes on the last step m - 1)."""
    running = it_n == n
    return (int((~running).sum()), int((running & (it_m < m)).sum()), int((it_m == m).sum()),
            int((running & (it_m == n)).sum()), int((running & (it_m == m - 1) & (it_m < m)).sum()))


# (finished before, escapes within, still running after, first step, last step), as stated with the feature and recomputed by
# tests/test_extend_cpu.py.  The Mandelbrot rows hold for F64 and F32; the Julia rows are F64's, and F32 parts from them by 2
# pixels in the 38 -> 200 link (TABLE_F32 holds what the oracle gives from there on).
TABLE = {
    ("mandelbrot", 1, 5): (0, 1094, 1921, 0, 997),
    ("mandelbrot", 5, 37): (1094, 1395, 526, 577, 0),
    ("mandelbrot", 37, 38): (2489, 2, 524, 2, 2),
    ("mandelbrot", 38, 200): (2491, 24, 500, 0, 0),
    ("mandelbrot", 200, 333): (2515, 4, 496, 0, 0),
    ("julia", 5, 37): (1079, 1500, 436, 638, 10),
    ("julia", 38, 200): (2589, 286, 140, 12, 2),
    ("julia", 200, 333): (2875, 78, 62, 0, 0),
}
TABLE_F32 = dict(TABLE)
TABLE_F32[("julia", 38, 200)] = (2589, 288, 138, 12, 2)
TABLE_F32[("julia", 200, 333)] = (2877, 80, 58, 0, 0)


def table(precision):
    return TABLE_F32 if precision == F32 else TABLE


def same_f64(a, b):
    """Bit-identical, zero signs included; any NaN matches any NaN (the platform picks the payload)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(
        a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])
