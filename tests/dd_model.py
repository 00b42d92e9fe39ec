"""ctypes front of tests/dd_model.c, the host restatement of FR_PRECISION_DD (include/fractal_hip.h, fr_precision),
plus the two deep reference views of the DD tests.

The C file is compiled on first use into a fresh temporary directory (never into the tree):
gcc -O2 -ffp-contract=off -fno-fast-math -fopenmp -shared.  At most 16 OpenMP threads."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "dd_model.c")
THREADS = max(1, min(16, os.cpu_count() or 1))

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is not None:
        return _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler for tests/dd_model.c")
    _dir = tempfile.mkdtemp(prefix="dd_model_")
    atexit.register(shutil.rmtree, _dir, True)
    so = os.path.join(_dir, "libdd_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-o", so,
                    SRC, "-lm"], check=True)
    L = C.CDLL(so)
    L.ddm_escape_rows.restype = None
    L.ddm_escape_rows.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int]
    L.ddm_start.restype = None
    L.ddm_start.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_void_p]
    L.ddm_pixel.restype = C.c_uint32
    L.ddm_pixel.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_void_p]
    L.ddm_count_iterations.restype = C.c_uint64
    L.ddm_count_iterations.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    _lib = L
    return L


def _cfg_ptr(cfg):
    assert C.sizeof(cfg) == 104, "an fr_config image is 104 bytes"
    return C.addressof(cfg)


def escape_rows(cfg, pos_lo=(0.0, 0.0), y0=0, y1=None):
    """(z float64 [rows, width, 4] = re.hi, re.lo, im.hi, im.lo; iters uint32 [rows, width])"""
    y1 = cfg.height if y1 is None else y1
    z = np.empty((y1 - y0, cfg.width, 4), dtype=np.float64)
    it = np.empty((y1 - y0, cfg.width), dtype=np.uint32)
    lib().ddm_escape_rows(_cfg_ptr(cfg), float(pos_lo[0]), float(pos_lo[1]), y0, y1, z.ctypes.data, it.ctypes.data, THREADS)
    return z, it


def start(cfg, x, y, pos_lo=(0.0, 0.0)):
    out = np.empty(4, dtype=np.float64)
    lib().ddm_start(_cfg_ptr(cfg), float(pos_lo[0]), float(pos_lo[1]), x, y, out.ctypes.data)
    return out


def pixel(cfg, x, y, pos_lo=(0.0, 0.0)):
    """one pixel at any u32 (x, y), inside the image or not: (z float64 [4] = re.hi, re.lo, im.hi, im.lo, index)"""
    z = np.empty(4, dtype=np.float64)
    it = lib().ddm_pixel(_cfg_ptr(cfg), float(pos_lo[0]), float(pos_lo[1]), x, y, z.ctypes.data)
    return z, int(it)


def count_iterations(cfg, y0=0, y1=None):
    y1 = cfg.height if y1 is None else y1
    return int(lib().ddm_count_iterations(_cfg_ptr(cfg), y0, y1, THREADS))


def deep_view(cfg, julia, width=64, height=48, iterations=3000):
    """The deep reference views on `cfg` (a Config of either binding, filled in place): centre (0, 1) — the Misiurewicz
    point c = i (Mandelbrot) or a point of the Julia set of c = i (Julia) — at scale 10^18 on both axes."""
    cfg.algo = 2 if julia else 0
    cfg.width, cfg.height, cfg.iterations = width, height, iterations
    cfg.limit = 65536.0
    cfg.pos.re, cfg.pos.im = 0.0, 1.0
    cfg.scale.re = cfg.scale.im = 1e18
    cfg.julia_set.re, cfg.julia_set.im = 0.0, 1.0
    return cfg
