"""ctypes front of tests/pt_model.c, the host restatement of FR_PRECISION_PT (include/fractal_hip.h, fr_precision), plus
the views of the PT tests.

The C file is compiled on first use into a fresh temporary directory (never into the tree):
gcc -O2 -ffp-contract=off -fno-fast-math -fopenmp -shared.  At most 16 OpenMP threads."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pt_model.c")
THREADS = max(1, min(16, os.cpu_count() or 1))

# the seahorse-valley centre of the long-orbit view
SEAHORSE_RE = "-0.743643887037158704752191506114774"
SEAHORSE_IM = "0.131825904205311970493132056385139"

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is not None:
        return _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler for tests/pt_model.c")
    _dir = tempfile.mkdtemp(prefix="pt_model_")
    atexit.register(shutil.rmtree, _dir, True)
    so = os.path.join(_dir, "libpt_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-o", so,
                    SRC, "-lm"], check=True)
    L = C.CDLL(so)
    L.ptm_escape_rows.restype = C.c_int
    L.ptm_escape_rows.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int]
    L.ptm_pixel.restype = C.c_int
    L.ptm_pixel.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.ptm_count_iterations.restype = C.c_uint64
    L.ptm_count_iterations.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    L.ptm_orbit_capacity.restype = C.c_uint32
    L.ptm_orbit_capacity.argtypes = [C.c_void_p]
    L.ptm_reference_orbit.restype = C.c_uint32
    L.ptm_reference_orbit.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p]
    _lib = L
    return L


def _cfg_ptr(cfg):
    assert C.sizeof(cfg) == 104, "an fr_config image is 104 bytes"
    return C.addressof(cfg)


def escape_rows(cfg, pos_lo=(0.0, 0.0), y0=0, y1=None):
    """(z float64 [rows, width, 2] = re, im; iters uint32 [rows, width])"""
    y1 = cfg.height if y1 is None else y1
    z = np.empty((y1 - y0, cfg.width, 2), dtype=np.float64)
    it = np.empty((y1 - y0, cfg.width), dtype=np.uint32)
    ok = lib().ptm_escape_rows(_cfg_ptr(cfg), float(pos_lo[0]), float(pos_lo[1]), y0, y1, z.ctypes.data, it.ctypes.data,
                               THREADS)
    assert ok, "pt_model: out of memory"
    return z, it


def pixel(cfg, x, y, pos_lo=(0.0, 0.0)):
    """one pixel at any u32 (x, y), inside the image or not: (z float64 [2] = re, im, index)"""
    z = np.empty(2, dtype=np.float64)
    it = C.c_uint32(0)
    ok = lib().ptm_pixel(_cfg_ptr(cfg), float(pos_lo[0]), float(pos_lo[1]), x, y, z.ctypes.data, C.byref(it))
    assert ok, "pt_model: out of memory"
    return z, it.value


def count_iterations(cfg, y0=0, y1=None):
    y1 = cfg.height if y1 is None else y1
    return int(lib().ptm_count_iterations(_cfg_ptr(cfg), y0, y1, THREADS))


def reference_orbit(cfg, pos_lo=(0.0, 0.0), which=0):
    """float64 [entries, 2] = re, im of the stored hi parts"""
    out = np.empty((lib().ptm_orbit_capacity(_cfg_ptr(cfg)), 2), dtype=np.float64)
    n = lib().ptm_reference_orbit(_cfg_ptr(cfg), float(pos_lo[0]), float(pos_lo[1]), which, out.ctypes.data)
    return out[:n].copy()


def split(text):
    """decimal string -> (hi, lo): hi the nearest f64, lo the nearest f64 to the rest (split_dd without the package)"""
    f = Fraction(text)
    hi = float(f)
    return hi, float(f - Fraction(hi))


def seahorse_view(cfg, width=32, height=24, iterations=20000, scale=1e20):
    """The long-orbit view on `cfg` (filled in place): Mandelbrot at the seahorse-valley centre, split into pos + pos_lo,
    at `scale` on both axes.  Returns pos_lo."""
    (re, re_lo), (im, im_lo) = split(SEAHORSE_RE), split(SEAHORSE_IM)
    cfg.algo = 0
    cfg.width, cfg.height, cfg.iterations = width, height, iterations
    cfg.limit = 2.0
    cfg.pos.re, cfg.pos.im = re, im
    cfg.scale.re = cfg.scale.im = scale
    return (re_lo, im_lo)


def early_escape_view(cfg, width=48, height=32, iterations=2000):
    """A Mandelbrot view centred on c = 0.26, just right of the cusp: the reference orbit escapes after 30 steps, while
    most pixels, the ones inside the main cardioid, run to the cap: they rebase at the orbit's end again and again."""
    cfg.algo = 0
    cfg.width, cfg.height, cfg.iterations = width, height, iterations
    cfg.limit = 2.0
    cfg.pos.re, cfg.pos.im = 0.26, 0.0
    cfg.scale.re = cfg.scale.im = 40.0
    return (0.0, 0.0)


def julia_rebase_view(cfg, width=48, height=32, iterations=3000):
    """A Julia view of c = -0.8 + 0.156i centred on a point just outside the filled Julia set: the view orbit V ends after
    201 steps, and the pixels, which escape after 197 to several hundred iterations, go on on the critical orbit K."""
    cfg.algo = 2
    cfg.width, cfg.height, cfg.iterations = width, height, iterations
    cfg.limit = 2.0
    cfg.julia_set.re, cfg.julia_set.im = -0.8, 0.156
    cfg.pos.re, cfg.pos.im = -0.815300184283871, -0.1992250950480455
    cfg.scale.re = cfg.scale.im = 1e11
    return (0.0, 0.0)
