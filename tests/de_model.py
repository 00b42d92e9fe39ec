"""ctypes front of tests/de_model.c, the host restatement of DE (include/fractal_hip.h, fr_precision: "DE"), plus the views of
the DE tests.

The C file is compiled on first use into a fresh temporary directory (never into the tree):
gcc -O2 -ffp-contract=off -fno-fast-math -shared, with oracle/ on the include path for the software log2.

Reference orbits are not restated here: a dd centre's come from tests/pt_model.py, a wide centre's from
tests/pt_wide_model.py (Python integers); dem_pt_rows runs PT's step sequence over whichever it is given.  The unshaded colour
bytes are the oracle's colour map in its software-log2 mode; dem_shade applies the definition's shading to them."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import oracle_lib as O
import pt_model as PTM

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "de_model.c")
ORACLE = os.path.join(os.path.dirname(HERE), "oracle")
THREADS = max(1, min(16, os.cpu_count() or 1))  # for the oracle's colour map, whose own default is a thread per processor

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler for tests/de_model.c")
    d = tempfile.mkdtemp(prefix="de_model_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libde_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-I", ORACLE, "-o", so, SRC,
                    "-lm"], check=True)
    L = C.CDLL(so)
    v, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    L.dem_config_size.restype = C.c_int
    L.dem_f64_rows.restype = None
    L.dem_f64_rows.argtypes = [v, u32, u32, v, v, v]
    L.dem_pt_rows.restype = None
    L.dem_pt_rows.argtypes = [v, v, u32, v, u32, u32, u32, v, v, v]
    L.dem_distance.restype = None
    L.dem_distance.argtypes = [v, v, v, v, sz, v]
    L.dem_shade.restype = None
    L.dem_shade.argtypes = [v, v, v, v, sz, C.c_double, v, C.c_int, v]
    assert L.dem_config_size() == 104
    _lib = L
    return L


def _cfg_ptr(cfg):
    assert C.sizeof(cfg) == 104, "an fr_config image is 104 bytes"
    return C.addressof(cfg)


def _empty(cfg, y0, y1):
    shape = (y1 - y0, cfg.width)
    return np.empty(shape + (2,), dtype=np.float64), np.empty(shape, dtype=np.uint32), np.empty(shape + (2,), dtype=np.float64)


def f64_rows(cfg, y0=0, y1=None):
    """the F64 road: (z float64 [rows, width, 2], iters uint32 [rows, width], der float64 [rows, width, 2])"""
    y1 = cfg.height if y1 is None else y1
    z, it, der = _empty(cfg, y0, y1)
    lib().dem_f64_rows(_cfg_ptr(cfg), y0, y1, z.ctypes.data, it.ctypes.data, der.ctypes.data)
    return z, it, der


def pt_rows_on(cfg, x_orbit, k_orbit, y0=0, y1=None):
    """PT over the orbits given as float64 [entries, 2] arrays (k_orbit None: Mandelbrot, the pixel rebases onto x_orbit)"""
    y1 = cfg.height if y1 is None else y1
    x = np.ascontiguousarray(x_orbit, dtype=np.float64)
    k = x if k_orbit is None else np.ascontiguousarray(k_orbit, dtype=np.float64)
    z, it, der = _empty(cfg, y0, y1)
    lib().dem_pt_rows(_cfg_ptr(cfg), x.ctypes.data, len(x) - 1, k.ctypes.data, len(k) - 1, y0, y1, z.ctypes.data, it.ctypes.data,
                      der.ctypes.data)
    return z, it, der


def pt_rows(cfg, pos_lo=(0.0, 0.0), y0=0, y1=None):
    """PT with the dd centre (cfg.pos, pos_lo): the orbits of tests/pt_model.c"""
    if cfg.algo not in (0, 2):
        return pt_rows_on(cfg, np.zeros((2, 2)), None, y0, y1)
    x = PTM.reference_orbit(cfg, pos_lo, 0)
    k = PTM.reference_orbit(cfg, pos_lo, 1) if cfg.algo == 2 else None
    return pt_rows_on(cfg, x, k, y0, y1)


def pt_wide_rows(cfg, orbits, y0=0, y1=None):
    """PT with a wide centre: `orbits` is a pt_wide_model.Orbits of (cfg, centre)"""
    return pt_rows_on(cfg, orbits.x[0], orbits.k[0] if orbits.julia else None, y0, y1)


def _stored(z, it, der):
    z = np.ascontiguousarray(z, dtype=np.float64)
    it = np.ascontiguousarray(it, dtype=np.uint32)
    der = np.ascontiguousarray(der, dtype=np.float64)
    assert z.shape == it.shape + (2,) and der.shape == z.shape
    return z, it, der


def distance(cfg, z, it, der):
    """D in pixels, float64 [...]"""
    z, it, der = _stored(z, it, der)
    out = np.empty(it.shape, dtype=np.float64)
    lib().dem_distance(_cfg_ptr(cfg), z.ctypes.data, it.ctypes.data, der.ctypes.data, it.size, out.ctypes.data)
    return out


def base_colours(cfg, z, it):
    """the reference's colour map over stored results, uint8 [..., 3], with the software log2 the library uses"""
    ocfg = O.Config.from_buffer_copy(bytes(cfg))
    mode = O.lib().fro_get_log2_mode()
    O.set_log2_mode(O.LOG2_SOFT)
    try:
        return O.colour_rows(ocfg, z, it, THREADS)
    finally:
        O.set_log2_mode(mode)


def colour(cfg, z, it, der, thickness, channels=3):
    """the shaded image, uint8 [..., channels]"""
    z, it, der = _stored(z, it, der)
    base = np.ascontiguousarray(base_colours(cfg, z, it))
    out = np.empty(it.shape + (channels,), dtype=np.uint8)
    lib().dem_shade(_cfg_ptr(cfg), z.ctypes.data, it.ctypes.data, der.ctypes.data, it.size, float(thickness), base.ctypes.data,
                    channels, out.ctypes.data)
    return out


def same_doubles(a, b):
    """equal as bits, except that a NaN equals any NaN (the definition leaves a NaN's sign and payload open)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


# ---- the views of the tests ----------------------------------------------------------------------------------------------


def default_view(cfg, width=48, height=32, iterations=200):
    """Config::new's Mandelbrot view (pos 0, scale 0.4, limit 2^16) at a small size"""
    cfg.width, cfg.height, cfg.iterations = width, height, iterations
    return cfg


def julia_view(cfg, width=40, height=24, iterations=300):
    """the Julia set of c = -0.8 + 0.156i, whole, on the F64 road"""
    cfg.algo = 2
    cfg.width, cfg.height, cfg.iterations = width, height, iterations
    cfg.julia_set.re, cfg.julia_set.im = -0.8, 0.156
    cfg.pos.re = cfg.pos.im = 0.0
    cfg.scale.re = cfg.scale.im = 0.3
    return cfg


def unit_circle_view(cfg, width=48, height=32):
    """Julia with c = 0: the set is the unit circle, and |z_n| = |z_0|^(2^n) exactly in the reals"""
    cfg.algo = 2
    cfg.width, cfg.height, cfg.iterations = width, height, 16
    cfg.julia_set.re = cfg.julia_set.im = 0.0
    cfg.pos.re = cfg.pos.im = 0.0
    cfg.scale.re = cfg.scale.im = 0.25
    cfg.limit = 65536.0
    return cfg


def seahorse_shallow(cfg, width=40, height=24, iterations=3000, scale=1e11):
    """Seahorse valley (tests/pt_model.py's centre) at a scale the F64 road still resolves, where most pixels need more than a
    thousand iterations: the derivative of a capped exterior pixel passes 2^1024.  Returns pos_lo."""
    pos_lo = PTM.seahorse_view(cfg, width, height, iterations, scale)
    return pos_lo
