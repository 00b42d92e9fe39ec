"""ctypes front of tests/de_scaled_model.c, the host restatement of DE ON SCALED PT (include/fractal_hip.h, "DE ON SCALED PT").

The model builds nothing of its own: the orbits come from tests/pt_wide_model.py (tests/pt_scaled_model.py's View holds them) and
the tables from tests/pt_scaled_model.c (ptsm_build_table); the distance is tests/de_model.py's, taken on the scaled view.  The C
file is compiled on first use into a fresh temporary directory: gcc -O2 -ffp-contract=off -fno-fast-math -shared."""
import atexit
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

import pt_scaled_model as S

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "de_scaled_model.c")
NO_TABLE = S.NO_TABLE

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler for tests/de_scaled_model.c")
    d = tempfile.mkdtemp(prefix="de_scaled_model_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libde_scaled_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", so, SRC, "-lm"],
                   check=True)
    L = C.CDLL(so)
    v, u32 = C.c_void_p, C.c_uint32
    L.desm_rows.restype = C.c_int
    L.desm_rows.argtypes = [C.POINTER(S._View), C.c_int, v, u32, v, v, u32, v, u32, v, v, u32, u32, u32, v, v, v, v, v, v]
    _lib = L
    return L


def _flat_table(cfg, orbit, bits):
    """tests/pt_scaled_model.c's table of `orbit` as it lays it out: (float64 [entries + 1, 5], uint32 [33] entries per level,
    levels); bits = -1: no table"""
    n = np.zeros(33, dtype=np.uint32)
    if bits < 0:
        return np.zeros((1, 5), dtype=np.float64), n, 0
    last = len(orbit) - 1
    v = S._view(cfg)
    L = S.lib()
    out = np.zeros((int(L.ptsm_table_entries(last)) + 1, 5), dtype=np.float64)
    levels = L.ptsm_build_table(C.byref(v), orbit.ctypes.data, last, bits, out.ctypes.data, n.ctypes.data)
    return out, n, int(levels)


def escape_rows(cfg, x_orbit=None, k_orbit=None, bits=NO_TABLE, y0=0, y1=None):
    """DE ON SCALED PT over rows [y0, y1) on the given orbits (k_orbit: Julia's K; Mandelbrot: None; an algorithm without orbits
    takes none); bits = -1: the plain scaled loop -> (z float64 [rows, width, 2], iters uint32 [rows, width], der float64 [rows,
    width, 2] holding u, passes uint32 [rows, width], skips uint32 [rows, width], (lo, hi, sub): the smallest and largest nonzero
    finite magnitude in the u chain and whether any was subnormal)"""
    y1 = cfg.height if y1 is None else y1
    shape = (y1 - y0, cfg.width)
    z = np.empty(shape + (2,), dtype=np.float64)
    der = np.empty(shape + (2,), dtype=np.float64)
    it = np.empty(shape, dtype=np.uint32)
    passes = np.empty(shape, dtype=np.uint32)
    skips = np.empty(shape, dtype=np.uint32)
    rng = np.zeros(2, dtype=np.float64)
    v = S._view(cfg)
    if cfg.algo not in (0, 2):
        lib().desm_rows(C.byref(v), 0, None, 0, None, None, 0, None, 0, None, None, 0, y0, y1, z.ctypes.data, it.ctypes.data,
                        der.ctypes.data, passes.ctypes.data, skips.ctypes.data, rng.ctypes.data)
        return z, it, der, passes, skips, (math.inf, 0.0, False)
    x = S._orbit(x_orbit)
    k = x if k_orbit is None else S._orbit(k_orbit)
    assert (cfg.algo == 2) == (k is not x)
    xt, xn, xl = _flat_table(cfg, x, bits)
    kt, kn, kl = (xt, xn, xl) if k is x else _flat_table(cfg, k, bits)
    sub = lib().desm_rows(C.byref(v), 1, x.ctypes.data, len(x) - 1, xt.ctypes.data, xn.ctypes.data, xl, k.ctypes.data, len(k) - 1,
                          kt.ctypes.data, kn.ctypes.data, kl, y0, y1, z.ctypes.data, it.ctypes.data, der.ctypes.data,
                          passes.ctypes.data, skips.ctypes.data, rng.ctypes.data)
    assert sub >= 0, "de_scaled_model: a step went past the end of an orbit"
    return z, it, der, passes, skips, (float(rng[0]), float(rng[1]), bool(sub))


_models = {}


def model(view, bits=NO_TABLE):
    """(z, iters, der, passes, skips, (lo, hi, sub)) of the model over the whole image of a tests/pt_scaled_model.py View (or
    anything with cfg, x and k), computed once"""
    key = (id(view), bits)
    if key not in _models:
        r = escape_rows(view.cfg, view.x, view.k, bits)
        for a in r[:5]:
            a.setflags(write=False)
        _models[key] = (view, r)  # the view is kept: its id stays its own
    return _models[key][1]


def scaled_view(cfg):
    """cfg_v of the definition: a copy of cfg with scale = (sre, sim) = scale 2^-e, both exact"""
    e = S.exponent(cfg)
    view = type(cfg).from_buffer_copy(bytes(cfg))
    view.scale.re, view.scale.im = math.ldexp(cfg.scale.re, -e), math.ldexp(cfg.scale.im, -e)
    return view
