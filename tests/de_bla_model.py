"""ctypes front of tests/de_bla_model.c, the host restatement of DE ON BLA-PT (include/fractal_hip.h, "DE ON BLA-PT").

The model builds nothing of its own: the orbits come from the PT models (tests/bla_model.py's View holds them) and the tables
from tests/bla_model.c (blam_build_table); the distance is tests/de_model.py's.  The C file is compiled on first use into a
fresh temporary directory: gcc -O2 -ffp-contract=off -fno-fast-math -shared."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import bla_model as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "de_bla_model.c")
DEFAULT_BITS = B.DEFAULT_BITS

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler for tests/de_bla_model.c")
    d = tempfile.mkdtemp(prefix="de_bla_model_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libde_bla_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", so, SRC, "-lm"],
                   check=True)
    L = C.CDLL(so)
    v, u32 = C.c_void_p, C.c_uint32
    L.debm_rows.restype = None
    L.debm_rows.argtypes = [C.POINTER(B._View), C.c_int, v, u32, v, v, u32, v, u32, v, v, u32, u32, u32, v, v, v, v, v]
    _lib = L
    return L


def _flat_table(cfg, orbit, bits):
    """tests/bla_model.c's table of `orbit` as it lays it out: (float64 [entries + 1, 5], uint32 [33] entries per level, levels)"""
    last = len(orbit) - 1
    v = B._view(cfg)
    L = B.lib()
    out = np.zeros((int(L.blam_table_entries(last)) + 1, 5), dtype=np.float64)
    n = np.zeros(33, dtype=np.uint32)
    levels = L.blam_build_table(orbit.ctypes.data, last, L.blam_D(C.byref(v)), 0.0 if cfg.algo == 2 else 1.0, bits, out.ctypes.data,
                                n.ctypes.data)
    return out, n, int(levels)


def escape_rows(cfg, x_orbit=None, k_orbit=None, bits=DEFAULT_BITS, y0=0, y1=None):
    """DE ON BLA-PT over rows [y0, y1) on the given orbits (k_orbit: Julia's K; Mandelbrot: None; an algorithm without orbits
    takes none) -> (z float64 [rows, width, 2], iters uint32 [rows, width], der float64 [rows, width, 2], passes uint32 [rows,
    width], skips uint32 [rows, width])"""
    y1 = cfg.height if y1 is None else y1
    shape = (y1 - y0, cfg.width)
    z = np.empty(shape + (2,), dtype=np.float64)
    der = np.empty(shape + (2,), dtype=np.float64)
    it = np.empty(shape, dtype=np.uint32)
    passes = np.empty(shape, dtype=np.uint32)
    skips = np.empty(shape, dtype=np.uint32)
    v = B._view(cfg)
    if cfg.algo not in (0, 2):
        lib().debm_rows(C.byref(v), 0, None, 0, None, None, 0, None, 0, None, None, 0, y0, y1, z.ctypes.data, it.ctypes.data,
                        der.ctypes.data, passes.ctypes.data, skips.ctypes.data)
        return z, it, der, passes, skips
    x = B._orbit(x_orbit)
    k = x if k_orbit is None else B._orbit(k_orbit)
    assert (cfg.algo == 2) == (k is not x)
    xt, xn, xl = _flat_table(cfg, x, bits)
    kt, kn, kl = (xt, xn, xl) if k is x else _flat_table(cfg, k, bits)
    lib().debm_rows(C.byref(v), 1, x.ctypes.data, len(x) - 1, xt.ctypes.data, xn.ctypes.data, xl, k.ctypes.data, len(k) - 1,
                    kt.ctypes.data, kn.ctypes.data, kl, y0, y1, z.ctypes.data, it.ctypes.data, der.ctypes.data, passes.ctypes.data,
                    skips.ctypes.data)
    return z, it, der, passes, skips


_models = {}


def model(view, bits=DEFAULT_BITS):
    """(z, iters, der, passes, skips) of the model over the whole image of a tests/bla_model.py View, computed once"""
    key = (id(view), bits)
    if key not in _models:
        r = escape_rows(view.cfg, view.x, view.k, bits)
        for a in r:
            a.setflags(write=False)
        _models[key] = (view, r)  # the view is kept: its id stays its own
    return _models[key][1]
