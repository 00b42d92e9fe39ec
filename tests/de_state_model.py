"""ctypes front of tests/de_state_model.c, the host restatement of RESUMABLE DE (include/fractal_hip.h, fr_precision:
"RESUMABLE DE"): the F64 continuation, the PT state run with the derivative, and its continuation.

The C file is compiled on first use into a fresh temporary directory (never into the tree):
gcc -O2 -ffp-contract=off -fno-fast-math -shared.

Reference orbits are not restated here: a dd centre's come from tests/pt_model.py, a wide centre's from tests/pt_wide_model.py;
the *_on functions run over whichever they are given, as tests/de_model.py's do.  A PT state is the tuple
(z float64 [rows, width, 2], iters uint32 [rows, width], dz float64 [rows, width, 2], m uint32 [rows, width], der float64
[rows, width, 2]); an F64 state is de_model's (z, iters, der)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import de_model as D
import pt_model as PTM

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "de_state_model.c")
ON_K = 0x80000000

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler for tests/de_state_model.c")
    d = tempfile.mkdtemp(prefix="de_state_model_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libde_state_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", so, SRC, "-lm"], check=True)
    L = C.CDLL(so)
    v, u32 = C.c_void_p, C.c_uint32
    L.desm_config_size.restype = C.c_int
    L.desm_f64_continue.restype = None
    L.desm_f64_continue.argtypes = [v, u32, u32, u32, v, v, v]
    L.desm_pt_rows.restype = None
    L.desm_pt_rows.argtypes = [v, v, u32, v, u32, u32, u32, u32, C.c_int, v, v, v, v, v, C.POINTER(C.c_uint64)]
    assert L.desm_config_size() == 104
    _lib = L
    return L


def _cfg_ptr(cfg):
    assert C.sizeof(cfg) == 104, "an fr_config image is 104 bytes"
    return C.addressof(cfg)


# ---- the F64 road ----------------------------------------------------------------------------------------------------------


def f64_continue(cfg, state, from_iterations, y0=0, y1=None):
    """(z, iters, der) at the cap from_iterations continued to cfg.iterations -> the new arrays (copies)"""
    y1 = cfg.height if y1 is None else y1
    z, it, der = (np.array(a, order="C") for a in state)
    assert z.dtype == np.float64 and der.dtype == np.float64 and it.dtype == np.uint32
    assert it.shape == (y1 - y0, cfg.width) and z.shape == it.shape + (2,) == der.shape
    lib().desm_f64_continue(_cfg_ptr(cfg), y0, y1, from_iterations, z.ctypes.data, it.ctypes.data, der.ctypes.data)
    return z, it, der


# ---- PT ----------------------------------------------------------------------------------------------------------------------


def _orbits(x_orbit, k_orbit):
    x = np.ascontiguousarray(x_orbit, dtype=np.float64)
    return x, (x if k_orbit is None else np.ascontiguousarray(k_orbit, dtype=np.float64))


def _run(cfg, x, k, y0, y1, from_iterations, fresh, st):
    z, it, dz, m, der = st
    viol = C.c_uint64(0)
    lib().desm_pt_rows(_cfg_ptr(cfg), x.ctypes.data, len(x) - 1, k.ctypes.data, len(k) - 1, y0, y1, from_iterations, int(fresh),
                       z.ctypes.data, it.ctypes.data, dz.ctypes.data, m.ctypes.data, der.ctypes.data, C.byref(viol))
    assert viol.value == 0, "a step began with m >= last of the orbit followed"
    return st


def pt_state_rows_on(cfg, x_orbit, k_orbit, y0=0, y1=None):
    """the state run over the orbits given as float64 [entries, 2] arrays (k_orbit None: Mandelbrot)"""
    y1 = cfg.height if y1 is None else y1
    x, k = _orbits(x_orbit, k_orbit)
    shape = (y1 - y0, cfg.width)
    st = (np.empty(shape + (2,), dtype=np.float64), np.empty(shape, dtype=np.uint32), np.empty(shape + (2,), dtype=np.float64),
          np.empty(shape, dtype=np.uint32), np.empty(shape + (2,), dtype=np.float64))
    return _run(cfg, x, k, y0, y1, 0, True, st)


def pt_continue_on(cfg, x_orbit, k_orbit, state, from_iterations, y0=0, y1=None):
    """`state` at the cap from_iterations continued to cfg.iterations on the orbits of cfg's cap -> the new state (copies)"""
    y1 = cfg.height if y1 is None else y1
    x, k = _orbits(x_orbit, k_orbit)
    st = tuple(np.array(a, order="C") for a in state)
    assert [a.dtype for a in st] == [np.float64, np.uint32, np.float64, np.uint32, np.float64]
    assert st[1].shape == (y1 - y0, cfg.width) == st[3].shape and st[0].shape == st[1].shape + (2,) == st[2].shape == st[4].shape
    return _run(cfg, x, k, y0, y1, from_iterations, False, st)


def _dd_orbits(cfg, pos_lo):
    if cfg.algo not in (0, 2):
        return np.zeros((2, 2)), None
    return PTM.reference_orbit(cfg, pos_lo, 0), (PTM.reference_orbit(cfg, pos_lo, 1) if cfg.algo == 2 else None)


def pt_state_rows(cfg, pos_lo=(0.0, 0.0), y0=0, y1=None):
    """PT with the dd centre (cfg.pos, pos_lo): the orbits of tests/pt_model.c"""
    return pt_state_rows_on(cfg, *_dd_orbits(cfg, pos_lo), y0, y1)


def pt_continue(cfg, state, from_iterations, pos_lo=(0.0, 0.0), y0=0, y1=None):
    return pt_continue_on(cfg, *_dd_orbits(cfg, pos_lo), state, from_iterations, y0, y1)


def pt_wide_state_rows(cfg, orbits, y0=0, y1=None):
    """PT with a wide centre: `orbits` is a pt_wide_model.Orbits of (cfg, centre)"""
    return pt_state_rows_on(cfg, orbits.x[0], orbits.k[0] if orbits.julia else None, y0, y1)


def pt_wide_continue(cfg, orbits, state, from_iterations, y0=0, y1=None):
    return pt_continue_on(cfg, orbits.x[0], orbits.k[0] if orbits.julia else None, state, from_iterations, y0, y1)


# ---- comparisons -------------------------------------------------------------------------------------------------------------


def same_f64_state(a, b):
    """(z, iters, der): the integers equal, the doubles as bits, a NaN equal to any NaN"""
    return bool(np.array_equal(a[1], b[1])) and D.same_doubles(a[0], b[0]) and D.same_doubles(a[2], b[2])


def same_state(a, b):
    """all five arrays: the integers equal, the doubles as bits, a NaN equal to any NaN (only der can hold one)"""
    return (bool(np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])) and D.same_doubles(a[0], b[0]) and D.same_doubles(a[2], b[2])
            and D.same_doubles(a[4], b[4]))


def classes(state, n, m_cap):
    """of a state (or an F64 triple) at the cap m_cap that was continued from n: pixels (finished below n, escaped in [n, m_cap),
    capped at m_cap)"""
    it = state[1]
    return int((it < n).sum()), int(((it >= n) & (it < m_cap)).sum()), int((it == m_cap).sum())
