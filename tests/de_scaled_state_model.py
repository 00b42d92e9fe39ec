"""ctypes front of tests/de_scaled_state_model.c, the host restatement of RESUMABLE SCALED DE (include/fractal_hip.h, "RESUMABLE
SCALED DE").

It runs on pt_wide_model.Orbits (Python integers), which carry each orbit's ended flag, and on the chains of caps of
tests/pt_scaled_state_model.py (Chain / CHAINS): the derivative changes nothing about (z, iters, w, m), so the conditions
tests/test_pt_scaled_state_cpu.py asserts on those chains carry over.  The C file is compiled on first use into a fresh temporary
directory: gcc -O2 -ffp-contract=off -fno-fast-math -shared."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import de_state_model as DS
import pt_scaled_state_model as T

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "de_scaled_state_model.c")
ON_K = T.ON_K
CHAINS = T.CHAINS
TYPES = (np.float64, np.uint32, np.float64, np.uint32, np.float64)  # z, iters, w, m, der

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler for tests/de_scaled_state_model.c")
    d = tempfile.mkdtemp(prefix="de_scaled_state_model_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libde_scaled_state_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", so, SRC, "-lm"],
                   check=True)
    L = C.CDLL(so)
    v, u32 = C.c_void_p, C.c_uint32
    L.dessm_rows.restype = None
    L.dessm_rows.argtypes = [C.POINTER(T._View), C.c_int, v, u32, C.c_int, v, u32, C.c_int, u32, u32, u32, C.c_int, v, v, v, v, v,
                             C.POINTER(C.c_uint64)]
    _lib = L
    return L


def _empty(shape):
    return tuple(np.empty(shape + ((2,) if ty is np.float64 else ()), dtype=ty) for ty in TYPES)


def _run(cfg, orbits, y0, y1, from_iterations, fresh, state):
    z, it, w, m, der = state
    viol = C.c_uint64(0)
    if orbits is None:  # an algorithm without orbits
        v = T._View(cfg.width, cfg.height, cfg.iterations, 0, cfg.limit, cfg.scale.re, cfg.scale.im)
        lib().dessm_rows(C.byref(v), 0, None, 0, 0, None, 0, 0, y0, y1, from_iterations, int(fresh), z.ctypes.data, it.ctypes.data,
                         w.ctypes.data, m.ctypes.data, der.ctypes.data, C.byref(viol))
        return state
    v = T._View(cfg.width, cfg.height, cfg.iterations, int(orbits.julia), cfg.limit, cfg.scale.re, cfg.scale.im)
    (xa, xe, _), (ka, ke, _) = orbits.x, orbits.k
    lib().dessm_rows(C.byref(v), 1, xa.ctypes.data, len(xa) - 1, int(xe), ka.ctypes.data, len(ka) - 1, int(ke), y0, y1,
                     from_iterations, int(fresh), z.ctypes.data, it.ctypes.data, w.ctypes.data, m.ctypes.data, der.ctypes.data,
                     C.byref(viol))
    assert viol.value == 0, "a step began with m >= last of the orbit followed"
    return state


def state_rows(cfg, orbits, y0=0, y1=None):
    """the state after cfg.iterations steps on `orbits` (pt_wide_model.Orbits of cfg's cap; None: an algorithm without orbits):
    (z float64 [rows, width, 2], iters uint32 [rows, width], w float64 [rows, width, 2], m uint32 [rows, width], der float64
    [rows, width, 2] holding u)"""
    y1 = cfg.height if y1 is None else y1
    return _run(cfg, orbits, y0, y1, 0, True, _empty((y1 - y0, cfg.width)))


def continue_rows(cfg, orbits, state, from_iterations, y0=0, y1=None):
    """`state` at the cap from_iterations continued to cfg.iterations on `orbits` (those of cfg's cap) -> the new state (copies)"""
    y1 = cfg.height if y1 is None else y1
    return _run(cfg, orbits, y0, y1, from_iterations, False, tuple(np.array(a, order="C") for a in state))


same_state = DS.same_state  # all five arrays: the integers equal, the doubles as bits, a NaN equal to any NaN

_states = {}


def state(chain, cap):
    """the model's fresh run of a pt_scaled_state_model.Chain at `cap`, made once and read-only"""
    key = (chain.name, cap)
    if key not in _states:
        st = state_rows(chain.cfg(cap), chain.orbits(cap))
        for a in st:
            a.setflags(write=False)
        _states[key] = st
    return _states[key]
