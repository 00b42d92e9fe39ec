"""ctypes front of tests/pt_state_model.c, the host restatement of the resumable PT state (include/fractal_hip.h,
fr_precision: "RESUMABLE PT"), plus the views and the cap chain of its tests.

The C file is compiled on first use into a fresh temporary directory (never into the tree):
gcc -O2 -ffp-contract=off -fno-fast-math -fopenmp -shared.  At most 16 OpenMP threads."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import pt_model as PM

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pt_state_model.c")
THREADS = PM.THREADS
ON_K = 0x80000000

# every link is continued from the one before; 37 -> 38 is a link of one step, 0 -> 1 the first step of all
CHAIN = (0, 1, 2, 5, 37, 38, 200, 333, 1500, 4000)

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler for tests/pt_state_model.c")
    d = tempfile.mkdtemp(prefix="pt_state_model_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libpt_state_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-o", so,
                    SRC, "-lm"], check=True)
    L = C.CDLL(so)
    L.ptsm_rows.restype = C.c_int
    L.ptsm_rows.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    L.ptsm_orbit_info.restype = C.c_int
    L.ptsm_orbit_info.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_uint32)]
    _lib = L
    return L


def _cfg_ptr(cfg):
    assert C.sizeof(cfg) == 104, "an fr_config image is 104 bytes"
    return C.addressof(cfg)


def state_rows(cfg, pos_lo=(0.0, 0.0), y0=0, y1=None, rule=0):
    """the state after cfg.iterations steps: (z float64 [rows, width, 2], iters uint32 [rows, width], dz float64
    [rows, width, 2], m uint32 [rows, width], bit 31 = on K)"""
    y1 = cfg.height if y1 is None else y1
    shape = (y1 - y0, cfg.width)
    z, dz = np.empty(shape + (2,), dtype=np.float64), np.empty(shape + (2,), dtype=np.float64)
    it, m = np.empty(shape, dtype=np.uint32), np.empty(shape, dtype=np.uint32)
    viol = C.c_uint64(0)
    ok = lib().ptsm_rows(_cfg_ptr(cfg), float(pos_lo[0]), float(pos_lo[1]), y0, y1, 0, 1, rule, z.ctypes.data, it.ctypes.data,
                         dz.ctypes.data, m.ctypes.data, C.byref(viol), THREADS)
    assert ok, "pt_state_model: out of memory"
    assert viol.value == 0, "a fresh run met m >= last at the top of a step"
    return z, it, dz, m


def continue_rows(cfg, state, from_iterations, pos_lo=(0.0, 0.0), y0=0, y1=None, rule=0):
    """`state` at the cap from_iterations continued to cfg.iterations on the orbits of cfg's cap -> (the new state, copies;
    the number of resumed steps that began with m >= last)"""
    y1 = cfg.height if y1 is None else y1
    z, it, dz, m = (np.array(a, order="C") for a in state)
    assert z.dtype == np.float64 and dz.dtype == np.float64 and it.dtype == np.uint32 and m.dtype == np.uint32
    assert it.shape == (y1 - y0, cfg.width) == m.shape and z.shape == it.shape + (2,) == dz.shape
    viol = C.c_uint64(0)
    ok = lib().ptsm_rows(_cfg_ptr(cfg), float(pos_lo[0]), float(pos_lo[1]), y0, y1, from_iterations, 0, rule, z.ctypes.data,
                         it.ctypes.data, dz.ctypes.data, m.ctypes.data, C.byref(viol), THREADS)
    assert ok, "pt_state_model: out of memory"
    return (z, it, dz, m), viol.value


def orbit_info(cfg, pos_lo=(0.0, 0.0), which=0):
    """(last, ended by escape) of orbit `which` (0: R or V, 1: K) at cfg's cap"""
    out = (C.c_uint32 * 2)()
    assert lib().ptsm_orbit_info(_cfg_ptr(cfg), float(pos_lo[0]), float(pos_lo[1]), which, out)
    return out[0], bool(out[1])


def same_state(a, b):
    """all four arrays equal, the doubles as bits"""
    return (np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
            and np.array_equal(np.ascontiguousarray(a[0]).view(np.uint64), np.ascontiguousarray(b[0]).view(np.uint64))
            and np.array_equal(np.ascontiguousarray(a[2]).view(np.uint64), np.ascontiguousarray(b[2]).view(np.uint64)))


def cut_end_class(cfg, state, pos_lo=(0.0, 0.0)):
    """Running pixels of `state` (at cfg's cap N >= 1) that never rebased and met m == last of X at the final step on an X cut
    by the cap: the pixels on which PT's rule and the state rule leave different (dz, m).  -> (running, in the class)"""
    z, it, dz, m = state
    running = it == cfg.iterations
    last, ended = orbit_info(cfg, pos_lo, 0)
    if ended or cfg.iterations == 0:
        return int(running.sum()), 0
    return int(running.sum()), int((running & (m == last)).sum())  # bit 31 clear: still on X; m == last: never rebased


# ---- views: name -> fill(cfg) -> pos_lo -------------------------------------------------------------------


def shallow_mandelbrot_view(cfg, width=67, height=45, iterations=4000):
    cfg.algo = 0
    cfg.width, cfg.height, cfg.iterations = width, height, iterations
    cfg.pos.re, cfg.pos.im = -0.6, 0.0
    cfg.scale.re = cfg.scale.im = 0.4
    return (0.0, 0.0)


def shallow_julia_view(cfg, width=67, height=45, iterations=4000):
    cfg.algo = 2
    cfg.width, cfg.height, cfg.iterations = width, height, iterations
    cfg.julia_set.re, cfg.julia_set.im = -0.8, 0.156
    cfg.pos.re, cfg.pos.im = 0.0, 0.0
    cfg.scale.re = cfg.scale.im = 0.4
    return (0.0, 0.0)


VIEWS = {
    "seahorse": PM.seahorse_view,  # 32 x 24, pos_lo != 0: the orbit R is cut by every cap of the chain
    "early_escape": PM.early_escape_view,  # 48 x 32: R is ended by escape after 30 steps
    "julia_rebase": PM.julia_rebase_view,  # 48 x 32: V is ended by escape after 201 steps, K is cut
    "shallow_mandelbrot": shallow_mandelbrot_view,  # 67 x 45: edge tiles
    "shallow_julia": shallow_julia_view,
}


def view(name, new_cfg, iterations):
    """(cfg, pos_lo) of the named view at the cap `iterations`; new_cfg() makes a default Config of 104 bytes"""
    cfg = new_cfg()
    pos_lo = VIEWS[name](cfg)
    cfg.iterations = iterations
    return cfg, pos_lo
