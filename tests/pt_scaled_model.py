"""ctypes front of tests/pt_scaled_model.c, the host restatement of SCALED PT (include/fractal_hip.h, "SCALED PT"), plus the
views of the scaled tests, past the 2^440 edge of WIDE PT and inside it.

Orbits and centres come from tests/pt_wide_model.py (Python integers, mpmath), so the model shares nothing with the library.
The C file is compiled on first use into a fresh temporary directory: gcc -O2 -ffp-contract=off -fno-fast-math -shared."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import pt_wide_model as W

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pt_scaled_model.c")
NO_TABLE = -1  # bits: the plain scaled loop


class _View(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("julia", C.c_int),
                ("limit", C.c_double), ("scale_re", C.c_double), ("scale_im", C.c_double)]


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler for tests/pt_scaled_model.c")
    d = tempfile.mkdtemp(prefix="pt_scaled_model_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libpt_scaled_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", so, SRC, "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.ptsm_e.restype = C.c_int
    L.ptsm_e.argtypes = [C.POINTER(_View)]
    L.ptsm_Dw.restype = C.c_double
    L.ptsm_Dw.argtypes = [C.POINTER(_View)]
    L.ptsm_table_entries.restype = C.c_uint64
    L.ptsm_table_entries.argtypes = [C.c_uint32]
    L.ptsm_build_table.restype = C.c_uint32
    L.ptsm_build_table.argtypes = [C.POINTER(_View), C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    L.ptsm_rows.restype = C.c_int
    L.ptsm_rows.argtypes = [C.POINTER(_View), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ptsm_rows_table_of.restype = C.c_int
    L.ptsm_rows_table_of.argtypes = [C.POINTER(_View), C.POINTER(_View)] + L.ptsm_rows.argtypes[1:]
    _lib = L
    return L


def _view(cfg):
    return _View(cfg.width, cfg.height, cfg.iterations, int(cfg.algo == 2), cfg.limit, cfg.scale.re, cfg.scale.im)


def _orbit(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.ndim == 2 and a.shape[1] == 2 and len(a) >= 2
    return a


def exponent(cfg):
    """e of the view: max |scale| = f 2^e with 0.5 <= f < 1"""
    return int(lib().ptsm_e(C.byref(_view(cfg))))


def table(cfg, orbit, bits):
    """the scaled table of `orbit` (float64 [entries, 2]) for cfg's image -> a list of levels, each float64 [n_k, 5] =
    A.re, A.im, B.re, B.im, R; [] for an orbit with last < 2"""
    orbit = _orbit(orbit)
    last = len(orbit) - 1
    v = _view(cfg)
    total = int(lib().ptsm_table_entries(last))
    out = np.zeros((total + 1, 5), dtype=np.float64)
    n = np.zeros(33, dtype=np.uint32)
    levels = lib().ptsm_build_table(C.byref(v), orbit.ctypes.data, last, bits, out.ctypes.data, n.ctypes.data)
    res, off = [], 0
    for k in range(levels):
        res.append(out[off:off + int(n[k])].copy())
        off += int(n[k])
    assert off == total
    return res


def escape_rows(cfg, x_orbit, k_orbit=None, bits=NO_TABLE, y0=0, y1=None):
    """SCALED PT over rows [y0, y1) on the given orbits (k_orbit: Julia's K; Mandelbrot: None); bits = -1: no table ->
    (z float64 [rows, width, 2], iters uint32 [rows, width], passes uint32 [rows, width], rebases uint32 [rows, width])"""
    y1 = cfg.height if y1 is None else y1
    x_orbit = _orbit(x_orbit)
    k_orbit = x_orbit if k_orbit is None else _orbit(k_orbit)
    assert (cfg.algo == 2) == (k_orbit is not x_orbit)
    v = _view(cfg)
    shape = (y1 - y0, cfg.width)
    z = np.empty(shape + (2,), dtype=np.float64)
    it, passes, reb = (np.empty(shape, dtype=np.uint32) for _ in range(3))
    ok = lib().ptsm_rows(C.byref(v), x_orbit.ctypes.data, len(x_orbit) - 1, k_orbit.ctypes.data, len(k_orbit) - 1, bits, y0, y1,
                         z.ctypes.data, it.ctypes.data, passes.ctypes.data, reb.ctypes.data)
    assert ok, "pt_scaled_model: out of memory, or a step went past the end of an orbit"
    return z, it, passes, reb


def escape_rows_table_of(cfg, table_cfg, x_orbit, k_orbit=None, bits=40, y0=0, y1=None):
    """escape_rows with a FOREIGN table: the tables are built with table_cfg's Dw and S, everything else is cfg's — what a
    kernel computes that is handed another view's tables on the same orbits.  table_cfg = cfg: escape_rows, bit for bit."""
    assert bits >= 0
    y1 = cfg.height if y1 is None else y1
    x_orbit = _orbit(x_orbit)
    k_orbit = x_orbit if k_orbit is None else _orbit(k_orbit)
    assert (cfg.algo == 2) == (k_orbit is not x_orbit)
    v, tv = _view(cfg), _view(table_cfg)
    shape = (y1 - y0, cfg.width)
    z = np.empty(shape + (2,), dtype=np.float64)
    it, passes, reb = (np.empty(shape, dtype=np.uint32) for _ in range(3))
    ok = lib().ptsm_rows_table_of(C.byref(v), C.byref(tv), x_orbit.ctypes.data, len(x_orbit) - 1, k_orbit.ctypes.data,
                                  len(k_orbit) - 1, bits, y0, y1, z.ctypes.data, it.ctypes.data, passes.ctypes.data, reb.ctypes.data)
    assert ok, "pt_scaled_model: out of memory, or a step went past the end of an orbit"
    return z, it, passes, reb


def steps(cfg, iters):
    """the nominal iterations of a result: escape index + 1, or the cap"""
    it = np.asarray(iters, dtype=np.uint64)
    return int(np.where(it < cfg.iterations, it + 1, cfg.iterations).sum())


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


# ---- the deep minibrot ----------------------------------------------------------------------------------------------------

MINI_PREC = 1400
MINI_PERIOD = 267


@functools.lru_cache(maxsize=None)
def minibrot_centre():
    """(re, im) as mpmath numbers of 1400 bits: the nucleus of period 267 that Newton's method on z_267(c) = 0 reaches from
    c0 = M + (0.3 + 0.2i) 2^-445, M the Misiurewicz point of tests/pt_wide_model.py.  It lies about 2^-431 from c0."""
    import mpmath

    with mpmath.workprec(MINI_PREC):
        mre, mim = W.centre("M")
        c0 = mpmath.mpc(mre, mim) + mpmath.mpc("0.3", "0.2") * mpmath.mpf(2) ** -445
        c, step = c0, None
        for _ in range(60):
            z, d = mpmath.mpc(0), mpmath.mpc(0)
            for _k in range(MINI_PERIOD):
                d = 2 * z * d + 1
                z = z * z + c
            step = z / d
            c = c - step
            if abs(step) < mpmath.mpf(2) ** -1350:
                break
        dist = abs(c - c0)
        assert mpmath.mpf(2) ** -432 < dist < mpmath.mpf(2) ** -430, mpmath.log(dist, 2)
        assert abs(step) < mpmath.mpf(2) ** -1350
        return +c.real, +c.imag


def centre_ints(name, n):
    """the centre floored to n words: pt_wide_model's M, N, J, or "MINI" """
    if name == "MINI":
        re, im = minibrot_centre()
        return W.floor_scaled(re, n), W.floor_scaled(im, n)
    return W.centre_ints(name, n)


# ---- the views of the scaled tests -----------------------------------------------------------------------------------------


class View:
    """spec = (name, n, scale_log2, width, height, cap): a view on one of the centres with its orbits from pt_wide_model and
    the scaled model's results per bits, each computed once and read-only."""

    def __init__(self, new_config, spec):
        name, n, scale_log2, width, height, cap = spec
        self.n = n
        self.cfg = W.view(new_config(), "M" if name == "MINI" else name, scale_log2, width, height, cap)
        self.ints = centre_ints(name, n)
        self.words = W.to_words(self.ints[0], n), W.to_words(self.ints[1], n)
        self.orbits = W.Orbits(self.cfg, *self.ints, n)
        self.x = self.orbits.x[0]
        self.k = self.orbits.k[0] if self.cfg.algo == 2 else None
        for a in (self.x, self.k):
            if a is not None:
                a.setflags(write=False)
        self.shape = (height, width)
        self._models = {}

    def model(self, bits=NO_TABLE):
        """(z, iters, passes, rebases) of the scaled model over the whole image"""
        if bits not in self._models:
            r = escape_rows(self.cfg, self.x, self.k, bits)
            for a in r:
                a.setflags(write=False)
            self._models[bits] = r
        return self._models[bits]

    def centre(self, native):
        """the fr_wide_centre of the view (it points into self.words)"""
        p64 = C.POINTER(C.c_uint64)
        return native.fr_wide_centre(self.n, self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64))


_views = {}


def view(new_config, spec):
    """the View of one of the specs below (or of another), made once per process"""
    if spec not in _views:
        _views[spec] = View(new_config, spec)
    return _views[spec]


# inside WIDE PT's domain: the scaled road must reproduce the existing ones
M_200 = ("M", 5, 200, 16, 12, 5000)
M_440 = ("M", 9, 440, 37, 21, 5000)
N_300 = ("N", 6, 300, 16, 12, 3000)
J_300 = ("J", 6, 300, 16, 12, 5000)
M_300 = ("M", 6, 300, 16, 12, 5000)
# past it
M_900 = ("M", 16, 900, 37, 21, 6000)
N_900 = ("N", 16, 900, 16, 12, 1000)
J_900 = ("J", 16, 900, 16, 12, 5000)
MINI_861 = ("MINI", 16, 861, 24, 16, 3204)
