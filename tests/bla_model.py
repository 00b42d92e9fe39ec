"""ctypes front of tests/bla_model.c, the host restatement of BLA-PT (include/fractal_hip.h, "BLA-PT"), plus the views of
the BLA tests.

The model takes reference orbits as arrays: the dd road's come from tests/pt_model.py (reference_orbit), the wide road's from
tests/pt_wide_model.py (orbit), so the model shares nothing with the library.  The C file is compiled on first use into a
fresh temporary directory: gcc -O2 -ffp-contract=off -fno-fast-math -shared."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "bla_model.c")
DEFAULT_BITS = 40  # FR_BLA_DEFAULT_BITS


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
        raise RuntimeError("no C compiler for tests/bla_model.c")
    d = tempfile.mkdtemp(prefix="bla_model_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libbla_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", so, SRC, "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.blam_D.restype = C.c_double
    L.blam_D.argtypes = [C.POINTER(_View)]
    L.blam_table_entries.restype = C.c_uint64
    L.blam_table_entries.argtypes = [C.c_uint32]
    L.blam_build_table.restype = C.c_uint32
    L.blam_build_table.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    L.blam_rows.restype = C.c_int
    L.blam_rows.argtypes = [C.POINTER(_View), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                            C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = L
    return L


def _view(cfg):
    return _View(cfg.width, cfg.height, cfg.iterations, int(cfg.algo == 2), cfg.limit, cfg.scale.re, cfg.scale.im)


def _orbit(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.ndim == 2 and a.shape[1] == 2 and len(a) >= 2
    return a


def table(cfg, orbit, bits=DEFAULT_BITS):
    """the table of `orbit` (float64 [entries, 2]) for cfg's image -> a list of levels, each float64 [n_k, 5] =
    A.re, A.im, B.re, B.im, r2; [] for an orbit with last < 2"""
    orbit = _orbit(orbit)
    last = len(orbit) - 1
    v = _view(cfg)
    total = int(lib().blam_table_entries(last))
    out = np.zeros((total + 1, 5), dtype=np.float64)
    n = np.zeros(33, dtype=np.uint32)
    levels = lib().blam_build_table(orbit.ctypes.data, last, lib().blam_D(C.byref(v)), 0.0 if cfg.algo == 2 else 1.0, bits,
                                    out.ctypes.data, n.ctypes.data)
    res, off = [], 0
    for k in range(levels):
        res.append(out[off:off + int(n[k])].copy())
        off += int(n[k])
    assert off == total
    return res


def escape_rows(cfg, x_orbit, k_orbit=None, bits=DEFAULT_BITS, y0=0, y1=None):
    """BLA-PT over rows [y0, y1) on the given orbits (k_orbit: Julia's K; Mandelbrot: None) -> (z float64 [rows, width, 2],
    iters uint32 [rows, width], passes uint32 [rows, width])"""
    y1 = cfg.height if y1 is None else y1
    x_orbit = _orbit(x_orbit)
    k_orbit = x_orbit if k_orbit is None else _orbit(k_orbit)
    assert (cfg.algo == 2) == (k_orbit is not x_orbit)
    v = _view(cfg)
    shape = (y1 - y0, cfg.width)
    z = np.empty(shape + (2,), dtype=np.float64)
    it = np.empty(shape, dtype=np.uint32)
    passes = np.empty(shape, dtype=np.uint32)
    ok = lib().blam_rows(C.byref(v), x_orbit.ctypes.data, len(x_orbit) - 1, k_orbit.ctypes.data, len(k_orbit) - 1, bits, y0, y1,
                         z.ctypes.data, it.ctypes.data, passes.ctypes.data)
    assert ok, "bla_model: out of memory"
    return z, it, passes


def steps(cfg, iters):
    """the nominal iterations of a result: escape index + 1, or the cap"""
    it = np.asarray(iters, dtype=np.uint64)
    return int(np.where(it < cfg.iterations, it + 1, cfg.iterations).sum())


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


# ---- the views of the BLA tests -----------------------------------------------------------------------------------------


class View:
    """A view with its orbits from the PT models (never from the library), plain PT's result and the BLA model's per bits,
    each computed once.  kind "wide": spec = (name, n, scale_log2, width, height, cap) on tests/pt_wide_model.py's centres;
    kind "dd": spec = (a view function of tests/pt_model.py, keyword arguments)."""

    def __init__(self, new_config, kind, spec):
        import pt_model as P
        import pt_wide_model as W

        self.kind = kind
        self._models = {}
        if kind == "wide":
            name, n, scale_log2, width, height, cap = spec
            self.n = n
            self.cfg = W.view(new_config(), name, scale_log2, width, height, cap)
            self.ints = W.centre_ints(name, n)
            self.words = W.to_words(self.ints[0], n), W.to_words(self.ints[1], n)
            orbits = W.Orbits(self.cfg, *self.ints, n)
            self.x = orbits.x[0]
            self.k = orbits.k[0] if self.cfg.algo == 2 else None
            (z, it, _, _), _ = W.state_rows(self.cfg, orbits, rule=1)  # PT's own rule: plain WIDE PT
            self.pos_lo = None
        else:
            fn, kw = spec
            self.cfg = new_config()
            self.pos_lo = getattr(P, fn)(self.cfg, **kw)
            self.x = P.reference_orbit(self.cfg, self.pos_lo, 0)
            self.k = P.reference_orbit(self.cfg, self.pos_lo, 1) if self.cfg.algo == 2 else None
            z, it = P.escape_rows(self.cfg, self.pos_lo)
        self.pt = (z, it)
        for a in (self.x, self.k, z, it):
            if a is not None:
                a.setflags(write=False)
        self.shape = (self.cfg.height, self.cfg.width)

    def model(self, bits=DEFAULT_BITS):
        """(z, iters, passes) of the BLA model over the whole image"""
        if bits not in self._models:
            r = escape_rows(self.cfg, self.x, self.k, bits)
            for a in r:
                a.setflags(write=False)
            self._models[bits] = r
        return self._models[bits]

    def args(self, native):
        """(pos_lo, centre) of the fr_*_pt_bla calls and what keeps them alive"""
        if self.kind == "wide":
            p64 = C.POINTER(C.c_uint64)
            st = native.fr_wide_centre(self.n, self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64))
            return None, C.byref(st), st
        lo = native.Imaginary(*self.pos_lo)
        return C.byref(lo), None, lo


_views = {}


def view(new_config, kind, *spec):
    """the View of one of the specs below (or of another), made once per process"""
    key = (kind,) + tuple(repr(s) for s in spec)
    if key not in _views:
        _views[key] = View(new_config, kind, spec)
    return _views[key]


M_16 = ("wide", "M", 6, 300, 16, 12, 5000)
M_37 = ("wide", "M", 6, 300, 37, 21, 5000)
M_64 = ("wide", "M", 6, 300, 64, 48, 5000)
M_DEEP = ("wide", "M", 9, 440, 16, 12, 5000)  # the edge of WIDE PT's domain
N_64 = ("wide", "N", 6, 300, 64, 48, 3000)
N_16 = ("wide", "N", 6, 300, 16, 12, 3000)
J_64 = ("wide", "J", 6, 300, 64, 48, 5000)
J_48 = ("wide", "J", 6, 300, 48, 32, 5000)
SEAHORSE = ("dd", "seahorse_view", {})
EARLY = ("dd", "early_escape_view", {})
JULIA_REBASE = ("dd", "julia_rebase_view", {})
