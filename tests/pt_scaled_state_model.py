"""ctypes front of tests/pt_scaled_state_model.c, the host restatement of RESUMABLE SCALED PT (include/fractal_hip.h,
"RESUMABLE SCALED PT"), plus the chains of caps the state tests walk.

It runs on pt_wide_model.Orbits (Python integers), which carry each orbit's ended flag, so the model shares nothing with the
library.  The C file is compiled on first use into a fresh temporary directory: gcc -O2 -ffp-contract=off -fno-fast-math
-shared."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import pt_scaled_model as S
import pt_wide_model as W

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pt_scaled_state_model.c")
ON_K = 0x80000000


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
        raise RuntimeError("no C compiler for tests/pt_scaled_state_model.c")
    d = tempfile.mkdtemp(prefix="pt_scaled_state_model_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libpt_scaled_state_model.so")
    subprocess.run([cc, "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", so, SRC, "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.ptssm_rows.restype = None
    L.ptssm_rows.argtypes = [C.POINTER(_View), C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32,
                             C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.POINTER(C.c_uint64)]
    _lib = L
    return L


def _run(cfg, orbits, y0, y1, from_iterations, fresh, state):
    v = _View(cfg.width, cfg.height, cfg.iterations, int(orbits.julia), cfg.limit, cfg.scale.re, cfg.scale.im)
    z, it, w, m = state
    reb = np.zeros(it.shape, dtype=np.uint32)
    at_end = np.zeros(it.shape, dtype=np.uint32)
    viol = C.c_uint64(0)
    (xa, xe, _), (ka, ke, _) = orbits.x, orbits.k
    lib().ptssm_rows(C.byref(v), xa.ctypes.data, len(xa) - 1, int(xe), ka.ctypes.data, len(ka) - 1, int(ke), y0, y1,
                     from_iterations, int(fresh), z.ctypes.data, it.ctypes.data, w.ctypes.data, m.ctypes.data, reb.ctypes.data,
                     at_end.ctypes.data, C.byref(viol))
    assert viol.value == 0, "a step began with m >= last of the orbit followed"
    return (z, it, w, m), reb, at_end


def state_rows(cfg, orbits, y0=0, y1=None):
    """the state after cfg.iterations steps on `orbits` (pt_wide_model.Orbits of cfg's cap): ((z float64 [rows, width, 2], iters
    uint32 [rows, width], w float64 [rows, width, 2], m uint32 [rows, width]), rebases per pixel, those of them taken on
    m == last of an orbit ended by escape)"""
    y1 = cfg.height if y1 is None else y1
    shape = (y1 - y0, cfg.width)
    st = (np.empty(shape + (2,), dtype=np.float64), np.empty(shape, dtype=np.uint32), np.empty(shape + (2,), dtype=np.float64),
          np.empty(shape, dtype=np.uint32))
    return _run(cfg, orbits, y0, y1, 0, True, st)


def continue_rows(cfg, orbits, state, from_iterations, y0=0, y1=None):
    """`state` at the cap from_iterations continued to cfg.iterations on `orbits` (those of cfg's cap) -> (the new state
    (copies), rebases and m == end rebases of the continued steps per pixel)"""
    y1 = cfg.height if y1 is None else y1
    st = tuple(np.array(a, order="C") for a in state)
    return _run(cfg, orbits, y0, y1, from_iterations, False, st)


same_state = W.same_state


# ---- the chains: pt_scaled_model's views with the cap replaced ---------------------------------------------------------------

# J2_900 is not one of pt_scaled_model's views.  On J_900 (julia_set -0.8 + 0.156i, limit 2) no pixel ever meets m == last of an
# orbit ended by escape, at any cap: the last entry of such an orbit has re*re + im*im > 4, a pixel that has followed the orbit
# that far without a rebase is still close to it and escapes at limit 2 in the same step, and K there is 253 entries long
# while a pixel on K rebases about every 20 steps.  J2_900 is the same kind of view — the repelling fixed point of a Julia set,
# at 2^900 on 16 x 12 pixels — built so that both ends are met: julia_set = 1.1i, whose critical orbit K escapes after 4 steps,
# and the library's default limit 65536, under which a pixel outlives the orbit it follows.
J2_SET = (0.0, 1.1)
J2_900 = ("J", 16, 900, 16, 12, 3000)

CHAINS = {
    "M_900": (S.M_900, (0, 1, 300, 560, 600, 6000), None),  # 37 x 21, ragged against the 16 x 16 workgroup
    "N_900": (S.N_900, (0, 1, 7, 1000, 4000), None),
    "J_900": (S.J_900, (0, 100, 400, 631, 632, 800, 5000), None),
    "MINI_861": (S.MINI_861, (0, 267, 1000, 3204, 5000), None),
    "J2_900": (J2_900, (0, 1, 4, 400, 600, 647, 648, 652, 3000), {"julia_set": J2_SET, "limit": 65536.0}),
}


def _fixed_point_ints(julia_set, n):
    """the repelling fixed point (1 + sqrt(1 - 4J)) / 2 of J = julia_set (its f64 values) at 1200 bits, floored to n words"""
    import mpmath

    with mpmath.workprec(W.PREC):
        j = mpmath.mpc(mpmath.mpf(julia_set[0]), mpmath.mpf(julia_set[1]))
        c = (1 + mpmath.sqrt(1 - 4 * j)) / 2
        assert abs(c * c + j - c) < mpmath.mpf(2) ** (20 - W.PREC) and abs(2 * c) > 1
        return W.floor_scaled(+c.real, n), W.floor_scaled(+c.imag, n)


class Chain:
    """one view of CHAINS (pt_scaled_model's spec with the cap replaced; J2_900: see above): per cap the config, the orbits
    (pt_wide_model.Orbits at that cap, so the last caps of N_900 and MINI_861, above pt_scaled_model's, are covered) and the
    model's state run, each made once and read-only"""

    def __init__(self, new_config, name):
        self.name = name
        self.spec, self.caps, self.extra = CHAINS[name]
        centre, self.n, self.scale_log2, self.width, self.height, _cap = self.spec
        self._view_name = "M" if centre == "MINI" else centre
        self._new_config = new_config
        self.ints = _fixed_point_ints(self.extra["julia_set"], self.n) if self.extra else S.centre_ints(centre, self.n)
        self.words = W.to_words(self.ints[0], self.n), W.to_words(self.ints[1], self.n)
        self.shape = (self.height, self.width)
        self._orbits, self._states, self._plain = {}, {}, {}

    def cfg(self, cap):
        cfg = W.view(self._new_config(), self._view_name, self.scale_log2, self.width, self.height, cap)
        if self.extra:
            cfg.julia_set.re, cfg.julia_set.im = self.extra["julia_set"]
            cfg.limit = self.extra["limit"]
        return cfg

    def orbits(self, cap):
        if cap not in self._orbits:
            o = W.Orbits(self.cfg(cap), *self.ints, self.n)
            for a in (o.x[0], o.k[0]):
                a.setflags(write=False)
            self._orbits[cap] = o
        return self._orbits[cap]

    def state(self, cap):
        """(state, rebases, end rebases) of the model's fresh run at `cap`"""
        if cap not in self._states:
            r = state_rows(self.cfg(cap), self.orbits(cap))
            for a in r[0] + r[1:]:
                a.setflags(write=False)
            self._states[cap] = r
        return self._states[cap]

    def plain(self, cap):
        """(z, iters, passes, rebases) of pt_scaled_model's plain loop (bits = -1) at `cap`"""
        if cap not in self._plain:
            o = self.orbits(cap)
            r = S.escape_rows(self.cfg(cap), o.x[0], o.k[0] if o.julia else None, S.NO_TABLE)
            for a in r:
                a.setflags(write=False)
            self._plain[cap] = r
        return self._plain[cap]

    def links(self):
        return list(zip(self.caps[:-1], self.caps[1:]))

    def centre(self, native):
        """the fr_wide_centre of the view (it points into self.words)"""
        p64 = C.POINTER(C.c_uint64)
        return native.fr_wide_centre(self.n, self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64))


_chains = {}


def chain(new_config, name):
    """the Chain of one of CHAINS, made once per process"""
    if name not in _chains:
        _chains[name] = Chain(new_config, name)
    return _chains[name]
