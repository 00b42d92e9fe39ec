"""fractal-renderer_amd — MI355X (gfx950) drop-in for Icelk/fractal-renderer's escape-time path.

Host-side mirror of the reference's public surface for this path, over the C ABI of
include/fractal_hip.h (libfractal_hip.so; hand-written HIP kernels in csrc/):

    reference (Rust)                                   here
    ------------------------------------------------   ---------------------------------
    calc::Config, Config::new(algo)  lib.rs:21-69      Config, Config.new(algo)
    calc::Algo                       lib.rs:150-154    Algo
    calc::Imaginary / calc::RGB      lib.rs:79-82,121  Imaginary / RGB (RGB.new(r, b, g))
    calc::recursive                  lib.rs:245-257    recursive(iterations, start, c, limit)
    calc::get_recursive_pixel        lib.rs:199-235    get_recursive_pixel(config, x, y)
    get_image (Mandelbrot|Julia arm) src/lib.rs:253    get_image(config)

There is no CPU fallback anywhere in this package: without the built library and a HIP device
every compute call raises.
"""
import ctypes as C
import enum
from fractions import Fraction

import numpy as np

from . import _native
from ._native import RGB, FractalHipError, Imaginary  # noqa: F401

__all__ = [
    "Algo", "Config", "Imaginary", "RGB", "Precision", "FractalHipError",
    "get_image", "get_image_rows", "get_image_rgba", "get_recursive_pixel", "recursive", "recursive_batch",
    "escape_rows", "colour_image", "count_iterations", "init", "shutdown", "device_count", "device_name",
    "RenderOpts", "init_devices", "get_image_multi", "multi_stats", "build_id", "get_image_fern", "split_dd",
    "box_filter", "ss_workspace_bytes", "SS_MAX",
    "escape_rows_device", "extend_rows_device", "extend_rows", "colour_rows_device",
    "escape_rows_pt_state", "extend_rows_pt", "escape_rows_pt_state_device", "extend_rows_pt_device", "pt_orbit_cache",
    "WideCentre", "reference_orbit_wide",
    "bla_table", "bla_count", "bla_cache", "BLA_DEFAULT_BITS",
    "get_image_ss_pt", "colour_rows_ss_device", "colour_image_ss",
    "ViewStats", "view_stats", "view_stats_device", "stats_percentile", "auto_exposure", "get_image_auto",
    "escape_rows_de", "distance_rows", "colour_image_de", "get_image_de", "escape_rows_de_device", "distance_rows_device",
    "colour_de_rows_device",
    "extend_rows_de", "extend_rows_de_device", "escape_rows_de_pt_state", "escape_rows_de_pt_state_device", "extend_rows_de_pt",
    "extend_rows_de_pt_device",
    "ss_de_workspace_bytes", "colour_image_de_ss", "colour_de_rows_ss_device",
    "de_scaled_view",
    "escape_rows_de_pt_scaled_state", "extend_rows_de_pt_scaled", "get_image_de_scaled_ss",
    "get_image_ss_adaptive", "ss_adaptive_workspace_bytes",
    "get_image_de_adaptive", "get_image_de_adaptive_scaled", "ss_adaptive_de_workspace_bytes",
    "ss_transfer_tables",
]


class Algo(enum.IntEnum):
    """calc/src/lib.rs:150-154; from_str mirrors FromStr (:165-179)."""

    Mandelbrot = 0
    BarnsleyFern = 1
    Julia = 2

    @classmethod
    def from_str(cls, s):
        t = s.lower()
        if t == "mandelbrot":
            return cls.Mandelbrot
        if t in ("fern", "barnsleyfern"):
            return cls.BarnsleyFern
        if t == "julia":
            return cls.Julia
        raise ValueError("invalid algorithm name")


class Precision(enum.IntEnum):
    F64 = 0  # the reference's arithmetic
    F32 = 1  # build-defined fast path (include/fractal_hip.h, fr_precision)
    DD = 2  # double-double deep zoom, ~106-bit significands (include/fractal_hip.h, fr_precision)
    PT = 3  # perturbation deep zoom: one dd reference orbit, f64 offsets per pixel (include/fractal_hip.h, fr_precision)


def split_dd(value):
    """An exact value -> (hi, lo), two floats with hi = the nearest f64 and lo = the nearest f64 to the rest, so that
    hi + lo carries ~106 significant bits and (hi, lo) is a normalised pos / pos_lo pair.  `value` may be a str
    ("-0.743643887037158704752191506114774"), a Decimal, a Fraction, an int, a float or an mpmath mpf (converted through
    its exact binary value): the split is done in rational arithmetic, with no rounding before the two f64 roundings."""
    if isinstance(value, str):
        f = Fraction(value.strip())
    elif isinstance(value, Fraction):
        f = value
    elif hasattr(value, "man_exp"):  # mpmath.mpf: mantissa * 2^exponent, exactly
        man, exp = value.man_exp
        f = Fraction(int(man)) * (Fraction(2) ** int(exp))
    else:  # int, float, Decimal: Fraction takes each exactly
        f = Fraction(value)
    hi = float(f)
    lo = float(f - Fraction(hi))
    return hi, lo


class WideCentre:
    """The view centre of WIDE PT (include/fractal_hip.h, "WIDE PT"): per axis `words` little-endian uint64 words in two's
    complement, value I / 2^(64 words - 8) — up to 1016 bits where (pos, pos_lo) carries ~106.  Pass it as centre= to
    get_image, get_image_rows, get_image_rgba, escape_rows and the PT state calls with precision=Precision.PT."""

    def __init__(self, words, re=None, im=None):
        self.words = int(words)
        if not 2 <= self.words <= _native.FR_WIDE_MAX_WORDS:
            raise ValueError("a wide centre has 2 .. %d words" % _native.FR_WIDE_MAX_WORDS)
        self.re = np.zeros(self.words, dtype=np.uint64) if re is None else np.array(re, dtype=np.uint64)
        self.im = np.zeros(self.words, dtype=np.uint64) if im is None else np.array(im, dtype=np.uint64)
        if self.re.shape != (self.words,) or self.im.shape != (self.words,):
            raise ValueError("re and im hold `words` uint64 words each")

    @staticmethod
    def words_for_scale(scale):
        """the smallest word count of the domain rule F >= e + 64, where max |scale| = f 2^e with 0.5 <= f < 1"""
        import math

        e = math.frexp(max(abs(float(v)) for v in (scale if hasattr(scale, "__iter__") else (scale,))))[1]
        return max(2, -(-(e + 72) // 64))

    @classmethod
    def from_str(cls, re_text, im_text, scale=None, words=None):
        """Decimal strings of any length ("-0.2281554936539618...", "1e-3") through fr_wide_from_decimal: each component is
        the floor of the string's exact value.  words: the word count, or None to size it from `scale` (a number or the
        config's scale pair) by the domain rule."""
        if words is None:
            if scale is None:
                raise ValueError("from_str needs words= or scale=")
            words = cls.words_for_scale(scale)
        c = cls(words)
        for text, w in ((re_text, c.re), (im_text, c.im)):
            _native.check(_native.load().fr_wide_from_decimal(str(text).strip().encode(), w.ctypes.data, c.words))
        return c

    def add(self, dre, dim):
        """pan: I += floor(d 2^F) per axis (fr_wide_add_double) — a pan step or a clicked pixel's off; returns self"""
        _native.check(_native.load().fr_wide_add_double(self.re.ctypes.data, self.words, float(dre)))
        _native.check(_native.load().fr_wide_add_double(self.im.ctypes.data, self.words, float(dim)))
        return self

    def to_dd(self):
        """((re_hi, im_hi), (re_lo, im_lo)) through fr_wide_to_double: a normalised pos / pos_lo pair, which hands the view
        over to Precision.PT or Precision.DD at shallow scales"""
        out = []
        for w in (self.re, self.im):
            hi, lo = C.c_double(0.0), C.c_double(0.0)
            _native.check(_native.load().fr_wide_to_double(w.ctypes.data, self.words, C.byref(hi), C.byref(lo)))
            out.append((hi.value, lo.value))
        return (out[0][0], out[1][0]), (out[0][1], out[1][1])

    def c_struct(self):
        """the fr_wide_centre of the C calls; it points into this object's arrays, which must outlive the call"""
        p64 = C.POINTER(C.c_uint64)
        return _native.fr_wide_centre(self.words, self.re.ctypes.data_as(p64), self.im.ctypes.data_as(p64))


def _deep_call(precision, pos_lo=None, centre=None, bla=None, supersample=1, opts=None, scaled=False):
    """Which C family a call's keyword arguments select, in the order bla, centre, scaled, supersample, pos_lo:
    (family, the family's leading arguments behind the config, what keeps their memory alive).
      "scaled" (centre pointer, bits)                  the fr_*_pt_scaled calls; bits -1 without bla=
      "bla"   (pos_lo pointer, centre pointer, bits)   the fr_*_pt_bla calls
      "wide"  (centre pointer,)                        the fr_*_pt_wide calls
      "ss"    (pos_lo pointer,)                        fr_render_rows_ss
      "lo"    (pos_lo pointer,)                        the calls that take pos_lo
      "plain" ()                                       pos_lo is None, the C NULL: the calls without one, or (None,)"""
    if bla is not None:
        if int(precision) != Precision.PT:
            raise ValueError("bla= needs precision=Precision.PT")
        if supersample != 1:
            raise ValueError("supersample does not take bla=")
        if opts is not None:
            raise ValueError("bla= takes no opts: BLA-PT has one kernel")
        bits = int(bla)
        if bits != 0 and not 24 <= bits <= 53:
            raise ValueError("bla= is None (off), 0 (%d bits) or 24 .. 53" % BLA_DEFAULT_BITS)
    if centre is not None:
        if int(precision) != Precision.PT:
            raise ValueError("centre= needs precision=Precision.PT")
        if pos_lo is not None:
            raise ValueError("centre= and pos_lo= exclude each other")
        if supersample != 1:
            raise ValueError("supersample does not take centre= yet")
        st = centre.c_struct()
        if scaled:
            if opts is not None:
                raise ValueError("scaled= takes no opts: SCALED PT has one kernel per form")
            return "scaled", (C.byref(st), -1 if bla is None else bits), (st, centre)
        if bla is not None:
            return "bla", (None, C.byref(st), bits), (st, centre)
        return "wide", (C.byref(st),), (st, centre)
    if scaled:
        raise ValueError("scaled= needs centre= (a WideCentre); it takes neither pos_lo= nor supersample")
    lo = None if pos_lo is None else Imaginary(*(float(v) for v in pos_lo))
    lo_ptr = None if lo is None else C.byref(lo)
    if bla is not None:
        return "bla", (lo_ptr, None, bits), lo
    if supersample != 1:
        return "ss", (lo_ptr,), lo
    if pos_lo is not None:
        return "lo", (lo_ptr,), lo
    return "plain", (), None


def reference_orbit_wide(config, centre, which=0):
    """fr_debug_reference_orbit_wide: WIDE PT's reference orbit on the host (no device needed), float64 [entries, 2]"""
    st = centre.c_struct()
    n = C.c_uint32(0)
    out = np.empty((int(config.iterations) + 2, 2), dtype=np.float64)
    _native.check(_native.load().fr_debug_reference_orbit_wide(C.byref(config), C.byref(st), int(which), out.ctypes.data, len(out),
                                                               C.byref(n)))
    return out[:n.value].copy()


BLA_DEFAULT_BITS = _native.FR_BLA_DEFAULT_BITS


def bla_table(config, level, which=0, pos_lo=None, centre=None, bla=0, scaled=False):
    """fr_debug_bla_table: level `level` of the BLA-PT table of orbit `which` (0: R or V, 1: K, Julia only) on the host (no
    device needed): float64 [n_level, 5] = A.re, A.im, B.re, B.im, r2; empty past the top level.
    scaled=True (needs centre=): fr_debug_bla_table_scaled, SCALED PT's table, whose fifth column is the stored R."""
    lib = _native.load()
    n = C.c_uint32(0)
    if scaled:
        _, (ptr, bits), _keep = _deep_call(Precision.PT, pos_lo, centre, bla, scaled=True)
        _native.check(lib.fr_debug_bla_table_scaled(C.byref(config), ptr, bits, int(which), int(level), None, 0, C.byref(n)))
        out = np.empty((n.value, 5), dtype=np.float64)
        _native.check(lib.fr_debug_bla_table_scaled(C.byref(config), ptr, bits, int(which), int(level), out.ctypes.data, len(out),
                                                    C.byref(n)))
        return out
    _, (lo, ptr, bits), _keep = _deep_call(Precision.PT, pos_lo, centre, bla)
    _native.check(lib.fr_debug_bla_table(C.byref(config), lo, ptr, bits, int(which), int(level), None, 0, C.byref(n)))
    out = np.empty((n.value, 5), dtype=np.float64)
    _native.check(lib.fr_debug_bla_table(C.byref(config), lo, ptr, bits, int(which), int(level), out.ctypes.data, len(out), C.byref(n)))
    return out


def bla_count(config, y0=0, y1=None, pos_lo=None, centre=None, bla=0):
    """fr_debug_bla_count over rows [y0, y1): (passes through the BLA loop, nominal iterations), summed over the pixels on
    the device; their ratio is what the skips save."""
    y1 = config.height if y1 is None else y1
    _, (lo, ptr, bits), _keep = _deep_call(Precision.PT, pos_lo, centre, bla)
    passes, steps = C.c_uint64(0), C.c_uint64(0)
    _native.check(_native.load().fr_debug_bla_count(C.byref(config), lo, ptr, bits, y0, y1, C.byref(passes), C.byref(steps)))
    return passes.value, steps.value


def pt_scaled_count(config, centre, y0=0, y1=None, bla=None):
    """fr_debug_pt_scaled_count over rows [y0, y1): (passes through the scaled loop, nominal iterations), summed over the
    pixels on the device; bla=None: the plain scaled loop, one pass per step."""
    y1 = config.height if y1 is None else y1
    _, (ptr, bits), _keep = _deep_call(Precision.PT, None, centre, bla, scaled=True)
    passes, steps = C.c_uint64(0), C.c_uint64(0)
    _native.check(_native.load().fr_debug_pt_scaled_count(C.byref(config), ptr, bits, y0, y1, C.byref(passes), C.byref(steps)))
    return passes.value, steps.value


def bla_cache():
    """fr_debug_bla_cache: (bits of the cached table, levels of X's table, entries of all levels, 1 if the last request built
    it / 0 if it was served)."""
    out = (C.c_uint32 * 4)()
    _native.check(_native.load().fr_debug_bla_cache(out))
    return tuple(out)


class Config(_native.fr_config):
    """calc::Config (calc/src/lib.rs:21-37).  Fields keep the reference's names; colours hold the
    stored RGB struct fields."""

    @classmethod
    def new(cls, algo=Algo.Mandelbrot):
        """Config::new(algo) — calc/src/lib.rs:39-69 (filled in by the library)."""
        cfg = cls()
        _native.load().fr_config_new(C.byref(cfg), int(algo))
        return cfg

    def clone(self):
        other = type(self)()
        C.memmove(C.byref(other), C.byref(self), C.sizeof(self))
        return other


class RenderOpts(_native.fr_render_opts):
    """fr_render_opts: implementation selectors of ONE call (none changes an output byte).
    RenderOpts(tile=9, cycle_shortcut=1) starts from the process defaults."""

    def __init__(self, **kw):
        super().__init__()
        _native.load().fr_render_opts_init(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_) or k == "size":
                raise AttributeError(k)
            setattr(self, k, v)


def build_id():
    return _native.load().fr_build_id().decode()


def init_devices(devices):
    """fr_init_devices: the device set of the multi-GPU get_image; an index may repeat (logical devices)."""
    arr = (C.c_int * len(devices))(*devices)
    _native.check(_native.load().fr_init_devices(arr, len(devices)))


def get_image_multi(config, precision=0, block_rows=0, out=None):
    """get_image across the device set into a host array: every device DMAs its row blocks to their
    final place (fr_render_rgb8_multi)."""
    if out is None:
        out = np.empty((config.height, config.width, 3), dtype=np.uint8)
    _native.check(_native.load().fr_render_rgb8_multi(C.byref(config), int(precision), block_rows, out.ctypes.data,
                                                      out.nbytes))
    return out


def multi_stats():
    st = _native.fr_multi_stats()
    _native.check(_native.load().fr_multi_last_stats(C.byref(st)))
    n = st.n_devices
    return {"n_devices": n, "kernels": list(st.kernels[:n]), "kernel_ms": list(st.kernel_ms[:n]),
            "rows": list(st.rows[:n]), "wall_ms": st.wall_ms, "transfer_span_ms": list(st.transfer_span_ms[:n]),
            "job_ms": list(st.job_ms[:n]), "bytes_moved": list(st.bytes_moved[:n])}


def init(device=-1):
    _native.check(_native.load().fr_init(device))


def shutdown():
    _native.check(_native.load().fr_shutdown())


def device_count():
    n = C.c_int(0)
    _native.check(_native.load().fr_device_count(C.byref(n)))
    return n.value


def device_name():
    buf = C.create_string_buffer(256)
    _native.check(_native.load().fr_device_name(buf, len(buf)))
    return buf.value.decode()


SS_MAX = 8  # FR_SS_MAX


def _check_transfer(transfer):
    """A `transfer` that reaches no _tf call (supersample = 1 on a road without one) is still the library's to refuse: an empty
    fr_box_filter_rgb8_tf, which needs no device.  Returns it as an int."""
    t = int(transfer)
    if t != 0:
        _native.check(_native.load().fr_box_filter_rgb8_tf(None, 0, 0, 1, t, 3, None, 0))
    return t


def ss_transfer_tables():
    """fr_ss_transfer_tables: the library's own (L, T) of LINEAR-LIGHT SUPERSAMPLING (include/fractal_hip.h) as uint16 arrays —
    L[v], v = 0 .. 255, a byte as linear light, and T[k - 1], k = 1 .. 255, the least linear value that encodes to k.  No device."""
    dec, thr = C.POINTER(C.c_uint16)(), C.POINTER(C.c_uint16)()
    _native.check(_native.load().fr_ss_transfer_tables(C.byref(dec), C.byref(thr)))
    return np.array(dec[:256], dtype=np.uint16), np.array(thr[:255], dtype=np.uint16)


def _render_rows(config, y0, y1, channels, out, precision, opts, pos_lo, supersample, centre, bla, scaled=False, transfer=0):
    """rows [y0, y1) into `out` as `channels` bytes per pixel, by the C row render of the arguments' family"""
    lib, cfg = _native.load(), C.byref(config)
    transfer = _check_transfer(transfer)
    family, pre, _keep = _deep_call(precision, pos_lo, centre, bla, supersample, opts, scaled)
    o = C.byref(opts) if opts is not None else None
    tail = (y0, y1, channels, out.ctypes.data, out.nbytes)
    if family == "scaled":
        rc = lib.fr_render_rows_pt_scaled(cfg, *pre, *tail)
    elif family == "bla":
        rc = lib.fr_render_rows_pt_bla(cfg, *pre, *tail)
    elif family == "wide":
        rc = lib.fr_render_rows_pt_wide(cfg, *pre, *tail)
    elif family == "ss":  # s x s samples per pixel, box-filtered on the device
        rc = lib.fr_render_rows_ss_tf(cfg, int(precision), *pre, int(supersample), transfer, *tail, o)
    elif family == "lo":
        rc = _render_rows_lo(precision)(cfg, *pre, *tail)
    elif channels == 4:
        rc = lib.fr_render_rows_rgba8(cfg, int(precision), y0, y1, out.ctypes.data, out.nbytes)
    else:
        rc = lib.fr_render_rows_rgb8_opts(cfg, int(precision), y0, y1, out.ctypes.data, out.nbytes, o)
    _native.check(rc)
    return out


def ss_workspace_bytes(config, supersample, y0=0, y1=None):
    """fr_ss_workspace_bytes: (min_bytes, best_bytes) of the device workspace fr_render_rows_ss_device wants for rows
    [y0, y1) — one band of 8 * supersample source rows, and the whole range (at most 1 GiB)."""
    y1 = config.height if y1 is None else y1
    mn, best = C.c_size_t(0), C.c_size_t(0)
    _native.check(_native.load().fr_ss_workspace_bytes(C.byref(config), int(supersample), y0, y1, C.byref(mn), C.byref(best)))
    return mn.value, best.value


def box_filter(image, s, channels=3, transfer=0):
    """The box filter of the supersampled renders alone (fr_box_filter_rgb8_tf): image uint8 [s*rows, s*width, 3] ->
    uint8 [rows, width, channels], each byte (sum of its s x s block + s*s // 2) // (s*s); channels=4 adds alpha 255.
    E.g. to re-filter a large render the caller already holds.
    transfer = 1 (FR_SS_TRANSFER_SRGB; include/fractal_hip.h, "LINEAR-LIGHT SUPERSAMPLING"): the samples are averaged as linear
    light — decoded by the table L, summed, divided the same way, encoded by the thresholds T (ss_transfer_tables) — so a thin
    bright line keeps its light; 0 is the byte average; the library refuses any other value."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    s = int(s)
    if image.ndim != 3 or image.shape[2] != 3 or s < 1 or image.shape[0] % s or image.shape[1] % s:
        raise ValueError("image must be uint8 [s*rows, s*width, 3]")
    rows, width = image.shape[0] // s, image.shape[1] // s
    out = np.empty((rows, width, channels), dtype=np.uint8)
    _native.check(_native.load().fr_box_filter_rgb8_tf(image.ctypes.data, width, rows, s, int(transfer), channels, out.ctypes.data,
                                                       out.nbytes))
    return out


def _ss_pt_road(pos_lo, centre, bla, scaled):
    """get_image_ss_pt's keywords -> (road, bits) by _deep_call's rules; ValueError before any C call"""
    if bla is not None:
        bits = int(bla)
        if bits != 0 and not 24 <= bits <= 53:
            raise ValueError("bla= is None (off), 0 (%d bits) or 24 .. 53" % BLA_DEFAULT_BITS)
    if centre is not None and pos_lo is not None:
        raise ValueError("centre= and pos_lo= exclude each other")
    if scaled:
        if centre is None:
            raise ValueError("scaled= needs centre= (a WideCentre); it takes no pos_lo=")
        return _native.FR_PT_ROAD_SCALED, -1 if bla is None else bits
    if bla is not None:
        return _native.FR_PT_ROAD_BLA, bits
    return _native.FR_PT_ROAD_PLAIN, 0


def get_image_ss_pt(config, supersample, pos_lo=None, centre=None, bla=None, scaled=False, y0=0, y1=None, channels=3, out=None,
                    transfer=0):
    """Anti-aliased deep renders (fr_render_rows_ss_pt; include/fractal_hip.h, "supersampled rendering on the deep roads"):
    rows [y0, y1) of the Precision.PT image with supersample x supersample samples per pixel, box-filtered on the device, as
    uint8 [y1-y0, width, channels].  pos_lo, centre, bla and scaled select the road as they do in get_image_rows: plain PT
    (pos_lo or neither), WIDE PT (centre), BLA-PT (bla = 0 or 24 .. 53, with pos_lo or centre or neither), SCALED PT
    (scaled=True, needs centre; combines with bla).  supersample = 1 is the road's plain render. transfer: see box_filter."""
    s = int(supersample)
    if not 1 <= s <= SS_MAX:
        raise ValueError("supersample is 1 .. %d" % SS_MAX)
    if int(channels) not in (3, 4):
        raise ValueError("channels is 3 or 4")
    road, bits = _ss_pt_road(pos_lo, centre, bla, scaled)
    y0, y1 = _rows(config, y0, y1)
    if out is None:
        out = np.empty((max(y1 - y0, 0), config.width, int(channels)), dtype=np.uint8)
    lo = None if pos_lo is None else Imaginary(*(float(v) for v in pos_lo))
    st = None if centre is None else centre.c_struct()
    _native.check(_native.load().fr_render_rows_ss_pt_tf(C.byref(config), None if lo is None else C.byref(lo),
                                                         None if st is None else C.byref(st), road, bits, s, int(transfer), y0, y1,
                                                         int(channels), out.ctypes.data, out.nbytes))
    return out


def get_image_rows(config, y0, y1, precision=Precision.F64, out=None, opts=None, pos_lo=None, supersample=1, centre=None,
                   bla=None, scaled=False, transfer=0):
    """Rows [y0, y1) of get_image — the unit of the reference's rayon loop (src/lib.rs:256-264).
    Returns uint8 [y1-y0, width, 3].  pos_lo (Precision.DD or Precision.PT only): the low halves (re, im) of the view
    centre (split_dd), so that the centre is pos + pos_lo; None = (0, 0).
    supersample = s > 1: s x s samples per pixel, box-filtered on the device (include/fractal_hip.h, "supersampled
    rendering"); only the [y1-y0, width] result leaves the device.  transfer (0 or 1): see box_filter.
    centre (Precision.PT only, exclusive with pos_lo): a WideCentre in place of (config.pos, pos_lo) for views past a scale
    of 10^30 (include/fractal_hip.h, "WIDE PT").  supersample combines with neither centre, bla nor scaled here:
    anti-aliased deep renders on those roads are get_image_ss_pt's.
    bla (Precision.PT only, with pos_lo or centre or neither): None = plain PT; 0 or 24 .. 53 = BLA-PT at that many bits
    (0: BLA_DEFAULT_BITS), PT with iterations skipped in bulk — an approximation, defined in include/fractal_hip.h, "BLA-PT".
    scaled=True (needs centre=; combines with bla=; no pos_lo, supersample or opts): SCALED PT, the pixel loop that carries
    its offsets scaled by the view's exponent, for scales past 2^440 up to just under 2^952 (include/fractal_hip.h,
    "SCALED PT"); inside WIDE PT's domain it gives the same bytes as the call without it."""
    if out is None:
        out = np.empty((max(int(y1) - int(y0), 0), config.width, 3), dtype=np.uint8)
    return _render_rows(config, y0, y1, 3, out, precision, opts, pos_lo, supersample, centre, bla, scaled, transfer)


def get_image(config, precision=Precision.F64, pos_lo=None, supersample=1, centre=None, bla=None, scaled=False, transfer=0):
    """get_image(&Config) -> Vec<RGB> (src/lib.rs:253-270): uint8 [height, width, 3], row-major,
    bytes r,g,b.  Algo.BarnsleyFern is outside this path (random IFS, src/lib.rs:271-319): the
    per-pixel function returns BLACK for it (calc/src/lib.rs:211) and so does this.
    pos_lo: see get_image_rows (Precision.DD or Precision.PT only).  supersample, centre, bla, scaled, transfer: see
    get_image_rows."""
    out = np.empty((config.height, config.width, 3), dtype=np.uint8)
    if transfer == 0 and not scaled and bla is None and centre is None and supersample == 1 and pos_lo is None and int(precision) == Precision.F64:
        _native.check(_native.load().fr_render_rgb8(C.byref(config), out.ctypes.data, out.nbytes))
        return out
    return _render_rows(config, 0, config.height, 3, out, precision, None, pos_lo, supersample, centre, bla, scaled, transfer)


def _dd_only(precision):
    if int(precision) != Precision.DD:
        raise ValueError("pos_lo needs precision=Precision.DD")


def _render_rows_lo(precision):
    """the C row render that takes pos_lo for this precision"""
    if int(precision) == Precision.PT:
        return _native.load().fr_render_rows_pt
    if int(precision) != Precision.DD:
        raise ValueError("pos_lo needs precision=Precision.DD or Precision.PT")
    return _native.load().fr_render_rows_dd


def get_image_fern(config, threads=1, seed=0, walkers=0):
    """get_image's Algo::BarnsleyFern arm (src/lib.rs:271-319, 417-463) on the GPU: uint8 [height, width, 3].
    threads = the rayon thread count being modelled (the reference returns ONE thread's image of
    iterations / threads points); seed keys the build's deterministic RNG; walkers = parallel orbits (0 = auto)."""
    out = np.empty((config.height, config.width, 3), dtype=np.uint8)
    _native.check(_native.load().fr_render_fern_rgb8(C.byref(config), threads, seed, walkers, out.ctypes.data, out.nbytes))
    return out


def get_image_rgba(config, precision=Precision.F64, out=None, pos_lo=None, supersample=1, centre=None, bla=None, scaled=False,
                   transfer=0):
    """get_image as RGBA8 (alpha 255): uint8 [height, width, 4] — the GUI's upload format
    (src/gui.rs:71-72) produced on the device.  pos_lo: see get_image_rows (Precision.DD or Precision.PT only).
    supersample, centre, bla, scaled, transfer: see get_image_rows."""
    if out is None:
        out = np.empty((config.height, config.width, 4), dtype=np.uint8)
    return _render_rows(config, 0, config.height, 4, out, precision, None, pos_lo, supersample, centre, bla, scaled, transfer)


def get_recursive_pixel(config, x, y, precision=Precision.F64):
    """calc::get_recursive_pixel(&Config, x, y) -> RGB (calc/src/lib.rs:199-235)."""
    out = RGB()
    _native.check(_native.load().fr_pixel_p(C.byref(config), int(precision), x, y, C.byref(out)))
    return out


def recursive(iterations, start, c, limit):
    """calc::recursive(iterations, start, c, limit) -> (Imaginary, u32) (calc/src/lib.rs:245-257)."""
    pos, it = Imaginary(), C.c_uint32(0)
    _native.check(
        _native.load().fr_recursive(iterations, Imaginary(*start), Imaginary(*c), limit, C.byref(pos), C.byref(it))
    )
    return pos, it.value


def recursive_batch(iterations, start, c, limit, precision=Precision.F64):
    """recursive() over arrays: start, c float64 [n, 2] -> (pos float64 [n, 2], iters uint32 [n])."""
    start = np.ascontiguousarray(start, dtype=np.float64).reshape(-1, 2)
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(-1, 2)
    if start.shape != c.shape:
        raise ValueError("start and c must have the same shape")
    n = start.shape[0]
    pos = np.empty((n, 2), dtype=np.float64)
    it = np.empty(n, dtype=np.uint32)
    _native.check(
        _native.load().fr_recursive_batch(iterations, start.ctypes.data, c.ctypes.data, n, limit, int(precision),
                                          pos.ctypes.data, it.ctypes.data)
    )
    return pos, it


def escape_rows(config, y0=0, y1=None, precision=Precision.F64, pos_lo=None, with_lo=False, centre=None, bla=None, scaled=False):
    """recursive() results of every pixel of rows [y0, y1): (z float64 [rows, width, 2],
    iters uint32 [rows, width]).  Precision.DD: z holds the hi parts; with_lo=True returns z as [rows, width, 4] =
    re.hi, re.lo, im.hi, im.lo (Precision.DD only).  pos_lo: see get_image_rows (Precision.DD or Precision.PT only).
    centre: a WideCentre (Precision.PT only, exclusive with pos_lo): fr_escape_rows_pt_wide.
    bla (Precision.PT only): see get_image_rows; fr_escape_rows_pt_bla.
    scaled (needs centre=; combines with bla=): see get_image_rows; fr_escape_rows_pt_scaled."""
    y1 = config.height if y1 is None else y1
    if with_lo and (bla is not None or centre is not None):
        raise ValueError("with_lo needs precision=Precision.DD")
    lib = _native.load()
    family, pre, _keep = _deep_call(precision, pos_lo, centre, bla, scaled=scaled)
    zw = 2
    if family == "scaled":
        fn = lib.fr_escape_rows_pt_scaled
    elif family == "bla":
        fn = lib.fr_escape_rows_pt_bla
    elif family == "wide":
        fn = lib.fr_escape_rows_pt_wide
    elif family == "lo" and not with_lo and int(precision) == Precision.PT:
        fn = lib.fr_escape_rows_pt
    elif family == "lo" or with_lo:
        _dd_only(precision)
        fn, pre, zw = lib.fr_escape_rows_dd, pre or (None,), 4
    else:
        fn, pre = lib.fr_escape_rows, (int(precision),)
    z = np.empty((y1 - y0, config.width, zw), dtype=np.float64)
    it = np.empty((y1 - y0, config.width), dtype=np.uint32)
    _native.check(fn(C.byref(config), *pre, y0, y1, z.ctypes.data, it.ctypes.data))
    return (z if zw == 2 or with_lo else np.ascontiguousarray(z[..., 0::2])), it


def _stream(stream):
    """a hipStream_t handle as an int (None = the null stream) -> void pointer for the C call"""
    return C.c_void_p(int(stream)) if stream else None


def _rows(config, y0, y1):
    return int(y0), int(config.height if y1 is None else y1)


def _lo(pos_lo):
    """pos_lo argument -> (pointer for the C call, keep-alive); None = (0, 0), the C NULL"""
    _, pre, keep = _deep_call(Precision.DD, pos_lo)
    return (pre or (None,))[0], keep


def _pt_state_fn(name, device, pos_lo, centre, scaled=False):
    """the PT state call `name` ("fr_escape_rows_pt%s_state" / "fr_escape_extend_pt%s"; %s: "_wide" with a centre, "_scaled"
    with a centre and scaled=True) in its host or device form, with its centre argument and what keeps it alive"""
    family, pre, keep = _deep_call(Precision.PT, pos_lo, centre, scaled=scaled)
    infix = {"wide": "_wide", "scaled": "_scaled"}.get(family, "")  # the scaled state calls take no bits: pre[0] alone
    fn = getattr(_native.load(), name % infix + ("_device" if device else ""))
    return fn, (pre or (None,))[0], keep


def escape_rows_device(config, z_ptr, iters_ptr, y0=0, y1=None, precision=Precision.F64, pos_lo=None, z_width=2, stream=None,
                       opts=None):
    """fr_escape_rows_device: recursive() results of rows [y0, y1) into DEVICE arrays, asynchronously on `stream`.
    z_ptr / iters_ptr: raw device pointers as ints (either may be 0 / None) to z_width float64 and one uint32 per pixel;
    z_width=4 (Precision.DD only) keeps the low parts.  This is the state a GUI keeps per view: 20 bytes per pixel, 36 for
    DD with its low parts."""
    y0, y1 = _rows(config, y0, y1)
    lo, _keep = _lo(pos_lo)
    _native.check(_native.load().fr_escape_rows_device(C.byref(config), int(precision), lo, y0, y1, int(z_width), z_ptr or None,
                                                       iters_ptr or None, _stream(stream), C.byref(opts) if opts is not None else None))


def extend_rows_device(config, z_ptr, iters_ptr, from_iterations, y0=0, y1=None, precision=Precision.F64, pos_lo=None, z_width=2,
                       stream=None, opts=None):
    """fr_escape_extend_device: raise the cap of the stored results of rows [y0, y1) from `from_iterations` to
    config.iterations IN PLACE, asynchronously on `stream`.  The arrays must hold what escape_rows_device wrote for the same
    view at the lower cap (the library cannot check that); afterwards they hold the render at config.iterations, bit for
    bit.  Precision.DD needs z_width=4; Precision.PT is refused."""
    y0, y1 = _rows(config, y0, y1)
    lo, _keep = _lo(pos_lo)
    _native.check(_native.load().fr_escape_extend_device(C.byref(config), int(precision), lo, y0, y1, int(from_iterations),
                                                         int(z_width), z_ptr or None, iters_ptr or None, _stream(stream),
                                                         C.byref(opts) if opts is not None else None))


def extend_rows(config, z, iters, from_iterations, precision=Precision.F64, pos_lo=None, y0=0, y1=None):
    """fr_escape_extend over numpy arrays: z float64 [rows, width, 2] ([rows, width, 4] for Precision.DD) and iters uint32
    [rows, width] as escape_rows returned them at the cap `from_iterations` -> the same pair at config.iterations (copies;
    the arguments are left alone)."""
    y0, y1 = _rows(config, y0, y1)
    zw = 4 if int(precision) == Precision.DD else 2
    z = np.array(z, dtype=np.float64, order="C")
    iters = np.array(iters, dtype=np.uint32, order="C")
    shape = (max(y1 - y0, 0), config.width)
    if z.shape != shape + (zw,) or iters.shape != shape:
        raise ValueError("z must be [rows, width, %d] and iters [rows, width] for rows [y0, y1)" % zw)
    lo, _keep = _lo(pos_lo)
    _native.check(_native.load().fr_escape_extend(C.byref(config), int(precision), lo, y0, y1, int(from_iterations), zw,
                                                  z.ctypes.data, iters.ctypes.data))
    return z, iters


def escape_rows_pt_state(config, pos_lo=None, y0=0, y1=None, centre=None, scaled=False):
    """fr_escape_rows_pt_state: rows [y0, y1) in Precision.PT with their resumable state: (z float64 [rows, width, 2], iters
    uint32 [rows, width], dz float64 [rows, width, 2], m uint32 [rows, width]; bit 31 of m: a Julia pixel on K).  z and iters
    are escape_rows' for Precision.PT, bit for bit (include/fractal_hip.h, "RESUMABLE PT").
    scaled=True (needs centre=): fr_escape_rows_pt_scaled_state, the state of SCALED PT's plain loop for views past 2^440;
    the third array then holds w = dz 2^e, not dz ("RESUMABLE SCALED PT"), and only the scaled extension continues it."""
    y0, y1 = _rows(config, y0, y1)
    shape = (max(y1 - y0, 0), config.width)
    z, dz = np.empty(shape + (2,), dtype=np.float64), np.empty(shape + (2,), dtype=np.float64)
    it, m = np.empty(shape, dtype=np.uint32), np.empty(shape, dtype=np.uint32)
    fn, where, _keep = _pt_state_fn("fr_escape_rows_pt%s_state", False, pos_lo, centre, scaled)
    _native.check(fn(C.byref(config), where, y0, y1, z.ctypes.data, it.ctypes.data, dz.ctypes.data, m.ctypes.data))
    return z, it, dz, m


def extend_rows_pt(config, z, iters, dz, m, from_iterations, pos_lo=None, y0=0, y1=None, centre=None, scaled=False):
    """fr_escape_extend_pt over numpy arrays: the state escape_rows_pt_state returned at the cap `from_iterations` -> the
    state at config.iterations (copies; the arguments are left alone).  The arrays must be that view's; the library cannot
    check it.  scaled=True (needs centre=): fr_escape_extend_pt_scaled, on a state that escape_rows_pt_state(scaled=True)
    returned (dz is its w)."""
    y0, y1 = _rows(config, y0, y1)
    shape = (max(y1 - y0, 0), config.width)
    z, dz = np.array(z, dtype=np.float64, order="C"), np.array(dz, dtype=np.float64, order="C")
    iters, m = np.array(iters, dtype=np.uint32, order="C"), np.array(m, dtype=np.uint32, order="C")
    if z.shape != shape + (2,) or dz.shape != shape + (2,) or iters.shape != shape or m.shape != shape:
        raise ValueError("z and dz must be [rows, width, 2], iters and m [rows, width] for rows [y0, y1)")
    fn, where, _keep = _pt_state_fn("fr_escape_extend_pt%s", False, pos_lo, centre, scaled)
    _native.check(fn(C.byref(config), where, y0, y1, int(from_iterations), z.ctypes.data, iters.ctypes.data, dz.ctypes.data,
                     m.ctypes.data))
    return z, iters, dz, m


def escape_rows_pt_state_device(config, z_ptr, iters_ptr, dz_ptr, m_ptr, y0=0, y1=None, pos_lo=None, stream=None, centre=None,
                                scaled=False):
    """fr_escape_rows_pt_state_device: the Precision.PT state of rows [y0, y1) into DEVICE arrays (raw pointers as ints:
    z, dz 2 float64 per pixel, iters, m one uint32), asynchronously on `stream`: 40 bytes per pixel.  scaled=True (needs
    centre=): fr_escape_rows_pt_scaled_state_device; dz_ptr then receives w."""
    y0, y1 = _rows(config, y0, y1)
    fn, where, _keep = _pt_state_fn("fr_escape_rows_pt%s_state", True, pos_lo, centre, scaled)
    _native.check(fn(C.byref(config), where, y0, y1, z_ptr or None, iters_ptr or None, dz_ptr or None, m_ptr or None, _stream(stream)))


def extend_rows_pt_device(config, z_ptr, iters_ptr, dz_ptr, m_ptr, from_iterations, y0=0, y1=None, pos_lo=None, stream=None,
                          centre=None, scaled=False):
    """fr_escape_extend_pt_device: raise the cap of the stored Precision.PT state of rows [y0, y1) from `from_iterations` to
    config.iterations IN PLACE, asynchronously on `stream`; the view's reference orbit is continued, not recomputed.
    scaled=True (needs centre=): fr_escape_extend_pt_scaled_device, on a state the scaled state render wrote."""
    y0, y1 = _rows(config, y0, y1)
    fn, where, _keep = _pt_state_fn("fr_escape_extend_pt%s", True, pos_lo, centre, scaled)
    _native.check(fn(C.byref(config), where, y0, y1, int(from_iterations), z_ptr or None, iters_ptr or None, dz_ptr or None,
                     m_ptr or None, _stream(stream)))


def pt_orbit_cache():
    """fr_debug_pt_orbit_cache: (iterations the cached PT orbit is for, entries of X, entries of K, entries the last request
    computed on the host)."""
    out = (C.c_uint32 * 4)()
    _native.check(_native.load().fr_debug_pt_orbit_cache(out))
    return tuple(out)


def colour_rows_device(config, z_ptr, iters_ptr, n, out_ptr, channels=3, z_width=2, stream=None):
    """fr_colour_rows_device: the colour map alone over n stored results in DEVICE memory into channels * n bytes at out_ptr
    (3: r,g,b; 4: r,g,b,255, 4-byte aligned), asynchronously on `stream`.  z_width=4 colours DD results on their hi parts."""
    n = int(n)
    _native.check(_native.load().fr_colour_rows_device(C.byref(config), z_ptr or None, int(z_width), iters_ptr or None, n,
                                                       int(channels), out_ptr or None, int(channels) * n, _stream(stream)))


def colour_rows_ss_device(config, z_ptr, iters_ptr, width, rows, supersample, out_ptr, channels=3, z_width=2, stream=None, transfer=0):
    """fr_colour_rows_ss_device: colour map + box filter in one kernel over a KEPT anti-aliased view — the stored results of
    supersample * rows rows of supersample * width samples in DEVICE memory (what the escape_rows*_device calls write for the
    config with width and height times supersample) — into channels * width * rows bytes at out_ptr, asynchronously on
    `stream`.  The bytes are colour_rows_device's followed by the box filter's; no RGB workspace in between. transfer: see box_filter."""
    width, rows, s = int(width), int(rows), int(supersample)
    if not 1 <= s <= SS_MAX:
        raise ValueError("supersample is 1 .. %d" % SS_MAX)
    if int(z_width) not in (2, 4):
        raise ValueError("z_width is 2 or 4")
    if int(channels) not in (3, 4):
        raise ValueError("channels is 3 or 4")
    _native.check(_native.load().fr_colour_rows_ss_tf_device(C.byref(config), z_ptr or None, int(z_width), iters_ptr or None, width, rows,
                                                             s, int(transfer), int(channels), out_ptr or None,
                                                             int(channels) * width * rows, _stream(stream)))


def colour_image_ss(config, z, iters, supersample, channels=3, transfer=0):
    """fr_colour_ss_rgb8 over numpy arrays: z float64 [s*rows, s*width, 2] (or [..., 4]: DD with its low parts, coloured on
    the hi parts) and iters uint32 [s*rows, s*width] -> uint8 [rows, width, channels], each pixel the box-filtered colours
    of its s x s samples: box_filter(colour_image(config, z, iters), s, transfer=transfer), byte for byte. transfer: see box_filter."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    iters = np.ascontiguousarray(iters, dtype=np.uint32)
    s = int(supersample)
    if not 1 <= s <= SS_MAX:
        raise ValueError("supersample is 1 .. %d" % SS_MAX)
    if int(channels) not in (3, 4):
        raise ValueError("channels is 3 or 4")
    if z.ndim != 3 or z.shape[:2] != iters.shape or z.shape[2] not in (2, 4) or iters.shape[0] % s or iters.shape[1] % s:
        raise ValueError("z must be [s*rows, s*width, 2 or 4] and iters [s*rows, s*width]")
    rows, width = iters.shape[0] // s, iters.shape[1] // s
    out = np.empty((rows, width, int(channels)), dtype=np.uint8)
    _native.check(_native.load().fr_colour_ss_rgb8_tf(C.byref(config), z.ctypes.data, z.shape[2], iters.ctypes.data, width, rows, s,
                                                      int(transfer), int(channels), out.ctypes.data, out.nbytes))
    return out


def colour_image(config, z, iters):
    """The colour map alone (calc/src/lib.rs:214-234) over stored recursive() results: z float64
    [..., 2], iters uint32 [...] -> uint8 [..., 3].  Re-colouring (exposure, colours, smooth, inside)
    without re-iterating."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    iters = np.ascontiguousarray(iters, dtype=np.uint32)
    if z.shape[:-1] != iters.shape or z.shape[-1] != 2:
        raise ValueError("z must be [..., 2] and iters [...]")
    out = np.empty(iters.shape + (3,), dtype=np.uint8)
    _native.check(
        _native.load().fr_colour_rgb8(C.byref(config), z.ctypes.data, iters.ctypes.data, iters.size, out.ctypes.data,
                                      out.nbytes)
    )
    return out


class ViewStats(_native.fr_view_stats):
    """fr_view_stats (include/fractal_hip.h, "statistics of a kept view"): n, stable, capped, escaped, sum_iters, min_iters,
    max_iters, shift, and hist, the 1024 bins of the escape indices of the escaped pixels."""

    def histogram(self):
        """hist as a numpy uint64 [1024] (a copy)"""
        return np.frombuffer(self.hist, dtype=np.uint64).copy()

    @classmethod
    def from_bytes(cls, raw):
        """the record a device buffer held, e.g. the 8248 bytes view_stats_device wrote"""
        return cls.from_buffer_copy(bytes(raw))


def view_stats(config, z, iters):
    """fr_view_stats over numpy arrays: z float64 [..., 2] (or [..., 4]: DD with its low parts, read on the hi parts) and
    iters uint32 [...] -> ViewStats, reduced on the device; 8 KB come back.  Only config.iterations and config.stable_limit
    are read."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    iters = np.ascontiguousarray(iters, dtype=np.uint32)
    if z.ndim < 1 or z.shape[:-1] != iters.shape or z.shape[-1] not in (2, 4):
        raise ValueError("z must be [..., 2 or 4] and iters [...]")
    st = ViewStats()
    _native.check(_native.load().fr_view_stats(C.byref(config), z.ctypes.data if iters.size else None, z.shape[-1],
                                               iters.ctypes.data if iters.size else None, iters.size, C.byref(st)))
    return st


def view_stats_device(config, z_ptr, iters_ptr, n, stats_ptr, z_width=2, stream=None):
    """fr_view_stats_device: the statistics of n stored results in DEVICE memory into the 8248 bytes at stats_ptr (device
    memory, 8-byte aligned, overwritten whatever they held), asynchronously on `stream`; ViewStats.from_bytes reads them once
    they are on the host."""
    _native.check(_native.load().fr_view_stats_device(C.byref(config), z_ptr or None, int(z_width), iters_ptr or None, int(n),
                                                      stats_ptr or None, _stream(stream)))


def stats_percentile(stats, p):
    """fr_stats_percentile (host only): the escape index at quantile p in [0, 1] of the escaped pixels; 0 when none escaped"""
    out = C.c_uint32(0)
    _native.check(_native.load().fr_stats_percentile(C.byref(stats), float(p), C.byref(out)))
    return out.value


def auto_exposure(config, stats, percentile=0.99):
    """fr_auto_exposure (host only): the exposure at which an escaped pixel at that percentile of the escape indices gets the
    full primary colour, config.iterations / max(percentile index, 1); config.exposure when no pixel escaped.  0.99 is a
    presentation default — a lone pixel beside a minibrot should not darken the frame; 1.0 takes the maximum."""
    out = C.c_double(0.0)
    _native.check(_native.load().fr_auto_exposure(C.byref(config), C.byref(stats), float(percentile), C.byref(out)))
    return out.value


def get_image_auto(config, percentile=0.99, precision=Precision.F64, pos_lo=None, centre=None, bla=None, scaled=False, supersample=1,
                   transfer=0):
    """get_image at the exposure the view's own escape indices call for: (uint8 [height, width, 3], exposure).  escape_rows
    on the road the keywords select (of the supersample times larger config when supersample > 1), view_stats over the
    result, auto_exposure, then colour_image / colour_image_ss with config's clone carrying that exposure: the reference's
    colour map, byte for byte the render of that clone.  config itself is left alone.  transfer: see box_filter (the
    statistics are the samples', whichever way they are averaged)."""
    transfer = _check_transfer(transfer)
    s = int(supersample)
    if not 1 <= s <= SS_MAX:
        raise ValueError("supersample is 1 .. %d" % SS_MAX)
    big = config.clone()
    big.width, big.height = config.width * s, config.height * s
    z, it = escape_rows(big, precision=precision, pos_lo=pos_lo, centre=centre, bla=bla, scaled=scaled)
    exposure = auto_exposure(config, view_stats(big, z, it), percentile)
    shown = config.clone()
    shown.exposure = exposure
    image = colour_image(shown, z, it) if s == 1 else colour_image_ss(shown, z, it, s, transfer=transfer)
    return image, exposure


def _de_call(precision, pos_lo, centre, device, bla=None, opts=None, scaled=False):
    """the DE render the keywords select, in its host or device form: (function, leading arguments behind the config, keep-alive)"""
    suffix = "_device" if device else ""
    lib = _native.load()
    if scaled:  # DE ON SCALED PT; _deep_call's checks: centre=, Precision.PT, no pos_lo, no opts, the bits of bla=
        _family, pre, keep = _deep_call(precision, pos_lo, centre, bla=bla, opts=opts, scaled=True)
        return getattr(lib, "fr_escape_rows_de_pt_scaled" + suffix), pre, keep
    if bla is not None:  # DE ON BLA-PT; _deep_call's checks: Precision.PT, no opts, the bits, no pos_lo beside a centre
        _family, pre, keep = _deep_call(precision, pos_lo, centre, bla=bla, opts=opts)
        return getattr(lib, "fr_escape_rows_de_pt_bla" + suffix), pre, keep
    if opts is not None:
        raise ValueError("opts= goes with bla= only, which refuses it: a DE render has one kernel per road")
    if centre is not None:
        family, pre, keep = _deep_call(precision, pos_lo, centre)  # its checks: Precision.PT, no pos_lo
        return getattr(lib, "fr_escape_rows_de_pt_wide" + suffix), pre, keep
    lo, keep = _lo(pos_lo)
    return getattr(lib, "fr_escape_rows_de" + suffix), (int(precision), lo), keep


def escape_rows_de(config, y0=0, y1=None, precision=Precision.F64, pos_lo=None, centre=None, bla=None, opts=None, scaled=False):
    """fr_escape_rows_de / fr_escape_rows_de_pt_wide: rows [y0, y1) with the orbit's derivative (include/fractal_hip.h, "DE"):
    (z float64 [rows, width, 2], iters uint32 [rows, width], der float64 [rows, width, 2]).  z and iters are the road's own,
    bit for bit; der is the derivative of the returned position (d/dc for Mandelbrot, d/dz0 for Julia).  precision is
    Precision.F64 or Precision.PT (pos_lo= or centre=, a WideCentre, as escape_rows takes them); everything else is refused.
    bla= (None: off; 0: the default bits; 24 .. 53; needs Precision.PT and takes no opts, as bla= does elsewhere): DE ON BLA-PT,
    fr_escape_rows_de_pt_bla — z and iters are escape_rows(..., bla=)'s bit for bit, der goes through the table's skips.
    scaled=True (needs centre= and Precision.PT; combines with bla=; no pos_lo, no opts): DE ON SCALED PT,
    fr_escape_rows_de_pt_scaled, for views past 2^440 — der then holds the SCALED derivative u = d 2^-e, and the distance and the
    shading are taken on de_scaled_view(config)."""
    y0, y1 = _rows(config, y0, y1)
    fn, pre, _keep = _de_call(precision, pos_lo, centre, False, bla, opts, scaled)
    z = np.empty((y1 - y0, config.width, 2), dtype=np.float64)
    it = np.empty((y1 - y0, config.width), dtype=np.uint32)
    der = np.empty((y1 - y0, config.width, 2), dtype=np.float64)
    _native.check(fn(C.byref(config), *pre, y0, y1, z.ctypes.data, it.ctypes.data, der.ctypes.data))
    return z, it, der


def escape_rows_de_device(config, z_ptr, iters_ptr, der_ptr, y0=0, y1=None, precision=Precision.F64, pos_lo=None, centre=None,
                          stream=None, bla=None, opts=None, scaled=False):
    """fr_escape_rows_de_device / fr_escape_rows_de_pt_wide_device / fr_escape_rows_de_pt_bla_device (bla=, as escape_rows_de takes
    it) / fr_escape_rows_de_pt_scaled_device (scaled=True, as there): the same into DEVICE arrays (raw pointers as ints, all three
    required), asynchronously on `stream`: the 36 bytes per pixel a GUI keeps to vary thickness without an orbit."""
    y0, y1 = _rows(config, y0, y1)
    fn, pre, _keep = _de_call(precision, pos_lo, centre, True, bla, opts, scaled)
    _native.check(fn(C.byref(config), *pre, y0, y1, z_ptr or None, iters_ptr or None, der_ptr or None, _stream(stream)))


def _de_state_call(name, pos_lo, centre, device):
    """a PT call of RESUMABLE DE in its host or device form: (function, pos_lo pointer, centre pointer, keep-alive).  pos_lo= and
    centre= are exclusive, as everywhere (ValueError)."""
    fn = getattr(_native.load(), name + ("_device" if device else ""))
    if centre is not None:
        _family, pre, keep = _deep_call(Precision.PT, pos_lo, centre)  # its checks: no pos_lo beside a centre
        return fn, None, pre[0], keep
    lo, keep = _lo(pos_lo)
    return fn, lo, None, keep


def _de_state_arrays(config, y0, y1, z, iters, dz, m, der):
    shape = (max(y1 - y0, 0), config.width)
    z, dz, der = (np.array(a, dtype=np.float64, order="C") for a in (z, dz, der))
    iters, m = np.array(iters, dtype=np.uint32, order="C"), np.array(m, dtype=np.uint32, order="C")
    if any(a.shape != shape + (2,) for a in (z, dz, der)) or iters.shape != shape or m.shape != shape:
        raise ValueError("z, dz and der must be [rows, width, 2], iters and m [rows, width] for rows [y0, y1)")
    return z, iters, dz, m, der


def extend_rows_de(config, z, iters, der, from_iterations, precision=Precision.F64, y0=0, y1=None):
    """fr_escape_extend_de over numpy arrays: (z, iters, der) as escape_rows_de returned them on the F64 road at the cap
    `from_iterations` -> the same triple at config.iterations, bit for bit what escape_rows_de gives there (copies; the arguments
    are left alone).  Precision.PT is refused: its state has five arrays (escape_rows_de_pt_state, extend_rows_de_pt)."""
    y0, y1 = _rows(config, y0, y1)
    shape = (max(y1 - y0, 0), config.width)
    z, der = np.array(z, dtype=np.float64, order="C"), np.array(der, dtype=np.float64, order="C")
    iters = np.array(iters, dtype=np.uint32, order="C")
    if z.shape != shape + (2,) or der.shape != shape + (2,) or iters.shape != shape:
        raise ValueError("z and der must be [rows, width, 2] and iters [rows, width] for rows [y0, y1)")
    _native.check(_native.load().fr_escape_extend_de(C.byref(config), int(precision), y0, y1, int(from_iterations), z.ctypes.data,
                                                     iters.ctypes.data, der.ctypes.data))
    return z, iters, der


def extend_rows_de_device(config, z_ptr, iters_ptr, der_ptr, from_iterations, precision=Precision.F64, y0=0, y1=None, stream=None):
    """fr_escape_extend_de_device: raise the cap of the F64 road's stored (z, iters, der) of rows [y0, y1) from `from_iterations`
    to config.iterations IN PLACE, asynchronously on `stream` (raw device pointers as ints)."""
    y0, y1 = _rows(config, y0, y1)
    _native.check(_native.load().fr_escape_extend_de_device(C.byref(config), int(precision), y0, y1, int(from_iterations), z_ptr or None,
                                                            iters_ptr or None, der_ptr or None, _stream(stream)))


def escape_rows_de_pt_state(config, pos_lo=None, centre=None, y0=0, y1=None):
    """fr_escape_rows_de_pt_state: rows [y0, y1) in Precision.PT with their resumable DE state (include/fractal_hip.h, "RESUMABLE
    DE"): (z float64 [rows, width, 2], iters uint32 [rows, width], dz float64 [rows, width, 2], m uint32 [rows, width], der
    float64 [rows, width, 2]).  z, iters, der are escape_rows_de's, dz and m escape_rows_pt_state's.  pos_lo= or centre= (a
    WideCentre), not both."""
    y0, y1 = _rows(config, y0, y1)
    fn, lo, wide, _keep = _de_state_call("fr_escape_rows_de_pt_state", pos_lo, centre, False)
    shape = (max(y1 - y0, 0), config.width)
    z, dz, der = (np.empty(shape + (2,), dtype=np.float64) for _ in range(3))
    it, m = np.empty(shape, dtype=np.uint32), np.empty(shape, dtype=np.uint32)
    _native.check(fn(C.byref(config), lo, wide, y0, y1, z.ctypes.data, it.ctypes.data, dz.ctypes.data, m.ctypes.data, der.ctypes.data))
    return z, it, dz, m, der


def escape_rows_de_pt_state_device(config, z_ptr, iters_ptr, dz_ptr, m_ptr, der_ptr, pos_lo=None, centre=None, y0=0, y1=None,
                                   stream=None):
    """fr_escape_rows_de_pt_state_device: the same into DEVICE arrays (raw pointers as ints, all five required), asynchronously on
    `stream`: the 56 bytes per pixel a GUI keeps to vary thickness AND the cap without rendering again."""
    y0, y1 = _rows(config, y0, y1)
    fn, lo, wide, _keep = _de_state_call("fr_escape_rows_de_pt_state", pos_lo, centre, True)
    _native.check(fn(C.byref(config), lo, wide, y0, y1, z_ptr or None, iters_ptr or None, dz_ptr or None, m_ptr or None, der_ptr or None,
                     _stream(stream)))


def extend_rows_de_pt(config, z, iters, dz, m, der, from_iterations, pos_lo=None, centre=None, y0=0, y1=None):
    """fr_escape_extend_de_pt over numpy arrays: the state escape_rows_de_pt_state returned at the cap `from_iterations` -> the
    state at config.iterations (copies; the arguments are left alone).  The arrays must be that view's; the library cannot check
    it."""
    y0, y1 = _rows(config, y0, y1)
    z, iters, dz, m, der = _de_state_arrays(config, y0, y1, z, iters, dz, m, der)
    fn, lo, wide, _keep = _de_state_call("fr_escape_extend_de_pt", pos_lo, centre, False)
    _native.check(fn(C.byref(config), lo, wide, y0, y1, int(from_iterations), z.ctypes.data, iters.ctypes.data, dz.ctypes.data,
                     m.ctypes.data, der.ctypes.data))
    return z, iters, dz, m, der


def extend_rows_de_pt_device(config, z_ptr, iters_ptr, dz_ptr, m_ptr, der_ptr, from_iterations, pos_lo=None, centre=None, y0=0,
                             y1=None, stream=None):
    """fr_escape_extend_de_pt_device: raise the cap of the stored DE state of rows [y0, y1) from `from_iterations` to
    config.iterations IN PLACE, asynchronously on `stream`; the view's reference orbit is continued, not recomputed."""
    y0, y1 = _rows(config, y0, y1)
    fn, lo, wide, _keep = _de_state_call("fr_escape_extend_de_pt", pos_lo, centre, True)
    _native.check(fn(C.byref(config), lo, wide, y0, y1, int(from_iterations), z_ptr or None, iters_ptr or None, dz_ptr or None,
                     m_ptr or None, der_ptr or None, _stream(stream)))


def _de_arrays(z, iters, der):
    z = np.ascontiguousarray(z, dtype=np.float64)
    iters = np.ascontiguousarray(iters, dtype=np.uint32)
    der = np.ascontiguousarray(der, dtype=np.float64)
    if z.shape[:-1] != iters.shape or z.shape[-1] != 2 or der.shape != z.shape:
        raise ValueError("z and der must be [..., 2] and iters [...]")
    return z, iters, der


def distance_rows(config, z, iters, der):
    """fr_distance_rows over numpy arrays: the exterior distance estimate |z| ln|z| / |z'| in PIXELS, float64 [...]; 0 for a
    capped pixel and where the derivative overflowed, +inf where it is 0.  Only height, scale and iterations are read."""
    z, iters, der = _de_arrays(z, iters, der)
    out = np.empty(iters.shape, dtype=np.float64)
    _native.check(_native.load().fr_distance_rows(C.byref(config), z.ctypes.data, iters.ctypes.data, der.ctypes.data, iters.size,
                                                  out.ctypes.data))
    return out


def distance_rows_device(config, z_ptr, iters_ptr, der_ptr, n, out_ptr, stream=None):
    """fr_distance_rows_device: D of n stored results in DEVICE memory into n float64 at out_ptr, asynchronously on `stream`"""
    _native.check(_native.load().fr_distance_rows_device(C.byref(config), z_ptr or None, iters_ptr or None, der_ptr or None, int(n),
                                                         out_ptr or None, _stream(stream)))


def colour_image_de(config, z, iters, der, thickness):
    """fr_colour_de_rgb8 over numpy arrays -> uint8 [..., 3]: colour_image's bytes, and where an escaped pixel lies closer than
    `thickness` pixels to the set every byte times distance / thickness, truncated.  thickness 0 is colour_image."""
    z, iters, der = _de_arrays(z, iters, der)
    out = np.empty(iters.shape + (3,), dtype=np.uint8)
    _native.check(_native.load().fr_colour_de_rgb8(C.byref(config), z.ctypes.data, iters.ctypes.data, der.ctypes.data, iters.size,
                                                   float(thickness), out.ctypes.data, out.nbytes))
    return out


def colour_de_rows_device(config, z_ptr, iters_ptr, der_ptr, n, thickness, out_ptr, channels=3, stream=None):
    """fr_colour_de_rows_device: the shaded colour map over n stored results in DEVICE memory into channels * n bytes at out_ptr
    (3: r,g,b at any alignment; 4: r,g,b,255, 4-byte aligned), asynchronously on `stream`."""
    _native.check(_native.load().fr_colour_de_rows_device(C.byref(config), z_ptr or None, iters_ptr or None, der_ptr or None, int(n),
                                                          float(thickness), int(channels), out_ptr or None, _stream(stream)))


def de_scaled_view(config):
    """fr_de_scaled_view: the scaled view cfg_v of DE ON SCALED PT, a copy of `config` with scale = (sre, sim) = scale 2^-e; the
    distance and the shading of escape_rows_de(..., scaled=True)'s arrays are distance_rows / colour_image_de on it.  Host only."""
    view = Config.from_buffer_copy(bytes(config))
    _native.check(_native.load().fr_de_scaled_view(C.byref(config), C.byref(view)))
    return view


def get_image_de(config, thickness=1.0, precision=Precision.F64, pos_lo=None, centre=None, bla=None, opts=None, supersample=1, y0=0,
                 y1=None, channels=3, scaled=False, transfer=0):
    """get_image with distance shading: uint8 [height, width, 3].  escape_rows_de on the road the keywords select (bla=: DE ON
    BLA-PT), then colour_image_de: filaments thinner than a pixel stay visible as dark lines `thickness` pixels wide.
    supersample = s > 1, a row range y0= / y1= or channels=4: fr_render_rows_ss_de (include/fractal_hip.h, "SUPERSAMPLED DE") —
    rows [y0, y1) with s x s samples per pixel, each shaded with the thickness thickness * s in sample pixels (the line stays
    `thickness` OUTPUT pixels wide) and box-filtered on the device, uint8 [y1-y0, width, channels]; the s times larger DE arrays
    exist only a band at a time.  supersample = 1 gives the bytes of the call without it.  transfer: see box_filter; the
    shade stays on the sample's bytes, before the filter.
    scaled=True (needs centre=; combines with bla=): DE ON SCALED PT — escape_rows_de(..., scaled=True), then colour_image_de on
    de_scaled_view(config); the whole image at one sample per pixel and 3 channels only."""
    transfer = _check_transfer(transfer)
    s = int(supersample)
    if not 1 <= s <= SS_MAX:
        raise ValueError("supersample is 1 .. %d" % SS_MAX)
    if int(channels) not in (3, 4):
        raise ValueError("channels is 3 or 4")
    if scaled:
        if s != 1 or y0 != 0 or y1 is not None or int(channels) != 3:
            raise ValueError("scaled=True: supersample > 1, a row range and channels=4 are out of scope of DE ON SCALED PT "
                             "(fr_render_rows_ss_de refuses FR_PT_ROAD_SCALED); get_image_de_scaled_ss renders them")
        z, it, der = escape_rows_de(config, precision=precision, pos_lo=pos_lo, centre=centre, bla=bla, opts=opts, scaled=True)
        return colour_image_de(de_scaled_view(config), z, it, der, thickness)
    if s == 1 and y0 == 0 and y1 is None and int(channels) == 3:
        z, it, der = escape_rows_de(config, precision=precision, pos_lo=pos_lo, centre=centre, bla=bla, opts=opts)
        return colour_image_de(config, z, it, der, thickness)
    if opts is not None:
        raise ValueError("a DE render takes no opts: it has one kernel per road")
    road, bits = _ss_pt_road(pos_lo, centre, bla, False)
    if (centre is not None or bla is not None) and int(precision) != Precision.PT:
        raise ValueError("centre= and bla= need precision=Precision.PT")
    y0, y1 = _rows(config, y0, y1)
    out = np.empty((max(y1 - y0, 0), config.width, int(channels)), dtype=np.uint8)
    lo = None if pos_lo is None else Imaginary(*(float(v) for v in pos_lo))
    st = None if centre is None else centre.c_struct()
    _native.check(_native.load().fr_render_rows_ss_de_tf(C.byref(config), int(precision), None if lo is None else C.byref(lo),
                                                         None if st is None else C.byref(st), road, bits, float(thickness), s, transfer,
                                                         y0, y1, int(channels), out.ctypes.data, out.nbytes))
    return out


def _scaled_centre(centre):
    if centre is None:
        raise ValueError("the scaled calls need centre= (a WideCentre)")
    return centre.c_struct()


def escape_rows_de_pt_scaled_state(config, centre, y0=0, y1=None):
    """fr_escape_rows_de_pt_scaled_state: rows [y0, y1) on SCALED PT's plain loop with their resumable DE state
    (include/fractal_hip.h, "RESUMABLE SCALED DE"): (z float64 [rows, width, 2], iters uint32 [rows, width], w float64 [rows,
    width, 2], m uint32 [rows, width], der float64 [rows, width, 2] holding u = d 2^-e).  z, iters, der are
    escape_rows_de(..., scaled=True)'s, w and m escape_rows_pt_state(..., scaled=True)'s.  centre: a WideCentre, required."""
    st = _scaled_centre(centre)
    y0, y1 = _rows(config, y0, y1)
    shape = (max(y1 - y0, 0), config.width)
    z, w, der = (np.empty(shape + (2,), dtype=np.float64) for _ in range(3))
    it, m = np.empty(shape, dtype=np.uint32), np.empty(shape, dtype=np.uint32)
    _native.check(_native.load().fr_escape_rows_de_pt_scaled_state(C.byref(config), C.byref(st), y0, y1, z.ctypes.data, it.ctypes.data,
                                                                   w.ctypes.data, m.ctypes.data, der.ctypes.data))
    return z, it, w, m, der


def extend_rows_de_pt_scaled(config, z, iters, w, m, der, from_iterations, centre, y0=0, y1=None):
    """fr_escape_extend_de_pt_scaled over numpy arrays: the state escape_rows_de_pt_scaled_state returned at the cap
    `from_iterations` -> the state at config.iterations (copies; the arguments are left alone).  The arrays must be that view's;
    the library cannot check it."""
    st = _scaled_centre(centre)
    y0, y1 = _rows(config, y0, y1)
    z, iters, w, m, der = _de_state_arrays(config, y0, y1, z, iters, w, m, der)
    _native.check(_native.load().fr_escape_extend_de_pt_scaled(C.byref(config), C.byref(st), y0, y1, int(from_iterations), z.ctypes.data,
                                                               iters.ctypes.data, w.ctypes.data, m.ctypes.data, der.ctypes.data))
    return z, iters, w, m, der


def get_image_de_scaled_ss(config, thickness, centre, supersample, bla=None, y0=0, y1=None, channels=3, transfer=0):
    """fr_render_rows_ss_de_pt_scaled (include/fractal_hip.h, "SUPERSAMPLED SCALED DE"): rows [y0, y1) of the distance-shaded image
    past a scale of 2^440 with supersample x supersample samples per pixel — escape_rows_de(..., scaled=True) on the s times larger
    image a band at a time, shaded on its scaled view with thickness * s in sample pixels and box-filtered on the device — as uint8
    [y1-y0, width, channels].  centre: a WideCentre, required; bla: None (the plain scaled loop), 0 or 24 .. 53. transfer: see box_filter."""
    s = int(supersample)
    if not 1 <= s <= SS_MAX:
        raise ValueError("supersample is 1 .. %d" % SS_MAX)
    if int(channels) not in (3, 4):
        raise ValueError("channels is 3 or 4")
    _road, bits = _ss_pt_road(None, centre, bla, True)
    st = centre.c_struct()
    y0, y1 = _rows(config, y0, y1)
    out = np.empty((max(y1 - y0, 0), config.width, int(channels)), dtype=np.uint8)
    _native.check(_native.load().fr_render_rows_ss_de_pt_scaled_tf(C.byref(config), C.byref(st), bits, float(thickness), s, int(transfer),
                                                                   y0, y1, int(channels), out.ctypes.data, out.nbytes))
    return out


def ss_de_workspace_bytes(config, supersample, y0=0, y1=None):
    """fr_ss_de_workspace_bytes: (min_bytes, best_bytes) of the device workspace fr_render_rows_ss_de_device wants for rows
    [y0, y1) — one band of 8 * supersample source rows at 36 bytes per sample, and the whole range (at most 1 GiB).  Unlike
    ss_workspace_bytes, supersample = 1 needs one too."""
    y1 = config.height if y1 is None else y1
    mn, best = C.c_size_t(0), C.c_size_t(0)
    _native.check(_native.load().fr_ss_de_workspace_bytes(C.byref(config), int(supersample), y0, y1, C.byref(mn), C.byref(best)))
    return mn.value, best.value


def _adaptive_road(precision, pos_lo, centre, bla, scaled):
    """The road arguments of the adaptive calls — (pos_lo pointer, centre pointer, road, bits) and what keeps their memory
    alive — from the keywords, resolved through _deep_call: its families are the roads"""
    if int(precision) not in (Precision.F64, Precision.PT):
        raise ValueError("adaptive supersampling takes precision=Precision.F64 or Precision.PT")
    family, pre, keep = _deep_call(precision, pos_lo, centre, bla, scaled=scaled)
    if int(precision) != Precision.PT and family != "plain":
        raise ValueError("pos_lo= needs precision=Precision.PT")
    if family == "scaled":
        return (None, pre[0], _native.FR_PT_ROAD_SCALED, pre[1]), keep
    if family == "bla":
        return (pre[0], pre[1], _native.FR_PT_ROAD_BLA, pre[2]), keep
    if family == "wide":
        return (None, pre[0], _native.FR_PT_ROAD_PLAIN, 0), keep
    if family == "lo":
        return (pre[0], None, _native.FR_PT_ROAD_PLAIN, 0), keep
    return (None, None, _native.FR_PT_ROAD_PLAIN, 0), keep


def ss_adaptive_workspace_bytes(config, supersample, y0=0, y1=None):
    """fr_ss_adaptive_workspace_bytes: the bytes of device workspace fr_render_rows_ss_adaptive_device wants for rows [y0, y1) —
    the probe colours of the rows and their two neighbours, the edge list and two counters; one size, no banding."""
    y1 = config.height if y1 is None else y1
    n = C.c_size_t(0)
    _native.check(_native.load().fr_ss_adaptive_workspace_bytes(C.byref(config), int(supersample), y0, y1, C.byref(n)))
    return n.value


def get_image_ss_adaptive(config, supersample, threshold=8, precision=Precision.F64, pos_lo=None, centre=None, bla=None, scaled=False,
                          y0=0, y1=None, channels=3, out=None, transfer=0):
    """Adaptive supersampling (fr_render_rows_ss_adaptive; include/fractal_hip.h, "ADAPTIVE SUPERSAMPLING"): rows [y0, y1) with
    supersample x supersample samples only at EDGE pixels — those whose probe sample differs from a neighbour's by more than
    `threshold` (0 .. 255; -1: every pixel, the bytes of the supersampled render; 255: none, the probe image) in some channel —
    and the probe sample everywhere else.  Returns (image uint8 [y1-y0, width, channels], refined: the number of edge pixels).
    precision is Precision.F64 or Precision.PT; pos_lo, centre, bla and scaled select the deep road as in get_image_rows.  A
    non-edge pixel's interior samples are never looked at: get_image_de is the tool for features thinner than a pixel.
    transfer: see box_filter; it changes the filter of the edge pixels only — the probe and the edge rule stay on the bytes."""
    s = int(supersample)
    if not 1 <= s <= SS_MAX:
        raise ValueError("supersample is 1 .. %d" % SS_MAX)
    if not -1 <= int(threshold) <= 255:
        raise ValueError("threshold is -1 .. 255")
    if int(channels) not in (3, 4):
        raise ValueError("channels is 3 or 4")
    (lo, ptr, road, bits), _keep = _adaptive_road(precision, pos_lo, centre, bla, scaled)
    y0, y1 = _rows(config, y0, y1)
    if out is None:
        out = np.empty((max(y1 - y0, 0), config.width, int(channels)), dtype=np.uint8)
    refined = C.c_uint64(0)
    _native.check(_native.load().fr_render_rows_ss_adaptive_tf(C.byref(config), int(precision), lo, ptr, road, bits, s, int(transfer),
                                                               int(threshold), y0, y1, int(channels), out.ctypes.data, out.nbytes,
                                                               C.byref(refined)))
    return out, refined.value


def ss_adaptive_de_workspace_bytes(config, supersample, y0=0, y1=None):
    """fr_ss_adaptive_de_workspace_bytes: the bytes of device workspace fr_render_rows_ss_adaptive_de_device wants for rows
    [y0, y1) — the probe's z, der, iters and colours of the rows and their two neighbours, the edge list and two counters; one
    size, no banding."""
    y1 = config.height if y1 is None else y1
    n = C.c_size_t(0)
    _native.check(_native.load().fr_ss_adaptive_de_workspace_bytes(C.byref(config), int(supersample), y0, y1, C.byref(n)))
    return n.value


def get_image_de_adaptive(config, thickness=1.0, supersample=2, threshold=8, reach=2.0, precision=Precision.F64, pos_lo=None, centre=None,
                          bla=None, y0=0, y1=None, channels=3, out=None, transfer=0):
    """Adaptive anti-aliased distance estimation (fr_render_rows_ss_adaptive_de; include/fractal_hip.h, "ADAPTIVE SUPERSAMPLED
    DE"): rows [y0, y1) of the distance-shaded image with supersample x supersample samples only at EDGE pixels — those whose
    shaded probe sample differs from a neighbour's by more than `threshold` in some channel (-1: every pixel, the bytes of
    get_image_de(..., supersample=s), which is the faster call for them) and those whose probe lies closer to the set than
    `reach` output pixels by its own distance estimate (0: the colour rule alone) — and the probe sample everywhere else.
    Returns (image uint8 [y1-y0, width, channels], refined: the number of edge pixels).  thickness is in output pixels.
    precision is Precision.F64 or Precision.PT; pos_lo, centre and bla select the deep road as in get_image_ss_adaptive; the
    scaled road is not offered.  transfer: see get_image_ss_adaptive."""
    s = int(supersample)
    if not 1 <= s <= SS_MAX:
        raise ValueError("supersample is 1 .. %d" % SS_MAX)
    if not -1 <= int(threshold) <= 255:
        raise ValueError("threshold is -1 .. 255")
    if int(channels) not in (3, 4):
        raise ValueError("channels is 3 or 4")
    (lo, ptr, road, bits), _keep = _adaptive_road(precision, pos_lo, centre, bla, False)
    y0, y1 = _rows(config, y0, y1)
    if out is None:
        out = np.empty((max(y1 - y0, 0), config.width, int(channels)), dtype=np.uint8)
    refined = C.c_uint64(0)
    _native.check(_native.load().fr_render_rows_ss_adaptive_de_tf(C.byref(config), int(precision), lo, ptr, road, bits, float(thickness), s,
                                                                  int(transfer), int(threshold), float(reach), y0, y1, int(channels),
                                                                  out.ctypes.data, out.nbytes, C.byref(refined)))
    return out, refined.value


def get_image_de_adaptive_scaled(config, thickness, centre, supersample=2, threshold=8, reach=2.0, bla=None, y0=0, y1=None, channels=3,
                                 out=None, transfer=0):
    """Adaptive anti-aliased distance estimation past a scale of 2^440 (fr_render_rows_ss_adaptive_de_pt_scaled;
    include/fractal_hip.h, "ADAPTIVE SUPERSAMPLED SCALED DE"): get_image_de_adaptive on SCALED PT's road, the probe and the samples
    those of get_image_de_scaled_ss.  Returns (image uint8 [y1-y0, width, channels], refined: the number of edge pixels).
    centre: a WideCentre, required; bla: None (the plain scaled loop), 0 or 24 .. 53; thickness and reach in output pixels;
    threshold -1 gives the bytes of get_image_de_scaled_ss, which is the faster call for them.  transfer: see
    get_image_ss_adaptive."""
    s = int(supersample)
    if not 1 <= s <= SS_MAX:
        raise ValueError("supersample is 1 .. %d" % SS_MAX)
    if not -1 <= int(threshold) <= 255:
        raise ValueError("threshold is -1 .. 255")
    if int(channels) not in (3, 4):
        raise ValueError("channels is 3 or 4")
    _road, bits = _ss_pt_road(None, centre, bla, True)
    st = centre.c_struct()
    y0, y1 = _rows(config, y0, y1)
    if out is None:
        out = np.empty((max(y1 - y0, 0), config.width, int(channels)), dtype=np.uint8)
    refined = C.c_uint64(0)
    _native.check(_native.load().fr_render_rows_ss_adaptive_de_pt_scaled_tf(C.byref(config), C.byref(st), bits, float(thickness), s,
                                                                            int(transfer), int(threshold), float(reach), y0, y1,
                                                                            int(channels), out.ctypes.data, out.nbytes, C.byref(refined)))
    return out, refined.value


def colour_image_de_ss(config, z, iters, der, supersample, thickness, channels=3, transfer=0):
    """fr_colour_de_ss_rgb8 over numpy arrays: z, der float64 [s*rows, s*width, 2] and iters uint32 [s*rows, s*width] — a DE
    render of the config with width and height times s — -> uint8 [rows, width, channels]: box_filter(colour_image_de(config_s,
    z, iters, der, thickness * s), s), byte for byte.  config is the OUTPUT image's: config.height is the whole image's height
    (the arrays may hold fewer rows), thickness is in output pixels. transfer: see box_filter."""
    z, iters, der = _de_arrays(z, iters, der)
    s = int(supersample)
    if not 1 <= s <= SS_MAX:
        raise ValueError("supersample is 1 .. %d" % SS_MAX)
    if int(channels) not in (3, 4):
        raise ValueError("channels is 3 or 4")
    if iters.ndim != 2 or iters.shape[0] % s or iters.shape[1] % s:
        raise ValueError("z and der must be [s*rows, s*width, 2] and iters [s*rows, s*width]")
    rows, width = iters.shape[0] // s, iters.shape[1] // s
    out = np.empty((rows, width, int(channels)), dtype=np.uint8)
    _native.check(_native.load().fr_colour_de_ss_rgb8_tf(C.byref(config), z.ctypes.data, iters.ctypes.data, der.ctypes.data, width, rows, s,
                                                         int(transfer), float(thickness), int(channels), out.ctypes.data, out.nbytes))
    return out


def colour_de_rows_ss_device(config, z_ptr, iters_ptr, der_ptr, width, rows, supersample, thickness, out_ptr, channels=3, stream=None,
                             transfer=0):
    """fr_colour_de_rows_ss_device: colour map + distance shade + box filter in one kernel over a KEPT anti-aliased DE view — the
    (z, iters, der) of supersample * rows rows of supersample * width samples in DEVICE memory (what escape_rows_de_device
    writes for the config with width and height times supersample) — into channels * width * rows bytes at out_ptr,
    asynchronously on `stream`.  config is the output image's (config.height the whole image's height); thickness in output
    pixels.  Thickness and exposure are a recolour: no orbit, no RGB image of the large view. transfer: see box_filter."""
    width, rows, s = int(width), int(rows), int(supersample)
    if not 1 <= s <= SS_MAX:
        raise ValueError("supersample is 1 .. %d" % SS_MAX)
    if int(channels) not in (3, 4):
        raise ValueError("channels is 3 or 4")
    _native.check(_native.load().fr_colour_de_rows_ss_tf_device(C.byref(config), z_ptr or None, iters_ptr or None, der_ptr or None, width,
                                                                rows, s, int(transfer), float(thickness), int(channels), out_ptr or None,
                                                                int(channels) * width * rows, _stream(stream)))


def count_iterations(config, y0=0, y1=None, sx=1, sy=1, precision=Precision.F64):
    """Exact Σ executed iterations over the sampled pixels; returns (total, pixels)."""
    y1 = config.height if y1 is None else y1
    total, npx = C.c_uint64(0), C.c_uint64(0)
    _native.check(
        _native.load().fr_count_iterations(C.byref(config), int(precision), y0, y1, sx, sy, C.byref(total),
                                           C.byref(npx))
    )
    return total.value, npx.value
