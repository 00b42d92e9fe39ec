"""The table behind tests/test_de_call_errors_cpu.py and tools/record_deep_call_errors.py --table de: every plain DE entry point
of the C ABI — the rows of F64 / PT, WIDE PT, BLA-PT and SCALED PT, the F64 extension, the PT and SCALED PT states and their
extensions, each in host and device form, the distance, the two recolours and fr_de_scaled_view — and the calls each must
refuse, or answer as a no-op, BEFORE any device work.  tests/deep_call_cases.py and tests/ss_call_cases.py are its models: an
entry is a C function and the order of its arguments as keys of one argument dict, a case edits that dict and applies to every
entry whose signature has the keys it edits, and a case made of two (`both`) pins which of two errors is reported, i.e. the
order of the checks.  calls(native) yields (id, function name, ctypes arguments, keep-alive, fake) for each pair, and
tests/golden/de_call_errors.json keeps the answers as ss_call_cases.py's matrix (pack, unpack).

No call here may reach the device.  The arrays of a device form are NULL unless the case is about a check that lies behind a
NULL check (one array of several NULL, a misaligned pointer, a lower cap, M == N): then the arrays the case does not spoil are
made-up, well aligned addresses, which is safe exactly because the call is refused, or has nothing to do, first.  Such calls
carry fake = True, and the test leaves them out on a machine that has a device.  On a machine without a device a call that got
through answers FR_ERR_NO_DEVICE, which is how the recorder and the test notice; base_calls() are the unspoiled calls, which
must do exactly that (fr_de_scaled_view needs no device and has none)."""
import ctypes as C
import math

import numpy as np

from ss_call_cases import pack, unpack  # noqa: F401  (the golden file's matrix)

WIDTH, HEIGHT, ITERATIONS, FROM = 33, 17, 300, 150
N = WIDTH * HEIGHT  # the stored results of the distance and the recolours
PT_MAX_ITERATIONS = 1 << 24
FAKE = 0x10000000  # a made-up device address, aligned to 256 bytes: never dereferenced (see above)
F64, F32, DD, PT = 0, 1, 2, 3
FERN = 1

ARRAYS = ("z", "it", "dz", "m", "der", "out", "dout")  # NULL or made-up in a device form, real in a host form
MISALIGN = {"z": 4, "it": 2, "dz": 4, "m": 2, "der": 4, "dout": 4, "out": 1}

# family -> (host signature, {road tag: constants})
FAMILIES = {
    "fr_escape_rows_de": ("cfg prec lo y0 y1 z it der", {"f64": {"prec": F64}, "pt": {"prec": PT, "lo": True}}),
    "fr_escape_rows_de_pt_wide": ("cfg wide y0 y1 z it der", {"wide": {"wide": True}}),
    "fr_escape_extend_de": ("cfg prec y0 y1 from z it der", {"f64": {"prec": F64}}),
    "fr_escape_rows_de_pt_state": ("cfg lo wide y0 y1 z it dz m der", {"dd": {"lo": True}, "wide": {"wide": True}}),
    "fr_escape_extend_de_pt": ("cfg lo wide y0 y1 from z it dz m der", {"dd": {"lo": True}, "wide": {"wide": True}}),
    "fr_escape_rows_de_pt_bla": ("cfg lo wide bits y0 y1 z it der", {"dd": {"lo": True}, "wide": {"wide": True}}),
    "fr_escape_rows_de_pt_scaled": ("cfg wide bits y0 y1 z it der", {"scaled": {"wide": True}}),
    "fr_escape_rows_de_pt_scaled_state": ("cfg wide y0 y1 z it dz m der", {"scaled": {"wide": True}}),
    "fr_escape_extend_de_pt_scaled": ("cfg wide y0 y1 from z it dz m der", {"scaled": {"wide": True}}),
    "fr_distance_rows": ("cfg z it der n dout", {"": {}}),
}

# name -> (C function, signature, constants of the entry)
ENTRIES = {}
for family, (sig, roads) in FAMILIES.items():
    for tag, consts in roads.items():
        for fn, s in ((family, sig), (family + "_device", sig + " stream")):
            ENTRIES[fn + ("[%s]" % tag if tag else "")] = (fn, s, consts)
ENTRIES["fr_colour_de_rows_device"] = ("fr_colour_de_rows_device", "cfg z it der n T ch out stream", {})
ENTRIES["fr_colour_de_rgb8"] = ("fr_colour_de_rgb8", "cfg z it der n T out out_len", {})
ENTRIES["fr_de_scaled_view"] = ("fr_de_scaled_view", "cfg view", {})


def is_device(entry):
    return "_device" in entry


class Call:
    """the arguments of one call: a valid call of the entry to start from (its device arrays apart), which the case then spoils"""

    def __init__(self, native, entry):
        self.native, self.entry = native, entry
        self.fn, sig, consts = ENTRIES[entry]
        self.sig, self.device = sig.split(), is_device(entry)
        lib = native.load()
        cfg = native.fr_config()
        lib.fr_config_new(C.byref(cfg), 0)
        cfg.width, cfg.height, cfg.iterations = WIDTH, HEIGHT, ITERATIONS
        cfg.pos.re, cfg.pos.im, cfg.scale.re, cfg.scale.im, cfg.limit = -0.75, 0.1, 1e12, 1e12, 2.0
        self.words = [np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)]
        lib.fr_wide_from_double(-0.75, self.words[0].ctypes.data, 3)
        lib.fr_wide_from_double(0.1, self.words[1].ctypes.data, 3)
        self.buffers = {"z": np.zeros(2 * N + 1), "dz": np.zeros(2 * N + 1), "der": np.zeros(2 * N + 1), "dout": np.zeros(N + 1),
                        "it": np.zeros(N + 1, dtype=np.uint32), "m": np.zeros(N + 1, dtype=np.uint32), "out": np.zeros(4 * N + 4, dtype=np.uint8)}
        self.view = native.fr_config()
        self.a = {"cfg": cfg, "prec": PT, "lo": None, "wide": None, "bits": 0, "y0": 0, "y1": HEIGHT, "from": FROM, "n": N, "T": 1.5, "ch": 3,
                  "out_len": 3 * N, "stream": None, "view": C.byref(self.view)}
        self.a.update(consts)
        self.a["lo"] = native.Imaginary(1e-20, -1e-20) if consts.get("lo") else None
        self.a["wide"] = self.centre() if consts.get("wide") else None
        self.explicit, self.reach, self.fake = {}, False, False

    def centre(self, n_words=3):
        p64 = C.POINTER(C.c_uint64)
        return self.native.fr_wide_centre(n_words, self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64))

    def has(self, *keys):
        return all(k in self.sig for k in keys)

    def f64(self):
        """the call is on the F64 road, which has no rule about the view's fields but DE's limit"""
        return self.has("prec") and self.a["prec"] == F64

    def wide(self):
        return self.a["wide"] is not None

    def scaled(self):
        return "scaled" in self.entry

    def array(self, key, value):
        """the case's own value for an array: None, or an offset from the array's own address (made-up in a device form)"""
        self.explicit[key] = value

    def behind(self):
        """the case is about a check behind the NULL checks: a device form's other arrays are made-up addresses"""
        self.reach = True

    def address(self, i, k):
        return FAKE * (i + 1) if self.device else self.buffers[k].ctypes.data

    def args(self):
        out = []
        for i, k in enumerate(self.sig):
            if k in ARRAYS:
                if k in self.explicit:
                    v = self.explicit[k] if self.explicit[k] is None else self.address(i, k) + self.explicit[k]
                elif not self.device:
                    v = self.buffers[k].ctypes.data
                else:
                    v = FAKE * (i + 1) if self.reach else None
                if self.device and v is not None:
                    self.fake = True
            else:
                v = self.a[k]
            out.append(C.byref(v) if k in ("cfg", "lo", "wide") and v is not None else v)
        return out


# ---- the cases: each returns False where it does not apply to the entry ------------------------------------------------------


def named(name):
    def deco(case):
        case.__name__ = name
        return case

    return deco


def setter(name, key, value, behind=False):
    """behind: the rule comes behind the arrays' (the calls over stored results), so a device form's are made up"""

    @named(name)
    def case(c):
        if not c.has(key):
            return False
        c.a[key] = value
        if behind:
            c.behind()

    return case


def cfg_null(c):
    c.a["cfg"] = None


def y0_above_y1(c):
    if not c.has("y0"):
        return False
    c.a["y0"], c.a["y1"] = 5, 4


def y1_above_height(c):
    if not c.has("y1"):
        return False
    c.a["y1"] = HEIGHT + 1


def y0_above_y1_above_height(c):
    if not c.has("y0"):
        return False
    c.a["y0"], c.a["y1"] = HEIGHT + 2, HEIGHT + 1


def limit_case(name, value):
    @named(name)
    def case(c):
        if not c.has("y0"):  # the calls over stored results and fr_de_scaled_view do not look at the limit
            return False
        c.a["cfg"].limit = value

    return case


limit_just_above_2_20 = limit_case("limit_just_above_2_20", math.nextafter(2.0 ** 20, math.inf))
limit_2_21 = limit_case("limit_2_21", 2.0 ** 21)
limit_inf = limit_case("limit_inf", math.inf)
limit_nan = limit_case("limit_nan", math.nan)


def limit_zero(c):
    """the deep roads' own rule; legal on the F64 road"""
    if c.f64() or not c.has("y0"):
        return False
    c.a["cfg"].limit = 0.0


def precision_case(name, value):
    @named(name)
    def case(c):
        if not c.has("prec"):
            return False
        c.a["prec"], c.a["lo"] = value, None

    return case


precision_f32 = precision_case("precision_f32", F32)
precision_dd = precision_case("precision_dd", DD)
precision_7 = precision_case("precision_7", 7)
precision_minus_1 = precision_case("precision_minus_1", -1)


def precision_pt_on_the_f64_extension(c):
    if not c.has("prec", "from"):
        return False
    c.a["prec"] = PT


def pos_lo_with_f64(c):
    if not c.has("prec", "lo"):
        return False
    c.a["prec"], c.a["lo"] = F64, c.native.Imaginary(1e-20, 0.0)


def pos_lo_with_centre(c):
    if not c.has("lo", "wide"):
        return False
    c.a["lo"], c.a["wide"] = c.native.Imaginary(1e-20, 0.0), c.centre()


def pos_lo_not_normalised(c):
    if not c.has("lo") or c.wide() or c.f64():
        return False
    c.a["lo"] = c.native.Imaginary(1.0, 0.0)


def pos_lo_not_finite(c):
    if not c.has("lo") or c.wide() or c.f64():
        return False
    c.a["lo"] = c.native.Imaginary(math.inf, 0.0)


def centre_null(c):
    """where the centre is required: the wide and the scaled calls (the others take NULL for the dd road with pos_lo)"""
    if not c.has("wide") or c.has("lo"):
        return False
    c.a["wide"] = None


def wide_case(name, edit):
    """a rule of the wide centre or of the view under it: the calls that have a centre"""

    @named(name)
    def case(c):
        if not c.wide():
            return False
        return edit(c)

    return case


def _n_words(n):
    def edit(c):
        c.a["wide"] = c.centre(n)

    return edit


def _words_null(c):
    c.a["wide"] = c.native.fr_wide_centre(c.a["wide"].n_words, None, None)


def _centre_above_2(c):
    c.words[0][:] = 0
    c.words[0][2] = 3 << 56  # 3.0: the value is I / 2^(64 n - 8)


def _too_coarse(c):
    c.a["cfg"].scale.re = c.a["cfg"].scale.im = 2.0 ** 130  # 64 * 3 - 8 = 184 < 131 + 64


def _julia_set_above_2(c):
    c.a["cfg"].julia_set.re = 2.5


n_words_1 = wide_case("n_words_1", _n_words(1))
n_words_17 = wide_case("n_words_17", _n_words(17))
words_null = wide_case("words_null", _words_null)
centre_too_coarse = wide_case("centre_too_coarse", _too_coarse)
julia_set_above_2 = wide_case("julia_set_above_2", _julia_set_above_2)
centre_above_2 = wide_case("centre_above_2", _centre_above_2)


def scale_above_2_440(c):
    """WIDE PT's upper bound: SCALED PT has none (and there 3 words would be too coarse), nor has the dd centre"""
    if not c.wide() or c.scaled():
        return False
    c.words.extend([np.zeros(9, dtype=np.uint64), np.zeros(9, dtype=np.uint64)])
    c.words[0], c.words[1] = c.words[2], c.words[3]
    c.native.load().fr_wide_from_double(-0.75, c.words[0].ctypes.data, 9)
    c.native.load().fr_wide_from_double(0.1, c.words[1].ctypes.data, 9)
    c.a["wide"] = c.centre(9)
    c.a["cfg"].scale.re = c.a["cfg"].scale.im = 2.0 ** 441


def scale_below_2_minus_64(c):
    if c.f64() or not (c.has("y0") or c.has("view")):
        return False
    c.a["cfg"].scale.re = 2.0 ** -65
    if (c.scaled() or c.has("view")) and math.isfinite(c.a["cfg"].scale.im):  # the axes within 2^32 of each other: that rule comes behind
        c.a["cfg"].scale.im = 2.0 ** -65


def scale_anisotropic(c):
    if not (c.scaled() or c.has("view")):
        return False
    c.a["cfg"].scale.im = c.a["cfg"].scale.re * 2.0 ** -33


def scale_not_finite(c):
    if c.f64() or not (c.has("y0") or c.has("view")):
        return False
    c.a["cfg"].scale.im = math.inf


def exposure_not_finite(c):
    if c.f64() or not c.has("y0"):
        return False
    c.a["cfg"].exposure = math.nan


def pos_above_2_64(c):
    """the dd centre's rule; a wide centre does not read cfg->pos"""
    if c.f64() or c.wide() or not c.has("lo"):
        return False
    c.a["cfg"].pos.re, c.a["lo"] = 2.0 ** 65, None


def iterations_above_pt_max(c):
    if c.f64() or not c.has("y0"):
        return False
    c.a["cfg"].iterations = PT_MAX_ITERATIONS + 1


bits_23 = setter("bits_23", "bits", 23)
bits_54 = setter("bits_54", "bits", 54)
bits_minus_2 = setter("bits_minus_2", "bits", -2)


def bits_minus_1(c):
    if not c.has("bits") or c.scaled():  # SCALED PT's plain loop: legal there
        return False
    c.a["bits"] = -1


def from_above_iterations(c):
    """M < N; the device form's arrays stay NULL: the rule comes in front of them"""
    if not c.has("from"):
        return False
    c.a["from"] = c.a["cfg"].iterations + 1


thickness_negative = setter("thickness_negative", "T", -0.5, behind=True)
thickness_above_2_20 = setter("thickness_above_2_20", "T", math.nextafter(2.0 ** 20, math.inf), behind=True)
thickness_nan = setter("thickness_nan", "T", math.nan, behind=True)
thickness_inf = setter("thickness_inf", "T", math.inf, behind=True)
n_above_2_40 = setter("n_above_2_40", "n", (1 << 40) + 1)
channels_2 = setter("channels_2", "ch", 2, behind=True)
channels_5 = setter("channels_5", "ch", 5, behind=True)
view_null = setter("view_null", "view", None)


def out_too_small(c):
    if not c.has("out_len"):
        return False
    c.a["out_len"] = 3 * N - 1
    c.behind()


def all_null(c):
    """every array NULL with a range that is not empty: a device form as it stands, a host form without its buffers"""
    if not any(c.has(k) for k in ARRAYS):
        return False
    for k in ARRAYS:
        c.array(k, None)


def null_case(key):
    @named(key + "_null")
    def case(c):
        if not c.has(key):
            return False
        c.array(key, None)
        c.behind()

    return case


def misaligned_case(key):
    @named(key + "_misaligned")
    def case(c):
        if not c.has(key):
            return False
        if key == "dout" and not c.device:  # the host forms' outputs have no alignment rule: the call would get through
            return False
        if key == "out":
            if not c.has("ch"):
                return False
            c.a["ch"] = 4
        c.array(key, MISALIGN[key])
        c.behind()

    return case


NULLS = {k: null_case(k) for k in ARRAYS}
MISALIGNED = {k: misaligned_case(k) for k in ARRAYS}


def noop_empty_rows(c):
    """y0 == y1: FR_OK with NULL arrays"""
    if not c.has("y0"):
        return False
    c.a["y0"] = c.a["y1"] = 5
    all_null(c)


def noop_width_0(c):
    if not c.has("y0"):
        return False
    c.a["cfg"].width = 0
    all_null(c)


def noop_m_equals_n(c):
    """M == N: the arrays are checked and not touched"""
    if not c.has("from"):
        return False
    c.a["from"] = c.a["cfg"].iterations
    c.behind()


def noop_no_orbits(c):
    """an extension on an algorithm without orbits: the arrays are checked and not touched"""
    if not c.has("from"):
        return False
    c.a["cfg"].algo = FERN
    c.behind()


def noop_n_0(c):
    if not c.has("n"):
        return False
    c.a["n"] = 0
    all_null(c)


def both(first, second):
    """a call wrong in two ways: which error it reports pins the order of the checks"""

    @named(first.__name__ + "+" + second.__name__)
    def case(c):
        if first(c) is False or second(c) is False:
            return False

    return case


SINGLES = [cfg_null, y0_above_y1, y1_above_height, y0_above_y1_above_height, limit_just_above_2_20, limit_2_21, limit_inf, limit_nan,
           limit_zero, precision_f32, precision_dd, precision_7, precision_minus_1, precision_pt_on_the_f64_extension, pos_lo_with_f64,
           pos_lo_with_centre, pos_lo_not_normalised, pos_lo_not_finite, centre_null, n_words_1, n_words_17, words_null,
           centre_too_coarse, julia_set_above_2, centre_above_2, scale_above_2_440, scale_below_2_minus_64, scale_anisotropic, scale_not_finite,
           exposure_not_finite, pos_above_2_64, iterations_above_pt_max, bits_23, bits_54, bits_minus_1, bits_minus_2,
           from_above_iterations, thickness_negative, thickness_above_2_20, thickness_nan, thickness_inf, n_above_2_40, channels_2,
           channels_5, view_null, out_too_small, all_null] + list(NULLS.values()) + list(MISALIGNED.values())
NOOPS = [noop_empty_rows, noop_width_0, noop_m_equals_n, noop_no_orbits, noop_n_0]
_N, _M = NULLS, MISALIGNED
# every adjacent pair of the calls' check orders (include/fractal_hip.h): rows; the road (precision, pos_lo, centre); the
# road's own domain; bits; DE's limit; the lower cap; the arrays, NULL before misaligned; thickness; channels; the output
ADJACENT = [(cfg_null, y0_above_y1), (cfg_null, n_above_2_40), (cfg_null, view_null), (y1_above_height, precision_7),
            (y1_above_height, precision_pt_on_the_f64_extension), (y1_above_height, centre_null), (y1_above_height, pos_lo_with_f64),
            (y1_above_height, pos_lo_with_centre), (y0_above_y1, scale_not_finite), (y0_above_y1, limit_2_21),
            (precision_7, limit_2_21), (precision_f32, limit_inf), (precision_dd, all_null), (precision_pt_on_the_f64_extension, limit_2_21),
            (precision_pt_on_the_f64_extension, from_above_iterations), (pos_lo_with_f64, limit_2_21), (pos_lo_with_f64, all_null),
            (pos_lo_with_centre, n_words_1), (pos_lo_with_centre, scale_not_finite), (pos_lo_with_centre, bits_23),
            (pos_lo_with_centre, limit_2_21), (centre_null, limit_2_21), (centre_null, bits_23), (centre_null, scale_not_finite),
            (centre_null, from_above_iterations), (n_words_1, words_null), (n_words_17, scale_not_finite), (words_null, exposure_not_finite),
            (exposure_not_finite, limit_zero), (scale_not_finite, limit_2_21), (limit_zero, iterations_above_pt_max),
            (limit_2_21, iterations_above_pt_max), (iterations_above_pt_max, scale_below_2_minus_64),
            (scale_below_2_minus_64, scale_anisotropic), (scale_below_2_minus_64, scale_above_2_440), (scale_below_2_minus_64, pos_lo_not_normalised),
            (pos_above_2_64, scale_below_2_minus_64), (limit_zero, pos_above_2_64), (scale_anisotropic, julia_set_above_2),
            (scale_above_2_440, julia_set_above_2), (julia_set_above_2, centre_above_2), (centre_above_2, centre_too_coarse), (centre_too_coarse, bits_23),
            (centre_too_coarse, limit_2_21), (pos_lo_not_normalised, iterations_above_pt_max), (pos_lo_not_normalised, limit_2_21),
            (iterations_above_pt_max, bits_23), (iterations_above_pt_max, limit_2_21), (julia_set_above_2, bits_54), (bits_23, limit_2_21),
            (bits_54, limit_nan), (bits_minus_1, limit_2_21), (bits_minus_2, all_null), (bits_23, all_null), (bits_23, _M["z"]),
            (limit_2_21, from_above_iterations), (limit_just_above_2_20, all_null), (limit_2_21, _N["der"]), (limit_nan, _M["it"]),
            (from_above_iterations, all_null), (from_above_iterations, _N["z"]), (from_above_iterations, _M["der"]),
            (centre_too_coarse, from_above_iterations), (iterations_above_pt_max, from_above_iterations),
            (_N["z"], _M["it"]), (_N["it"], _M["z"]), (_N["der"], _M["z"]), (_N["dz"], _M["m"]), (_N["m"], _M["dz"]), (_N["der"], _M["dz"]),
            (_M["z"], _M["it"]), (_M["z"], _M["der"]), (_M["it"], _M["der"]), (_M["dz"], _M["m"]), (_M["der"], _M["m"]),
            (n_above_2_40, all_null), (n_above_2_40, _M["z"]), (n_above_2_40, thickness_negative), (_N["z"], thickness_negative),
            (_M["der"], thickness_negative), (_M["it"], channels_2), (thickness_negative, channels_2), (thickness_nan, _N["out"]),
            (thickness_above_2_20, out_too_small), (channels_2, _N["out"]), (channels_5, _M["out"]), (_N["out"], out_too_small),
            (_N["z"], _N["out"]), (_N["z"], _N["dout"]), (_M["der"], _N["dout"]), (_M["it"], _M["dout"]), (_M["z"], _M["out"]),
            (_N["der"], out_too_small), (view_null, scale_not_finite), (scale_not_finite, scale_below_2_minus_64),
            (scale_not_finite, scale_anisotropic)]
# a call with nothing to do against the domain and the arrays: the domain still refuses, the arrays are looked at only where
# the call says so (M == N and an algorithm without orbits come behind them)
EMPTY = [(noop_empty_rows, limit_2_21), (noop_empty_rows, precision_7), (noop_empty_rows, bits_23), (noop_empty_rows, centre_null),
         (noop_empty_rows, from_above_iterations), (noop_empty_rows, iterations_above_pt_max), (noop_empty_rows, _M["z"]),
         (noop_empty_rows, noop_m_equals_n), (noop_width_0, y1_above_height), (noop_width_0, limit_inf), (noop_width_0, from_above_iterations),
         (noop_m_equals_n, all_null), (noop_m_equals_n, _N["der"]), (noop_m_equals_n, _M["m"]), (noop_m_equals_n, _M["z"]),
         (noop_m_equals_n, limit_2_21), (noop_m_equals_n, noop_no_orbits), (noop_no_orbits, all_null), (noop_no_orbits, _M["der"]),
         (noop_no_orbits, from_above_iterations), (noop_no_orbits, limit_2_21), (noop_no_orbits, precision_pt_on_the_f64_extension),
         (noop_n_0, cfg_null), (noop_n_0, thickness_negative), (noop_n_0, channels_2), (noop_n_0, out_too_small), (noop_n_0, _M["z"]),
         (noop_n_0, _M["out"])]
CASES = SINGLES + NOOPS + [both(a, b) for a, b in ADJACENT + EMPTY]


def calls(native):
    """(id, C function name, arguments, keep-alive, fake) of every case of every entry it applies to"""
    for entry in ENTRIES:
        for case in CASES:
            c = Call(native, entry)
            if case(c) is False:
                continue
            args = c.args()
            yield "%s :: %s" % (entry, case.__name__), c.fn, args, c, c.fake


def base_calls(native):
    """the unspoiled call of every entry that needs a device, a device form's arrays made up: on a machine WITHOUT a device (only
    there may it be made) it answers FR_ERR_NO_DEVICE — so each case above is wrong in what it spoils and in nothing else"""
    for entry in ENTRIES:
        if entry == "fr_de_scaled_view":
            continue
        c = Call(native, entry)
        c.behind()
        yield entry, c.fn, c.args(), c
