"""The table behind tests/test_deep_call_errors_cpu.py and tools/record_deep_call_errors.py: every deep entry point of the C
ABI (DD, PT, PT state, PT extend, their wide variants, BLA-PT and its debug hooks, SCALED PT with its state, its extension
and its debug hooks, supersampling with pos_lo; host and device forms) and the invalid calls each must refuse BEFORE any device work, with a code and a message.

An entry is a C function and the order of its arguments, written as keys of one argument dict; a case edits that dict and
applies to every entry whose signature has the keys it edits.  calls(native) yields (id, function name, ctypes arguments,
keep-alive) for each pair; the ids are the keys of tests/golden/deep_call_errors.json.

No call here may reach the device: the device forms get NULL or made-up addresses for their arrays, which is safe exactly
because every case is refused first.  On a machine without a device a call that got through answers FR_ERR_NO_DEVICE, which
is how the recorder and the test notice."""
import ctypes as C
import math

import numpy as np

WIDTH, HEIGHT, ITERATIONS = 33, 17, 300
PT_MAX_ITERATIONS = 1 << 24
FAKE = 0x10000000  # a made-up, well aligned device address: never dereferenced (see above)

RGB_HOST = "cfg {where} y0 y1 ch out out_len"
RAW_HOST = "cfg {where} y0 y1 z it"
STATE_HOST = "cfg {where} y0 y1 z it dz m"
EXTEND_HOST = "cfg {where} y0 y1 from z it dz m"

# name -> (C function, signature, constants of the entry)
ENTRIES = {}
for road, where in (("dd", "lo"), ("pt", "lo"), ("pt_wide", "wide")):
    ENTRIES["fr_render_rows_" + road] = ("fr_render_rows_" + road, RGB_HOST.format(where=where), {})
    ENTRIES["fr_render_rows_%s_device" % road] = ("fr_render_rows_%s_device" % road, RGB_HOST.format(where=where) + " stream", {})
    ENTRIES["fr_escape_rows_" + road] = ("fr_escape_rows_" + road, RAW_HOST.format(where=where), {})
for wide, where in (("", "lo"), ("_wide", "wide")):
    ENTRIES["fr_escape_rows_pt%s_state" % wide] = ("fr_escape_rows_pt%s_state" % wide, STATE_HOST.format(where=where), {})
    ENTRIES["fr_escape_rows_pt%s_state_device" % wide] = (
        "fr_escape_rows_pt%s_state_device" % wide, STATE_HOST.format(where=where) + " stream", {})
    ENTRIES["fr_escape_extend_pt" + wide] = ("fr_escape_extend_pt" + wide, EXTEND_HOST.format(where=where), {})
    ENTRIES["fr_escape_extend_pt%s_device" % wide] = ("fr_escape_extend_pt%s_device" % wide, EXTEND_HOST.format(where=where) + " stream", {})
ENTRIES.update({
    "fr_escape_rows_device[pt]": ("fr_escape_rows_device", "cfg prec lo y0 y1 zw z it stream opts", {"prec": 3, "zw": 2}),
    "fr_escape_rows_device[dd]": ("fr_escape_rows_device", "cfg prec lo y0 y1 zw z it stream opts", {"prec": 2, "zw": 4}),
    "fr_escape_extend[dd]": ("fr_escape_extend", "cfg prec lo y0 y1 from zw z it", {"prec": 2, "zw": 4}),
    "fr_escape_extend_device[dd]": ("fr_escape_extend_device", "cfg prec lo y0 y1 from zw z it stream opts", {"prec": 2, "zw": 4}),
    "fr_render_rows_pt_bla": ("fr_render_rows_pt_bla", "cfg lo wide bits y0 y1 ch out out_len", {}),
    "fr_render_rows_pt_bla_device": ("fr_render_rows_pt_bla_device", "cfg lo wide bits y0 y1 ch out out_len stream", {}),
    "fr_escape_rows_pt_bla": ("fr_escape_rows_pt_bla", "cfg lo wide bits y0 y1 z it", {}),
    "fr_escape_rows_pt_bla_device": ("fr_escape_rows_pt_bla_device", "cfg lo wide bits y0 y1 z it stream", {}),
    "fr_debug_bla_count": ("fr_debug_bla_count", "cfg lo wide bits y0 y1 passes steps", {}),
    "fr_debug_bla_table": ("fr_debug_bla_table", "cfg lo wide bits which level table cap len", {}),
    "fr_render_rows_ss[pt]": ("fr_render_rows_ss", "cfg prec lo s y0 y1 ch out out_len opts", {"prec": 3, "s": 2}),
    "fr_render_rows_ss_device[pt]": (
        "fr_render_rows_ss_device", "cfg prec lo s y0 y1 ch out out_len work work_len stream opts", {"prec": 3, "s": 2}),
    # SCALED PT: the centre is required and there is no pos_lo; the rows and the hooks take bits, the state calls do not
    "fr_render_rows_pt_scaled": ("fr_render_rows_pt_scaled", "cfg wide bits y0 y1 ch out out_len", {}),
    "fr_render_rows_pt_scaled_device": ("fr_render_rows_pt_scaled_device", "cfg wide bits y0 y1 ch out out_len stream", {}),
    "fr_escape_rows_pt_scaled": ("fr_escape_rows_pt_scaled", "cfg wide bits y0 y1 z it", {}),
    "fr_escape_rows_pt_scaled_device": ("fr_escape_rows_pt_scaled_device", "cfg wide bits y0 y1 z it stream", {}),
    "fr_debug_pt_scaled_count": ("fr_debug_pt_scaled_count", "cfg wide bits y0 y1 passes steps", {}),
    "fr_debug_bla_table_scaled": ("fr_debug_bla_table_scaled", "cfg wide bits which level table cap len", {}),
    "fr_escape_rows_pt_scaled_state": ("fr_escape_rows_pt_scaled_state", STATE_HOST.format(where="wide"), {}),
    "fr_escape_rows_pt_scaled_state_device": ("fr_escape_rows_pt_scaled_state_device", STATE_HOST.format(where="wide") + " stream", {}),
    "fr_escape_extend_pt_scaled": ("fr_escape_extend_pt_scaled", EXTEND_HOST.format(where="wide"), {}),
    "fr_escape_extend_pt_scaled_device": ("fr_escape_extend_pt_scaled_device", EXTEND_HOST.format(where="wide") + " stream", {}),
})


def is_device(entry):
    return "_device" in entry


def is_dd(entry):
    return "dd" in entry


def is_bla(entry):
    return "bla" in entry


def is_scaled(entry):
    return "scaled" in entry


class Call:
    """the arguments of one call: a valid call of the entry to start from, which the case then spoils"""

    def __init__(self, native, entry):
        self.native, self.entry = native, entry
        self.fn, sig, consts = ENTRIES[entry]
        self.sig = sig.split()
        cfg = native.fr_config()
        native.load().fr_config_new(C.byref(cfg), 0)
        cfg.width, cfg.height, cfg.iterations = WIDTH, HEIGHT, ITERATIONS
        cfg.pos.re, cfg.pos.im, cfg.scale.re, cfg.scale.im, cfg.limit = -0.75, 0.1, 1e12, 1e12, 2.0
        self.words = [np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)]
        native.load().fr_wide_from_double(-0.75, self.words[0].ctypes.data, 3)
        native.load().fr_wide_from_double(0.1, self.words[1].ctypes.data, 3)
        npx = WIDTH * HEIGHT
        self.buffers = {"out": np.zeros(4 * npx, dtype=np.uint8), "z": np.zeros(4 * npx), "dz": np.zeros(2 * npx),
                        "it": np.zeros(npx, dtype=np.uint32), "m": np.zeros(npx, dtype=np.uint32), "table": np.zeros(5 * 8)}
        self.counts = {"passes": C.c_uint64(0), "steps": C.c_uint64(0), "len": C.c_uint32(0)}
        self.a = {"cfg": cfg, "lo": native.Imaginary(1e-20, -1e-20) if "lo" in self.sig and not is_bla(entry) else None,
                  "wide": self.centre() if "wide" in self.sig and "lo" not in self.sig else None, "bits": 0, "y0": 0, "y1": HEIGHT, "ch": 3,
                  "from": 150, "out_len": 4 * npx, "stream": None, "opts": None, "which": 0, "level": 1, "cap": 8, "work": None,
                  "work_len": 0}
        self.a.update(consts)
        for k in ("out", "z", "it", "dz", "m", "table"):  # host forms: real arrays; device forms: NULL (never reached)
            self.a[k] = None if is_device(entry) else self.buffers[k].ctypes.data
        for k, v in self.counts.items():
            self.a[k] = C.byref(v)

    def centre(self):
        p64 = C.POINTER(C.c_uint64)
        return self.native.fr_wide_centre(3, self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64))

    def has(self, *keys):
        return all(k in self.sig for k in keys)

    def args(self):
        out = []
        for k in self.sig:
            v = self.a[k]
            out.append(C.byref(v) if k in ("cfg", "lo", "wide") and v is not None else v)
        return out


# ---- the cases: each returns False where it does not apply to the entry ------------------------------------------------------


def y0_above_y1(c):
    if not c.has("y0"):
        return False
    c.a["y0"], c.a["y1"] = 5, 4


def y1_above_height(c):
    if not c.has("y1"):
        return False
    c.a["y1"] = HEIGHT + 1


def channels_2(c):
    if not c.has("ch"):
        return False
    c.a["ch"] = 2


def limit_not_finite(c):
    c.a["cfg"].limit = math.inf


def pos_lo_not_normalised(c):
    if not c.has("lo"):
        return False
    c.a["lo"] = c.native.Imaginary(1.0, 0.0)


def iterations_above_pt_max(c):
    if is_dd(c.entry):  # a legal DD call
        return False
    c.a["cfg"].iterations = PT_MAX_ITERATIONS + 1
    c.a["from"] = PT_MAX_ITERATIONS


def wide_centre_null(c):
    if not c.has("wide") or c.has("lo"):  # the BLA calls take NULL for both: the dd road with pos_lo = (0, 0)
        return False
    c.a["wide"] = None


def pos_lo_with_centre(c):
    if not c.has("lo", "wide"):
        return False
    c.a["lo"], c.a["wide"] = c.native.Imaginary(1e-20, 0.0), c.centre()


def bits_23(c):
    if not c.has("bits"):
        return False
    c.a["bits"] = 23


def bits_54(c):
    if not c.has("bits"):
        return False
    c.a["bits"] = 54


def no_table(c):
    """bits = -1: SCALED PT's plain loop; no answer where the call is about a table, and BLA-PT has no such value"""
    if not c.has("bits"):
        return False
    c.a["bits"] = -1


def bits_minus_1(c):
    if is_scaled(c.entry) and not c.has("table"):  # legal for SCALED PT's rows and count: the pairs with no_table below pin that
        return False
    return no_table(c)


def from_above_iterations(c):
    if not c.has("from"):
        return False
    c.a["from"] = c.a["cfg"].iterations + 1


def misaligned_pointer(c):
    if not is_device(c.entry) or not (c.has("out") or c.has("z")):
        return False
    if c.has("out"):
        c.a["ch"], c.a["out"] = 4, FAKE + 1
    else:
        c.a["z"], c.a["it"] = FAKE + 4, FAKE
        if c.has("dz"):
            c.a["dz"], c.a["m"] = FAKE, FAKE


def null_output(c):
    """with a non-empty range; the escape rows calls take NULL for either array, so they have no such error"""
    if c.has("out"):
        c.a["out"] = None
    elif c.has("dz") or c.has("from"):
        c.a["z"] = None
        if is_device(c.entry):
            c.a["it"] = FAKE
            if c.has("dz"):
                c.a["dz"], c.a["m"] = FAKE, FAKE
    elif c.has("passes"):
        c.a["passes"] = None
    elif c.has("len"):
        c.a["len"] = None
    else:
        return False


def both(first, second):
    """a call wrong in two ways: which error it reports pins the order of the checks"""

    def case(c):
        if first(c) is False or second(c) is False:
            return False

    case.__name__ = first.__name__ + "+" + second.__name__
    return case


def short_and_misaligned(c):
    if not is_device(c.entry) or not c.has("out"):
        return False
    c.a["ch"], c.a["out"], c.a["out_len"] = 4, FAKE + 1, 4 * WIDTH * HEIGHT - 1


CASES = [y0_above_y1, y1_above_height, channels_2, limit_not_finite, pos_lo_not_normalised, iterations_above_pt_max,
         wide_centre_null, pos_lo_with_centre, bits_23, bits_54, from_above_iterations, misaligned_pointer, null_output,
         both(channels_2, y0_above_y1), both(y0_above_y1, limit_not_finite), both(limit_not_finite, iterations_above_pt_max),
         both(iterations_above_pt_max, from_above_iterations), both(wide_centre_null, channels_2), both(bits_54, pos_lo_with_centre),
         both(pos_lo_not_normalised, bits_23), both(null_output, y1_above_height), both(from_above_iterations, null_output),
         short_and_misaligned, bits_minus_1, both(no_table, null_output), both(no_table, misaligned_pointer),
         both(wide_centre_null, bits_54), both(bits_23, null_output)]


def calls(native):
    """(id, C function name, arguments, keep-alive) of every case of every entry it applies to"""
    for entry in ENTRIES:
        for case in CASES:
            c = Call(native, entry)
            if case(c) is False:
                continue
            yield "%s :: %s" % (entry, case.__name__), c.fn, c.args(), c
