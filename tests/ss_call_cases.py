"""The table behind tests/test_ss_call_errors_cpu.py and tools/record_deep_call_errors.py --table ss: every supersampled entry
point of the C ABI — fr_render_rows_ss, _ss_pt, _ss_de, _ss_de_pt_scaled, _ss_adaptive, _ss_adaptive_de, the filter and the two
fused recolours, each in plain and _tf spelling, host and device form, on each of its roads, and the four workspace calls — and
the calls each must refuse, or answer as a no-op, BEFORE any device work.  tests/deep_call_cases.py is its model: an entry is a
C function and the order of its arguments as keys of one argument dict, a case edits that dict and applies to every entry whose
signature has the keys it edits, and a case made of two (`both`) pins which of two errors is reported, i.e. the order of the
checks.  calls(native) yields (id, function name, ctypes arguments, keep-alive, fake) for each pair.  A plain call and its _tf
twin share their ids — the plain call IS the twin with transfer 0, so one recorded answer holds for both, and the recorder
refuses to write a file if they differ — and tests/golden/ss_call_errors.json keeps the answers as a matrix (pack, unpack
below): the distinct answers once, the cases once, and one row of answer numbers per entry.

No call here may reach the device.  The arrays of a device form are NULL unless the case is about a check that lies behind a
NULL check (a short out_len, a misaligned pointer, the workspace rules behind fr_render_rows_ss_device's output rules): then
the arrays the case does not spoil are made-up, well aligned addresses, which is safe exactly because the call is refused
first.  Such calls carry fake = True, and the test leaves them out on a machine that has a device, where a regression would
launch a kernel on a made-up address.  On a machine without a device a call that got through answers FR_ERR_NO_DEVICE, which is
how the recorder and the test notice; base_calls() are the unspoiled calls, which must do exactly that."""
import ctypes as C
import math

import numpy as np

WIDTH, HEIGHT, ITERATIONS, S = 33, 17, 300, 2
PT_MAX_ITERATIONS = 1 << 24
FAKE = 0x10000000  # a made-up device address, aligned to 256 bytes: never dereferenced (see above)
F64, F32, DD, PT = 0, 1, 2, 3
PLAIN, BLA, SCALED = 0, 1, 2

DEVICE_ARRAYS = ("out", "work", "src", "z", "it", "der")  # NULL or made-up in a device form, real in a host form
WORKSPACE_OF = {"ss": "fr_ss_workspace_bytes", "ss_pt": "fr_ss_workspace_bytes", "ss_de": "fr_ss_de_workspace_bytes",
                "ss_de_pt_scaled": "fr_ss_de_workspace_bytes", "ss_adaptive": "fr_ss_adaptive_workspace_bytes",
                "ss_adaptive_de": "fr_ss_adaptive_de_workspace_bytes"}

# family -> (host signature, what the device form has behind out_len, {road tag: constants})
RENDERS = {
    "ss": ("cfg prec lo s y0 y1 ch out out_len opts", "work work_len stream opts", {"f64": {"prec": F64}, "pt": {"prec": PT, "lo": True}}),
    "ss_pt": ("cfg lo wide road bits s y0 y1 ch out out_len", "work work_len stream",
              {"plain": {"road": PLAIN, "lo": True}, "bla": {"road": BLA, "lo": True}, "scaled": {"road": SCALED, "wide": True}}),
    "ss_de": ("cfg prec lo wide road bits T s y0 y1 ch out out_len", "work work_len stream",
              {"f64": {"prec": F64}, "pt": {"prec": PT, "lo": True}, "bla": {"prec": PT, "road": BLA, "lo": True}}),
    "ss_de_pt_scaled": ("cfg wide bits T s y0 y1 ch out out_len", "work work_len stream", {"scaled": {"wide": True}}),
    "ss_adaptive": ("cfg prec lo wide road bits s thr y0 y1 ch out out_len refined", "work work_len refined stream",
                    {"f64": {"prec": F64}, "pt": {"prec": PT, "lo": True}, "bla": {"prec": PT, "road": BLA, "lo": True},
                     "scaled": {"prec": PT, "road": SCALED, "wide": True}}),
    "ss_adaptive_de": ("cfg prec lo wide road bits T s thr reach y0 y1 ch out out_len refined", "work work_len refined stream",
                       {"f64": {"prec": F64}, "pt": {"prec": PT, "lo": True}, "bla": {"prec": PT, "road": BLA, "lo": True}}),
}


def tf_spelling(fn, sig):
    """fr_x -> fr_x_tf, fr_x_device -> fr_x_tf_device, with `transfer` behind `supersample`"""
    fn = fn[:-len("_device")] + "_tf_device" if fn.endswith("_device") else fn + "_tf"
    return fn, sig.replace(" s ", " s tf ")


# name -> (C function, signature, constants of the entry, family)
ENTRIES = {}
for family, (host_sig, device_tail, roads) in RENDERS.items():
    head = host_sig.split(" out_len")[0] + " out_len "
    device_sig = head + device_tail
    for tag, consts in roads.items():
        for fn, sig in (("fr_render_rows_" + family, host_sig), ("fr_render_rows_%s_device" % family, device_sig)):
            for f, s in ((fn, sig), tf_spelling(fn, sig)):
                ENTRIES["%s[%s]" % (f, tag)] = (f, s, consts, family)
for fn, sig in (("fr_box_filter_rgb8", "src width rows s ch out out_len"), ("fr_box_filter_rgb8_device", "src width rows s ch out out_len stream"),
                ("fr_colour_ss_rgb8", "cfg z zw it width rows s ch out out_len"),
                ("fr_colour_rows_ss_device", "cfg z zw it width rows s ch out out_len stream"),
                ("fr_colour_de_ss_rgb8", "cfg z it der width rows s T ch out out_len"),
                ("fr_colour_de_rows_ss_device", "cfg z it der width rows s T ch out out_len stream")):
    for f, s in ((fn, sig), tf_spelling(fn, sig)):
        ENTRIES[f] = (f, s, {}, "filter")
for fn in ("fr_ss_workspace_bytes", "fr_ss_de_workspace_bytes"):
    ENTRIES[fn] = (fn, "cfg s y0 y1 minb bestb", {}, "workspace")
for fn in ("fr_ss_adaptive_workspace_bytes", "fr_ss_adaptive_de_workspace_bytes"):
    ENTRIES[fn] = (fn, "cfg s y0 y1 bytes", {}, "workspace")


def is_device(entry):
    return "_device" in entry


class Call:
    """the arguments of one call: a valid call of the entry to start from (its device arrays apart), which the case then spoils"""

    def __init__(self, native, entry):
        self.native, self.entry = native, entry
        self.fn, sig, consts, self.family = ENTRIES[entry]
        self.sig, self.device = sig.split(), is_device(entry)
        lib = native.load()
        cfg = native.fr_config()
        lib.fr_config_new(C.byref(cfg), 0)
        cfg.width, cfg.height, cfg.iterations = WIDTH, HEIGHT, ITERATIONS
        cfg.pos.re, cfg.pos.im, cfg.scale.re, cfg.scale.im, cfg.limit = -0.75, 0.1, 1e12, 1e12, 2.0
        self.words = [np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)]
        lib.fr_wide_from_double(-0.75, self.words[0].ctypes.data, 3)
        lib.fr_wide_from_double(0.1, self.words[1].ctypes.data, 3)
        n = S * S * WIDTH * HEIGHT  # samples of the kept views
        self.buffers = {"out": np.zeros(4 * WIDTH * HEIGHT, dtype=np.uint8), "src": np.zeros(3 * n, dtype=np.uint8),
                        "z": np.zeros(4 * n), "der": np.zeros(2 * n), "it": np.zeros(n, dtype=np.uint32)}
        self.counts = {"minb": C.c_size_t(0), "bestb": C.c_size_t(0), "bytes": C.c_size_t(0), "refined": C.c_uint64(0)}
        self.a = {"cfg": cfg, "prec": PT, "lo": None, "wide": None, "road": PLAIN, "bits": 0, "s": S, "tf": 0, "y0": 0, "y1": HEIGHT, "ch": 3,
                  "T": 1.5, "thr": 10, "reach": 2.0, "out_len": 4 * WIDTH * HEIGHT, "stream": None, "opts": None, "width": WIDTH,
                  "rows": HEIGHT, "zw": 2, "work_len": 0}
        self.a.update(consts)
        self.a["lo"] = native.Imaginary(1e-20, -1e-20) if consts.get("lo") else None
        self.a["wide"] = self.centre() if consts.get("wide") else None
        for k, v in self.counts.items():
            self.a[k] = C.byref(v)
        if self.device:
            self.a["refined"] = None
        if "work" in self.sig:  # the smallest legal workspace of the unspoiled call
            sizes = [C.c_size_t(0), C.c_size_t(0)]
            which = WORKSPACE_OF[self.family]
            rc = getattr(lib, which)(C.byref(cfg), S, 0, HEIGHT, *[C.byref(x) for x in sizes[:1 if "adaptive" in which else 2]])
            assert rc == 0 and sizes[0].value > 0, (which, rc)
            self.a["work_len"] = sizes[0].value
        self.explicit, self.reach, self.fake = {}, False, False

    def centre(self):
        p64 = C.POINTER(C.c_uint64)
        return self.native.fr_wide_centre(3, self.words[0].ctypes.data_as(p64), self.words[1].ctypes.data_as(p64))

    def has(self, *keys):
        return all(k in self.sig for k in keys)

    def array(self, key, value):
        """the case's own value for an array: None, or for a device form a made-up address"""
        self.explicit[key] = value

    def behind(self):
        """the case is about a check behind the NULL checks: a device form's other arrays are made-up addresses"""
        self.reach = True

    def args(self):
        out = []
        for i, k in enumerate(self.sig):
            if k in DEVICE_ARRAYS:
                if k in self.explicit:
                    v = self.explicit[k]
                elif not self.device:
                    v = self.buffers[k].ctypes.data
                else:
                    v = FAKE * (i + 1) if self.reach else None
            elif k == "refined" and k in self.explicit:
                v = self.explicit[k]
            else:
                v = self.a[k]
            if self.device and (k in DEVICE_ARRAYS or k == "refined") and v is not None:
                self.fake = True
            out.append(C.byref(v) if k in ("cfg", "lo", "wide") and v is not None else v)
        return out

    def need(self):
        a = self.a
        return a["ch"] * (a["cfg"].width * (a["y1"] - a["y0"]) if self.has("y0") else a["width"] * a["rows"])


# ---- the cases: each returns False where it does not apply to the entry ------------------------------------------------------


def setter(name, key, value, *also):
    def case(c):
        if not c.has(key, *also):
            return False
        c.a[key] = value

    case.__name__ = name
    return case


transfer_2 = setter("transfer_2", "tf", 2)
transfer_minus_1 = setter("transfer_minus_1", "tf", -1)
s_0 = setter("s_0", "s", 0)
s_9 = setter("s_9", "s", 9)
channels_2 = setter("channels_2", "ch", 2)
channels_5 = setter("channels_5", "ch", 5)
thickness_negative = setter("thickness_negative", "T", -0.5)
thickness_nan = setter("thickness_nan", "T", math.nan)
thickness_above_2_20 = setter("thickness_above_2_20", "T", float(2 ** 20))  # times s
reach_negative = setter("reach_negative", "reach", -1.0)
reach_inf = setter("reach_inf", "reach", math.inf)
threshold_minus_2 = setter("threshold_minus_2", "thr", -2)
threshold_256 = setter("threshold_256", "thr", 256)
precision_7 = setter("precision_7", "prec", 7)
precision_f32 = setter("precision_f32", "prec", F32, "road")  # fr_render_rows_ss takes F32 and DD
precision_dd = setter("precision_dd", "prec", DD, "road")
road_3 = setter("road_3", "road", 3)
bits_23 = setter("bits_23", "bits", 23)
bits_54 = setter("bits_54", "bits", 54)
zw_3 = setter("zw_3", "zw", 3)
arg_width_overflow = setter("arg_width_overflow", "width", 1 << 31)
arg_rows_overflow = setter("arg_rows_overflow", "rows", 1 << 31)


def y0_above_y1(c):
    if not c.has("y0"):
        return False
    c.a["y0"], c.a["y1"] = 5, 4


def y1_above_height(c):
    if not c.has("y1"):
        return False
    c.a["y1"] = HEIGHT + 1


def cfg_null(c):
    if not c.has("cfg"):
        return False
    c.a["cfg"] = None


def cfg_width_overflow(c):
    if not c.has("cfg", "y0"):
        return False
    c.a["cfg"].width = 1 << 31


def cfg_height_overflow(c):
    if not (c.has("cfg", "y0") or c.has("cfg", "der")):  # the DE recolour reads cfg->height, the plain one does not
        return False
    c.a["cfg"].height = 1 << 31


def list_overflow(c):
    """width * (y1 - y0) = 2^32 with every product of the plan in 32 bits: the adaptive calls' edge list"""
    if not c.has("thr"):
        return False
    c.a["cfg"].width, c.a["y0"], c.a["y1"] = 1 << 28, 0, 16


def limit_not_finite(c):
    if not c.has("y0", "ch") or "[f64]" in c.entry and c.family in ("ss", "ss_adaptive"):  # no DE, no deep road: the limit is not looked at
        return False
    c.a["cfg"].limit = math.inf


def iterations_above_pt_max(c):
    if not c.has("y0", "ch") or "[f64]" in c.entry:
        return False
    c.a["cfg"].iterations = PT_MAX_ITERATIONS + 1


def road_scaled_refused(c):
    """FR_PT_ROAD_SCALED where the call refuses it by name: the DE calls"""
    if not c.has("road") or c.family not in ("ss_de", "ss_adaptive_de"):
        return False
    c.a["road"] = SCALED


def road_bla_with_f64(c):
    if not c.has("prec", "road"):
        return False
    c.a["prec"], c.a["road"], c.a["lo"], c.a["wide"] = F64, BLA, None, None


def bits_minus_1(c):
    if not c.has("bits") or "scaled" in c.entry:  # SCALED PT's plain loop
        return False
    c.a["bits"] = -1


def bits_with_f64(c):
    if not c.has("prec", "bits"):
        return False
    c.a["prec"], c.a["road"], c.a["lo"], c.a["wide"], c.a["bits"] = F64, PLAIN, None, None, 30


def pos_lo_not_normalised(c):
    if not c.has("lo"):
        return False
    c.a["lo"] = c.native.Imaginary(1.0, 0.0)


def pos_lo_with_centre(c):
    if not c.has("lo", "wide"):
        return False
    c.a["lo"], c.a["wide"] = c.native.Imaginary(1e-20, 0.0), c.centre()


def pos_lo_with_f64(c):
    if not c.has("prec", "lo"):
        return False
    c.a["prec"], c.a["lo"], c.a["wide"] = F64, c.native.Imaginary(1e-20, 0.0), None
    if c.has("road"):
        c.a["road"] = PLAIN


def centre_with_f64(c):
    if not c.has("prec", "wide"):
        return False
    c.a["prec"], c.a["road"], c.a["lo"], c.a["wide"] = F64, PLAIN, None, c.centre()


def centre_null_scaled(c):
    if "scaled" not in c.entry:
        return False
    c.a["wide"] = None


def bytes_null(c):
    if not c.has("bytes"):
        return False
    c.a["bytes"] = None


def all_null(c):
    """every array NULL with a range that is not empty: a device form as it stands, a host form without its buffers"""
    if not c.has("out"):
        return False
    for k in DEVICE_ARRAYS:
        c.array(k, None)


def out_null(c):
    """the output alone: a device form's other arrays are made-up addresses"""
    if not c.has("out"):
        return False
    c.array("out", None)
    c.behind()


def input_null(c):
    if not (c.has("src") or c.has("z")):
        return False
    c.array("src" if c.has("src") else "it", None)
    c.behind()


def out_too_small(c):
    if not c.has("out_len"):
        return False
    c.a["out_len"] = c.need() - 1
    c.behind()


def out_misaligned(c):
    if not c.device or not c.has("out"):
        return False
    c.a["ch"] = 4
    c.array("out", FAKE + 1)
    c.behind()


def input_misaligned(c):
    if not c.device or not c.has("z"):
        return False
    c.array("z", FAKE + 4)
    c.behind()


def iters_misaligned(c):
    if not c.device or not c.has("it"):
        return False
    c.array("it", FAKE + 2)
    c.behind()


def work_short(c):
    if not c.has("work"):
        return False
    c.a["work_len"] -= 1
    c.behind()


def work_null(c):
    if not c.has("work"):
        return False
    c.array("work", None)
    c.behind()


def work_misaligned(c):
    if not c.has("work") or c.family in ("ss", "ss_pt"):  # packed r,g,b bands: no alignment rule, the call would get through
        return False
    c.array("work", FAKE + 4)
    c.behind()


def refined_misaligned(c):
    if not c.device or not c.has("refined"):
        return False
    c.explicit["refined"] = FAKE + 4
    c.behind()


def s_1_without_workspace(c):
    """s = 1 of the packed-RGB bands needs no workspace: what is refused is the output"""
    if not c.has("work") or c.family not in ("ss", "ss_pt"):
        return False
    c.a["s"], c.a["work_len"] = 1, 0
    c.array("work", None)
    c.array("out", None)


def noop_empty_rows(c):
    """y0 == y1: FR_OK with NULL buffers (the workspace calls: sizes of 0)"""
    if not c.has("y0"):
        return False
    c.a["y0"] = c.a["y1"] = 5
    all_null(c)


def noop_width_0(c):
    if not (c.has("cfg", "y0") or c.has("width")):
        return False
    if c.has("width"):
        c.a["width"] = 0
    else:
        c.a["cfg"].width = 0
    all_null(c)


def noop_rows_0(c):
    if not c.has("rows"):
        return False
    c.a["rows"] = 0
    all_null(c)


def both(first, second):
    """a call wrong in two ways: which error it reports pins the order of the checks"""

    def case(c):
        if first(c) is False or second(c) is False:
            return False

    case.__name__ = first.__name__ + "+" + second.__name__
    return case


SINGLES = [transfer_2, transfer_minus_1, s_0, s_9, y0_above_y1, y1_above_height, channels_2, channels_5, thickness_negative, thickness_nan,
           thickness_above_2_20, reach_negative, reach_inf, threshold_minus_2, threshold_256, precision_7, precision_f32, precision_dd,
           road_3, road_scaled_refused, road_bla_with_f64, bits_23, bits_54, bits_minus_1, bits_with_f64, zw_3, pos_lo_not_normalised,
           pos_lo_with_centre, pos_lo_with_f64, centre_with_f64, centre_null_scaled, cfg_null, cfg_width_overflow, cfg_height_overflow,
           arg_width_overflow, arg_rows_overflow, list_overflow, limit_not_finite, iterations_above_pt_max, bytes_null, all_null,
           out_null, input_null, out_too_small, out_misaligned, input_misaligned, iters_misaligned, work_short, work_null,
           work_misaligned, refined_misaligned, s_1_without_workspace]
NOOPS = [noop_empty_rows, noop_width_0, noop_rows_0]
# every adjacent pair of the calls' documented check orders
ADJACENT = [(cfg_null, s_0), (s_0, cfg_width_overflow), (s_9, arg_width_overflow), (cfg_width_overflow, cfg_height_overflow),
            (arg_width_overflow, arg_rows_overflow), (cfg_height_overflow, y0_above_y1), (cfg_height_overflow, channels_2),
            (y0_above_y1, channels_2), (y1_above_height, channels_2), (arg_rows_overflow, channels_2), (zw_3, s_0), (cfg_null, zw_3),
            (channels_2, thickness_negative), (thickness_negative, reach_negative), (reach_negative, threshold_256),
            (thickness_negative, threshold_256), (channels_2, threshold_256), (threshold_256, list_overflow), (list_overflow, precision_f32),
            (list_overflow, road_scaled_refused), (list_overflow, road_3), (road_scaled_refused, precision_f32), (precision_f32, road_3),
            (precision_dd, road_3), (precision_7, road_3), (road_3, pos_lo_with_centre), (road_3, bits_23), (pos_lo_with_centre, road_bla_with_f64),
            (pos_lo_with_centre, bits_23), (pos_lo_with_centre, bits_54), (centre_with_f64, bits_23), (pos_lo_with_f64, bits_with_f64),
            (centre_with_f64, pos_lo_with_f64), (bits_23, pos_lo_not_normalised), (bits_23, limit_not_finite), (bits_54, iterations_above_pt_max),
            (pos_lo_not_normalised, limit_not_finite), (limit_not_finite, iterations_above_pt_max), (channels_2, precision_7),
            (channels_2, pos_lo_with_f64), (channels_2, bits_23), (channels_2, road_3), (thickness_negative, road_3),
            (thickness_negative, road_scaled_refused), (thickness_negative, precision_7), (thickness_negative, bits_23),
            (threshold_256, precision_7), (threshold_256, road_3), (centre_null_scaled, bits_23), (centre_null_scaled, channels_2),
            (centre_null_scaled, thickness_negative), (precision_7, pos_lo_not_normalised), (precision_7, pos_lo_with_f64),
            (s_0, bytes_null), (y0_above_y1, bytes_null)]
# the domain against the buffers, and the buffer rules among themselves: workspace against output is where
# fr_render_rows_ss_device and the _pt / _de / adaptive calls differ
BUFFERS = [(limit_not_finite, all_null), (bits_23, all_null), (precision_7, all_null), (road_3, out_too_small), (channels_2, out_too_small),
           (pos_lo_not_normalised, work_short), (iterations_above_pt_max, work_null), (limit_not_finite, refined_misaligned),
           (threshold_256, refined_misaligned), (thickness_negative, work_misaligned), (zw_3, input_null), (thickness_negative, input_null),
           (channels_5, out_misaligned), (s_9, out_null), (input_null, out_too_small), (input_null, input_misaligned), (out_too_small, input_misaligned),
           (input_misaligned, out_misaligned), (iters_misaligned, out_misaligned), (out_too_small, iters_misaligned),
           (work_short, out_null), (work_short, out_too_small), (work_short, out_misaligned), (work_short, work_null), (work_short, work_misaligned),
           (work_null, out_null), (work_null, out_too_small), (work_null, out_misaligned), (work_misaligned, out_null),
           (work_misaligned, out_too_small), (work_misaligned, out_misaligned), (out_too_small, out_misaligned), (out_null, refined_misaligned),
           (out_too_small, refined_misaligned), (out_misaligned, refined_misaligned), (work_short, refined_misaligned),
           (work_null, refined_misaligned), (work_misaligned, refined_misaligned)]
# a range without pixels against the domain and the buffers: the domain still refuses, the buffers are not looked at
EMPTY = [(noop_empty_rows, bits_23), (noop_empty_rows, precision_7), (noop_empty_rows, limit_not_finite), (noop_empty_rows, channels_2),
         (noop_empty_rows, thickness_negative), (noop_empty_rows, threshold_256), (noop_empty_rows, work_short), (noop_empty_rows, out_too_small),
         (noop_empty_rows, refined_misaligned), (noop_width_0, refined_misaligned), (noop_width_0, channels_2), (noop_width_0, work_short),
         (noop_width_0, road_3), (noop_rows_0, zw_3), (noop_rows_0, s_0), (noop_rows_0, thickness_negative), (noop_rows_0, out_too_small)]
CASES = (SINGLES + NOOPS + [both(transfer_2, x) for x in SINGLES[2:] + NOOPS] + [both(a, b) for a, b in ADJACENT + BUFFERS + EMPTY])


def calls(native):
    """(id, C function name, arguments, keep-alive, fake) of every case of every entry it applies to"""
    for entry in ENTRIES:
        for case in CASES:
            c = Call(native, entry)
            if case(c) is False:
                continue
            args = c.args()
            yield "%s :: %s" % (entry.replace("_tf", ""), case.__name__), c.fn, args, c, c.fake


def pack(results):
    """{id: [code, text]} -> the golden file's matrix: row[entry][k] numbers the answer to cases[k], -1 where it does not apply"""
    answers = sorted({(rc, text) for rc, text in results.values()})
    cases = sorted({key.split(" :: ")[1] for key in results})
    rows = {}
    for key, (rc, text) in results.items():
        entry, case = key.split(" :: ")
        rows.setdefault(entry, [-1] * len(cases))[cases.index(case)] = answers.index((rc, text))
    return {"answers": [list(a) for a in answers], "cases": cases, "rows": rows}


def unpack(golden):
    """the golden file -> {id: [code, text]}"""
    return {"%s :: %s" % (entry, case): golden["answers"][k]
            for entry, row in golden["rows"].items() for case, k in zip(golden["cases"], row) if k >= 0}


def base_calls(native):
    """the unspoiled call of every entry, a device form's arrays made up: on a machine WITHOUT a device (only there may it be
    made) it answers FR_ERR_NO_DEVICE, the workspace calls FR_OK — so each case above is wrong in what it spoils and nothing else"""
    for entry in ENTRIES:
        c = Call(native, entry)
        c.behind()
        if c.device and c.has("refined"):
            c.explicit["refined"] = FAKE
        yield entry, c.fn, c.args(), c
