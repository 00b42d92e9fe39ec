"""The table behind tests/test_stream_order_cases_cpu.py and tests/test_gpu_stream_order.py: every entry point of the C ABI that
takes a caller's stream (`void *hip_stream` in include/fractal_hip.h, "STREAM ORDER"), one record per entry point and, where the
roads differ in their launches, one per road (F64 / F32 / DD / PT with a dd centre / WIDE PT / BLA-PT / SCALED PT).  Importable
without a device and without the library: building a call (Call) needs the library, the table does not.

A record is
  fn      the C function;
  sig     the order of its arguments, as keys of one argument dict (tests/deep_call_cases.py's style);
  view    one of VIEWS, the small asymmetric view the call runs on;
  arrays  every device pointer argument with its class:
            INPUT      read only (the kept arrays of a recolour, a filter's source);
            STATE      read and written in place (the extend calls);
            OUTPUT     written;
            WORKSPACE  lent to the call, which keeps its lists and their counters there;
  consts  the remaining arguments (precision, road, bits, supersample, transfer, channels, ...);
  source  for a record with INPUT or STATE arrays: (id of the record whose outputs are its true inputs, how that call differs:
          `low` = at the cap an extend record starts from, `big` = it renders cfg_s, `rename` = {its key: this record's key});
  roll    by how many pixels each INPUT / STATE array is rolled to make the POISON (below);
  waits   a reason, where the header itself lets the call block the host even with its caches warm; None otherwise.

POISON.  The gated test fills inputs and state with poison before the true bytes are copied in on the caller's stream.  Poison is
the TRUE arrays of the same view and cap rolled by a few pixels (ROLL; all arrays of a record by the same amount), so every
escape index and every orbit index m in it is valid for this view's orbits and tables: a misordered kernel that reads poison
computes something wrong, never something out of bounds.  Never another view's state, never random bits.  One exception to "the
same amount": fr_view_stats_device is invariant under a joint permutation of its pixels, so its iters are rolled further than
its z — the statistics of the mismatched pairs differ.

The views are the suite's own: the seahorse valley of shallow_random_views.EDGES for F64 / F32 (61 x 47 at a scale of 60 x 42 and
a cap of 1000, where a third of the pixels are stable, the escape indices fill 700 bins of the statistics and the border is long
enough for the teeth condition of fr_view_stats_device: tests/test_shallow_random_cpu.py's models give 3 % there), and deep_truth's
small views for the deep roads (DD_1E25 for DD and the dd-centred PT roads, M_OFF_299 for WIDE PT and BLA-PT, MINI_OFF_860 past
2^440).  The caps follow deep_truth's recorded escape indices — 55 .. 75 on DD_1E25, 187 .. 201 on M_OFF_299, 2189 .. 3204 on
MINI_OFF_860 — so that every pixel escapes below the cap of the first two, and an extend record starts from the MEDIAN index:
half the pixels are still running at the lower cap and the extension has work to do."""
import ctypes as C
from collections import namedtuple

INPUT, STATE, OUTPUT, WORKSPACE = "input", "state", "output", "workspace"
F64, F32, DD, PT = 0, 1, 2, 3
PLAIN, BLA, SCALED = 0, 1, 2  # fr_pt_road
S = 2  # the supersample of every record that has one
ROLL = 3  # pixels
STATS_BYTES = 8248  # sizeof(struct fr_view_stats)
THICKNESS, THRESHOLD, REACH = 1.5, 1, 2.0  # a threshold of one grey level: the deep views are smooth, and their calls must refine

# view -> (deep_truth view or None, width, height, cap, the cap an extend record starts from)
VIEWS = {
    "shallow": (None, 61, 47, 1000, 300),
    "dd": ("DD_1E25", 32, 24, 200, 58),
    "wide": ("M_OFF_299", 37, 21, 400, 189),
    "scaled": ("MINI_OFF_860", 24, 16, 3204, 2362),
}

Record = namedtuple("Record", "id fn sig view arrays consts source roll waits")
RECORDS = {}

# bytes per unit of an array, and its unit: "px" = a pixel of rows [y0, y1) of cfg, "big" = a pixel of cfg_s, "one" = the array
WIDTHS = {"it": 4, "dz": 16, "m": 4, "der": 16, "src": 3, "stats": STATS_BYTES, "refined": 8, "dist": 8}


def add(id, fn, sig, view, arrays, source=None, roll=None, waits=None, **consts):
    assert id not in RECORDS, id
    arrays = dict(arrays)
    assert set(arrays) <= set(sig.split()), (id, arrays)
    needs = any(c in (INPUT, STATE) for c in arrays.values())
    assert needs == (source is not None), id
    r = {k: ROLL for k, c in arrays.items() if c in (INPUT, STATE)}
    r.update(roll or {})
    RECORDS[id] = Record(id, fn, sig, view, arrays, consts, source, r, waits)


def tf(sig):
    """the signature of a _tf twin: `int transfer` behind `supersample`"""
    return sig.replace(" s ", " s tf ")


OUT = {"out": OUTPUT}
ZI = {"z": OUTPUT, "it": OUTPUT}
ZID = dict(ZI, der=OUTPUT)
ST = dict(ZI, dz=OUTPUT, m=OUTPUT)
STD = dict(ST, der=OUTPUT)
SS = {"out": OUTPUT, "work": WORKSPACE}
AD = dict(SS, refined=OUTPUT)


def state(arrays):
    return {k: STATE for k in arrays}


def inputs(arrays, **more):
    return dict({k: INPUT for k in arrays}, **more)


# ---- whole-image and row renders: F64 / F32 take the strip kernels, DD and PT (pos_lo = 0) their own ------------------------------
ROWS = "cfg prec y0 y1 out out_len stream"
for tag, prec, view in (("f64", F64, "shallow"), ("f32", F32, "shallow"), ("dd", DD, "dd"), ("pt", PT, "dd")):
    add("render_rows_rgb8[%s]" % tag, "fr_render_rows_rgb8_device", ROWS, view, OUT, prec=prec)
add("render_rows_rgba8[f64]", "fr_render_rows_rgba8_device", ROWS, "shallow", OUT, prec=F64, ch=4)
add("render_rows_rgb8_opts[f64]", "fr_render_rows_rgb8_device_opts", ROWS + " opts", "shallow", OUT, prec=F64)
add("render_rows_rgb8_opts[f32 two-pass]", "fr_render_rows_rgb8_device_opts", ROWS + " opts", "shallow", OUT, prec=F32, tile=11)
add("render_rows_rgba8_opts[f64 two-pass]", "fr_render_rows_rgba8_device_opts", ROWS + " opts", "shallow", OUT, prec=F64, ch=4, tile=11)
add("render_rows_rgba8_opts[f32 no palette]", "fr_render_rows_rgba8_device_opts", ROWS + " opts", "shallow", OUT, prec=F32, ch=4,
    smooth=0, palette=0)
add("render_rows_rgb8[f64 palette]", "fr_render_rows_rgb8_device", ROWS, "shallow", OUT, prec=F64, smooth=0)
CYCLIC = "cfg prec block_rows first_block block_stride out out_len stream rows_written"
RANGE = "cfg prec block_rows first_block block_stride max_blocks dest_is_image out out_len stream rows_written"
add("block_cyclic[f64]", "fr_render_block_cyclic_rgb8_device", CYCLIC, "shallow", OUT, prec=F64, block_rows=5, first_block=1, block_stride=2)
add("block_cyclic_range[f32 packed]", "fr_render_block_cyclic_range_rgb8_device", RANGE, "shallow", OUT, prec=F32, block_rows=3,
    first_block=0, block_stride=3, max_blocks=2, dest_is_image=0)
add("block_cyclic_range[f64 in place]", "fr_render_block_cyclic_range_rgb8_device", RANGE, "shallow", OUT, prec=F64, block_rows=8,
    first_block=1, block_stride=2, max_blocks=0, dest_is_image=1)
add("block_cyclic_range_opts[f64 in place]", "fr_render_block_cyclic_range_rgb8_device_opts", RANGE + " opts", "shallow", OUT, prec=F64,
    block_rows=8, first_block=0, block_stride=2, max_blocks=0, dest_is_image=1, tile=11)
DEEP_ROWS = "cfg {c} y0 y1 ch out out_len stream"
add("render_rows_dd", "fr_render_rows_dd_device", DEEP_ROWS.format(c="lo"), "dd", OUT)
add("render_rows_dd[rgba]", "fr_render_rows_dd_device", DEEP_ROWS.format(c="lo"), "dd", OUT, ch=4)
add("render_rows_pt", "fr_render_rows_pt_device", DEEP_ROWS.format(c="lo"), "dd", OUT)
add("render_rows_pt[rgba]", "fr_render_rows_pt_device", DEEP_ROWS.format(c="lo"), "dd", OUT, ch=4)
add("render_rows_pt_wide", "fr_render_rows_pt_wide_device", DEEP_ROWS.format(c="wide"), "wide", OUT)
add("render_rows_pt_wide[rgba]", "fr_render_rows_pt_wide_device", DEEP_ROWS.format(c="wide"), "wide", OUT, ch=4)
add("render_rows_pt_bla[dd]", "fr_render_rows_pt_bla_device", DEEP_ROWS.format(c="lo wide bits"), "dd", OUT, bits=0)
add("render_rows_pt_bla[wide]", "fr_render_rows_pt_bla_device", DEEP_ROWS.format(c="lo wide bits"), "wide", OUT, bits=0, ch=4)
add("render_rows_pt_scaled[plain]", "fr_render_rows_pt_scaled_device", DEEP_ROWS.format(c="wide bits"), "scaled", OUT, bits=-1)
add("render_rows_pt_scaled[table]", "fr_render_rows_pt_scaled_device", DEEP_ROWS.format(c="wide bits"), "scaled", OUT, bits=0, ch=4)

# ---- raw results and resumable states --------------------------------------------------------------------------------------------
ESCAPE = "cfg prec lo y0 y1 zw z it stream opts"
for tag, prec, view, zw in (("f64", F64, "shallow", 2), ("f32", F32, "shallow", 2), ("dd", DD, "dd", 4), ("pt", PT, "dd", 2)):
    add("escape_rows[%s]" % tag, "fr_escape_rows_device", ESCAPE, view, ZI, prec=prec, zw=zw)
add("escape_rows_pt_bla[dd]", "fr_escape_rows_pt_bla_device", "cfg lo wide bits y0 y1 z it stream", "dd", ZI, bits=0)
add("escape_rows_pt_bla[wide]", "fr_escape_rows_pt_bla_device", "cfg lo wide bits y0 y1 z it stream", "wide", ZI, bits=53)
add("escape_rows_pt_scaled[plain]", "fr_escape_rows_pt_scaled_device", "cfg wide bits y0 y1 z it stream", "scaled", ZI, bits=-1)
add("escape_rows_pt_scaled[table]", "fr_escape_rows_pt_scaled_device", "cfg wide bits y0 y1 z it stream", "scaled", ZI, bits=0)
add("escape_rows_pt_state", "fr_escape_rows_pt_state_device", "cfg lo y0 y1 z it dz m stream", "dd", ST)
add("escape_rows_pt_wide_state", "fr_escape_rows_pt_wide_state_device", "cfg wide y0 y1 z it dz m stream", "wide", ST)
add("escape_rows_pt_scaled_state", "fr_escape_rows_pt_scaled_state_device", "cfg wide y0 y1 z it dz m stream", "scaled", ST)
add("escape_rows_de[f64]", "fr_escape_rows_de_device", "cfg prec lo y0 y1 z it der stream", "shallow", ZID, prec=F64)
add("escape_rows_de[pt]", "fr_escape_rows_de_device", "cfg prec lo y0 y1 z it der stream", "dd", ZID, prec=PT)
add("escape_rows_de_pt_wide", "fr_escape_rows_de_pt_wide_device", "cfg wide y0 y1 z it der stream", "wide", ZID)
add("escape_rows_de_pt_bla[dd]", "fr_escape_rows_de_pt_bla_device", "cfg lo wide bits y0 y1 z it der stream", "dd", ZID, bits=0)
add("escape_rows_de_pt_bla[wide]", "fr_escape_rows_de_pt_bla_device", "cfg lo wide bits y0 y1 z it der stream", "wide", ZID, bits=0)
add("escape_rows_de_pt_scaled[plain]", "fr_escape_rows_de_pt_scaled_device", "cfg wide bits y0 y1 z it der stream", "scaled", ZID, bits=-1)
add("escape_rows_de_pt_scaled[table]", "fr_escape_rows_de_pt_scaled_device", "cfg wide bits y0 y1 z it der stream", "scaled", ZID, bits=0)
add("escape_rows_de_pt_state[dd]", "fr_escape_rows_de_pt_state_device", "cfg lo wide y0 y1 z it dz m der stream", "dd", STD)
add("escape_rows_de_pt_state[wide]", "fr_escape_rows_de_pt_state_device", "cfg lo wide y0 y1 z it dz m der stream", "wide", STD)
add("escape_rows_de_pt_scaled_state", "fr_escape_rows_de_pt_scaled_state_device", "cfg wide y0 y1 z it dz m der stream", "scaled", STD)

# ---- the extend calls: the state of the source at the lower cap, continued in place ---------------------------------------------------
EXTEND = "cfg prec lo y0 y1 from zw z it stream opts"
for tag, prec, view, zw in (("f64", F64, "shallow", 2), ("f32", F32, "shallow", 2), ("dd", DD, "dd", 4)):
    add("escape_extend[%s]" % tag, "fr_escape_extend_device", EXTEND, view, state(ZI), source=("escape_rows[%s]" % tag, {"low": True}),
        prec=prec, zw=zw)
add("escape_extend_pt", "fr_escape_extend_pt_device", "cfg lo y0 y1 from z it dz m stream", "dd", state(ST),
    source=("escape_rows_pt_state", {"low": True}))
add("escape_extend_pt_wide", "fr_escape_extend_pt_wide_device", "cfg wide y0 y1 from z it dz m stream", "wide", state(ST),
    source=("escape_rows_pt_wide_state", {"low": True}))
add("escape_extend_pt_scaled", "fr_escape_extend_pt_scaled_device", "cfg wide y0 y1 from z it dz m stream", "scaled", state(ST),
    source=("escape_rows_pt_scaled_state", {"low": True}))
add("escape_extend_de[f64]", "fr_escape_extend_de_device", "cfg prec y0 y1 from z it der stream", "shallow", state(ZID),
    source=("escape_rows_de[f64]", {"low": True}), prec=F64)
add("escape_extend_de_pt[dd]", "fr_escape_extend_de_pt_device", "cfg lo wide y0 y1 from z it dz m der stream", "dd", state(STD),
    source=("escape_rows_de_pt_state[dd]", {"low": True}))
add("escape_extend_de_pt[wide]", "fr_escape_extend_de_pt_device", "cfg lo wide y0 y1 from z it dz m der stream", "wide", state(STD),
    source=("escape_rows_de_pt_state[wide]", {"low": True}))
add("escape_extend_de_pt_scaled", "fr_escape_extend_de_pt_scaled_device", "cfg wide y0 y1 from z it dz m der stream", "scaled", state(STD),
    source=("escape_rows_de_pt_scaled_state", {"low": True}))

# ---- recolour, distance, statistics, filter: plain arrays in, plain arrays out -------------------------------------------------------
add("colour_rgb8", "fr_colour_rgb8_device", "cfg z it n out out_len stream", "shallow", inputs(ZI, out=OUTPUT), source=("escape_rows[f64]", {}))
add("colour_rows[f64 rgb]", "fr_colour_rows_device", "cfg z zw it n ch out out_len stream", "shallow", inputs(ZI, out=OUTPUT),
    source=("escape_rows[f64]", {}), zw=2)
add("colour_rows[dd rgba]", "fr_colour_rows_device", "cfg z zw it n ch out out_len stream", "dd", inputs(ZI, out=OUTPUT),
    source=("escape_rows[dd]", {}), zw=4, ch=4)
add("view_stats[f64]", "fr_view_stats_device", "cfg z zw it n stats stream", "shallow", inputs(ZI, stats=OUTPUT),
    source=("escape_rows[f64]", {}), roll={"it": 11}, zw=2)
add("distance_rows", "fr_distance_rows_device", "cfg z it der n dist stream", "shallow", inputs(ZID, dist=OUTPUT),
    source=("escape_rows_de[f64]", {}))
add("colour_de_rows[rgb]", "fr_colour_de_rows_device", "cfg z it der n thick ch out stream", "shallow", inputs(ZID, out=OUTPUT),
    source=("escape_rows_de[f64]", {}))
add("colour_de_rows[rgba wide]", "fr_colour_de_rows_device", "cfg z it der n thick ch out stream", "wide", inputs(ZID, out=OUTPUT),
    source=("escape_rows_de_pt_wide", {}), ch=4)
BOX = "src width rows s ch out out_len stream"
add("box_filter[rgb]", "fr_box_filter_rgb8_device", BOX, "shallow", {"src": INPUT, "out": OUTPUT},
    source=("render_rows_rgb8[f64]", {"big": True, "rename": {"out": "src"}}))
add("box_filter_tf[rgba]", "fr_box_filter_rgb8_tf_device", tf(BOX), "shallow", {"src": INPUT, "out": OUTPUT},
    source=("render_rows_rgb8[f64]", {"big": True, "rename": {"out": "src"}}), tf=1, ch=4)
COLOUR_SS = "cfg z zw it width rows s ch out out_len stream"
add("colour_rows_ss[rgb]", "fr_colour_rows_ss_device", COLOUR_SS, "shallow", inputs(ZI, out=OUTPUT), source=("escape_rows[f64]", {"big": True}), zw=2)
add("colour_rows_ss_tf[rgba]", "fr_colour_rows_ss_tf_device", tf(COLOUR_SS), "shallow", inputs(ZI, out=OUTPUT),
    source=("escape_rows[f64]", {"big": True}), zw=2, tf=1, ch=4)
COLOUR_DE_SS = "cfg z it der width rows s thick ch out out_len stream"
add("colour_de_rows_ss[rgba]", "fr_colour_de_rows_ss_device", COLOUR_DE_SS, "shallow", inputs(ZID, out=OUTPUT),
    source=("escape_rows_de[f64]", {"big": True}), ch=4)
add("colour_de_rows_ss_tf[rgb]", "fr_colour_de_rows_ss_tf_device", "cfg z it der width rows s tf thick ch out out_len stream", "shallow",
    inputs(ZID, out=OUTPUT), source=("escape_rows_de[f64]", {"big": True}), tf=1)

# ---- supersampled renders: band loops through a lent workspace ---------------------------------------------------------------------------
SS_F = "cfg prec lo s y0 y1 ch out out_len work work_len stream opts"
for tag, prec, view in (("f64", F64, "shallow"), ("f32", F32, "shallow"), ("dd", DD, "dd"), ("pt", PT, "dd")):
    add("render_rows_ss[%s]" % tag, "fr_render_rows_ss_device", SS_F, view, SS, prec=prec, ws="ss")
add("render_rows_ss_tf[f64 rgba]", "fr_render_rows_ss_tf_device", tf(SS_F), "shallow", SS, prec=F64, ws="ss", tf=1, ch=4)
add("render_rows_ss_tf[pt]", "fr_render_rows_ss_tf_device", tf(SS_F), "dd", SS, prec=PT, ws="ss", tf=1)
SS_PT = "cfg lo wide road bits s y0 y1 ch out out_len work work_len stream"
for tag, view, road, bits in (("dd", "dd", PLAIN, 0), ("wide", "wide", PLAIN, 0), ("bla", "wide", BLA, 0), ("scaled", "scaled", SCALED, -1),
                              ("scaled table", "scaled", SCALED, 0)):
    add("render_rows_ss_pt[%s]" % tag, "fr_render_rows_ss_pt_device", SS_PT, view, SS, road=road, bits=bits, ws="ss")
add("render_rows_ss_pt_tf[bla rgba]", "fr_render_rows_ss_pt_tf_device", tf(SS_PT), "wide", SS, road=BLA, bits=0, ws="ss", tf=1, ch=4)
add("render_rows_ss_pt_tf[scaled]", "fr_render_rows_ss_pt_tf_device", tf(SS_PT), "scaled", SS, road=SCALED, bits=-1, ws="ss", tf=1)
SS_DE = "cfg prec lo wide road bits thick s y0 y1 ch out out_len work work_len stream"
DE_ROADS = (("f64", "shallow", F64, PLAIN), ("pt dd", "dd", PT, PLAIN), ("pt wide", "wide", PT, PLAIN), ("bla dd", "dd", PT, BLA),
            ("bla wide", "wide", PT, BLA))
for tag, view, prec, road in DE_ROADS:
    add("render_rows_ss_de[%s]" % tag, "fr_render_rows_ss_de_device", SS_DE, view, SS, prec=prec, road=road, bits=0, ws="ss_de")
add("render_rows_ss_de_tf[f64 rgba]", "fr_render_rows_ss_de_tf_device", tf(SS_DE), "shallow", SS, prec=F64, road=PLAIN, bits=0, ws="ss_de",
    tf=1, ch=4)
add("render_rows_ss_de_tf[bla wide]", "fr_render_rows_ss_de_tf_device", tf(SS_DE), "wide", SS, prec=PT, road=BLA, bits=0, ws="ss_de", tf=1)
SS_DE_SC = "cfg wide bits thick s y0 y1 ch out out_len work work_len stream"
add("render_rows_ss_de_pt_scaled[plain]", "fr_render_rows_ss_de_pt_scaled_device", SS_DE_SC, "scaled", SS, bits=-1, ws="ss_de")
add("render_rows_ss_de_pt_scaled[table rgba]", "fr_render_rows_ss_de_pt_scaled_device", SS_DE_SC, "scaled", SS, bits=0, ws="ss_de", ch=4)
add("render_rows_ss_de_pt_scaled_tf[plain]", "fr_render_rows_ss_de_pt_scaled_tf_device", tf(SS_DE_SC), "scaled", SS, bits=-1, ws="ss_de", tf=1)

# ---- adaptive supersampling: base image, mark, list, refine, filter; the count of refined pixels is an output --------------------------------
AD_F = "cfg prec lo wide road bits s thr y0 y1 ch out out_len work work_len refined stream"
AD_ROADS = (("f64", "shallow", F64, PLAIN, 0), ("pt dd", "dd", PT, PLAIN, 0), ("pt wide", "wide", PT, PLAIN, 0),
            ("bla wide", "wide", PT, BLA, 0), ("scaled", "scaled", PT, SCALED, -1), ("scaled table", "scaled", PT, SCALED, 0))
for tag, view, prec, road, bits in AD_ROADS:
    add("render_rows_ss_adaptive[%s]" % tag, "fr_render_rows_ss_adaptive_device", AD_F, view, AD, prec=prec, road=road, bits=bits, ws="ss_adaptive")
add("render_rows_ss_adaptive_tf[f64 rgba]", "fr_render_rows_ss_adaptive_tf_device", tf(AD_F), "shallow", AD, prec=F64, road=PLAIN, bits=0,
    ws="ss_adaptive", tf=1, ch=4)
add("render_rows_ss_adaptive_tf[bla wide]", "fr_render_rows_ss_adaptive_tf_device", tf(AD_F), "wide", AD, prec=PT, road=BLA, bits=0,
    ws="ss_adaptive", tf=1)
AD_DE = "cfg prec lo wide road bits thick s thr reach y0 y1 ch out out_len work work_len refined stream"
for tag, view, prec, road in DE_ROADS:
    add("render_rows_ss_adaptive_de[%s]" % tag, "fr_render_rows_ss_adaptive_de_device", AD_DE, view, AD, prec=prec, road=road, bits=0,
        ws="ss_adaptive_de")
add("render_rows_ss_adaptive_de_tf[f64 rgba]", "fr_render_rows_ss_adaptive_de_tf_device", tf(AD_DE), "shallow", AD, prec=F64, road=PLAIN,
    bits=0, ws="ss_adaptive_de", tf=1, ch=4)
add("render_rows_ss_adaptive_de_tf[pt wide]", "fr_render_rows_ss_adaptive_de_tf_device", tf(AD_DE), "wide", AD, prec=PT, road=PLAIN, bits=0,
    ws="ss_adaptive_de", tf=1)
AD_DE_SC = "cfg wide bits thick s thr reach y0 y1 ch out out_len work work_len refined stream"
add("render_rows_ss_adaptive_de_pt_scaled[plain]", "fr_render_rows_ss_adaptive_de_pt_scaled_device", AD_DE_SC, "scaled", AD, bits=-1,
    ws="ss_adaptive_de")
add("render_rows_ss_adaptive_de_pt_scaled[table rgba]", "fr_render_rows_ss_adaptive_de_pt_scaled_device", AD_DE_SC, "scaled", AD, bits=0,
    ws="ss_adaptive_de", ch=4)
add("render_rows_ss_adaptive_de_pt_scaled_tf[plain]", "fr_render_rows_ss_adaptive_de_pt_scaled_tf_device", tf(AD_DE_SC), "scaled", AD, bits=-1,
    ws="ss_adaptive_de", tf=1)

# A stream-taking entry point of the header that has no record: name -> why.  (fr_render_rgb8_multi_device takes no stream: it
# renders on streams of its own by contract, and is not one of them.)
EXCLUDED = {}

WORKSPACE_CALLS = {"ss": ("fr_ss_workspace_bytes", 2), "ss_de": ("fr_ss_de_workspace_bytes", 2),
                   "ss_adaptive": ("fr_ss_adaptive_workspace_bytes", 1), "ss_adaptive_de": ("fr_ss_adaptive_de_workspace_bytes", 1)}
OPTS_FIELDS = ("tile", "loop_mode", "palette")
CFG_FIELDS = ("smooth", "inside", "exposure")


def functions():
    return {r.fn for r in RECORDS.values()}


def header_stream_functions(text):
    """every function of a C header that has a `void *hip_stream` parameter"""
    import re

    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(fr_\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bvoid\s*\*\s*hip_stream\b", m.group(2))}


# ---- building a call: needs the package (ctypes structures) and, for the workspace sizes and the default config, the library -------------


class View:
    """cfg, pos_lo and the wide centre of one of VIEWS at a cap; big: cfg_s, S times as wide and as high"""

    def __init__(self, native, name, cap=None, big=False):
        truth, width, height, top, low = VIEWS[name]
        self.name, self.low = name, low
        cfg = native.fr_config()
        native.load().fr_config_new(C.byref(cfg), 0)
        self.lo = self.wide = self.keep = None
        if truth is None:  # the seahorse valley of shallow_random_views.EDGES, with unequal axes
            cfg.width, cfg.height = width, height
            cfg.pos.re, cfg.pos.im, cfg.scale.re, cfg.scale.im = -0.745, 0.11, 60.0, 42.0
        else:
            import deep_truth

            v = deep_truth.View(truth)
            assert (v.width, v.height) == (width, height) and top <= v.cap
            v.fill(cfg)
            if v.kind == "wide":
                p64 = C.POINTER(C.c_uint64)
                self.keep = v.words
                self.wide = native.fr_wide_centre(v.n, v.words[0].ctypes.data_as(p64), v.words[1].ctypes.data_as(p64))
            else:
                self.lo = native.Imaginary(*v.pos_lo)
        cfg.iterations = top if cap is None else cap
        self.width, self.height = cfg.width, cfg.height  # of the OUTPUT
        if big:
            cfg.width, cfg.height = cfg.width * S, cfg.height * S
        self.cfg = cfg


class Call:
    """One valid call of a record.  sizes: bytes of every array; args(ptrs, stream): the ctypes arguments."""

    def __init__(self, native, rec, cap=None, big=False):
        self.native, self.rec, self.sig = native, rec, rec.sig.split()
        c = rec.consts
        self.view = v = View(native, rec.view, cap=cap, big=big)
        for f in CFG_FIELDS:
            if f in c:
                setattr(v.cfg, f, c[f])
        self.ch = c.get("ch", 3)
        self.y0, self.y1 = 0, v.cfg.height
        px = v.cfg.width * v.cfg.height
        in_big = {k for k in ("z", "it", "der", "src") if "width" in self.sig}  # the filter calls: arrays of cfg_s, output of cfg
        self.rows_written = C.c_uint64(0)
        if "block_rows" in self.sig:
            lib = native.load()
            rows = lib.fr_block_cyclic_rows(v.cfg.height, c["block_rows"], c["first_block"], c["block_stride"])
            if c.get("max_blocks"):
                rows = min(rows, c["max_blocks"] * c["block_rows"])
            self.rows = rows
        self.sizes = {}
        for k in rec.arrays:
            if k == "work":
                self.sizes[k] = self.workspace_bytes()
            elif k in ("stats", "refined"):
                self.sizes[k] = WIDTHS[k]
            elif k == "out" and "block_rows" in self.sig:
                self.sizes[k] = 3 * v.cfg.width * (v.cfg.height if c.get("dest_is_image") else self.rows)
            else:
                width = 8 * c.get("zw", 2) if k == "z" else self.ch if k == "out" else WIDTHS[k]
                self.sizes[k] = width * px * (S * S if k in in_big else 1)
        self.opts = None
        if "opts" in self.sig and any(f in c for f in OPTS_FIELDS):
            self.opts = native.fr_render_opts()
            native.load().fr_render_opts_init(C.byref(self.opts))
            for f in OPTS_FIELDS:
                if f in c:
                    setattr(self.opts, f, c[f])

    def pixel_bytes(self, key):
        """bytes of one pixel of an array: what a roll by one pixel moves"""
        c = self.rec.consts
        return 8 * c.get("zw", 2) if key == "z" else self.ch if key == "out" else WIDTHS[key]

    def workspace_bytes(self):
        fn, outs = WORKSPACE_CALLS[self.rec.consts["ws"]]
        n = [C.c_size_t(0) for _ in range(outs)]
        self.native.check(getattr(self.native.load(), fn)(C.byref(self.view.cfg), S, self.y0, self.y1, *[C.byref(x) for x in n]))
        return n[0].value  # the smallest workspace: the most bands

    def args(self, ptrs, stream):
        v, c = self.view, self.rec.consts
        a = {"cfg": C.byref(v.cfg), "lo": None if v.lo is None else C.byref(v.lo), "wide": None if v.wide is None else C.byref(v.wide),
             "y0": self.y0, "y1": self.y1, "ch": self.ch, "s": S, "tf": 0, "thick": THICKNESS, "thr": THRESHOLD, "reach": REACH,
             "from": v.low, "n": v.cfg.width * v.cfg.height, "width": v.width, "rows": v.height, "stream": stream,
             "opts": None if self.opts is None else C.byref(self.opts), "rows_written": C.byref(self.rows_written), "zw": 2}
        a.update({k: c[k] for k in c if k not in ("ws",) + OPTS_FIELDS + CFG_FIELDS})
        for k in self.rec.arrays:
            a[k] = ptrs[k]
            if k + "_len" in self.sig:
                a[k + "_len"] = self.sizes[k]
        return [a[k] for k in self.sig]
