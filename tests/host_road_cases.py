"""The host-buffer render roads of fractal-renderer_amd/csrc/fr_host.hip, restated in plain Python, and the table of
shapes the host-road tests render (test_host_road_shapes_cpu.py, test_gpu_host_roads.py, host_road_driver.py).

fr_host.hip renders nothing itself but decides where every byte of fr_render_rgb8 / fr_render_rows_rgb8 /
fr_render_rows_rgba8 lands: which road a request takes, how it is cut into bands, which bands leave HBM through
copy_out_kernel (with its head / tail byte paths) and which through the copy engine, and where the caller's buffer is cut
into pinned chunks.  `geometry()` below mirrors that arithmetic; the constants are checked against the source by
test_host_road_shapes_cpu.py, and every class of CLASSES must be hit by a case of CASES according to the mirror.

Nothing here needs a GPU or the built library.
"""
MIB = 1 << 20

# fr_host.hip's constants (test_host_road_shapes_cpu.py reads them out of the source and compares)
K_PAGE = 4096
K_CHUNK = 64 * MIB          # kChunk: a pin-road chunk ...
K_LAST_STRETCH = K_CHUNK // 4   # ... and kChunk / 4 over the last kChunk + kChunk / 4 bytes
K_PIN_THRESHOLD = 16 * MIB  # kPinThreshold: below, without staging: one kernel + one plain copy
K_STAGE_MAX = 40 * MIB      # kStageMax: up to here the staged road
K_SDMA_MIN = 5 * MIB        # kSdmaMin: staged bands from here up leave HBM through the copy engine
BAND_TARGET = 6 * MIB       # host_render_staged: ~6 MiB a band ...
TWO_BANDS_FROM = 3 * MIB    # ... two bands from 3 MiB ...
MAX_BANDS = 4               # ... four at the most, of whole 8-row tiles
HELPERS_FROM = 3 * MIB      # the copy pool joins in from here (need)
SPLIT_FROM = 1 * MIB        # a band (or the first touch) is cut into pieces from here (len)
PREFAULT_FROM = 1 * MIB     # a non-resident caller buffer is faulted in first from here (need)
PIECE_ALIGN = 4096          # pieces are cut at multiples of 4096 bytes of the band

GUARD = 8192                # bytes of fixed pattern in front of and behind the caller's payload (host_road_driver.py)


def _ceil_div(a, b):
    return (a + b - 1) // b


def chunk_end(host_off, need, a):
    """ChunkPinner::chunk_end: the end of the chunk that starts at byte `a` of a buffer whose host address is
    host_off (mod 4096): 64 MiB on (16 MiB over the last stretch), moved back to a page boundary of the host address."""
    left = need - a
    b = a + (K_LAST_STRETCH if left <= K_CHUNK + K_LAST_STRETCH else K_CHUNK)
    if b >= need:
        return need
    b -= (host_off + b) % K_PAGE
    return b if b > a else need


def chunk_bounds(host_off, need):
    """ChunkPinner's bounds_: [0, ..., need]"""
    bounds, a = [], 0
    while a < need:
        bounds.append(a)
        a = chunk_end(host_off, need, a)
    bounds.append(need)
    return bounds


def pin_ranges(host_off, need):
    """What ChunkPinner::pin registers for each chunk, as offsets relative to the buffer's start (may be negative / past
    need: the two outer boundaries are rounded outwards to page boundaries of the host address)."""
    bounds = chunk_bounds(host_off, need)
    out = []
    for k in range(len(bounds) - 1):
        a, b = bounds[k], bounds[k + 1]
        ra = a - (host_off + a) % K_PAGE
        rb = b if b < need else b + (-(host_off + b)) % K_PAGE
        out.append((ra, rb))
    return out


def _kernel_band(a, length):
    """copy_out_kernel's split of a band at byte offset `a` of the (page-aligned) staging buffer: head bytes in front of
    the first 16-byte boundary, 16-byte units, tail bytes"""
    head = (16 - a % 16) % 16
    h = min(head, length)
    return h, (length - h) // 16, (length - h) % 16


def staged_bands(width, rows, bpp):
    """host_render_staged's bands of rows [0, rows) (relative to y0)"""
    row_bytes = bpp * width
    need = row_bytes * rows
    nb = _ceil_div(need, BAND_TARGET)
    if need >= TWO_BANDS_FROM and nb < 2:
        nb = 2
    nb = max(1, min(nb, MAX_BANDS))
    band_rows = (_ceil_div(rows, nb) + 7) & ~7
    if band_rows == 0:
        band_rows = 8
    nb = _ceil_div(rows, band_rows)
    bands = []
    for b in range(nb):
        ra, rb = b * band_rows, min((b + 1) * band_rows, rows)
        a, length = row_bytes * ra, row_bytes * (rb - ra)
        band = {"row0": ra, "row1": rb, "offset": a, "len": length, "via": "engine" if length >= K_SDMA_MIN else "kernel",
                "stream": b & 1}
        if band["via"] == "kernel":
            band["head"], band["units"], band["tail"] = _kernel_band(a, length)
        bands.append(band)
    return bands


def bit_reversed(n):
    """the order in which the pin road issues its n bands"""
    pow2, bits = 1, 0
    while pow2 < n:
        pow2, bits = pow2 << 1, bits + 1
    order = []
    for i in range(pow2):
        r = 0
        for k in range(bits):
            r |= ((i >> k) & 1) << (bits - 1 - k)
        if r < n:
            order.append(r)
    return order


def pin_bands(width, rows, bpp, host_off):
    """host_render_rows' bands on the chunked-pin road: each reaches to the chunk end seen from ITS start, rounded up to
    whole 8-row tiles (so bands and pinned chunks drift apart, and a band's DMA is split where two pins meet)"""
    row_bytes = bpp * width
    need = row_bytes * rows
    bands, ra, a = [], 0, 0
    while ra < rows:
        target = chunk_end(host_off, need, a)
        r = _ceil_div(_ceil_div(target - a, row_bytes), 8) * 8
        rb = min(ra + r, rows)
        b = row_bytes * rb
        bands.append({"row0": ra, "row1": rb, "offset": a, "len": b - a, "via": "pinned-dma"})
        ra, a = rb, b
    for i, k in enumerate(bit_reversed(len(bands))):
        bands[k]["issue"] = i
        bands[k]["stream"] = i & 1
    return bands


def copy_pieces(length, threads):
    """`spread` in host_render_staged: how a band (or the first touch of the whole buffer) of `length` bytes is cut for
    `threads` = helpers + 1 copying threads: [(offset, len), ...]; one piece when there are no helpers or under 1 MiB"""
    if threads <= 1 or length < SPLIT_FROM:
        return [(0, length)]
    piece = (_ceil_div(length, threads) + PIECE_ALIGN - 1) & ~(PIECE_ALIGN - 1)
    out = [(0, min(piece, length))]
    off = piece
    while off < length:
        out.append((off, min(piece, length - off)))
        off += piece
    return out


def geometry(width, rows, bpp, host_off=0, staging=True, deep=False):
    """Where fr_host.hip puts the bytes of `rows` rows of `width` pixels of `bpp` bytes in a caller buffer whose address
    is host_off (mod 4096).  staging=False: FR_HOST_STAGING=0 (or a failed staging allocation); deep: DD / PT."""
    row_bytes = bpp * width
    need = row_bytes * rows
    g = {"need": need, "row_bytes": row_bytes, "chunks": None, "helpers": False, "prefault": False}
    if deep:
        g["road"] = "deep"
        g["bands"] = [{"row0": 0, "row1": rows, "offset": 0, "len": need, "via": "plain-copy"}]
    elif need <= K_STAGE_MAX and staging:
        g["road"] = "staged"
        g["bands"] = staged_bands(width, rows, bpp)
        g["helpers"] = need >= HELPERS_FROM
        g["prefault"] = need >= PREFAULT_FROM  # if the caller's pages are not resident
    elif need < K_PIN_THRESHOLD:
        g["road"] = "plain"
        g["bands"] = [{"row0": 0, "row1": rows, "offset": 0, "len": need, "via": "plain-copy"}]
    else:
        g["road"] = "pin"
        g["bands"] = pin_bands(width, rows, bpp, host_off)
        g["chunks"] = chunk_bounds(host_off, need)
        g["prefault"] = True
    return g


def locate(g, byte):
    """(band index, chunk index or None, row relative to y0) of a byte offset of the payload, per the mirror"""
    band = next((i for i, b in enumerate(g["bands"]) if b["offset"] <= byte < b["offset"] + b["len"]), None)
    chunk = None
    if g["chunks"]:
        chunk = next((k for k in range(len(g["chunks"]) - 1) if g["chunks"][k] <= byte < g["chunks"][k + 1]), None)
    return band, chunk, byte // g["row_bytes"] if g["row_bytes"] else 0


# ---- views: asymmetric, cheap, smooth-coloured ---------------------------------------------------------------------
# The default Mandelbrot view is mirror-symmetric in y: two swapped bands could go unseen.  These are not; the cap is low
# so that the CPU oracle of the 108 MB case takes about a second.  "poison" is a second, unrelated view of the same shape:
# the driver renders it before every checked frame, so that what a dropped copy would leave behind in the library's
# staging buffer is never the frame under test.

ITERATIONS = 48
VIEWS = {
    "mandelbrot": dict(algo=0, pos=(-0.6, 0.17)),
    "julia": dict(algo=2, julia_set=(-0.8, 0.156), pos=(0.11, -0.07)),
}
POISON = dict(algo=0, pos=(-0.31, -0.45), exposure=2.0, primary_color=(200, 30, 90), secondary_color=(20, 250, 60))


def oracle_config(O, case, poison=False):
    """the oracle's Config of a case (O = oracle_lib)"""
    w, h = case["width"], case["height"]
    kw = dict(POISON if poison else VIEWS[case["view"]])
    algo = kw.pop("algo")
    # the reference maps x by the HEIGHT (calc/src/lib.rs:194): a very wide image is squeezed back over the view
    scale = (0.4 * w / h, 0.4) if w > 4 * h else (0.4, 0.4)
    return O.cli_config(w, h, algo, iterations=ITERATIONS, scale=scale, **kw)


# ---- the table -----------------------------------------------------------------------------------------------------


def pick_split_pair(rows=24):
    """Two neighbouring widths at `rows` rows of RGB around the 3 MiB line: the narrower is ONE band that nobody helps
    with (need just under 3 MiB), the wider is two bands with the helpers on, the second a few bytes over the 1 MiB
    from which a band is cut into pieces.  Found with the mirror; returns (narrow, wide)."""
    for width in range(max(2, HELPERS_FROM // (3 * rows) - 64), 1 << 20):
        g = geometry(width, rows, 3)
        if g["helpers"] and len(g["bands"]) == 2 and SPLIT_FROM <= g["bands"][1]["len"] < SPLIT_FROM + 4096:
            n = geometry(width - 1, rows, 3)
            if not n["helpers"] and len(n["bands"]) == 1:
                return width - 1, width
    raise AssertionError("no width puts a band just over the 1 MiB split: re-derive the table from fr_host.hip")


_NARROW, _WIDE = pick_split_pair()


def _case(width, height, bpp=3, view="mandelbrot", y0=0, y1=None, **kw):
    d = dict(width=width, height=height, bpp=bpp, view=view, y0=y0, y1=height if y1 is None else y1)
    d.update(kw)
    return d


CASES = {
    "head8_1031": _case(1031, 1031),                       # 2 kernel bands of 520 / 511 rows, the second at 8 (mod 16)
    "four_kernel_bands": _case(2555, 2501),                # 4 x 632 rows = 4 844 280 B each: heads 0 / 8 / 0 / 8
    "four_engine_bands": _case(3840, 2160),                # 544-row bands of 6 266 880 B through the copy engine
    "mixed_engine_kernel": _case(200001, 17),              # 16 rows = 9.6 MB through the engine, 1 row through the kernel
    "stage_max_exact": _case(4096, 2560, 4, "julia"),      # 41 943 040 B = kStageMax: still staged
    "stage_max_plus_row": _case(4096, 2561, 4, "julia"),   # one row more: the pin road, 16 MiB chunks
    "pin_road_108mb": _case(6000, 6000),                   # a 64 MiB chunk and a last stretch of 16 MiB chunks
    "one_band_no_helpers": _case(_NARROW, 24),             # just under 3 MiB: one band, the caller copies alone
    "split_just_over": _case(_WIDE, 24),                   # second band a few bytes over 1 MiB: cut into pieces
    "one_band_prefault": _case(701, 601),                  # 1.26 MB: one band, first touch on, helpers off, tail 15
    "tiny_one_band": _case(401, 301),                      # under 1 MiB: no helpers, no first touch
    "rgba_1080p": _case(1920, 1080, 4, "julia"),           # RGBA, two kernel bands
    "rows_four_kernel_bands": _case(2555, 2501, y0=3, y1=2501 - 5),   # y0 % 8 != 0 on a four-band frame
    "rows_mixed": _case(200001, 17, y0=3, y1=17 - 5),      # 8 rows + 1 row, the second band at 8 (mod 16)
    "rows_1031": _case(1031, 1031, y0=3, y1=1031 - 5),     # FR_HOST_STAGING=0: the plain-copy road with y0 = 3
}


def case_geometry(name, host_off=0, staging=True):
    c = CASES[name]
    return geometry(c["width"], c["y1"] - c["y0"], c["bpp"], host_off, staging)


def _kernel_bands(g):
    return [b for b in g["bands"] if b["via"] == "kernel"]


def _vias(g):
    return [b["via"] for b in g["bands"]]


# class name -> predicate over (case, geometry at host offset 0, default environment)
CLASSES = {
    "two kernel bands, head 8, odd tails": lambda c, g: g["road"] == "staged" and _vias(g) == ["kernel"] * 2
    and g["bands"][1]["head"] == 8 and g["bands"][0]["tail"] == 8 and g["bands"][1]["tail"] % 2 == 1,
    "four kernel bands, heads 0/8/0/8": lambda c, g: g["road"] == "staged" and _vias(g) == ["kernel"] * 4
    and [b["head"] for b in g["bands"]] == [0, 8, 0, 8],
    "four copy-engine bands": lambda c, g: g["road"] == "staged" and _vias(g) == ["engine"] * 4,
    "mixed: copy-engine band, then kernel band": lambda c, g: g["road"] == "staged" and _vias(g) == ["engine", "kernel"],
    "exactly kStageMax, staged": lambda c, g: g["road"] == "staged" and g["need"] == K_STAGE_MAX,
    "one row over kStageMax: pin road, 16 MiB chunks": lambda c, g: g["road"] == "pin"
    and g["need"] - g["row_bytes"] <= K_STAGE_MAX and g["chunks"][1] == K_LAST_STRETCH,
    "pin road: a 64 MiB chunk and a last stretch": lambda c, g: g["road"] == "pin" and g["chunks"][1] == K_CHUNK
    and len(g["chunks"]) >= 4 and g["chunks"][2] - g["chunks"][1] == K_LAST_STRETCH,
    "one band, helpers off, first touch on": lambda c, g: g["road"] == "staged" and len(g["bands"]) == 1
    and not g["helpers"] and g["prefault"],
    "one band under 1 MiB": lambda c, g: g["road"] == "staged" and len(g["bands"]) == 1 and not g["prefault"],
    "a band just over the 1 MiB split, helpers on": lambda c, g: g["road"] == "staged" and g["helpers"]
    and any(SPLIT_FROM <= b["len"] < SPLIT_FROM + 4096 for b in g["bands"]),
    "need just under the 3 MiB of the helpers": lambda c, g: g["road"] == "staged" and not g["helpers"]
    and g["need"] + 2 * g["row_bytes"] > HELPERS_FROM,
    "RGBA, multi-band": lambda c, g: c["bpp"] == 4 and g["road"] == "staged" and len(g["bands"]) >= 2,
    "row range with y0 % 8 != 0, multi-band": lambda c, g: c["y0"] % 8 != 0 and c["y1"] < c["height"]
    and g["road"] == "staged" and len(g["bands"]) >= 2,
    "row range whose second band has head 8": lambda c, g: c["y0"] % 8 != 0 and g["road"] == "staged"
    and len(g["bands"]) >= 2 and g["bands"][1].get("head") == 8,
    "a kernel band with head 8": lambda c, g: any(b["head"] == 8 for b in _kernel_bands(g)),
    "a kernel band with a tail in 1..7": lambda c, g: any(1 <= b["tail"] <= 7 for b in _kernel_bands(g)),
    "a kernel band with a tail in 9..15": lambda c, g: any(9 <= b["tail"] <= 15 for b in _kernel_bands(g)),
}

# without the staging buffer (FR_HOST_STAGING=0): name -> predicate over (case, geometry with staging=False)
CLASSES_NO_STAGING = {
    "plain copy under 16 MiB with y0 = 3": lambda c, g: g["road"] == "plain" and c["y0"] == 3,
    "pin road between 16 and 40 MiB, 16 MiB chunks": lambda c, g: g["road"] == "pin" and g["need"] <= K_STAGE_MAX
    and g["chunks"][1] == K_LAST_STRETCH and len(g["chunks"]) >= 3,
}


def cases_of_class(name):
    if name in CLASSES:
        return [n for n in CASES if CLASSES[name](CASES[n], case_geometry(n))]
    return [n for n in CASES if CLASSES_NO_STAGING[name](CASES[n], case_geometry(n, staging=False))]


# ---- a case as the driver is told it: "name" or "name:off=1,mem=fresh,prec=f32,slack=4096" -------------------------

SPEC_DEFAULTS = {"off": 0, "mem": "resident", "prec": "f64", "slack": 0}


def make_spec(name, **kw):
    bad = set(kw) - set(SPEC_DEFAULTS)
    if bad or name not in CASES:
        raise KeyError((name, sorted(bad)))
    opts = ",".join("%s=%s" % (k, kw[k]) for k in sorted(kw) if kw[k] != SPEC_DEFAULTS[k])
    return name + (":" + opts if opts else "")


def parse_spec(spec):
    name, _, rest = spec.partition(":")
    if name not in CASES:
        raise KeyError("unknown case %r (known: %s)" % (name, ", ".join(sorted(CASES))))
    opts = dict(SPEC_DEFAULTS)
    for item in filter(None, rest.split(",")):
        k, _, v = item.partition("=")
        if k not in opts:
            raise KeyError("unknown option %r in %r" % (k, spec))
        opts[k] = int(v) if k in ("off", "slack") else v
    if opts["mem"] not in ("resident", "fresh", "fenced") or opts["prec"] not in ("f64", "f32") or not 0 <= opts["off"] < K_PAGE:
        raise ValueError(spec)
    return name, opts
