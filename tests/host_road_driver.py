"""Render host-road cases (host_road_cases.py) into guarded caller buffers and compare them with the CPU oracle.

    python tests/host_road_driver.py <case> [<case> ...]

A case is a name of host_road_cases.CASES, optionally with ":off=1,mem=fresh,prec=f32,slack=4096": the payload's offset
from a page boundary, a written numpy array ("resident") or a never-touched anonymous mmap ("fresh"), the precision, and
how much longer than needed the buffer is declared (out_len = need + slack).  mem=fenced is a fresh mmap whose payload ends
at a page boundary with an inaccessible page behind it (off then follows from the size): a touch past the end that
changes no byte, which no guard pattern can see, ends the process.  One JSON line per case goes to stdout; what
the library writes to stderr (FR_TRACE) passes through.  Exit status 0 when every case matched.

Not a test module: test_gpu_host_roads.py imports it for its in-process tests and runs it as a child process for what is
read from the environment once per process (FR_HOST_STAGING, FR_COPY_THREADS, FR_TOUCH_THREADS, FR_TRACE).

The caller's buffer is  guard | payload | (slack) | guard  with 8192-byte guards of a fixed pattern.  Expected bytes come
from oracle_lib alone (O.get_image, 16 threads), never from another entry point of the library.
"""
import os
import sys

try:  # before anything loads libfractal_hip.so, as conftest.py does
    import torch  # noqa: F401
except ImportError:
    pass

import ctypes as C
import json
import mmap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import host_road_cases as H  # noqa: E402
import oracle_lib as O  # noqa: E402

ORACLE_THREADS = 16
PAGE = H.K_PAGE


def pattern(start, stop):
    """the fixed guard pattern, a function of the byte's index in the allocation (period 251: no power of two)"""
    return ((np.arange(start, stop, dtype=np.int64) % 251) + 3).astype(np.uint8)


class Guarded:
    """guard | payload | slack | guard in one page-aligned allocation; the payload starts `off` bytes after a page
    boundary.  Resident: a numpy array, every byte written (the pattern, payload included).  Fresh: an anonymous mmap of
    which only the guards (and the bytes in front of the first) are written: the payload's pages do not exist yet."""

    def __init__(self, need, off=0, fresh=False, slack=0, fenced=False):
        self.need, self.off, self.fresh, self.slack = need, off, fresh, slack
        if fenced:
            # fresh memory whose payload ENDS at a page boundary, and behind it a page that may be neither read nor
            # written: a touch past the end, even one that changes no byte, ends the process.  No guard behind, and the
            # offset of the payload follows from its size.
            self.fresh, self.slack = True, 0
            self.total = (H.GUARD + need + PAGE - 1) // PAGE * PAGE + PAGE
            self.start = self.total - need
            self.off = self.start % PAGE
            self._keep = mmap.mmap(-1, self.total + PAGE)
            whole = np.frombuffer(self._keep, dtype=np.uint8)
            self.arr = whole[:self.total]
            self.base = self.arr.ctypes.data
            libc = C.CDLL(None, use_errno=True)
            if libc.mprotect(C.c_void_p(self.base + self.total), C.c_size_t(PAGE), 0) != 0:
                raise OSError(C.get_errno(), "mprotect")
            self.arr[:self.start] = pattern(0, self.start)
            return
        self.start = H.GUARD + off
        self.total = (self.start + need + slack + H.GUARD + PAGE - 1) // PAGE * PAGE
        if fresh:
            self._keep = mmap.mmap(-1, self.total)
            self.arr = np.frombuffer(self._keep, dtype=np.uint8)
        else:
            self._keep = np.empty(self.total + PAGE, dtype=np.uint8)
            shift = (-self._keep.ctypes.data) % PAGE
            self.arr = self._keep[shift:shift + self.total]
        self.base = self.arr.ctypes.data
        assert self.base % PAGE == 0
        self.arr[:self.start] = pattern(0, self.start)
        tail0 = self.start + need if fresh else self.start
        self.arr[tail0:] = pattern(tail0, self.total)

    @property
    def out(self):
        return self.base + self.start

    @property
    def out_len(self):
        return self.need + self.slack

    def payload(self):
        return self.arr[self.start:self.start + self.need]

    def refill(self):
        """a resident payload back to the pattern (between two renders into the same buffer)"""
        self.arr[self.start:self.start + self.need] = pattern(self.start, self.start + self.need)

    def guards_intact(self):
        """None, or a description of the first damaged byte outside [out, out + need)"""
        front = np.flatnonzero(self.arr[:self.start] != pattern(0, self.start))
        if front.size:
            return "byte %d in FRONT of the payload was written (%d bytes damaged)" % (self.start - int(front[-1]), front.size)
        end = self.start + self.need
        back = np.flatnonzero(self.arr[end:] != pattern(end, self.total))
        if back.size:
            return "byte %d BEHIND the payload was written (%d bytes damaged, slack %d)" % (int(back[0]), back.size, self.slack)
        return None

    def payload_untouched(self):
        return bool(np.array_equal(self.payload(), pattern(self.start, self.start + self.need)))


def expected_bytes(name, prec, poison=False):
    """the case's bytes from the CPU oracle, flat.  The oracle runs with the software log2 the kernels carry
    (test_gpu_parity.py pins the device's log2 to it bit for bit, and both to libm on every compared image)."""
    case = H.CASES[name]
    ocfg = H.oracle_config(O, case, poison)
    O.set_log2_mode(O.LOG2_SOFT)
    try:
        rgb = O.get_image(ocfg, O.F32 if prec == "f32" else O.F64, case["y0"], case["y1"], threads=ORACLE_THREADS)
    finally:
        O.set_log2_mode(O.LOG2_LIBM)
    if case["bpp"] == 3:
        return rgb.reshape(-1)
    rgba = np.full(rgb.shape[:2] + (4,), 255, dtype=np.uint8)
    rgba[..., :3] = rgb
    return rgba.reshape(-1)


def render(fr, name, prec, out, out_len, poison=False):
    """one call of the host entry point the case stands for; returns the fr_status"""
    from fractal_renderer_amd import _native

    lib = _native.load()
    case = H.CASES[name]
    cfg = fr.Config.from_buffer_copy(bytes(H.oracle_config(O, case, poison)))
    p = 1 if prec == "f32" else 0
    out = C.c_void_p(out)
    if case["bpp"] == 4:
        return lib.fr_render_rows_rgba8(C.byref(cfg), p, case["y0"], case["y1"], out, out_len)
    if p == 0 and case["y0"] == 0 and case["y1"] == case["height"]:
        return lib.fr_render_rgb8(C.byref(cfg), out, out_len)
    return lib.fr_render_rows_rgb8(C.byref(cfg), p, case["y0"], case["y1"], out, out_len)


def describe_mismatch(got, want, g):
    """the first differing byte, and the band / chunk / row it falls in per the mirror"""
    diff = np.flatnonzero(got != want)
    k = int(diff[0])
    band, chunk, row = H.locate(g, k)
    b = g["bands"][band]
    d = {"n_diff": int(diff.size), "first_diff": k, "last_diff": int(diff[-1]), "band": band, "band_offset": b["offset"],
         "offset_in_band": k - b["offset"], "band_via": b["via"], "chunk": chunk, "row": row,
         "got": got[k:k + 16].tolist(), "want": want[k:k + 16].tolist()}
    if "head" in b:
        d["band_head"], d["band_tail"] = b["head"], b["tail"]
    return d


def check(buf, want, g):
    """{} when the payload equals `want` byte for byte and nothing outside it was written, else what went wrong"""
    problems = {}
    guards = buf.guards_intact()
    if guards:
        problems["guards"] = guards
    got = buf.payload()
    if not np.array_equal(got, want):
        problems["mismatch"] = describe_mismatch(got, want, g)
    return problems


def staging_on():
    e = os.environ.get("FR_HOST_STAGING")
    try:
        return not (e is not None and int(e.strip() or 0) == 0)
    except ValueError:
        return False  # atoi of a non-number is 0


def run_spec(fr, spec, want=None, poison=True):
    """render one case spec into a new guarded buffer and check it; returns the report (report["ok"])"""
    from fractal_renderer_amd import _native

    name, o = H.parse_spec(spec)
    case = H.CASES[name]
    fenced = o["mem"] == "fenced"
    if fenced:  # the payload ends at a page boundary: its offset follows from its size
        o["off"] = (-case["bpp"] * case["width"] * (case["y1"] - case["y0"])) % PAGE
    g = H.geometry(case["width"], case["y1"] - case["y0"], case["bpp"], o["off"], staging_on())
    rep ={"case": spec, "road": g["road"], "bands": len(g["bands"]), "need": g["need"], "ok": False}
    if want is None:
        want = expected_bytes(name, o["prec"])
    if poison and g["road"] == "staged":
        # another view of the same shape first: whatever a dropped copy leaves in the staging buffer is not this frame
        # (guarded too: a stray write must end up in a report, not in the heap)
        scratch = Guarded(g["need"], o["off"])
        rc = render(fr, name, o["prec"], scratch.out, scratch.out_len, poison=True)
        if rc != _native.FR_OK:
            rep["error"] = "the poison frame failed: fr_status %d: %s" % (rc, _native.load().fr_last_error().decode())
            return rep
        if scratch.guards_intact():
            rep["guards"] = "poison frame: " + scratch.guards_intact()
            return rep
    buf = Guarded(g["need"], o["off"], o["mem"] == "fresh", o["slack"], fenced)
    assert buf.out % PAGE == o["off"]
    rc = render(fr, name, o["prec"], buf.out, buf.out_len)
    if rc != _native.FR_OK:
        rep["error"] = "fr_status %d: %s" % (rc, _native.load().fr_last_error().decode())
        return rep
    rep.update(check(buf, want, g))
    rep["ok"] = "guards" not in rep and "mismatch" not in rep
    return rep


def main(argv):
    if not argv:
        print(__doc__)
        return 2
    for spec in argv:
        H.parse_spec(spec)  # a typo ends the run before the GPU is opened
    import fractal_renderer_amd as fr

    fr.init(0)
    cache, bad = {}, 0
    for spec in argv:
        name, o = H.parse_spec(spec)
        if (name, o["prec"]) not in cache:
            cache.clear()  # one image at a time: the largest is 108 MB
            cache[(name, o["prec"])] = expected_bytes(name, o["prec"])
        rep = run_spec(fr, spec, cache[(name, o["prec"])])
        bad += not rep["ok"]
        sys.stderr.flush()
        print(json.dumps(rep), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
