"""STREAM ORDER (include/fractal_hip.h): all the work of a call that takes a caller's stream is ordered on THAT stream.  Every record
of tests/stream_order_cases.py runs behind a GATE on a non-blocking stream S, where work issued on any other stream — the null
stream, the context's own — cannot hide: under NULL it would synchronise with everything and give the right bytes.

The gate is torch.cuda._sleep(cycles) queued on S, calibrated once to about 100 ms and measured (G) in every test; a sleep always
ends.  Behind it, with no synchronisation in between, S gets: device-to-device copies of the TRUE inputs and state over the POISON
the arrays held before; a fill of the outputs with a second pattern over the guard fill; the library call; a copy of outputs and
state to a second buffer.  Then S alone is synchronised — never the device — and the second buffer is compared with the result of
the same call on the NULL stream with the device synchronised before and after, the form the other GPU suites pin to the CPU
models.  A library step that ran on another stream did not wait for the gate: it read poison, or the gated fill overwrote what it
wrote.  If the library is right the test passes whatever the timing; timing only decides whether a wrong library is caught.

TEETH: for every record with inputs or state the synchronous call on the poison must differ from the expected result in at least
1 % of its bytes, or the gate could not tell a misordered read.  The poison is safe to compute on (stream_order_cases.py: the true
arrays of the same view and cap rolled by a few pixels).

WORKSPACES ARE NEVER WRITTEN BEHIND THE GATE.  The lists of the adaptive calls live there with their counters, and a list append is
not bounded by a capacity: a counter that a misordered memset found poisoned, or that a gated fill overwrote, would index past the
list.  Every call, gated or not, gets its own fresh zero-filled workspace, written before the gate and by the library alone after.

NO HOST WAIT: every call is made ungated first (orbits and tables are cached), and the host time of the gated call must stay under
G / 2 — a call that waits for its stream takes about G, one that only enqueues takes microseconds to a few milliseconds.  The
chain, ring and cache tests below are exempt by the header's own words (a cache miss, a full ring), apart from the F64 chains,
which have neither.

PROFILING (fr_set_profiling) is off in every gated call: the default path is the one under test.  It is switched on only around
the synchronous calls whose kernel name is checked (the two-pass records and the survivor ring)."""
import ctypes as C
import threading
import time

import pytest

import stream_order_cases as T

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_BYTE, FILL, COPY_FILL = 0xA5, 0x3C, 0xEE  # around every array and in an untouched output; the gated fill; the second buffer
GATE_MS = 100.0
TEETH = 0.01
HIP_STREAM_NON_BLOCKING = 0x01


@pytest.fixture(scope="module")
def fr():
    import fractal_renderer_amd

    assert fractal_renderer_amd.device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    fractal_renderer_amd.init(0)
    assert fractal_renderer_amd.device_name().startswith("gfx950")
    return fractal_renderer_amd


def hip_runtime():
    """the HIP runtime this process has already loaded (torch's), by its path"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "no HIP runtime is loaded"
    return C.CDLL(sorted(paths)[0])


class Harness:
    def __init__(self, fr):
        import torch
        from fractal_renderer_amd import _native

        self.fr, self.torch, self.native, self.lib = fr, torch, _native, _native.load()
        self.dev = torch.device("cuda", 0)
        self.hip = hip_runtime()
        self.hip.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        self.created = []
        self.S, self.S2 = self.stream(), self.stream()
        self.cycles = self.calibrate()
        self.sources = {}

    def stream(self):
        """a caller's stream that is really non-blocking: torch's, or one made with hipStreamCreateWithFlags and wrapped"""
        s = self.torch.cuda.Stream(self.dev)
        if not self.flags(s) & HIP_STREAM_NON_BLOCKING:
            raw = C.c_void_p()
            self.hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
            assert self.hip.hipStreamCreateWithFlags(C.byref(raw), HIP_STREAM_NON_BLOCKING) == 0
            self.created.append(raw)
            s = self.torch.cuda.ExternalStream(raw.value, device=self.dev)
        assert self.flags(s) & HIP_STREAM_NON_BLOCKING, "the caller's stream is not non-blocking: the gate would prove nothing"
        return s

    def flags(self, s):
        f = C.c_uint(0xFFFF)
        assert self.hip.hipStreamGetFlags(C.c_void_p(s.cuda_stream), C.byref(f)) == 0
        return f.value

    def sleep_ms(self, cycles):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.S):
            e0.record(self.S)
            torch.cuda._sleep(cycles)
            e1.record(self.S)
        self.S.synchronize()
        return e0.elapsed_time(e1)

    def calibrate(self):
        cycles = 10_000_000
        self.sleep_ms(cycles)  # the first launch pays for loading the kernel
        for _ in range(3):
            ms = self.sleep_ms(cycles)
            assert ms > 0.0
            if 0.8 * GATE_MS <= ms <= 1.25 * GATE_MS:
                break
            cycles = max(1000, int(cycles * GATE_MS / ms))
        return cycles

    # ---- buffers ---------------------------------------------------------------------------------------------------------------

    def guarded(self, size, content):
        """GUARD bytes, `size` bytes of `content` (a byte value or a uint8 tensor), GUARD bytes"""
        t = self.torch.full((GUARD + size + GUARD,), GUARD_BYTE, dtype=self.torch.uint8, device=self.dev)
        if isinstance(content, int):
            t[GUARD:GUARD + size].fill_(content)
        else:
            assert content.numel() == size, (content.numel(), size)
            t[GUARD:GUARD + size].copy_(content)
        assert (t.data_ptr() + GUARD) % 8 == 0
        return t

    def inner(self, t):
        return t[GUARD:t.numel() - GUARD]

    def guards_intact(self, t):
        return bool((t[:GUARD] == GUARD_BYTE).all()) and bool((t[t.numel() - GUARD:] == GUARD_BYTE).all())

    def check(self, rc, what):
        if rc != 0:
            msg = self.lib.fr_last_error()
            raise AssertionError("%s: status %d, %s" % (what, rc, msg.decode() if msg else ""))

    # ---- one call ----------------------------------------------------------------------------------------------------------------

    def results(self, call):
        return [k for k, c in call.rec.arrays.items() if c in (T.OUTPUT, T.STATE)]

    def taken(self, call):
        return [k for k, c in call.rec.arrays.items() if c in (T.INPUT, T.STATE)]

    def buffers(self, call, given, out_fill):
        """an array per pointer of the call: `given` in inputs and state, out_fill in outputs, zeros in the workspace"""
        bufs = {}
        for k, cls in call.rec.arrays.items():
            content = given[k] if cls in (T.INPUT, T.STATE) else 0 if cls == T.WORKSPACE else out_fill
            bufs[k] = self.guarded(call.sizes[k], content)
        return bufs

    def run(self, call, bufs, stream):
        fn = getattr(self.lib, call.rec.fn)
        args = call.args({k: t.data_ptr() + GUARD for k, t in bufs.items()}, stream)
        t0 = time.perf_counter()
        rc = fn(*args)
        ms = (time.perf_counter() - t0) * 1e3
        self.check(rc, call.rec.id)
        return ms

    def sync_call(self, call, given=None):
        """the call on the NULL stream with the device synchronised before and after -> {key: bytes} of outputs and state"""
        torch = self.torch
        bufs = self.buffers(call, given or {}, FILL)
        torch.cuda.synchronize()
        self.run(call, bufs, None)
        torch.cuda.synchronize()
        for k, t in bufs.items():
            assert self.guards_intact(t), "%s wrote outside %s" % (call.rec.id, k)
        return {k: self.inner(bufs[k]).clone() for k in self.results(call)}

    def true_inputs(self, rec):
        """the outputs of the record's source, computed once and left unchanged"""
        src, how = rec.source
        key = (src, bool(how.get("low")), bool(how.get("big")))
        if key not in self.sources:
            view = T.VIEWS[rec.view]
            call = T.Call(self.native, T.RECORDS[src], cap=view[4] if how.get("low") else None, big=bool(how.get("big")))
            self.sources[key] = self.sync_call(call)
        got = self.sources[key]
        return {how.get("rename", {}).get(k, k): v for k, v in got.items()}

    def poison(self, call, true):
        return {k: self.torch.roll(true[k], call.rec.roll[k] * call.pixel_bytes(k)) for k in self.taken(call)}


class Gated:
    """One call behind a gate: allocate (synchronously), enqueue on a stream, finish (synchronise that stream alone)."""

    def __init__(self, h, call, true, poison):
        self.h, self.call, self.true = h, call, true
        self.bufs = h.buffers(call, poison, GUARD_BYTE)  # the outputs hold the guard fill
        self.second = {k: h.torch.full_like(self.bufs[k], COPY_FILL) for k in h.results(call)}
        self.events = None
        self.host_ms = None

    def enqueue(self, s, gate=True):
        h, torch = self.h, self.h.torch
        with torch.cuda.stream(s):
            if gate:
                self.events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                self.events[0].record(s)
                torch.cuda._sleep(h.cycles)
                self.events[1].record(s)
            for k in h.taken(self.call):
                h.inner(self.bufs[k]).copy_(self.true[k])
            for k, cls in self.call.rec.arrays.items():
                if cls == T.OUTPUT:
                    h.inner(self.bufs[k]).fill_(FILL)
            self.host_ms = h.run(self.call, self.bufs, s.cuda_stream)
            for k, t in self.second.items():
                t.copy_(self.bufs[k])

    def finish(self, s):
        """-> ({key: bytes}, G in ms); the guards of every array are checked"""
        s.synchronize()
        g = self.events[0].elapsed_time(self.events[1]) if self.events else None
        for k, t in self.second.items():
            assert self.h.guards_intact(t), "%s wrote outside %s (gate %s ms)" % (self.call.rec.id, k, g)
        for k, t in self.bufs.items():
            assert self.h.guards_intact(t), "%s wrote outside %s (gate %s ms)" % (self.call.rec.id, k, g)
        return {k: self.h.inner(t) for k, t in self.second.items()}, g


@pytest.fixture(scope="module")
def h(fr):
    harness = Harness(fr)
    yield harness
    harness.torch.cuda.synchronize()
    harness.hip.hipStreamDestroy.argtypes = [C.c_void_p]
    for raw in harness.created:
        harness.hip.hipStreamDestroy(raw)


def profiled_sync_call(h, call, given=None):
    """sync_call with profiling on around it -> (result, the kernel name fr_last_kernel_name reports).  Profiling is per thread and
    records two events on the call's stream; it is on for these synchronous calls ONLY, so that every gated call in this file runs
    the default path, without them."""
    h.check(h.lib.fr_set_profiling(1), "fr_set_profiling")
    try:
        want = h.sync_call(call, given)
        name = C.create_string_buffer(256)
        h.check(h.lib.fr_last_kernel_name(name, len(name)), "fr_last_kernel_name")
    finally:
        h.lib.fr_set_profiling(0)
    return want, name.value.decode()


def differing(h, got, want):
    """(bytes that differ, bytes) over all the arrays of a result"""
    bad = sum(int((got[k] != want[k]).sum()) for k in want)
    return bad, sum(int(v.numel()) for v in want.values())


def same(h, got, want, what):
    for k in want:
        if not h.torch.equal(got[k], want[k]):
            n = int((got[k] != want[k]).sum())
            first = int((got[k] != want[k]).nonzero()[0])
            filled = int((got[k] == FILL).sum())
            raise AssertionError("%s: %s differs from the synchronous call in %d of %d bytes, first at %d (%d bytes hold the gated fill)"
                                 % (what, k, n, want[k].numel(), first, filled))


def expected(h, call, true):
    """the synchronous result, which must not be the fill pattern; for an adaptive call the pixels it refined; the kernel name
    of a two-pass record"""
    if "two-pass" in call.rec.id:
        want, name = profiled_sync_call(h, call, true)
        assert "escape_first_kernel + escape_second_kernel" in name, (call.rec.id, name)
    else:
        want = h.sync_call(call, true)
    for k, v in want.items():
        assert not bool((v == FILL).all()), "%s: the synchronous call left %s untouched" % (call.rec.id, k)
    if "refined" in want:
        refined = int(want["refined"].view(h.torch.int64)[0])
        print("%s: refined %d of %d" % (call.rec.id, refined, call.view.width * call.view.height))
        assert 0 < refined <= call.view.width * call.view.height, (call.rec.id, refined)
    return want


def prepared(h, rec):
    """(call, true inputs, poison, expected result) of a record, teeth checked; the last library call is the record's own at
    its own cap, so its orbits and tables are the cached ones"""
    call = T.Call(h.native, rec)
    true = h.true_inputs(rec) if rec.source else {}
    poison = h.poison(call, true)
    want = expected(h, call, true)
    if rec.source:
        bad, n = differing(h, h.sync_call(call, poison), want)
        print("%s: on the poison %d of %d bytes differ" % (rec.id, bad, n))
        assert bad >= TEETH * n, "%s: the poison changes only %d of %d bytes of the result: a misordered read would pass" % (rec.id, bad, n)
        h.sync_call(call, true)  # once more on the true arrays: the cache holds this call's orbits again, whatever the poison did
    return call, true, poison, want


def gate_message(rec, g, host_ms):
    return "%s behind a gate of %.1f ms (host time of the call %.3f ms)" % (rec.id, g, host_ms)


@pytest.mark.parametrize("name", sorted(T.RECORDS))
def test_record_behind_the_gate(h, name):
    rec = T.RECORDS[name]
    call, true, poison, want = prepared(h, rec)
    run = Gated(h, call, true, poison)
    h.torch.cuda.synchronize()
    run.enqueue(h.S)
    got, g = run.finish(h.S)
    what = gate_message(rec, g, run.host_ms)
    print(what)
    assert g >= GATE_MS / 4, "the gate did not hold: " + what
    same(h, got, want, what)
    if rec.waits is None:
        assert run.host_ms < g / 2, "the call waited for its stream: " + what


# ---- chains: each link reads what the previous one wrote, all behind one gate -------------------------------------------------------


def scaled_de_view(h, call):
    """DE ON SCALED PT: the distance and the shading run on cfg_v"""
    cfg_v = h.native.fr_config()
    h.check(h.lib.fr_de_scaled_view(C.byref(call.view.cfg), C.byref(cfg_v)), "fr_de_scaled_view")
    call.view.cfg = cfg_v
    return call


def on_view(rec_id, view):
    return T.RECORDS[rec_id]._replace(view=view, id="%s on %s" % (rec_id, view))


CHAINS = {
    "f64": ("shallow", "escape_rows[f64]", "escape_extend[f64]", ["colour_rows[f64 rgb]", "view_stats[f64]"]),
    "f64 de": ("shallow", "escape_rows_de[f64]", "escape_extend_de[f64]", ["distance_rows", "colour_de_rows[rgb]"]),
    "pt": ("dd", "escape_rows_pt_state", "escape_extend_pt", ["colour_rows[f64 rgb]", "view_stats[f64]"]),
    "de pt": ("dd", "escape_rows_de_pt_state[dd]", "escape_extend_de_pt[dd]", ["distance_rows", "colour_de_rows[rgb]"]),
    "scaled": ("scaled", "escape_rows_pt_scaled_state", "escape_extend_pt_scaled", ["colour_rows[f64 rgb]", "view_stats[f64]"]),
    "scaled de": ("scaled", "escape_rows_de_pt_scaled_state", "escape_extend_de_pt_scaled", ["distance_rows", "colour_de_rows[rgb]"]),
}


def chain_calls(h, name):
    view, render, extend, readers = CHAINS[name]
    low = T.VIEWS[view][4]
    calls = [T.Call(h.native, T.RECORDS[render], cap=low), T.Call(h.native, T.RECORDS[extend])]
    for r in readers:
        c = T.Call(h.native, on_view(r, view))
        calls.append(scaled_de_view(h, c) if name == "scaled de" else c)
    return calls


def run_chain(h, calls, stream, gate):
    """render state, extend, recolour / distance / statistics over ONE set of arrays; -> ({key: bytes}, G, host ms per link)"""
    torch = h.torch
    sizes = {}
    for c in calls:
        for k in c.rec.arrays:
            assert sizes.setdefault(k, c.sizes[k]) == c.sizes[k], k
    bufs = {k: h.guarded(n, FILL if stream is None else GUARD_BYTE) for k, n in sizes.items()}
    second = {k: torch.full_like(t, COPY_FILL) for k, t in bufs.items()}
    torch.cuda.synchronize()
    events, host = None, []
    if stream is None:
        for c in calls:
            host.append(h.run(c, {k: bufs[k] for k in c.rec.arrays}, None))
            torch.cuda.synchronize()
        for k, t in bufs.items():
            second[k].copy_(t)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            if gate:
                events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                events[0].record(stream)
                torch.cuda._sleep(h.cycles)
                events[1].record(stream)
            for t in bufs.values():
                h.inner(t).fill_(FILL)
            for c in calls:
                host.append(h.run(c, {k: bufs[k] for k in c.rec.arrays}, stream.cuda_stream))
            for k, t in bufs.items():
                second[k].copy_(t)
        stream.synchronize()
    for k, t in second.items():
        assert h.guards_intact(t), "the chain wrote outside %s" % k
    g = events[0].elapsed_time(events[1]) if events else None
    return {k: h.inner(t) for k, t in second.items()}, g, host


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_kept_view_chain_behind_one_gate(h, name):
    """The second link raises the cap of the state the first wrote, the readers colour and measure what the second left: on a PT
    road the extension continues the cached orbits while the render that reads the shorter ones is still pending (a cache miss:
    it may wait, and is exempt from the no-wait rule).  The F64 chains have no cache and no ring to fill: none of their links,
    each queued behind another library call, may wait for the stream."""
    calls = chain_calls(h, name)
    want, _, _ = run_chain(h, calls, None, False)
    for k, v in want.items():
        assert not bool((v == FILL).all()), (name, k)
    again, _, _ = run_chain(h, calls, None, False)
    same(h, again, want, "the synchronous chain %s, repeated" % name)
    got, g, host = run_chain(h, chain_calls(h, name), h.S, True)
    what = "chain %s behind a gate of %.1f ms (host ms per link: %s)" % (name, g, ", ".join("%.3f" % v for v in host))
    print(what)
    assert g >= GATE_MS / 4, "the gate did not hold: " + what
    same(h, got, want, what)
    if CHAINS[name][0] == "shallow":
        assert max(host) < g / 2, "a link waited for its stream: " + what


# ---- the rings: a slot released on one stream and reacquired for another ------------------------------------------------------------


def ring_calls(h, rec_id, count):
    """`count` different views of a record: the centre and the cap move with the index"""
    calls = []
    for i in range(count):
        c = T.Call(h.native, T.RECORDS[rec_id])
        c.view.cfg.pos.re += 0.0007 * i
        c.view.cfg.pos.im -= 0.0004 * i
        c.view.cfg.iterations = 400 + 23 * i
        calls.append(c)
    return calls


def run_ring(h, calls, gated, slots, two_pass=False):
    """The calls on S (gated[i % len(gated)]) or S2 (free), one gate in front of the first, nothing synchronised until all are
    queued.  `slots` is the ring's size: acquisition is round-robin, so call i + slots takes the slot of call i, and the pattern
    must put some such pair on DIFFERENT streams with call i on the gated one — a slot released by an event on S and reacquired for
    S2 while that event is still behind the gate.  Only the acquisition's wait for the event orders the two then: on one stream,
    plain stream order would."""
    on_s = [bool(gated[i % len(gated)]) for i in range(len(calls))]
    crossing = [i for i in range(len(calls) - slots) if on_s[i] and not on_s[i + slots]]
    assert on_s[0] and crossing and crossing[0] == 0, "the first reacquired slot must cross from the gated stream to the free one"
    if two_pass:  # the kernel names come from the synchronous calls: the gated ones run without profiling
        want = []
        for c in calls:
            w, name = profiled_sync_call(h, c)
            assert "escape_first_kernel + escape_second_kernel" in name, name
            want.append(w)
    else:
        want = [h.sync_call(c) for c in calls]
    assert all(not h.torch.equal(a["out"], b["out"]) for a, b in zip(want, want[1:])), "the views of the ring are one view"
    runs = [Gated(h, c, {}, {}) for c in calls]
    streams = [h.S if s else h.S2 for s in on_s]
    h.torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, r in enumerate(runs):
        r.enqueue(streams[i], gate=(i == 0))
    host_ms = (time.perf_counter() - t0) * 1e3
    g = None
    for i, r in enumerate(runs):
        got, gi = r.finish(streams[i])
        g = gi if gi is not None else g
        same(h, got, want[i], "render %d of the ring (%s)" % (i, "gated stream" if on_s[i] else "free stream"))
    print("ring of %d over %d slots: gate %.1f ms, host time of all the calls %.1f ms (per call: %s)"
          % (len(calls), slots, g, host_ms, ", ".join("%.2f" % r.host_ms for r in runs)))
    assert g >= GATE_MS / 4
    # one acquisition finds its slot's event behind the gate and waits for the rest of it; every later one finds the gate gone
    assert host_ms < 1.5 * g, "a full ring blocks for one gate at the most"
    assert sum(r.host_ms >= g / 2 for r in runs) <= 1, "more than one call waited"


def test_palette_ring_across_two_streams(h):
    """20 renders with smooth = 0 (each builds its palette in one of the 16 slots) on a gated and a free stream in the pattern
    S, S2, S: the 17th acquisition (render 16, on the FREE stream) finds the slot of render 0, whose event sits behind the gate on
    S, and must wait for it before its palette kernel may overwrite the slot — that wait is bounded by the sleep."""
    calls = ring_calls(h, "render_rows_rgb8[f64 palette]", 20)
    assert all(c.view.cfg.smooth == 0 for c in calls)
    run_ring(h, calls, gated=(True, False, True), slots=16)


def test_survivor_ring_across_two_streams(h):
    """5 two-pass renders (tile 11) over the 3 survivor-list buffers, alternating S, S2: render 3, on the free stream, takes the
    buffer of render 0, which is pending behind the gate"""
    run_ring(h, ring_calls(h, "render_rows_rgb8_opts[f32 two-pass]", 5), gated=(True, False), slots=3, two_pass=True)


# ---- the caches: an orbit or a table replaced while the launch that reads it is pending -----------------------------------------------


def other_scaled_view(h):
    """a second view past 2^440: the same centre at half the scale and a lower cap — another orbit length and another table"""
    c = T.Call(h.native, T.RECORDS["render_rows_pt_scaled[table]"], cap=T.VIEWS["scaled"][4])
    c.view.cfg.scale.re *= 0.5
    c.view.cfg.scale.im *= 0.5
    return c


CACHE_ROADS = {
    "pt": lambda h: (T.Call(h.native, T.RECORDS["render_rows_pt_wide"]), T.Call(h.native, T.RECORDS["render_rows_pt"])),
    "bla": lambda h: (T.Call(h.native, T.RECORDS["render_rows_pt_bla[wide]"]), T.Call(h.native, T.RECORDS["render_rows_pt_bla[dd]"])),
    "scaled": lambda h: (T.Call(h.native, T.RECORDS["render_rows_pt_scaled[table]"]), other_scaled_view(h)),
}


@pytest.mark.parametrize("road", sorted(CACHE_ROADS))
def test_cache_replacement_behind_one_gate(h, road):
    """View A, view B, view A again on S behind one gate: B replaces A's cached orbit (and table) while A's launch is pending, and
    the third call replaces B's.  All three images must be right.  The second and third call are cache misses and may wait."""
    a, b = CACHE_ROADS[road](h)
    want_a, want_b = h.sync_call(a), h.sync_call(b)
    assert a.sizes != b.sizes or not h.torch.equal(want_a["out"], want_b["out"])
    h.sync_call(a)  # A's orbit is the cached one when the gated sequence starts
    runs = [Gated(h, c, {}, {}) for c in (a, b, a)]
    h.torch.cuda.synchronize()
    for i, r in enumerate(runs):
        r.enqueue(h.S, gate=(i == 0))
    g = None
    for i, (r, want) in enumerate(zip(runs, (want_a, want_b, want_a))):
        got, gi = r.finish(h.S)
        g = gi if gi is not None else g
        same(h, got, want, "%s road, call %d of A B A behind a gate of %.1f ms (host ms %s)"
             % (road, i, g, ", ".join("%.3f" % x.host_ms for x in runs)))
    print("%s road: gate %.1f ms, host ms %s" % (road, g, ", ".join("%.3f" % x.host_ms for x in runs)))
    assert g >= GATE_MS / 4


# ---- two streams ----------------------------------------------------------------------------------------------------------------------

PAIR = ("render_rows_ss_adaptive_de[f64]", "render_rows_ss_pt[bla]")


def test_two_gated_streams_from_one_thread(h):
    """two unrelated calls, each with a workspace of its own, on two gated streams"""
    prepared_pair = [prepared(h, T.RECORDS[name]) for name in PAIR]
    # (the F64 call has no cache; the BLA call was prepared last, so its orbit and table are the cached ones)
    runs = [Gated(h, call, true, poison) for call, true, poison, _ in prepared_pair]
    h.torch.cuda.synchronize()
    for r, s in zip(runs, (h.S, h.S2)):
        r.enqueue(s)
    for r, s, (call, _, _, want) in zip(runs, (h.S, h.S2), prepared_pair):
        got, g = r.finish(s)
        what = gate_message(call.rec, g, r.host_ms) + ", two streams from one thread"
        assert g >= GATE_MS / 4, what
        same(h, got, want, what)
        assert r.host_ms < g / 2, "the call waited for a stream: " + what


def test_two_gated_streams_from_two_threads(h):
    prepared_pair = [prepared(h, T.RECORDS[name]) for name in PAIR]
    runs = [Gated(h, call, true, poison) for call, true, poison, _ in prepared_pair]
    h.torch.cuda.synchronize()
    errors, results = [], [None, None]
    barrier = threading.Barrier(2)

    def work(i, s):
        try:
            barrier.wait(timeout=30)
            runs[i].enqueue(s)
            results[i] = runs[i].finish(s)
        except BaseException as e:  # noqa: BLE001
            errors.append("thread %d: %r" % (i, e))

    threads = [threading.Thread(target=work, args=(i, s)) for i, s in enumerate((h.S, h.S2))]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    for r, (got, g), (call, _, _, want) in zip(runs, results, prepared_pair):
        what = gate_message(call.rec, g, r.host_ms) + ", two streams from two threads"
        assert g >= GATE_MS / 4, what
        same(h, got, want, what)
        assert r.host_ms < g / 2, "the call waited for a stream: " + what
