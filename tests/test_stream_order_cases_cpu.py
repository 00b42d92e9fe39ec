"""tests/stream_order_cases.py is complete: every function of include/fractal_hip.h with a `void *hip_stream` parameter has a record
there (which tests/test_gpu_stream_order.py runs behind a gate) or a written reason in EXCLUDED, and no record names a function the
header does not declare.  A new stream-taking entry point fails this file until it has a stream case.  No device."""
import os

import pytest

import stream_order_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "fractal_hip.h")) as f:
        return f.read()


def missing(header_text, functions, excluded):
    declared = T.header_stream_functions(header_text)
    return sorted(declared - set(functions) - set(excluded)), sorted((set(functions) | set(excluded)) - declared)


def test_every_stream_taking_entry_point_has_a_record_or_a_reason(header):
    declared = T.header_stream_functions(header)
    assert len(declared) >= 56, "the parser lost prototypes: %d" % len(declared)
    uncovered, stale = missing(header, T.functions(), T.EXCLUDED)
    assert not uncovered, "stream-taking entry points without a record in tests/stream_order_cases.py: %s" % uncovered
    assert not stale, "records or exclusions for functions the header no longer declares with a stream: %s" % stale
    assert not set(T.EXCLUDED) & T.functions(), "excluded AND recorded"
    assert all(isinstance(why, str) and len(why.split()) >= 5 for why in T.EXCLUDED.values()), "an exclusion needs a written reason"


def test_the_check_itself_can_fail(header):
    """a record taken out of the table, a new prototype in the header, and a record for a function that is gone"""
    victim = sorted(T.functions())[7]
    uncovered, stale = missing(header, T.functions() - {victim}, T.EXCLUDED)
    assert uncovered == [victim] and not stale
    extra = header + "\nint fr_new_thing_device(const fr_config *cfg, void *d_out,\n        size_t out_len, void *hip_stream);\n"
    uncovered, stale = missing(extra, T.functions(), T.EXCLUDED)
    assert uncovered == ["fr_new_thing_device"] and not stale
    uncovered, stale = missing(header, T.functions() | {"fr_gone_device"}, T.EXCLUDED)
    assert not uncovered and stale == ["fr_gone_device"]
    # a comment that mentions a stream, and a prototype without one, are not entry points of this kind
    assert T.header_stream_functions("/* int fr_x(void *hip_stream); */ int fr_y(void *d_out, size_t n);") == set()


def test_records_are_well_formed():
    """the signature of a record has the arity of the C prototype, every pointer class is one of the four, a source exists, has the
    arrays it is asked for and is itself a record without inputs"""
    from fractal_renderer_amd import _native

    for r in T.RECORDS.values():
        sig = r.sig.split()
        assert len(sig) == len(_native.PROTOTYPES[r.fn][1]), r.id
        assert sig.count("stream") == 1 and len(set(sig)) == len(sig), r.id
        assert set(r.arrays.values()) <= {T.INPUT, T.STATE, T.OUTPUT, T.WORKSPACE}, r.id
        assert any(c in (T.OUTPUT, T.STATE) for c in r.arrays.values()), r.id
        assert r.view in T.VIEWS and all(1 <= n <= 16 for n in r.roll.values()), r.id
        assert ("work" in r.arrays) == ("ws" in r.consts) and (r.arrays.get("work", T.WORKSPACE) == T.WORKSPACE), r.id
        if r.source is not None:
            src, how = r.source
            s = T.RECORDS[src]
            assert s.source is None and s.view == r.view, r.id
            given = {how.get("rename", {}).get(k, k) for k, c in s.arrays.items() if c == T.OUTPUT}
            assert {k for k, c in r.arrays.items() if c in (T.INPUT, T.STATE)} <= given, r.id
    for width, height in ((v[1], v[2]) for v in T.VIEWS.values()):
        assert width <= 64 and height <= 48 and width != height


def test_the_table_covers_the_roads_and_the_twins():
    """one record per road where the launches differ; a _tf twin with transfer = 1 per reduction kernel; RGBA beside RGB"""
    by_fn = {}
    for r in T.RECORDS.values():
        by_fn.setdefault(r.fn, []).append(r)
    assert {r.consts["prec"] for r in by_fn["fr_escape_rows_device"]} == {T.F64, T.F32, T.DD, T.PT}
    assert {r.consts["prec"] for r in by_fn["fr_escape_extend_device"]} == {T.F64, T.F32, T.DD}
    assert {r.consts["road"] for r in by_fn["fr_render_rows_ss_pt_device"]} == {T.PLAIN, T.BLA, T.SCALED}
    assert {r.consts["road"] for r in by_fn["fr_render_rows_ss_adaptive_device"]} == {T.PLAIN, T.BLA, T.SCALED}
    assert {r.consts["bits"] for r in by_fn["fr_render_rows_pt_scaled_device"]} == {-1, 0}
    for fn, records in by_fn.items():
        if "_tf_" in fn:
            assert any(r.consts.get("tf") == 1 for r in records), fn
        if "ch" in records[0].sig.split():  # the call and its _tf twin together: both channel counts
            base = fn.replace("_tf_device", "_device")
            family = by_fn[base] + by_fn.get(base[:-len("_device")] + "_tf_device", [])
            assert {r.consts.get("ch", 3) for r in family} == {3, 4}, fn
