"""What a deep entry point answers to an invalid call — the code and the exact fr_last_error text, and for a call wrong in
two ways which of the two — is part of the C ABI's behaviour and has no other test: the calls of tests/deep_call_cases.py
(every DD, PT, PT state, PT extend, wide, BLA-PT, SCALED PT and supersampling entry point, host and device form) against
tests/golden/deep_call_errors.json, which tools/record_deep_call_errors.py recorded from the library of the commit named in
the file's header.  Every call is refused before any device work, so this needs no device and touches none."""
import json
import os

import pytest

import deep_call_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "deep_call_errors.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge

    ge.build()
    from fractal_renderer_amd import _native

    return _native


def test_the_golden_file_names_its_commit_and_holds_refusals_only():
    assert len(GOLDEN["commit"]) == 40 and GOLDEN["commit"] in GOLDEN["header"]
    assert all(rc in (1, 2) and text for rc, text in GOLDEN["calls"].values())


def test_the_table_covers_every_deep_entry_point_in_both_forms():
    functions = {D.ENTRIES[e][0] for e in D.ENTRIES}
    for name in ("fr_render_rows_dd", "fr_render_rows_pt", "fr_escape_rows_pt_state", "fr_escape_extend_pt", "fr_render_rows_pt_wide",
                 "fr_escape_rows_pt_wide_state", "fr_escape_extend_pt_wide", "fr_render_rows_pt_bla", "fr_escape_rows_pt_bla",
                 "fr_render_rows_ss", "fr_escape_extend", "fr_render_rows_pt_scaled", "fr_escape_rows_pt_scaled",
                 "fr_escape_rows_pt_scaled_state", "fr_escape_extend_pt_scaled"):
        assert name in functions and name + "_device" in functions, name
    # the escape rows of DD, PT and wide PT have one device form between them (fr_escape_rows_device; wide PT has none)
    assert {"fr_escape_rows_dd", "fr_escape_rows_pt", "fr_escape_rows_pt_wide", "fr_escape_rows_device", "fr_debug_bla_count",
            "fr_debug_bla_table", "fr_debug_pt_scaled_count", "fr_debug_bla_table_scaled"} <= functions


def test_every_invalid_call_is_refused_with_the_recorded_code_and_text(native):
    lib, seen, wrong = native.load(), set(), []
    for key, fn, args, _keep in D.calls(native):
        seen.add(key)
        rc = getattr(lib, fn)(*args)
        got = [rc, lib.fr_last_error().decode()]
        if got != GOLDEN["calls"].get(key):
            wrong.append("%s: %r, recorded %r" % (key, got, GOLDEN["calls"].get(key)))
    assert seen == set(GOLDEN["calls"]), sorted(seen ^ set(GOLDEN["calls"]))
    assert not wrong, "\n".join(wrong)
