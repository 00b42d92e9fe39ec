"""What a plain DE entry point answers to an invalid call — the code and the exact fr_last_error text, and for a call wrong in
two ways which of the two — is part of the C ABI's behaviour: the calls of tests/de_call_cases.py (the DE rows of F64 / PT, WIDE
PT, BLA-PT and SCALED PT, the F64 extension, the PT and SCALED PT states and their extensions, host and device form, the
distance, the two recolours and fr_de_scaled_view) against tests/golden/de_call_errors.json, which
tools/record_deep_call_errors.py --table de recorded from the library of the commit named in the file's header.  Every call is
refused, or is a no-op, before any device work, so this needs no device and touches none; the calls that hand a device form a
made-up address are left out on a machine that has a device (de_call_cases.py says why)."""
import ctypes as C
import json
import os

import pytest

import de_call_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "de_call_errors.json")) as f:
    GOLDEN = json.load(f)
CALLS = D.unpack(GOLDEN)  # {id: [code, text]}

PAIRS = ("fr_escape_rows_de", "fr_escape_rows_de_pt_wide", "fr_escape_extend_de", "fr_escape_rows_de_pt_state", "fr_escape_extend_de_pt",
         "fr_escape_rows_de_pt_bla", "fr_escape_rows_de_pt_scaled", "fr_escape_rows_de_pt_scaled_state", "fr_escape_extend_de_pt_scaled",
         "fr_distance_rows")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge

    ge.build()
    from fractal_renderer_amd import _native

    return _native


def has_device(native):
    count = C.c_int(0)
    return native.load().fr_device_count(C.byref(count)) == native.FR_OK and count.value > 0


def test_the_golden_file_names_its_commit_and_holds_refusals_and_named_no_ops_only():
    assert len(GOLDEN["commit"]) == 40 and GOLDEN["commit"] in GOLDEN["header"]
    for key, (rc, text) in CALLS.items():
        assert (rc in (1, 2) and text) or (rc == 0 and "noop_" in key and not text), key
    assert sum(rc != 0 for rc, _ in CALLS.values()) > 1900 and sum(rc == 0 for rc, _ in CALLS.values()) > 100


def test_the_table_covers_every_plain_de_entry_point_in_both_forms():
    functions = {D.ENTRIES[e][0] for e in D.ENTRIES}
    for name in PAIRS:
        assert {name, name + "_device"} <= functions, name
    assert {"fr_colour_de_rows_device", "fr_colour_de_rgb8", "fr_de_scaled_view"} <= functions
    recorded = {key.split(" :: ")[0].split("[")[0] for key in CALLS}
    assert recorded == functions


def test_every_unspoiled_call_gets_as_far_as_the_missing_device(native):
    """so each case is wrong in what it spoils and in nothing else; made only where there is no device to reach"""
    if has_device(native):
        return
    lib = native.load()
    for entry, fn, args, _keep in D.base_calls(native):
        assert getattr(lib, fn)(*args) == native.FR_ERR_NO_DEVICE, (entry, lib.fr_last_error())


def test_every_invalid_call_is_refused_with_the_recorded_code_and_text(native):
    lib, device, seen, wrong = native.load(), has_device(native), set(), []
    for key, fn, args, _keep, fake in D.calls(native):
        seen.add(key)
        if fake and device:
            continue
        rc = getattr(lib, fn)(*args)
        got = [rc, lib.fr_last_error().decode() if rc else ""]
        if got != CALLS.get(key):
            wrong.append("%s (%s): %r, recorded %r" % (key, fn, got, CALLS.get(key)))
    assert seen == set(CALLS), sorted(seen ^ set(CALLS))
    assert not wrong, "\n".join(wrong)
