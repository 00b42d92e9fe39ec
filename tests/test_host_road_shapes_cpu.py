"""The shape table of the host-road tests (host_road_cases.py) against fr_host.hip and against the CPU oracle — no GPU.

The table only bites while its Python mirror of the band / chunk geometry is the geometry of fr_host.hip, while every
class of request still has a case that hits it, and while the reference images make a misplaced band visible.  All three
are asserted here, so that a changed constant or a dropped case fails on a machine without a GPU.
"""
import os
import re

import numpy as np
import pytest

import host_road_cases as H
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR_HOST = os.path.join(ROOT, "fractal-renderer_amd", "csrc", "fr_host.hip")
REDERIVE = ("fr_host.hip and tests/host_road_cases.py disagree about %s: re-derive the mirror AND the table of cases "
            "(the shapes were chosen for the old value; run tests/test_host_road_shapes_cpu.py until every class is hit)")


def _source():
    with open(FR_HOST) as f:
        return f.read()


def _shift_constant(src, name):
    m = re.search(r"constexpr\s+size_t\s+%s\s*=\s*\(size_t\)\s*(\d+)\s*<<\s*(\d+)\s*;" % name, src)
    assert m, REDERIVE % name
    return int(m.group(1)) << int(m.group(2))


def test_constants_are_those_of_fr_host_hip():
    src = _source()
    for name, mine in (("kStageMax", H.K_STAGE_MAX), ("kSdmaMin", H.K_SDMA_MIN), ("kPinThreshold", H.K_PIN_THRESHOLD),
                       ("kChunk", H.K_CHUNK)):
        assert _shift_constant(src, name) == mine, REDERIVE % name
    m = re.search(r"constexpr\s+size_t\s+kPage\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == H.K_PAGE, REDERIVE % "kPage"
    # the band rule of host_render_staged: nb = ceil(need / (6 << 20)); two bands from 3 << 20; at most four
    m = re.search(r"nb\s*=\s*\(uint32_t\)\(\(need \+ \(\(size_t\)(\d+) << (\d+)\) - 1\) / \(\(size_t\)(\d+) << (\d+)\)\);\s*"
                  r"if \(need >= \(\(size_t\)(\d+) << (\d+)\) && nb < 2\) nb = 2;\s*if \(nb > (\d+)\) nb = \7;", src)
    assert m, REDERIVE % "the band rule of host_render_staged"
    v = [int(x) for x in m.groups()]
    assert v[0] << v[1] == v[2] << v[3] == H.BAND_TARGET, REDERIVE % "the 6 << 20 of the band rule"
    assert v[4] << v[5] == H.TWO_BANDS_FROM, REDERIVE % "the 3 << 20 of the band rule"
    assert v[6] == H.MAX_BANDS, REDERIVE % "the most bands of a frame"
    assert re.search(r"band_rows = \(\(rows \+ nb - 1\) / nb \+ 7u\) & ~7u;", src), REDERIVE % "band_rows"
    # the last stretch of the pin road, the helpers, the split and the first touch
    assert re.search(r"left <= kChunk \+ kChunk / 4 \? kChunk / 4 : kChunk", src), REDERIVE % "the kChunk / 4 last stretch"
    assert H.K_LAST_STRETCH == H.K_CHUNK // 4
    # ... and its chunk ends moved back to a page boundary of the HOST address.  (On the GPU nothing observable depends on
    # this line: with it removed, neighbouring registrations share a page, and whether the runtime takes the second one
    # or refuses it and the chunk goes by plain copies, every byte still arrives: test_gpu_host_roads.py passed without
    # it — so the mirror, which has the rounding, is tied to the source here.)
    assert re.search(r"b -= \(reinterpret_cast<uintptr_t>\(out\) \+ b\) & \(kPage - 1\);\s*return b > a \? b : need;", src), \
        REDERIVE % "the page rounding of ChunkPinner::chunk_end"
    m = re.search(r"helpers = need >= \(\(size_t\)(\d+) << (\d+)\) \? copy_helpers\(\) : 0;", src)
    assert m and int(m.group(1)) << int(m.group(2)) == H.HELPERS_FROM, REDERIVE % "the size from which helpers copy"
    m = re.search(r"if \(!pool \|\| len < \(\(size_t\)(\d+) << (\d+)\)\)", src)
    assert m and int(m.group(1)) << int(m.group(2)) == H.SPLIT_FROM, REDERIVE % "the size from which a band is split"
    m = re.search(r"need >= \(\(size_t\)(\d+) << (\d+)\) && !looks_resident\(out, need\)", src)
    assert m and int(m.group(1)) << int(m.group(2)) == H.PREFAULT_FROM, REDERIVE % "the size from which pages are prefaulted"
    m = re.search(r"piece = \(\(len \+ parts - 1\) / parts \+ (\d+)\) & ~\(size_t\)(\d+);", src)
    assert m and int(m.group(1)) == int(m.group(2)) == H.PIECE_ALIGN - 1, REDERIVE % "the piece alignment"
    assert "need <= kStageMax && staging_enabled()" in src and "if (need < kPinThreshold)" in src, REDERIVE % "the road choice"
    assert "if (len < kSdmaMin)" in src, REDERIVE % "kernel versus copy engine"


@pytest.mark.parametrize("name", sorted(H.CLASSES) + sorted(H.CLASSES_NO_STAGING))
def test_every_class_has_a_case(name):
    assert H.cases_of_class(name), "no case of host_road_cases.CASES hits %r any more: add one (the mirror finds it)" % name


def test_the_table_s_shapes_are_what_the_mirror_derives():
    """the figures in the comments of host_road_cases.CASES, re-derived"""
    g = H.case_geometry("head8_1031")
    assert [(b["row1"] - b["row0"], b["offset"], b["head"], b["tail"]) for b in g["bands"]] == [(520, 0, 0, 8), (511, 1608360, 8, 3)]
    g = H.case_geometry("four_kernel_bands")
    assert [b["len"] for b in g["bands"][:3]] == [4844280] * 3 and g["bands"][0]["row1"] == 632
    assert all(b["len"] < H.K_SDMA_MIN for b in g["bands"])
    g = H.case_geometry("four_engine_bands")
    assert [b["len"] for b in g["bands"]] == [6266880] * 3 + [6082560]
    g = H.case_geometry("mixed_engine_kernel")
    assert [(b["row1"] - b["row0"], b["len"], b["via"]) for b in g["bands"]] == [(16, 9600048, "engine"), (1, 600003, "kernel")]
    assert H.case_geometry("stage_max_exact")["need"] == 41943040 == H.K_STAGE_MAX
    g = H.case_geometry("stage_max_plus_row")
    assert g["road"] == "pin" and g["chunks"] == [0, 16 << 20, 32 << 20, g["need"]]
    g = H.case_geometry("pin_road_108mb")
    assert g["need"] == 108000000 and g["chunks"] == [0, 64 << 20, 80 << 20, 96 << 20, 108000000]
    narrow, wide = H.pick_split_pair()
    assert (narrow, wide) == (H.CASES["one_band_no_helpers"]["width"], H.CASES["split_just_over"]["width"])
    # every stream-alternating band list is in image order and covers the request exactly once
    for name in H.CASES:
        for staging in (True, False):
            g = H.case_geometry(name, 1, staging)
            pos = 0
            for b in g["bands"]:
                assert b["offset"] == pos and b["len"] > 0 and (b["row0"] % 8 == 0 or g["road"] != "staged")
                pos += b["len"]
            assert pos == g["need"], (name, staging)


@pytest.mark.parametrize("name,staging", [("stage_max_plus_row", True), ("pin_road_108mb", True), ("four_engine_bands", False),
                                          ("four_kernel_bands", False)])
@pytest.mark.parametrize("off", [0, 1, 8, 4095])
def test_pin_road_chunks_are_page_aligned_and_cover_the_buffer_once(name, staging, off):
    g = H.case_geometry(name, off, staging)
    assert g["road"] == "pin"
    need, bounds = g["need"], g["chunks"]
    assert bounds[0] == 0 and bounds[-1] == need and len(bounds) >= 3
    assert all(a < b for a, b in zip(bounds, bounds[1:])), "chunks cover [0, need) exactly once, in order"
    for b in bounds[1:-1]:
        assert (off + b) % H.K_PAGE == 0, "an interior chunk boundary is a page boundary of the HOST address"
    assert all(b - a <= H.K_CHUNK for a, b in zip(bounds, bounds[1:]))
    # what gets registered: whole pages, no page in two registrations, outer edges within a page of the buffer
    regs = H.pin_ranges(off, need)
    for (ra, rb), (a, b) in zip(regs, zip(bounds, bounds[1:])):
        assert (off + ra) % H.K_PAGE == 0 and (off + rb) % H.K_PAGE == 0 and ra <= a < b <= rb
    assert all(r0[1] == r1[0] for r0, r1 in zip(regs, regs[1:]))
    assert -H.K_PAGE < regs[0][0] <= 0 and need <= regs[-1][1] < need + H.K_PAGE
    assert regs[0][0] >= -H.GUARD and regs[-1][1] <= need + H.GUARD, "the rounded-out pins stay inside the test's guards"
    # bands: image order, whole 8-row tiles, issued in a permutation
    assert sorted(b["issue"] for b in g["bands"]) == list(range(len(g["bands"])))
    assert all(b["row0"] % 8 == 0 for b in g["bands"])


@pytest.mark.parametrize("threads", [1, 2, 4, 16])
def test_copy_pieces_cover_a_band_once(threads):
    for name in ("head8_1031", "four_kernel_bands", "four_engine_bands", "split_just_over", "stage_max_exact"):
        g = H.case_geometry(name)
        for length in [b["len"] for b in g["bands"]] + [g["need"]]:
            pieces = H.copy_pieces(length, threads if g["helpers"] else 1)
            assert pieces[0][0] == 0 and sum(n for _, n in pieces) == length and len(pieces) <= threads
            assert all(a0 + n0 == a1 for (a0, n0), (a1, _) in zip(pieces, pieces[1:]))
            assert all(a % H.PIECE_ALIGN == 0 and n > 0 for a, n in pieces)


def test_specs_round_trip():
    s = H.make_spec("head8_1031", off=4095, mem="fresh", prec="f32", slack=4096)
    assert H.parse_spec(s) == ("head8_1031", {"off": 4095, "mem": "fresh", "prec": "f32", "slack": 4096})
    assert H.parse_spec("rgba_1080p") == ("rgba_1080p", dict(H.SPEC_DEFAULTS))
    for bad in ("nonesuch", "head8_1031:off=4096", "head8_1031:mem=swapped", "head8_1031:colour=1"):
        with pytest.raises((KeyError, ValueError)):
            H.parse_spec(bad)


def _oracle_rows(name, poison=False):
    case = H.CASES[name]
    ocfg = H.oracle_config(O, case, poison)
    O.set_log2_mode(O.LOG2_LIBM)
    img = O.get_image(ocfg, O.F64, case["y0"], case["y1"], threads=16)
    return img.reshape(img.shape[0], -1)  # [rows, row_bytes]


@pytest.mark.parametrize("name", ["head8_1031", "four_kernel_bands"])
def test_the_reference_image_makes_a_misplaced_band_visible(name):
    """Conditions on the oracle's image alone (CPU): with this view a band written 8 or 16 bytes off, two bands swapped,
    a band that stops a row early or a dropped head / tail cannot produce the right bytes by accident."""
    g = H.case_geometry(name)
    rows = _oracle_rows(name)
    flat = rows.reshape(-1)
    assert flat.size == g["need"] and len(g["bands"]) >= 2
    firsts = [rows[b["row0"]] for b in g["bands"]]
    for i, b in enumerate(g["bands"]):
        if i:
            assert not np.array_equal(rows[b["row0"] - 1], rows[b["row0"]]), "the rows at the seam of band %d are equal" % i
        for j in range(i):
            assert not np.array_equal(firsts[i], firsts[j]), "bands %d and %d start with the same row" % (j, i)
            n = min(b["len"], g["bands"][j]["len"])
            assert not np.array_equal(flat[b["offset"]:b["offset"] + n], flat[g["bands"][j]["offset"]:g["bands"][j]["offset"] + n])
        seg = flat[b["offset"]:b["offset"] + b["len"]]
        for shift in (8, 16):
            assert not np.array_equal(seg[shift:], seg[:-shift]), "band %d equals itself shifted by %d bytes" % (i, shift)
            # ... and not only somewhere: at the band's very start and end, where a shifted copy meets its neighbour
            a = b["offset"]
            if a:
                assert not np.array_equal(flat[a:a + 64], flat[a - shift:a - shift + 64])
            assert not np.array_equal(seg[-64:], seg[-64 - shift:-shift])
    # the vertical flip differs in every row pair (the default view would fail this: it is mirror-symmetric in y)
    half = rows.shape[0] // 2  # (the middle row of an odd height is its own mirror image)
    assert not (rows[:half] == rows[::-1][:half]).all(axis=1).any()
    # head and tail bytes of every kernel band: not what an untouched page holds (zeros), and not what the frame rendered
    # just before (the driver's poison view) left at the same place of the staging buffer
    poison = _oracle_rows(name, poison=True).reshape(-1)
    for i, b in enumerate(g["bands"]):
        edges = []
        if b["head"]:
            edges.append((b["offset"], b["offset"] + b["head"]))
        if b["tail"]:
            edges.append((b["offset"] + b["len"] - b["tail"], b["offset"] + b["len"]))
        for a, e in edges:
            assert flat[a:e].any(), "band %d: head/tail bytes [%d, %d) are all zero in the reference" % (i, a, e)
            assert not np.array_equal(flat[a:e], poison[a:e]), "band %d: the poison view has the same bytes at [%d, %d)" % (i, a, e)
    assert sum(1 for b in g["bands"] if b["head"] == 8) >= 1


def test_a_fenced_buffer_ends_a_process_that_touches_the_page_behind_it():
    """mem=fenced of host_road_driver.py: the payload's last byte is readable, the byte behind it is not — in a child
    process, with no GPU involved.  This is what makes a first touch that runs one page too far (it writes every byte
    back unchanged, so no guard pattern sees it) fail test_gpu_host_roads.py."""
    import signal
    import subprocess
    import sys

    code = ("import sys, ctypes; sys.path.insert(0, %r); import host_road_driver as D\n"
            "b = D.Guarded(1263903, fenced=True)\n"
            "assert (b.out + b.need) %% 4096 == 0 and b.guards_intact() is None and not b.payload().any()\n"
            "one = ctypes.create_string_buffer(1)\n"
            "ctypes.memmove(one, b.out + b.need - 1, 1)\n"
            "print('last byte read', flush=True)\n"
            "if sys.argv[1] == 'past': ctypes.memmove(one, b.out + b.need, 1)\n"
            "print('done', flush=True)\n") % os.path.dirname(os.path.abspath(__file__))
    ok = subprocess.run([sys.executable, "-c", code, "within"], capture_output=True, text=True, timeout=300)
    assert ok.returncode == 0 and ok.stdout.split() == ["last", "byte", "read", "done"], (ok.returncode, ok.stderr[-800:])
    past = subprocess.run([sys.executable, "-c", code, "past"], capture_output=True, text=True, timeout=300)
    assert past.returncode == -signal.SIGSEGV and "last byte read" in past.stdout and "done" not in past.stdout, (
        past.returncode, past.stdout, past.stderr[-800:])
