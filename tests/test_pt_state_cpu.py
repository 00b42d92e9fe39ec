"""Resumable perturbation (include/fractal_hip.h, fr_precision: "RESUMABLE PT"; fr_escape_rows_pt_state(_device),
fr_escape_extend_pt(_device), fr_debug_pt_orbit_cache), the part that needs no device:
  - the definition on the host: over five views and the cap chain 0, 1, 2, 5, 37, 38, 200, 333, 1500, 4000 the state run's
    (z, iters) ARE PT's (tests/pt_model.c) at every cap, and continuing the state N -> M on the orbits of cap M IS the state
    run at M, bit for bit in all four arrays, link by link and 0 -> 4000 in one jump, with m < last at the top of every
    resumed step;
  - the views have teeth: the table of running pixels that met the end of a cap-cut orbit at the final step — the pixels
    whose (dz, m) PT's own rule would leave different — is recomputed and pinned, and a state kept under PT's rule is shown
    NOT to continue to PT's results;
  - the domain of the four calls, checked before any device work, and their legal no-ops without a device;
  - header, ctypes prototypes, Rust shim and C++ wrapper agree."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import pt_model as PM
import pt_state_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000  # a non-NULL, aligned "device pointer" for calls that must be refused before they touch it
NAMES = list(SM.VIEWS)
SIZES = {"seahorse": (32, 24), "early_escape": (48, 32), "julia_rebase": (48, 32), "shallow_mandelbrot": (67, 45),
         "shallow_julia": (67, 45)}

# (running pixels, of them: never rebased and m == last of a cap-cut X at the final step) per view and cap N >= 1
CLASSES = {
    "seahorse": {n: (768, 768) for n in SM.CHAIN[1:]},  # R is cut by every cap and no pixel ever rebases
    "early_escape": {1: (1536, 1536), 2: (1536, 1536), 5: (1536, 1536), 37: (1265, 0), 38: (1259, 0), 200: (1194, 0),
                     333: (1188, 0), 1500: (1176, 0), 4000: (1172, 0)},  # R ends by escape at entry 30
    "julia_rebase": {1: (1536, 1536), 2: (1536, 1536), 5: (1536, 1536), 37: (1536, 1536), 38: (1536, 1536), 200: (778, 214),
                     333: (82, 0), 1500: (0, 0), 4000: (0, 0)},  # V ends by escape at entry 201
    "shallow_mandelbrot": {1: (3015, 1219), 2: (3015, 705), 5: (1921, 192), 37: (526, 90), 38: (524, 90), 200: (500, 90),
                           333: (496, 90), 1500: (494, 90), 4000: (494, 90)},
    "shallow_julia": {1: (3015, 1541), 2: (3015, 920), 5: (1936, 308), 37: (436, 18), 38: (426, 6), 200: (140, 0), 333: (62, 0),
                      1500: (0, 0), 4000: (0, 0)},  # V ends by escape at entry 252
}


@functools.lru_cache(maxsize=None)
def fresh(name, n):
    """(cfg, pos_lo, the model's state at cap n), computed once and never written to"""
    cfg, lo = SM.view(name, O.config_new, n)
    st = SM.state_rows(cfg, lo)
    for a in st:
        a.setflags(write=False)
    return cfg, lo, st


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("name", NAMES)
def test_state_run_gives_pt_results_at_every_cap(name):
    for n in SM.CHAIN:
        cfg, lo, st = fresh(name, n)
        assert (cfg.width, cfg.height) == SIZES[name]
        z, it = PM.escape_rows(cfg, lo)
        assert np.array_equal(st[1], it), (name, n, int((st[1] != it).sum()))
        assert same_bits(st[0], z), (name, n)
        done = st[1] != n
        assert not st[3][done].any() and not st[2][done].view(np.uint64).any(), "an escaped pixel stores dz = 0, m = 0"
    assert PM.split(PM.SEAHORSE_RE)[1] != 0.0  # the seahorse view runs with a non-zero pos_lo


@pytest.mark.parametrize("name", NAMES)
def test_initial_state(name):
    cfg, lo, (z, it, dz, m) = fresh(name, 0)
    julia = cfg.algo == 2
    assert not it.any() and (m == (0 if julia else 1)).all()
    x = np.arange(cfg.width, dtype=np.float64)
    y = np.arange(cfg.height, dtype=np.float64)
    w, h = float(cfg.width), float(cfg.height)
    off_re = ((x / h) - ((w / h) / 2.0)) / cfg.scale.re
    off_im = ((y / h) - 0.5) / cfg.scale.im
    assert same_bits(dz[..., 0], np.broadcast_to(off_re, it.shape)) and same_bits(dz[..., 1], np.broadcast_to(off_im[:, None], it.shape))
    start = PM.reference_orbit(cfg, lo, 0)[0 if julia else 1]
    assert same_bits(z[..., 0], start[0] + dz[..., 0]) and same_bits(z[..., 1], start[1] + dz[..., 1])


@pytest.mark.parametrize("name", NAMES)
def test_continuing_a_state_is_the_state_run_at_the_higher_cap(name):
    st = fresh(name, SM.CHAIN[0])[2]
    for n, m in zip(SM.CHAIN, SM.CHAIN[1:]):
        cfg, lo, want = fresh(name, m)
        st, violations = SM.continue_rows(cfg, st, n, lo)
        assert violations == 0, "m >= last at the top of a resumed step (%s, %d -> %d)" % (name, n, m)
        assert SM.same_state(st, want), (name, n, m)
    cfg, lo, want = fresh(name, SM.CHAIN[-1])
    jump, violations = SM.continue_rows(cfg, fresh(name, 0)[2], 0, lo)
    assert violations == 0 and SM.same_state(jump, want)


@pytest.mark.parametrize("name", NAMES)
def test_class_table(name):
    """how many running pixels sit at the end of a cap-cut orbit after the final step: where PT's rule would rebase"""
    got = {n: SM.cut_end_class(*fresh(name, n)[::2], pos_lo=fresh(name, n)[1]) for n in SM.CHAIN[1:]}
    assert got == CLASSES[name], got
    if name in ("seahorse", "shallow_mandelbrot", "shallow_julia"):
        assert any(c > 0 for _, c in got.values())
    assert SM.cut_end_class(*fresh(name, 0)[::2], pos_lo=fresh(name, 0)[1])[1] == 0  # no final step at cap 0


@pytest.mark.parametrize("name", ["seahorse", "shallow_mandelbrot", "shallow_julia"])
def test_a_state_kept_under_pts_own_rule_does_not_continue(name):
    """rule 1 = rebase at the end of X whatever ended it (PT's registers after the cap-cut rebase): its fresh results are
    PT's, but continued to the next cap it leaves PT's results wherever the class above is not empty"""
    n, m = 37, 38
    cfg_n, lo, _ = fresh(name, n)
    assert CLASSES[name][n][1] > 0
    st = SM.state_rows(cfg_n, lo, rule=1)
    z, it = PM.escape_rows(cfg_n, lo)
    assert np.array_equal(st[1], it) and same_bits(st[0], z)
    cfg_m = fresh(name, m)[0]
    st, _ = SM.continue_rows(cfg_m, st, n, lo, rule=1)
    z, it = PM.escape_rows(cfg_m, lo)
    assert not (np.array_equal(st[1], it) and same_bits(st[0], z))


def test_orbit_ends_of_the_views():
    """(last, ended by escape) of X at the chain's ends: which cache road each view takes when its cap is raised"""
    for name, at_37, at_4000 in (("seahorse", (38, False), (4001, False)), ("early_escape", (30, True), (30, True)),
                                 ("julia_rebase", (37, False), (201, True)), ("shallow_mandelbrot", (38, False), (4001, False)),
                                 ("shallow_julia", (37, False), (252, True))):
        cfg, lo, _ = fresh(name, 37)
        assert SM.orbit_info(cfg, lo, 0) == at_37, name
        assert len(PM.reference_orbit(cfg, lo, 0)) == at_37[0] + 1
        cfg, lo, _ = fresh(name, 4000)
        assert SM.orbit_info(cfg, lo, 0) == at_4000, name
    cfg, lo, _ = fresh("julia_rebase", 4000)
    assert SM.orbit_info(cfg, lo, 1) == (252, True)  # the critical orbit of this constant: shallow_julia's V, which starts at 0 too
    assert SM.orbit_info(fresh("julia_rebase", 200)[0], lo, 1) == (200, False)


# ---- the library, without a device ----------------------------------------------------------------------------


@pytest.fixture(scope="module")
def fr():
    import __graft_entry__ as ge

    ge.build()
    import fractal_renderer_amd

    return fractal_renderer_amd


@pytest.fixture(scope="module")
def lib(fr):
    from fractal_renderer_amd import _native

    return _native.load()


def small(fr, iterations=37):
    cfg = fr.Config.new()
    cfg.width, cfg.height, cfg.iterations = 67, 45, iterations
    return cfg


def state_dev(lib, cfg, n, z=FAKE, it=FAKE, dz=FAKE, m=FAKE, y0=0, y1=None, lo=None):
    y1 = cfg.height if y1 is None else y1
    return lib.fr_escape_rows_pt_state_device(C.byref(cfg) if cfg is not None else None, lo, y0, y1, z, it, dz, m, None)


def state_host(lib, cfg, n, z=FAKE, it=FAKE, dz=FAKE, m=FAKE, y0=0, y1=None, lo=None):
    y1 = cfg.height if y1 is None else y1
    return lib.fr_escape_rows_pt_state(C.byref(cfg) if cfg is not None else None, lo, y0, y1, z, it, dz, m)


def extend_dev(lib, cfg, n, z=FAKE, it=FAKE, dz=FAKE, m=FAKE, y0=0, y1=None, lo=None):
    y1 = cfg.height if y1 is None else y1
    return lib.fr_escape_extend_pt_device(C.byref(cfg) if cfg is not None else None, lo, y0, y1, n, z, it, dz, m, None)


def extend_host(lib, cfg, n, z=FAKE, it=FAKE, dz=FAKE, m=FAKE, y0=0, y1=None, lo=None):
    y1 = cfg.height if y1 is None else y1
    return lib.fr_escape_extend_pt(C.byref(cfg) if cfg is not None else None, lo, y0, y1, n, z, it, dz, m)


@pytest.mark.parametrize("call", [state_dev, state_host, extend_dev, extend_host], ids=["state_device", "state_host", "extend_device", "extend_host"])
def test_domain_is_checked_without_a_device(fr, lib, call):
    from fractal_renderer_amd import _native

    INVALID, OK = _native.FR_ERR_INVALID_ARGUMENT, _native.FR_OK
    extension = call in (extend_dev, extend_host)
    cfg = small(fr)
    # rows, cfg
    assert call(lib, cfg, 5, y0=9, y1=8) == INVALID and b"y0 > y1" in lib.fr_last_error()
    assert call(lib, cfg, 5, y1=cfg.height + 1) == INVALID and b"y1 > height" in lib.fr_last_error()
    assert call(lib, None, 5, y1=1) == INVALID and b"cfg is NULL" in lib.fr_last_error()
    # PT's domain on cfg and pos_lo
    bad = small(fr)
    bad.limit = float("inf")
    assert call(lib, bad, 5) == INVALID and b"FR_PRECISION_PT" in lib.fr_last_error()
    assert call(lib, cfg, 5, lo=C.byref(_native.Imaginary(1.0, 0.0))) == INVALID and b"normalised" in lib.fr_last_error()
    big = small(fr, (1 << 24) + 1)
    assert call(lib, big, 5) == INVALID and b"FR_PT_MAX_ITERATIONS" in lib.fr_last_error()
    assert call(lib, big, 5, y0=3, y1=3) == INVALID  # ... even with nothing to do
    # all four arrays, aligned
    for k in ("z", "it", "dz", "m"):
        assert call(lib, cfg, 5, **{k: None}) == INVALID and b"NULL" in lib.fr_last_error(), k
    for k, off in (("z", 4), ("dz", 4), ("it", 2), ("m", 2)):
        assert call(lib, cfg, 5, **{k: FAKE + off}) == INVALID and b"aligned" in lib.fr_last_error(), k
    assert call(lib, cfg, 5, z=FAKE + 8, dz=FAKE + 8, it=FAKE + 4, m=FAKE + 4, y0=2, y1=2) == OK
    # no rows: a legal no-op that needs neither arrays nor a device
    assert call(lib, cfg, 5, y0=7, y1=7) == OK
    assert call(lib, cfg, 5, y0=7, y1=7, z=None, it=None, dz=None, m=None) == OK
    if extension:
        assert call(lib, cfg, 38) == INVALID and b"lower cap cannot be derived" in lib.fr_last_error()
        assert call(lib, cfg, 37) == OK  # M == N
        assert call(lib, small(fr, 0), 0) == OK
        assert call(lib, cfg, 37, z=None) == INVALID  # ... but the arrays are required whatever the caps
        fern = small(fr)
        fern.algo = 1
        assert call(lib, fern, 5) == OK  # no orbits: nothing to continue


def test_the_f64_extension_still_refuses_pt_and_names_the_new_calls(fr, lib):
    from fractal_renderer_amd import _native

    cfg = small(fr)
    rc = lib.fr_escape_extend_device(C.byref(cfg), 3, None, 0, cfg.height, 5, 2, FAKE, FAKE, None, None)
    assert rc == _native.FR_ERR_INVALID_ARGUMENT
    msg = lib.fr_last_error()
    assert b"FR_PRECISION_PT" in msg and b"fr_escape_extend_pt" in msg and b"fr_escape_rows_pt_state" in msg


def test_orbit_cache_hook_needs_no_device(fr, lib):
    from fractal_renderer_amd import _native

    out = (C.c_uint32 * 4)(9, 9, 9, 9)
    assert lib.fr_debug_pt_orbit_cache(out) == _native.FR_OK
    if fr.device_count() == 0:
        assert tuple(out) == (0, 0, 0, 0)  # no context, no cached orbit
    assert lib.fr_debug_pt_orbit_cache(None) == _native.FR_ERR_INVALID_ARGUMENT


def test_python_wrappers_check_shapes_and_no_op_at_the_same_cap(fr):
    cfg = small(fr)
    shape = (cfg.height, cfg.width)
    z, dz = np.zeros(shape + (2,)), np.ones(shape + (2,))
    it, m = np.full(shape, 37, dtype=np.uint32), np.full(shape, 38, dtype=np.uint32)
    got = fr.extend_rows_pt(cfg, z, it, dz, m, 37)
    assert got[0] is not z and all(np.array_equal(a, b) for a, b in zip(got, (z, it, dz, m)))
    with pytest.raises(ValueError):
        fr.extend_rows_pt(cfg, z[:-1], it, dz, m, 37)
    with pytest.raises(ValueError):
        fr.extend_rows_pt(cfg, z, it, dz[..., :1], m, 37)
    with pytest.raises(fr.FractalHipError) as e:
        fr.extend_rows_pt(cfg, z, it, dz, m, 38)
    assert e.value.code == 1 and "lower cap" in str(e.value)
    empty = fr.escape_rows_pt_state(cfg, y0=4, y1=4)
    assert [a.shape for a in empty] == [(0, 67, 2), (0, 67), (0, 67, 2), (0, 67)]
    fr.escape_rows_pt_state_device(cfg, 0, 0, 0, 0, y0=4, y1=4)
    fr.extend_rows_pt_device(cfg, FAKE, FAKE, FAKE, FAKE, 37)


CALLS = ["fr_escape_rows_pt_state_device", "fr_escape_extend_pt_device", "fr_escape_rows_pt_state", "fr_escape_extend_pt"]


def test_header_prototypes_shim_and_wrapper_agree(fr):
    import test_rust_shim_abi as R
    from fractal_renderer_amd import _native

    _, hf = R.parse_header()
    _, rf, _ = R.parse_shim()
    for name in CALLS:
        assert name in hf and name in _native.PROTOTYPES
        assert rf.get(name) == hf[name], (name, rf.get(name), hf[name])
        assert len(_native.PROTOTYPES[name][1]) == len(hf[name][1])
    assert hf["fr_escape_extend_pt_device"] == ("c_int", ["*const fr_config", "*const fr_imaginary", "u32", "u32", "u32", "*mut c_void",
                                                          "*mut c_void", "*mut c_void", "*mut c_void", "*mut c_void"])
    assert hf["fr_debug_pt_orbit_cache"] == ("c_int", ["*mut u32"]) and "fr_debug_pt_orbit_cache" in _native.PROTOTYPES
    header = open(os.path.join(ROOT, "include", "fractal_hip.h")).read()
    assert re.search(r"#define FR_ABI_VERSION 3\b", header)
    hpp = open(os.path.join(ROOT, "fractal-renderer_amd", "host", "fractal.hpp")).read()
    assert "fr_escape_rows_pt_state_device(" in hpp and "fr_escape_extend_pt_device(" in hpp
