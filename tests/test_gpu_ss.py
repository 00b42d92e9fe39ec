"""Supersampled rendering on the device (fractal-renderer_amd/csrc/fr_ss.hip; include/fractal_hip.h, "supersampled
rendering"), byte for byte, no tolerance anywhere:
  - the box filter alone against numpy, over every s, ragged widths and rows, every source / destination alignment,
    guard bytes, inputs that separate truncation from the two roundings, and a source of more than 4 GiB;
  - supersampled renders against the oracle's image of cfg_s (soft log2, as tests/test_gpu_parity.py) filtered by numpy,
    over workspace lengths that put a band seam everywhere, row ranges, RGB and RGBA, F64 and F32 — with floors on the
    yardstick itself, so that a view that degenerates fails loudly;
  - DD and PT against the host models coloured by the oracle, then filtered;
  - s = 1, host road = device road, guards and the workspace canary, per-call selectors, two threads at once;
  - production sizes against the existing render of cfg_s filtered with torch integer arithmetic on the device."""
import ctypes as C
import threading

import numpy as np
import pytest

import dd_model as DM
import oracle_lib as O
import pt_model as PM

pytestmark = pytest.mark.gpu

F64, F32, DD, PT = 0, 1, 2, 3
GUARD = 64
S_RENDER = [2, 3, 4, 5, 8]


@pytest.fixture(scope="module")
def fr():
    import fractal_renderer_amd

    assert fractal_renderer_amd.device_count() > 0, "no HIP device: the GPU tests need a real MI355X"
    fractal_renderer_amd.init(0)
    assert fractal_renderer_amd.device_name().startswith("gfx950")
    return fractal_renderer_amd


@pytest.fixture(scope="module")
def lib(fr):
    from fractal_renderer_amd import _native

    return _native.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def check(rc):
    from fractal_renderer_amd import _native

    _native.check(rc)


# ---- the definition, in numpy ---------------------------------------------------------------------------


def np_filter(big, s, channels=3):
    """big uint8 [s*rows, s*width, 3] -> uint8 [rows, width, channels]: (block sum + s*s // 2) // (s*s), alpha 255"""
    rows, width = big.shape[0] // s, big.shape[1] // s
    sums = big.reshape(rows, s, width, s, 3).astype(np.uint32).sum(axis=(1, 3))
    rgb = ((sums + (s * s) // 2) // (s * s)).astype(np.uint8)
    if channels == 3:
        return rgb
    out = np.full((rows, width, 4), 255, dtype=np.uint8)
    out[..., :3] = rgb
    return out


def block_stats(big, s):
    """(share of s x s blocks that mix colours, number of exact half-way channel sums: 2 * (sum % s*s) == s*s)"""
    rows, width = big.shape[0] // s, big.shape[1] // s
    b = big.reshape(rows, s, width, s, 3)
    mixed = (b.max(axis=(1, 3)) != b.min(axis=(1, 3))).any(axis=-1)
    sums = b.astype(np.uint32).sum(axis=(1, 3))
    halfway = int((2 * (sums % (s * s)) == s * s).sum())
    return float(mixed.mean()), halfway


# ---- device calls -----------------------------------------------------------------------------------------


def device_filter(torch, lib, big, s, channels, src_off=0, dst_off=0, use_stream=None):
    """fr_box_filter_rgb8_device over a numpy source placed src_off bytes behind an aligned base, into a destination
    dst_off bytes behind one, with guard bytes on both sides; returns the output, guards checked"""
    rows, width = big.shape[0] // s, big.shape[1] // s
    dev = torch.device("cuda", 0)
    d_src = torch.empty(big.size + 16, dtype=torch.uint8, device=dev)
    d_src[src_off:src_off + big.size] = torch.from_numpy(big.reshape(-1)).to(dev)
    need = channels * width * rows
    d_out = torch.full((GUARD + 16 + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert d_src.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    at = GUARD + dst_off
    torch.cuda.synchronize()
    check(lib.fr_box_filter_rgb8_device(d_src.data_ptr() + src_off, width, rows, s, channels, d_out.data_ptr() + at, need,
                                        use_stream))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert (host[:at] == 0xA5).all() and (host[at + need:] == 0xA5).all(), "the filter wrote outside its destination"
    return host[at:at + need].reshape(rows, width, channels)


def ss_device(torch, lib, cfg, precision, s, y0, y1, channels, work_len, pos_lo=None, opts=None, stream=None):
    """fr_render_rows_ss_device into a guarded destination with a canary behind the workspace"""
    from fractal_renderer_amd import _native

    dev = torch.device("cuda", 0)
    need = channels * cfg.width * (y1 - y0)
    d_out = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_work = torch.full((work_len + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    lo = C.byref(_native.Imaginary(*pos_lo)) if pos_lo is not None else None
    st = stream.cuda_stream if stream is not None else None
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    torch.cuda.synchronize()
    check(lib.fr_render_rows_ss_device(C.byref(cfg), precision, lo, s, y0, y1, channels, d_out.data_ptr() + GUARD, need,
                                       d_work.data_ptr() if work_len else None, work_len, st,
                                       C.byref(opts) if opts is not None else None))
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    host = d_out.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "wrote outside the destination"
    assert (d_work[work_len:].cpu().numpy() == 0x5A).all(), "wrote behind work_len"
    return host[GUARD:GUARD + need].reshape(y1 - y0, cfg.width, channels)


def workspace(lib, cfg, s, y0, y1):
    mn, best = C.c_size_t(), C.c_size_t()
    check(lib.fr_ss_workspace_bytes(C.byref(cfg), s, y0, y1, C.byref(mn), C.byref(best)))
    return mn.value, best.value


# ---- the filter alone --------------------------------------------------------------------------------------


def crafted(s, width, rows):
    """an image whose block sums run through every residue modulo s*s in every channel, so that truncation, round half
    down and round half up all give different bytes somewhere: block (X, Y), channel c gets the sum
    (7 * (Y * width + X) + 3 * c) mod (255 * s * s + 1), spread over the block as evenly as the sum allows"""
    n = s * s
    Y, X, c = np.indices((rows, width, 3))
    total = (7 * (Y * width + X) + 3 * c) % (255 * n + 1)
    base, extra = total // n, total % n
    big = np.empty((rows, s, width, s, 3), dtype=np.uint8)
    for j in range(s):
        for i in range(s):
            big[:, j, :, i, :] = base + ((j * s + i) < extra)
    return big.reshape(rows * s, width * s, 3)


def filter_inputs(s, width, rows):
    rng = np.random.default_rng(1000 * s + 10 * width + rows)
    shape = (rows * s, width * s, 3)
    yield "random", rng.integers(0, 256, shape, dtype=np.uint8)
    yield "zeros", np.zeros(shape, dtype=np.uint8)
    yield "ones", np.full(shape, 255, dtype=np.uint8)
    if s in (2, 4, 8):
        yield "crafted", crafted(s, width, rows)


def test_the_crafted_image_separates_the_roundings():
    for s in (2, 4, 8):
        big = crafted(s, 64, 64)
        n = s * s
        sums = big.reshape(64, s, 64, s, 3).astype(np.uint32).sum(axis=(1, 3))
        assert set(np.unique(sums % n)) == set(range(n))
        trunc, half_down = sums // n, (sums + n // 2 - 1) // n
        want = np_filter(big, s)
        assert (want != trunc).any() and (want != half_down).any() and (2 * (sums % n) == n).sum() >= 50


@pytest.mark.parametrize("s", range(1, 9))
def test_box_filter_is_the_definition(fr, lib, torch, s):
    for width in (1, 5, 64, 257, 1000):
        for rows in (1, 7, 64):
            for name, big in filter_inputs(s, width, rows):
                want3, want4 = np_filter(big, s, 3), np_filter(big, s, 4)
                full = name == "random" or (name == "crafted" and width in (5, 257))
                offs = [(a, b) for a in range(4) for b in range(4)] if full else [(0, 0), (1, 2), (3, 1)]
                for a, b in offs:
                    got = device_filter(torch, lib, big, s, 3, a, b)
                    assert np.array_equal(got, want3), (s, width, rows, name, a, b, int((got != want3).sum()))
                for a in (range(4) if full else (0, 3)):
                    for b in (0, 4, 8):  # RGBA destinations stay 4-byte aligned
                        got = device_filter(torch, lib, big, s, 4, a, b)
                        assert np.array_equal(got, want4), (s, width, rows, name, a, b)


def test_box_filter_host_form_and_wrapper(fr, lib):
    rng = np.random.default_rng(5)
    for s, width, rows in [(1, 33, 9), (2, 257, 7), (3, 100, 31), (8, 300, 5)]:
        big = rng.integers(0, 256, (rows * s, width * s, 3), dtype=np.uint8)
        assert np.array_equal(fr.box_filter(big, s), np_filter(big, s))
        assert np.array_equal(fr.box_filter(big, s, channels=4), np_filter(big, s, 4))


def test_box_filter_over_a_source_larger_than_4_gib(fr, lib, torch):
    """s = 2, output 30000 x 12000: the source is 60000 x 24000 x 3 = 4.32e9 bytes, so byte offsets pass 2^32 (at source
    row 23860 = output row 11930).  Built and checked with torch on the device: the first 64 and the last 128 output
    rows, which include the rows around the 4 GiB mark."""
    s, width, rows = 2, 30000, 12000
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(77)
    src = torch.randint(0, 256, (rows * s * width * s * 3,), dtype=torch.uint8, device=dev, generator=g)
    assert src.numel() > (1 << 32)
    out = torch.zeros(rows * width * 3, dtype=torch.uint8, device=dev)
    check(lib.fr_box_filter_rgb8_device(src.data_ptr(), width, rows, s, 3, out.data_ptr(), out.numel(), None))
    torch.cuda.synchronize()
    out = out.view(rows, width, 3)
    big = src.view(rows * s, width * s, 3)
    for ra, rb in [(0, 64), (rows - 128, rows)]:
        part = big[ra * s:rb * s].view(rb - ra, s, width, s, 3).to(torch.int32).sum(dim=(1, 3))
        want = ((part + 2) // 4).to(torch.uint8)
        assert torch.equal(out[ra:rb], want), (ra, rb, int((out[ra:rb] != want).sum()))


# ---- supersampled renders against the oracle ------------------------------------------------------------------

VIEWS = {
    "default": dict(algo=O.MANDELBROT, iterations=256),
    "julia": dict(algo=O.JULIA, iterations=300, julia_set=(-0.8, 0.156)),
    "flat": dict(algo=O.MANDELBROT, iterations=100, smooth=0, inside=0),
    "zoom1e6": dict(algo=O.MANDELBROT, iterations=1024, pos=(-0.7436447860, 0.1318252536), scale=(1e6, 1e6)),
}
SIZES = [(96, 64), (257, 193)]
_yard = {}


def view_config(name, width, height):
    kw = dict(VIEWS[name])
    algo = kw.pop("algo")
    return O.cli_config(width, height, algo, **kw)


def yardstick(name, width, height, s, precision):
    """(the oracle's image of cfg_s, the oracle's s = 1 image) in soft-log2 mode"""
    key = (name, width, height, s, precision)
    if key not in _yard:
        O.set_log2_mode(O.LOG2_SOFT)
        try:
            big = O.get_image(view_config(name, width * s, height * s), precision)
            one = O.get_image(view_config(name, width, height), precision)
        finally:
            O.set_log2_mode(O.LOG2_LIBM)
        _yard[key] = (big, one)
    return _yard[key]


@pytest.mark.parametrize("precision", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("s", S_RENDER)
@pytest.mark.parametrize("size", SIZES, ids=["96x64", "257x193"])
@pytest.mark.parametrize("name", list(VIEWS))
def test_supersampled_render_is_the_filtered_oracle_image(fr, lib, torch, name, size, s, precision):
    width, height = size
    big, one = yardstick(name, width, height, s, precision)
    want3, want4 = np_filter(big, s, 3), np_filter(big, s, 4)
    # the yardstick itself must exercise the filter: a view that degenerates fails here, loudly
    differ = float((want3 != one).any(axis=-1).mean())
    mixed, halfway = block_stats(big, s)
    print("%s %dx%d s=%d prec=%d: %.1f%% of pixels differ from s=1, %.1f%% of blocks mixed, %d half-way sums"
          % (name, width, height, s, precision, 100 * differ, 100 * mixed, halfway))
    assert differ >= 0.10, "only %.1f%% of the output pixels differ from the s = 1 image" % (100 * differ)
    assert mixed >= 0.10, "only %.1f%% of the blocks mix colours" % (100 * mixed)
    if s % 2 == 0:
        assert halfway >= 50, "only %d exact half-way sums" % halfway
    cfg = fr.Config.from_buffer_copy(bytes(view_config(name, width, height)))
    for y0, y1 in [(0, height), (5, 37), (height - 1, height), (9, 9)]:
        mn, best = workspace(lib, cfg, s, y0, y1)
        for work_len in sorted({mn, best, (mn + best) // 2 | 1}):
            for channels, want in ((3, want3), (4, want4)):
                got = ss_device(torch, lib, cfg, precision, s, y0, y1, channels, work_len)
                assert np.array_equal(got, want[y0:y1]), (y0, y1, work_len, channels, int((got != want[y0:y1]).sum()))
    # the host road and the Python front ends
    assert np.array_equal(fr.get_image(cfg, precision, supersample=s), want3)
    assert np.array_equal(fr.get_image_rgba(cfg, precision, supersample=s), want4)
    assert np.array_equal(fr.get_image_rows(cfg, 5, 37, precision, supersample=s), want3[5:37])


# ---- DD and PT against the host models ---------------------------------------------------------------------------


def model_image(cfg_s, precision, pos_lo):
    ocfg = O.Config.from_buffer_copy(bytes(cfg_s))
    O.set_log2_mode(O.LOG2_LIBM)
    if precision == DD:
        z4, it = DM.escape_rows(cfg_s, pos_lo)
        z = np.ascontiguousarray(z4[..., 0::2])
    else:
        z, it = PM.escape_rows(cfg_s, pos_lo)
    return O.colour_rows(ocfg, z, it)


def deep_cases(fr):
    for julia in (False, True):
        for lo in ((0.0, 0.0), (0.0, 2.0 ** -66)):
            cfg = fr.Config.new()
            DM.deep_view(cfg, julia, 64, 48)
            cfg.exposure = 150.0
            yield "deep_%s_lo%d" % ("julia" if julia else "mandelbrot", int(lo[1] != 0)), cfg, lo, (DD, PT), 0.10, 50
    cfg = fr.Config.new()
    lo = PM.seahorse_view(cfg)
    yield "seahorse", cfg, lo, (PT,), 0.10, 0
    cfg = fr.Config.new()
    lo = PM.julia_rebase_view(cfg)
    yield "julia_rebase", cfg, lo, (PT,), 0.10, 0


@pytest.mark.parametrize("s", [2, 3])
def test_deep_supersampled_renders_are_the_filtered_models(fr, lib, torch, s):
    for name, cfg, lo, precisions, mixed_floor, half_floor in deep_cases(fr):
        cfg_s = cfg.clone()
        cfg_s.width, cfg_s.height = cfg.width * s, cfg.height * s
        for precision in precisions:
            big = model_image(cfg_s, precision, lo)
            mixed, halfway = block_stats(big, s)
            print("%s s=%d prec=%d: %.1f%% of blocks mixed, %d half-way sums" % (name, s, precision, 100 * mixed, halfway))
            assert mixed >= mixed_floor, (name, mixed)
            if s == 2:
                assert halfway >= half_floor, (name, halfway)
            want3, want4 = np_filter(big, s, 3), np_filter(big, s, 4)
            h = cfg.height
            for y0, y1 in [(0, h), (5, 23)]:
                mn, best = workspace(lib, cfg, s, y0, y1)
                for work_len in sorted({mn, best}):
                    got = ss_device(torch, lib, cfg, precision, s, y0, y1, 3, work_len, pos_lo=lo)
                    assert np.array_equal(got, want3[y0:y1]), (name, precision, y0, y1, work_len)
            got4 = ss_device(torch, lib, cfg, precision, s, 0, h, 4, workspace(lib, cfg, s, 0, h)[0], pos_lo=lo)
            assert np.array_equal(got4, want4), (name, precision)
            assert np.array_equal(fr.get_image(cfg, precision, pos_lo=lo, supersample=s), want3), (name, precision)
            assert np.array_equal(fr.get_image_rgba(cfg, precision, pos_lo=lo, supersample=s), want4), (name, precision)


# ---- further cases -------------------------------------------------------------------------------------------------


def small_view(fr, julia=False):
    cfg = fr.Config.from_buffer_copy(bytes(view_config("julia" if julia else "default", 257, 193)))
    return cfg


def test_supersample_one_is_the_plain_render(fr, lib, torch):
    cfg = small_view(fr)
    for precision in (F64, F32, DD, PT):
        plain3 = fr.get_image(cfg, precision)
        plain4 = fr.get_image_rgba(cfg, precision)
        assert workspace(lib, cfg, 1, 0, cfg.height) == (0, 0)
        assert np.array_equal(ss_device(torch, lib, cfg, precision, 1, 0, cfg.height, 3, 0), plain3)
        assert np.array_equal(ss_device(torch, lib, cfg, precision, 1, 17, 150, 4, 0), plain4[17:150])
        out = np.empty_like(plain3)
        check(lib.fr_render_rows_ss(C.byref(cfg), precision, None, 1, 0, cfg.height, 3, out.ctypes.data, out.nbytes, None))
        assert np.array_equal(out, plain3)
    deep = fr.Config.new()
    DM.deep_view(deep, False, 64, 48)
    lo = (0.0, 2.0 ** -66)
    for precision in (DD, PT):
        assert np.array_equal(ss_device(torch, lib, deep, precision, 1, 0, 48, 3, 0, pos_lo=lo),
                              fr.get_image(deep, precision, pos_lo=lo))


def test_host_road_equals_device_road_with_guards(fr, lib, torch):
    for julia in (False, True):
        cfg = small_view(fr, julia)
        for s in (2, 5):
            for precision in (F64, F32):
                for channels in (3, 4):
                    for y0, y1 in [(0, cfg.height), (5, 37)]:
                        mn, _ = workspace(lib, cfg, s, y0, y1)
                        dev = ss_device(torch, lib, cfg, precision, s, y0, y1, channels, mn)
                        need = dev.size
                        host = np.full(GUARD + need + GUARD, 0xA5, dtype=np.uint8)
                        check(lib.fr_render_rows_ss(C.byref(cfg), precision, None, s, y0, y1, channels,
                                                    host.ctypes.data + GUARD, need, None))
                        assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all()
                        assert np.array_equal(host[GUARD:GUARD + need].reshape(dev.shape), dev), (julia, s, precision, channels)


def test_the_fern_stays_black(fr, lib, torch):
    cfg = small_view(fr)
    cfg.algo = int(fr.Algo.BarnsleyFern)
    img = fr.get_image(cfg, supersample=3)
    assert img.shape == (193, 257, 3) and not img.any()
    rgba = fr.get_image_rgba(cfg, supersample=2)
    assert not rgba[..., :3].any() and (rgba[..., 3] == 255).all()


def test_selectors_do_not_change_a_byte(fr, lib, torch):
    for julia in (False, True):
        cfg = small_view(fr, julia)
        s = 3
        mn, best = workspace(lib, cfg, s, 0, cfg.height)
        want = ss_device(torch, lib, cfg, F64, s, 0, cfg.height, 3, best)
        for kw in (dict(tile=1), dict(tile=9), dict(tile=11), dict(loop_mode=0)):
            for work_len in (mn, best):
                got = ss_device(torch, lib, cfg, F64, s, 0, cfg.height, 3, work_len, opts=fr.RenderOpts(**kw))
                assert np.array_equal(got, want), (julia, kw, work_len)
            out = np.empty_like(want)
            check(lib.fr_render_rows_ss(C.byref(cfg), F64, None, s, 0, cfg.height, 3, out.ctypes.data, out.nbytes,
                                        C.byref(fr.RenderOpts(**kw))))
            assert np.array_equal(out, want), (julia, kw)


def test_profiling_spans_the_whole_call(fr, lib, torch):
    cfg = small_view(fr)
    mn, best = workspace(lib, cfg, 4, 0, cfg.height)
    check(lib.fr_set_profiling(1))
    try:
        ms, name = C.c_float(), C.create_string_buffer(160)
        ss_device(torch, lib, cfg, F64, 4, 0, cfg.height, 3, mn)
        check(lib.fr_last_kernel_ms(C.byref(ms)))
        many = ms.value
        check(lib.fr_last_kernel_name(name, len(name)))
        assert b"escape" in name.value, name.value
        ss_device(torch, lib, cfg, F64, 4, 0, 8, 3, mn)  # one band of the 25
        check(lib.fr_last_kernel_ms(C.byref(ms)))
        assert many > 0 and ms.value > 0 and many > ms.value, (many, ms.value)
    finally:
        check(lib.fr_set_profiling(0))


def test_two_threads_at_once(fr, lib, torch):
    cfgs = [small_view(fr, False), small_view(fr, True)]
    s = 4
    wants = []
    for cfg in cfgs:
        mn, best = workspace(lib, cfg, s, 0, cfg.height)
        wants.append(ss_device(torch, lib, cfg, F64, s, 0, cfg.height, 3, best))
    errors = []

    def device_worker(k):
        try:
            fr.init(-1)
            stream = torch.cuda.Stream(torch.device("cuda", 0))
            mn, _ = workspace(lib, cfgs[k], s, 0, cfgs[k].height)
            for _ in range(6):
                got = ss_device(torch, lib, cfgs[k], F64, s, 0, cfgs[k].height, 3, mn + 12345 * k, stream=stream)
                assert np.array_equal(got, wants[k]), "device road, thread %d" % k
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    def host_worker(k):
        try:
            for _ in range(6):
                assert np.array_equal(fr.get_image(cfgs[k], supersample=s), wants[k]), "host road, thread %d" % k
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    for worker in (device_worker, host_worker):
        threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors


# ---- production sizes, checked on the device ----------------------------------------------------------------------------


def torch_filter(torch, big, s):
    rows, width = big.shape[0] // s, big.shape[1] // s
    sums = big.view(rows, s, width, s, 3).to(torch.int32).sum(dim=(1, 3))
    return ((sums + (s * s) // 2) // (s * s)).to(torch.uint8)


PRODUCTION = [("default", 1920, 1080, 2, F64), ("default", 1920, 1080, 4, F64), ("default", 4096, 4096, 2, F64),
              ("default", 4096, 4096, 2, F32), ("c4_julia", 4096, 4096, 2, F64), ("c4_julia", 4096, 4096, 2, F32)]


@pytest.mark.parametrize("name,width,height,s,precision", PRODUCTION,
                         ids=["%s_%dx%d_s%d_%s" % (n, w, h, s, "f32" if p else "f64") for n, w, h, s, p in PRODUCTION])
def test_production_sizes_under_a_64_mib_workspace(fr, lib, torch, name, width, height, s, precision):
    """the existing render of cfg_s, whole, filtered with torch integer arithmetic, against the supersampled call whose
    64 MiB workspace puts band seams under the seven-tile strips and the two-pass kernels"""
    if name == "default":
        cfg = fr.Config.new()
        cfg.iterations = 1024
    else:
        cfg = fr.Config.from_buffer_copy(bytes(O.cli_config(width, height, O.JULIA, iterations=4096, julia_set=(-0.8, 0.156))))
    cfg.width, cfg.height = width, height
    cfg_s = cfg.clone()
    cfg_s.width, cfg_s.height = width * s, height * s
    dev = torch.device("cuda", 0)
    big = torch.empty(3 * cfg_s.width * cfg_s.height, dtype=torch.uint8, device=dev)
    check(lib.fr_render_rows_rgb8_device(C.byref(cfg_s), precision, 0, cfg_s.height, big.data_ptr(), big.numel(), None))
    torch.cuda.synchronize()
    want = torch_filter(torch, big.view(cfg_s.height, cfg_s.width, 3), s)
    work_len = 64 << 20
    mn, best = workspace(lib, cfg, s, 0, height)
    assert mn <= work_len and (best > work_len or (s, height) == (2, 1080))  # several bands, but for 1080p at s = 2
    work = torch.empty(work_len, dtype=torch.uint8, device=dev)
    for channels in (3, 4):
        out = torch.zeros(channels * width * height, dtype=torch.uint8, device=dev)
        check(lib.fr_render_rows_ss_device(C.byref(cfg), precision, None, s, 0, height, channels, out.data_ptr(), out.numel(),
                                           work.data_ptr(), work_len, None, None))
        torch.cuda.synchronize()
        got = out.view(height, width, channels)
        assert torch.equal(got[..., :3], want), (channels, int((got[..., :3] != want).sum()))
        if channels == 4:
            assert bool((got[..., 3] == 255).all())


# ---- the host form's bands under a small workspace cap ---------------------------------------------------------------------

HOOK_W, HOOK_H, HOOK_S, HOOK_Y0, HOOK_Y1 = 37, 21, 3, 2, 19


def host_bands_are_the_device_forms(lib, bytes_per_sample, device, host):
    """What the four banded host forms are tested for under fr_debug_ss_host_work_cap: a cap below min_bytes gives min_bytes —
    one band of 8 * s source rows, three bands over the 17 rows — and the bytes of the device form over ONE band (best_bytes).
    device(work_len) and host() render rows [HOOK_Y0, HOOK_Y1) of the 37 x 21 view at s = 3."""
    row_bytes, rows = bytes_per_sample * HOOK_S * HOOK_W, HOOK_S * (HOOK_Y1 - HOOK_Y0)
    mn, best = 8 * HOOK_S * row_bytes, rows * row_bytes
    assert -(-rows // (8 * HOOK_S)) == 3 and best > mn
    want = device(best)
    assert want.any()
    try:
        check(lib.fr_debug_ss_host_work_cap(8))
        got = host()
    finally:
        check(lib.fr_debug_ss_host_work_cap(0))
    assert np.array_equal(got, want), int((got != want).sum())
    return mn, best


@pytest.mark.parametrize("channels", [3, 4])
def test_host_form_under_a_cap_below_min_bytes_is_the_device_form(fr, lib, torch, channels):
    cfg = fr.Config.from_buffer_copy(bytes(view_config("default", HOOK_W, HOOK_H)))

    def host():
        out = np.zeros((HOOK_Y1 - HOOK_Y0, HOOK_W, channels), dtype=np.uint8)
        check(lib.fr_render_rows_ss(C.byref(cfg), F64, None, HOOK_S, HOOK_Y0, HOOK_Y1, channels, out.ctypes.data, out.nbytes, None))
        return out

    sizes = host_bands_are_the_device_forms(lib, 3, lambda n: ss_device(torch, lib, cfg, F64, HOOK_S, HOOK_Y0, HOOK_Y1, channels, n), host)
    assert sizes == workspace(lib, cfg, HOOK_S, HOOK_Y0, HOOK_Y1)
