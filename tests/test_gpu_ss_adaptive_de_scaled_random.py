"""ADAPTIVE SUPERSAMPLED SCALED DE on the device (fr_render_rows_ss_adaptive_de_pt_scaled(_tf)(_device): the scaled arm of
csrc/fr_ss_adaptive_de.hip and ss_refine_de_scaled_kernel, all eight instances), byte for byte and count for count against
ss_adaptive_de_model.adaptive_de run on the scaled view over the HOST MODEL arrays of cfg_s (de_scaled_model.escape_rows), on the
inputs of tests/ss_adaptive_de_scaled_views.py: every generated and edge view of tests/deep_ss_views.py — inside 2^440 and past it,
shifted centres, negative and unequal axes, drawn colour fields with `smooth` and `inside` off, limits up to 2^20, every lane
mapping s = 2, 3, 4, 5, 7, 8 (ppw = 16, 7, 4, 2, 1, 1, idle lanes at s = 3, 5, 7) — at bits -1 and at the view's table bits, the
view's own s and thickness, and a threshold and a reach derived on the scaled view.
tests/test_ss_adaptive_de_scaled_random_cpu.py asserts from the models alone that the set has teeth.  Nothing is compared against
the code under test.  Every device call gets a guarded destination, the smallest workspace between guards and a guarded d_refined
(test_gpu_ss_adaptive_de_scaled.ads_device); every assertion message carries the input's describe(); a de_mixed input asserts on
the model that it cannot pass emptily.  Per input: the whole image, the drawn row piece and the three-way split, alternately on
the device and the host form, transfers 0 and 1; on the first view of a seed and on the edge views also RGBA, the grid forced to 1
workgroup and d_refined NULL.  The views of a seed run in one process one after another."""
import numpy as np
import pytest

import ss_adaptive_de_scaled_views as SV
from test_gpu_deep_ss_random import case, differ
from test_gpu_deep_truth import check, fr, lib, native, torch  # noqa: F401  (fixtures and helpers)
from test_gpu_ss_adaptive_de_scaled import ads_device, ads_host

pytestmark = pytest.mark.gpu


def run(torch, c, inp, tau, reach, transfer, what, host=False, **more):
    """one call against the model: bytes and count"""
    want, count = inp.model(tau, reach, more.get("y0", 0), more.get("y1"), more.get("channels", 3), filter=SV.FILTERS[transfer])
    if host:
        got, n = ads_host(c.lib, c.cfg, c.centre, inp.call_bits, inp.s, inp.thickness, tau, reach, transfer=transfer, **more)
    else:
        got, n = ads_device(torch, c.lib, c.cfg, c.centre, inp.call_bits, inp.s, inp.thickness, tau, reach, transfer=transfer, **more)
    if more.get("want_refined", True) is False:
        n = count
    assert np.array_equal(got, want) and n == count, "%s, t %d, R %r, transfer %d: %d pixels differ, refined %d, the model %d; %s" % (
        what, tau, reach, transfer, differ(got, want), n, count, inp.describe())
    return count


def not_empty(inp):
    """a de_mixed input cannot pass emptily: by the model, 0 < refined < width * rows, a pixel that only `near` marks and a pixel
    of the union with F != P"""
    if inp.de_mixed:
        e, n = inp.sets
        count = inp.model(inp.tau, inp.reach)[1]
        assert 0 < count < inp.w * inp.h and (n & ~e).any() and ((e | n) & inp.differ).any(), inp.describe()


def check_view(c, torch, extras):
    v = c.v
    for k, (bits, _call_bits) in enumerate(SV.bits_of(v)):
        inp = SV.of_view(v, bits)
        not_empty(inp)
        tau, reach = inp.tau, inp.reach
        for transfer in (0, 1):
            host = (k + transfer) % 2 == 1  # each form sees each transfer over the two bits
            count = run(torch, c, inp, tau, reach, transfer, "the whole image", host=host)
            if not inp.orbits:
                assert count == 0 and not inp.model(tau, reach)[0].any()
            y0, y1 = v.piece
            run(torch, c, inp, tau, reach, transfer, "rows [%d, %d)" % (y0, y1), host=not host, y0=y0, y1=y1)
            if v.three_way() is not None:  # each piece against its slice: the bytes concatenate to the whole, the counts sum
                for y0, y1 in v.three_way():
                    run(torch, c, inp, tau, reach, transfer, "rows [%d, %d)" % (y0, y1), host=host, y0=y0, y1=y1)
        if not extras:
            continue
        run(torch, c, inp, tau, reach, 0, "RGBA", channels=4)
        run(torch, c, inp, tau, reach, 1, "d_refined NULL", want_refined=False)
        run(torch, c, inp, -1, reach, 0, "every pixel")
        try:
            check(c.lib.fr_debug_ss_adaptive_grid(1))
            for transfer in (0, 1):
                run(torch, c, inp, tau, reach, transfer, "1 workgroup")
        finally:
            check(c.lib.fr_debug_ss_adaptive_grid(0))


@pytest.mark.parametrize("seed", SV.SEEDS)
def test_random_views(fr, native, lib, torch, seed):
    for k, v in enumerate(SV.V.views(seed)):
        check_view(case(fr, native, lib, v), torch, extras=k == 0)


@pytest.mark.parametrize("name", SV.EDGES)
def test_edge_views(fr, native, lib, torch, name):
    check_view(case(fr, native, lib, SV.V.edge(name)), torch, extras=True)
