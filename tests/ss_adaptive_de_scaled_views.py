"""What the generated and edge views of tests/deep_ss_views.py gain for ADAPTIVE SUPERSAMPLED SCALED DE, shared by
tests/test_ss_adaptive_de_scaled_random_cpu.py (the models alone: does the set have teeth) and
tests/test_gpu_ss_adaptive_de_scaled_random.py (the kernels against the models on the same inputs).  No device and no library.

The inputs are EVERY view of deep_ss_views.everything() — inside 2^440 and past it — on the scaled road, twice: the plain scaled loop
(bits -1) and the table form at the view's table_bits.  An input is a tests/ss_adaptive_de_views.py Input whose config is the SCALED
VIEW of the view's config (de_scaled_model.scaled_view: scale = (sre, sim)), so that everything that file derives — H_de, tau_de,
the median reach, de_mixed, describe() — is derived as it derives them, on the scaled view:
  arrays     deep_ss_views.Ss.rows("de_scaled", bits): (z, iters, u) of de_scaled_model.escape_rows on cfg_s;
  s, thickness  the view's own (deep_ss_views: the thickness is the median distance of the escaped samples on the scaled view);
  H_de, tau_de, reach, de_mixed  as ss_adaptive_de_views states them, with cfg_sv where it has cfg_s.
The model is ss_adaptive_de_model.adaptive_de unchanged: run on the scaled view it is the definition."""
import functools

import de_scaled_model as DSM
import deep_random_views as G
import deep_ss_views as V
import ss_adaptive_de_views as AV

FILTERS = AV.FILTERS


def bits_of(v):
    """the two forms of a view: (the model's bits, the call's bits) of the plain scaled loop and of the table"""
    return ((-1, -1), (v.g.table_bits, v.g.call_bits))


@functools.lru_cache(maxsize=None)
def of_view(v, bits):
    """the input of a view on the scaled road at the MODEL's bits: -1 or the view's table_bits"""
    assert bits in (-1, v.g.table_bits)
    call_bits = -1 if bits < 0 else v.g.call_bits
    name = "SCALED PT, bits %d" % call_bits
    cfg_v = DSM.scaled_view(v.cfg)
    inp = AV.Input("%s, %s" % (v.g.label, name), cfg_v, v.s, v.thickness, lambda: v.rows("de_scaled", bits),
                   lambda: "%s, %s" % (name, v.g.describe(v.cfg)))
    inp.v, inp.bits, inp.call_bits = v, bits, call_bits
    return inp


def deep(v):
    """the view lies past 2^440: outside WIDE PT's domain"""
    return not v.g.wide


def inputs(table=False):
    """the inputs of every view, at bits -1 or at the view's table bits"""
    return [of_view(v, v.g.table_bits if table else -1) for v in V.everything()]


def inputs_of(seed):
    """both inputs of every view of a seed"""
    return [of_view(v, b) for v in V.views(seed) for b, _ in bits_of(v)]


def edge_inputs(name):
    v = V.edge(name)
    return [of_view(v, b) for b, _ in bits_of(v)]


SEEDS = V.SEEDS
EDGES = tuple(G.EDGES)
