"""SUPERSAMPLED DE (include/fractal_hip.h) restated in numpy on top of tests/de_model.py: the DE arrays of cfg_s are coloured
and shaded by de_model.colour with the thickness T * s — the distance then is in sample pixels, its last factor
(s * height) * min|scale| — and the bytes go through the integer box filter of "supersampled rendering"."""
import ctypes as C

import numpy as np

import de_model as DE


def config_s(cfg, s):
    """cfg with width * s and height * s, every other field unchanged (a copy)"""
    big = type(cfg).from_buffer_copy(bytes(cfg))
    big.width, big.height = cfg.width * s, cfg.height * s
    return big


def box(big, s, channels=3):
    """big uint8 [s*rows, s*width, 3] -> uint8 [rows, width, channels]: (block sum + s*s // 2) // (s*s), alpha 255"""
    big = np.asarray(big)
    rows, width = big.shape[0] // s, big.shape[1] // s
    sums = big.reshape(rows, s, width, s, 3).astype(np.uint32).sum(axis=(1, 3))
    rgb = ((sums + (s * s) // 2) // (s * s)).astype(np.uint8)
    if channels == 3:
        return rgb
    out = np.full((rows, width, 4), 255, dtype=np.uint8)
    out[..., :3] = rgb
    return out


def shaded(cfg, z, it, der, s, thickness):
    """H of the definition: the shaded bytes of the samples, uint8 [s*rows, s*width, 3].  cfg is the OUTPUT image's config: its
    height is the whole image's, whatever number of rows the arrays hold."""
    assert C.sizeof(cfg) == 104
    return DE.colour(config_s(cfg, s), z, it, der, float(thickness) * float(s), 3)


def colour(cfg, z, it, der, s, thickness, channels=3):
    """the image of the definition over the DE arrays of cfg_s: uint8 [rows, width, channels]"""
    return box(shaded(cfg, z, it, der, s, thickness), s, channels)
