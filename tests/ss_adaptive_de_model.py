"""ADAPTIVE SUPERSAMPLED DE (include/fractal_hip.h) restated in numpy on top of the models it is defined from: de_model.colour
and de_model.distance (the shaded bytes and D of the samples of cfg_s), ss_de_model.config_s / box (cfg_s and the box filter) and
ss_adaptive_model.edges (the neighbour rule on the probe colours).  The arrays (z, it, der) are the road's DE render of the WHOLE
image of cfg_s, whoever made them.  Nothing here knows a kernel."""
import numpy as np

import de_model as DE
import ss_adaptive_model as A
import ss_de_model as SD


def shaded(cfg, z, it, der, s, T):
    """H: the shaded bytes of the samples, uint8 [s*height, s*width, 3]"""
    return SD.shaded(cfg, z, it, der, s, T)


def near(cfg, z, it, der, s, reach):
    """near(X, Y), bool [height, width]: the probe escaped and its D, in sample pixels, lies under Rs = R * s"""
    p = s // 2
    rs = float(reach) * float(s)
    zp, ip, dp = (np.ascontiguousarray(a[p::s, p::s]) for a in (z, it, der))
    D = DE.distance(SD.config_s(cfg, s), zp, ip, dp)
    return (ip < cfg.iterations) & (D < rs)


def edge_sets(cfg, z, it, der, s, T, tau, reach):
    """(colour-edge, near) over the whole image, bool [height, width] each; edge is their union"""
    H = shaded(cfg, z, it, der, s, T)
    return A.edges(H, s, tau), near(cfg, z, it, der, s, reach)


def near_only(cfg, z, it, der, s, T, tau, reach):
    """the pixels that `near` marks and the colour rule does not, bool [height, width]"""
    e, n = edge_sets(cfg, z, it, der, s, T, tau, reach)
    return n & ~e


def adaptive_de(cfg, z, it, der, s, T, tau, reach, y0=0, y1=None, channels=3, filter=None, H=None):
    """(out uint8 [y1-y0, width, channels], refined) of rows [y0, y1): the edge set is the whole image's, cut to the rows.
    filter(H, s) -> uint8 [height, width, 3] is F; None is the byte filter ss_de_model.box, ss_linear_model.ss_filter with the
    sRGB transfer gives LINEAR-LIGHT SUPERSAMPLING's.  H: shaded(cfg, z, it, der, s, T) where the caller has it already"""
    h, w = cfg.height, cfg.width
    y1 = h if y1 is None else y1
    if cfg.algo not in (0, 2):
        out = np.zeros((y1 - y0, w, channels), dtype=np.uint8)
        if channels == 4:
            out[..., 3] = 255
        return out, 0
    if H is None:
        H = shaded(cfg, z, it, der, s, T)
    e = (A.edges(H, s, tau) | near(cfg, z, it, der, s, reach))[y0:y1]
    P = A.probe(H, s)[y0:y1]
    F = (SD.box if filter is None else filter)(H, s)[y0:y1]
    rgb = np.where(e[..., None], F, P)
    if channels == 4:
        out = np.full(rgb.shape[:2] + (4,), 255, dtype=np.uint8)
        out[..., :3] = rgb
    else:
        out = np.ascontiguousarray(rgb)
    return out, int(e.sum())


def workspace_bytes(width, height, y0, y1):
    """the workspace rule of include/fractal_hip.h restated: the probe's z, der, iters and colours of rows [ya, yb), the edge
    list of rows [y0, y1) and two counters, every array rounded up to 8 bytes"""
    if width == 0 or y1 == y0:
        return 0
    ya, yb = max(y0 - 1, 0), min(y1 + 1, height)
    n = width * (yb - ya)
    up8 = lambda v: (v + 7) // 8 * 8
    return 16 * n + 16 * n + up8(4 * n) + up8(3 * n) + up8(4 * width * (y1 - y0)) + 16
