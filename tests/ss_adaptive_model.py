"""ADAPTIVE SUPERSAMPLING (include/fractal_hip.h) restated in numpy from H alone: H is the road's plain render of cfg_s, uint8
[s*height, s*width, 3], whoever made it.  Nothing here knows a kernel."""
import numpy as np


def np_filter(big, s, channels=3):
    """F: big uint8 [s*rows, s*width, 3] -> uint8 [rows, width, channels]: (block sum + s*s // 2) // (s*s), alpha 255"""
    rows, width = big.shape[0] // s, big.shape[1] // s
    sums = big.reshape(rows, s, width, s, 3).astype(np.uint32).sum(axis=(1, 3))
    rgb = ((sums + (s * s) // 2) // (s * s)).astype(np.uint8)
    if channels == 3:
        return rgb
    out = np.full((rows, width, 4), 255, dtype=np.uint8)
    out[..., :3] = rgb
    return out


def probe(big, s):
    """P(X, Y) = H(s*X + p, s*Y + p), p = s // 2"""
    p = s // 2
    return big[p::s, p::s]


def edges(big, s, tau):
    """edge(X, Y) over the whole image, bool [height, width]: tau < 0, or a neighbour inside the image whose probe differs by
    more than tau in some channel"""
    P = probe(big, s).astype(np.int32)
    h, w = P.shape[:2]
    if tau < 0:
        return np.ones((h, w), dtype=bool)
    e = np.zeros((h, w), dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            # pixels (X, Y) with the neighbour (X + dx, Y + dy) inside the image
            ys = slice(max(0, -dy), h - max(0, dy))
            xs = slice(max(0, -dx), w - max(0, dx))
            yn = slice(max(0, dy), h - max(0, -dy))
            xn = slice(max(0, dx), w - max(0, -dx))
            e[ys, xs] |= (np.abs(P[ys, xs] - P[yn, xn]) > tau).any(axis=-1)
    return e


def adaptive(big, s, tau, y0=0, y1=None, channels=3, escape_algo=True, filter=None):
    """(out uint8 [y1-y0, width, channels], refined) of rows [y0, y1): the edge set is the whole image's, cut to the rows.
    filter(big, s) -> uint8 [height, width, 3] is F; None is the byte filter np_filter, ss_linear_model.ss_filter with the sRGB
    transfer gives LINEAR-LIGHT SUPERSAMPLING's"""
    h = big.shape[0] // s
    y1 = h if y1 is None else y1
    if not escape_algo:
        out = np.zeros((y1 - y0, big.shape[1] // s, channels), dtype=np.uint8)
        if channels == 4:
            out[..., 3] = 255
        return out, 0
    e = edges(big, s, tau)[y0:y1]
    P = probe(big, s)[y0:y1]
    F = (np_filter if filter is None else filter)(big, s)[y0:y1]
    rgb = np.where(e[..., None], F, P)
    if channels == 4:
        out = np.full(rgb.shape[:2] + (4,), 255, dtype=np.uint8)
        out[..., :3] = rgb
    else:
        out = np.ascontiguousarray(rgb)
    return out, int(e.sum())


def edge_share(big, s, tau):
    return float(edges(big, s, tau).mean())


def workspace_bytes(width, height, y0, y1):
    """the workspace rule of include/fractal_hip.h restated"""
    if width == 0 or y1 == y0:
        return 0
    ya, yb = max(y0 - 1, 0), min(y1 + 1, height)
    up8 = lambda n: (n + 7) // 8 * 8
    return up8(3 * width * (yb - ya)) + up8(4 * width * (y1 - y0)) + 16
