"""LINEAR-LIGHT SUPERSAMPLING (include/fractal_hip.h) restated in numpy from H, s, the transfer and the two tables alone.  H is
the s times larger image, uint8 [s*rows, s*width, 3], whoever made it; L is the decode table (256 values), T the thresholds
T[1 .. 255] (255 values, T[k] at index k - 1).  Nothing here knows the library or a kernel."""
import numpy as np

BYTES, SRGB = 0, 1


def encode(m, T):
    """E(m): the number of k in 1 .. 255 with m >= T[k]"""
    return np.searchsorted(np.asarray(T, dtype=np.int64), np.asarray(m, dtype=np.int64), side="right").astype(np.uint8)


def ss_filter(H, s, transfer, L, T, channels=3):
    """out uint8 [rows, width, channels]: per channel (sum of the s x s block + s*s // 2) // (s*s) — of the bytes for BYTES, of
    L[byte] followed by E for SRGB; alpha 255"""
    rows, width = H.shape[0] // s, H.shape[1] // s
    v = H.astype(np.int64) if transfer == BYTES else np.asarray(L, dtype=np.int64)[H]
    m = (v.reshape(rows, s, width, s, 3).sum(axis=(1, 3)) + (s * s) // 2) // (s * s)
    rgb = m.astype(np.uint8) if transfer == BYTES else encode(m, T)
    if channels == 3:
        return rgb
    out = np.full((rows, width, 4), 255, dtype=np.uint8)
    out[..., :3] = rgb
    return out
