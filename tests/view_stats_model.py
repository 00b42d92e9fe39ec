"""The statistics of a kept view (include/fractal_hip.h, "statistics of a kept view") restated in numpy and Python
integers, from the header text and not from the kernels: the yardstick of tests/test_view_stats_cpu.py and
tests/test_gpu_view_stats.py.

A record is a dict with the fields of struct fr_view_stats; hist is a list of FR_STATS_BINS Python ints."""
import math

import numpy as np

BINS = 1024
FIELDS = ("n", "stable", "capped", "escaped", "sum_iters", "min_iters", "max_iters", "shift", "reserved")
SIZEOF = 5 * 8 + 4 * 4 + 8 * BINS  # 8248


def classes(z, iters, iterations, stable_limit):
    """z float64 [n, 2 or 4], iters uint32 [n] -> boolean masks (S, C, E)"""
    z = np.asarray(z, dtype=np.float64)
    z = z.reshape(-1, z.shape[-1])
    it = np.asarray(iters, dtype=np.uint32).reshape(-1)
    assert z.shape[1] in (2, 4) and z.shape[0] == it.size
    re, im = z[:, 0], z[:, z.shape[1] // 2]  # z_width 4: re.hi, re.lo, im.hi, im.lo
    with np.errstate(all="ignore"):
        dist = re * re + im * im  # two multiplications and one addition, nothing fused
        outside = dist > np.float64(stable_limit)  # False for a NaN dist
    capped = outside & (it >= np.uint32(iterations))
    return ~outside, capped, outside & ~capped


def shift_of(lo, hi):
    s = 0
    while (hi - lo) >> s >= BINS:
        s += 1
    return s


def view_stats(z, iters, iterations, stable_limit):
    it = np.asarray(iters, dtype=np.uint32).reshape(-1)
    s, c, e = classes(z, iters, iterations, stable_limit)
    rec = dict(n=int(it.size), stable=int(s.sum()), capped=int(c.sum()), escaped=int(e.sum()), sum_iters=0, min_iters=0, max_iters=0,
               shift=0, reserved=0, hist=[0] * BINS)
    if rec["escaped"]:
        ie = it[e].astype(np.uint64)
        lo, hi = int(ie.min()), int(ie.max())
        rec.update(sum_iters=int(ie.sum(dtype=np.uint64)) % (1 << 64), min_iters=lo, max_iters=hi, shift=shift_of(lo, hi))
        bins = np.bincount(((ie - np.uint64(lo)) >> np.uint64(rec["shift"])).astype(np.int64), minlength=BINS)
        assert len(bins) == BINS
        rec["hist"] = [int(v) for v in bins]
    assert rec["n"] == rec["stable"] + rec["capped"] + rec["escaped"]
    return rec


def percentile(rec, p):
    if rec["escaped"] == 0:
        return 0
    k = min(max(int(math.ceil(p * float(rec["escaped"]))), 1), rec["escaped"])  # one f64 multiplication
    cum = 0
    for b in range(BINS):
        cum += rec["hist"][b]
        if cum >= k:
            return min(rec["max_iters"], rec["min_iters"] + ((b + 1) << rec["shift"]) - 1)
    raise ValueError("the histogram holds fewer pixels than `escaped`")


def auto_exposure(iterations, exposure, rec, p):
    """cfg->iterations, cfg->exposure, the record, p -> the exposure"""
    if rec["escaped"] == 0:
        return float(exposure)
    return float(iterations) / float(max(percentile(rec, p), 1))  # one f64 division


def from_struct(st):
    """a ctypes fr_view_stats -> record"""
    rec = {f: int(getattr(st, f)) for f in FIELDS}
    rec["hist"] = [int(v) for v in st.hist]
    return rec


def to_struct(rec, cls):
    st = cls()
    for f in FIELDS:
        setattr(st, f, rec[f])
    for b, v in enumerate(rec["hist"]):
        st.hist[b] = v
    return st


def diff(got, want):
    """the names of the fields in which two records differ (hist bins as hist[b])"""
    out = [f for f in FIELDS if got[f] != want[f]]
    out += ["hist[%d]" % b for b in range(BINS) if got["hist"][b] != want["hist"][b]]
    return out
