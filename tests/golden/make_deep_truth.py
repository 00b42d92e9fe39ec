#!/usr/bin/env python3
"""Exact per-pixel orbits of the deep views, from tests/deep_truth.py (Python integers): writes tests/golden/deep_truth.npz.

Per view of deep_truth.VIEWS: `<view>/iters` (uint32 [h, w]), `<view>/z` (float64 [h, w, 2], the f64 nearest to the exact z),
`<view>/settled` (bool [h, w]), `<view>/move` (float64 [h, w]) and `<view>/precision` (uint32 [2]: P = 2e + 320 and P + 320,
the fraction bits of the two runs).  The file holds only data computed by this project's own test code.

Every view is computed twice, at P and at P + 320 fraction bits, five orbits per pixel each time (the pixel and the four
displaced points).  Nothing is written unless, on every view, the two runs agree on every array bit for bit, at least 95 % of
the pixels are settled and there are at least 10 distinct escape indices.

The archive is written with fixed timestamps and no compression, so that a second run gives the same bytes.

Time, measured: 67 s with 8 worker processes, about 9 minutes of one CPU (--jobs 1); the two minibrot views take three
quarters of it.
Usage: python tests/golden/make_deep_truth.py [--jobs N]"""
import io
import multiprocessing
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import deep_truth as T  # noqa: E402


def main(argv):
    jobs = int(argv[argv.index("--jobs") + 1]) if "--jobs" in argv else min(16, os.cpu_count() or 1)
    arrays = {}
    t_all = time.time()
    for name in T.VIEWS:  # the centres (mpmath) once, before the workers are forked
        T.view(name)
    with multiprocessing.Pool(jobs) as pool:
        for name in T.VIEWS:
            t0 = time.time()
            v = T.view(name)
            first = T.view_truth(name, 0, pool)
            second = T.view_truth(name, T.EXTRA, pool)
            assert T.same_truth(first, second), "%s: %d and %d fraction bits disagree" % (name, v.P, v.P + T.EXTRA)
            share, indices = T.condition(first)
            print("%-13s e %4d  P %4d  %3d x %2d  settled %4d of %4d  indices %3d  max %5d  at cap %3d  %.0f s" % (
                name, v.e, v.P, v.width, v.height, int(first["settled"].sum()), first["settled"].size, indices,
                int(first["iters"].max()), int((first["iters"] == v.cap).sum()), time.time() - t0), flush=True)
            assert share >= T.MIN_SETTLED, "%s: only %.1f %% of the pixels are settled" % (name, 100 * share)
            assert indices >= T.MIN_INDICES, "%s: only %d distinct escape indices" % (name, indices)
            for k in T.FIELDS:
                arrays["%s/%s" % (name, k)] = first[k]
            arrays["%s/precision" % name] = np.array([v.P, v.P + T.EXTRA], dtype=np.uint32)
    with zipfile.ZipFile(T.FIXTURE, "w", zipfile.ZIP_STORED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), version=(1, 0), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
    print("%s: %d bytes, %.0f s" % (os.path.relpath(T.FIXTURE), os.path.getsize(T.FIXTURE), time.time() - t_all))


if __name__ == "__main__":
    main(sys.argv[1:])
