#!/usr/bin/env python3
"""Exact orbit derivatives of the deep views, from tests/de_scaled_truth.py (Python integers): writes
tests/golden/de_scaled_truth.npz.

Per view of de_scaled_truth.VIEWS (deep_truth's PAST and WIDE_DOMAIN): `<view>/iters` (uint32 [h, w]), `<view>/u` (float64
[h, w, 2]: d 2^-e, the f64 nearest to the exact value) and `<view>/precision` (uint32 [2]: P = 2e + 320 and P + 320, the fraction
bits of the two runs).  The file holds only data computed by this project's own test code.

Every view is computed twice, at P and at P + 320 fraction bits.  Nothing is written unless, on every view, the two runs agree
on both arrays bit for bit and the indices are those of tests/golden/deep_truth.npz.

The archive is written with fixed timestamps and no compression, so that a second run gives the same bytes.
Usage: python tests/golden/make_de_scaled_truth.py [--jobs N]"""
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
import de_scaled_truth as U  # noqa: E402


def main(argv):
    jobs = int(argv[argv.index("--jobs") + 1]) if "--jobs" in argv else min(16, os.cpu_count() or 1)
    arrays = {}
    t_all = time.time()
    for name in U.VIEWS:  # the centres (mpmath) once, before the workers are forked
        T.view(name)
    with multiprocessing.Pool(jobs) as pool:
        for name in U.VIEWS:
            t0 = time.time()
            v = T.view(name)
            first = U.view_truth(name, 0, pool)
            second = U.view_truth(name, T.EXTRA, pool)
            assert T.same_truth(first, second), "%s: %d and %d fraction bits disagree" % (name, v.P, v.P + T.EXTRA)
            assert np.array_equal(first["iters"], T.load(name)["iters"]), "%s: not deep_truth's indices" % name
            esc = first["iters"] < v.cap
            print("%-13s e %4d  P %4d  %3d x %2d  escaped %4d of %4d  finite u on all of them: %s  %.0f s" % (
                name, v.e, v.P, v.width, v.height, int(esc.sum()), esc.size, bool(np.isfinite(first["u"][esc]).all()),
                time.time() - t0), flush=True)
            for k in U.FIELDS:
                arrays["%s/%s" % (name, k)] = first[k]
            arrays["%s/precision" % name] = np.array([v.P, v.P + T.EXTRA], dtype=np.uint32)
    with zipfile.ZipFile(U.FIXTURE, "w", zipfile.ZIP_STORED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), version=(1, 0), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
    print("%s: %d bytes, %.0f s" % (os.path.relpath(U.FIXTURE), os.path.getsize(U.FIXTURE), time.time() - t_all))


if __name__ == "__main__":
    main(sys.argv[1:])
