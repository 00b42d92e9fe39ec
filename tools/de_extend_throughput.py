"""What raising a DE view's cap in place costs (RESUMABLE DE; csrc/fr_de.hip) beside rendering it again, on the
views of tools/pt_throughput.py:

  - PT: the state render (fr_escape_rows_de_pt_state_device, escape_pt_de_state_kernel) beside the DE render of the same build
    (fr_escape_rows_de_device, escape_pt_de_kernel) at the same cap: what keeping (dz, m) costs;
  - F64 and PT: the extension N -> M for N = M / 2 and N = 0.9 M beside a fresh fr_escape_rows_de_device at M.

Kernel time is fr_set_profiling's events around the kernel, median of --reps after a warm-up, all in one process.  An extension
is not idempotent, so the arrays at N are rendered once, kept, and copied back (device to device, outside the events) before
every timed extension; after the warm-up the context's orbit is the one of cap M and is served as it is.  `running` is the
number of pixels at the cap N, the only ones an extension continues; pixel-iterations are exact, from the escape indices.
--view NAME runs one view, so that a job can give each its own time limit; --out appends.

    python3 tools/de_extend_throughput.py [--view NAME] [--reps 5] [--out profiles/de_extend_throughput.txt]"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: the library binds to the HIP runtime torch carries)

import fractal_renderer_amd as fr  # noqa: E402
from fractal_renderer_amd import _native  # noqa: E402


def pt_views():
    spec = importlib.util.spec_from_file_location("pt_throughput", os.path.join(ROOT, "tools", "pt_throughput.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.views()


def kernel_ms(lib, call, reps, before=None):
    """median material: `reps` kernel times after one warm-up; before() runs ahead of every call, outside the events"""
    ms, times = C.c_float(), []
    _native.check(lib.fr_set_profiling(1))
    try:
        for _ in range(reps + 1):
            if before:
                before()
            _native.check(call())
            _native.check(lib.fr_last_kernel_ms(C.byref(ms)))
            times.append(ms.value)
        name = C.create_string_buffer(160)
        _native.check(lib.fr_last_kernel_name(name, len(name)))
    finally:
        _native.check(lib.fr_set_profiling(0))
    return times[1:], name.value.decode()


def at_cap(cfg, cap):
    c = fr.Config.from_buffer_copy(bytes(cfg))
    c.iterations = cap
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--view", default=None)
    ap.add_argument("--out", default=None, help="also append the printed lines to this file")
    args = ap.parse_args()
    fr.init(0)
    lib = _native.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    lines = ["# tools/de_extend_throughput.py on %s, build %s, %d timed launches per figure (median)"
             % (fr.device_name(), fr.build_id(), args.reps)]
    for vname, cfg, lo in pt_views():
        if args.view and vname != args.view:
            continue
        n, m_cap, h = cfg.width * cfg.height, cfg.iterations, cfg.height
        plo = C.byref(_native.Imaginary(*lo))
        f64 = lambda: torch.empty(2 * n, dtype=torch.float64, device=dev)  # noqa: E731
        u32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
        live = dict(z=f64(), it=u32(), dz=f64(), m=u32(), der=f64())
        kept = {k: torch.empty_like(v) for k, v in live.items()}
        p = {k: v.data_ptr() for k, v in live.items()}

        def restore():
            with torch.cuda.stream(stream):
                for k in live:
                    live[k].copy_(kept[k])

        def keep():
            with torch.cuda.stream(stream):
                for k in live:
                    kept[k].copy_(live[k])
            stream.synchronize()

        def indices():
            stream.synchronize()
            return live["it"].cpu().numpy().view(np.uint32).astype(np.int64)

        for road in ("F64", "PT"):
            pt = road == "PT"
            fresh, fk = kernel_ms(lib, lambda: lib.fr_escape_rows_de_device(C.byref(cfg), 3 if pt else 0, plo if pt else None, 0, h, p["z"],
                                                                            p["it"], p["der"], s), args.reps)
            fresh_ms = statistics.median(fresh)
            final = indices()
            total = int(np.where(final < m_cap, final + 1, m_cap).sum())
            if pt:
                st, sk = kernel_ms(lib, lambda: lib.fr_escape_rows_de_pt_state_device(C.byref(cfg), plo, None, 0, h, p["z"], p["it"], p["dz"],
                                                                                      p["m"], p["der"], s), args.reps)
                st_ms = statistics.median(st)
                lines.append(json.dumps({"view": vname, "road": road, "width": cfg.width, "height": h, "iterations": m_cap,
                                         "pixel_iterations": total, "de_kernel": fk, "de_ms_median": round(fresh_ms, 4),
                                         "de_ms_all": [round(t, 4) for t in fresh], "state_kernel": sk, "state_ms_median": round(st_ms, 4),
                                         "state_ms_all": [round(t, 4) for t in st], "state_over_de": round(st_ms / fresh_ms, 3)}))
            for n_cap in (m_cap // 2, m_cap * 9 // 10):
                cfg_n = at_cap(cfg, n_cap)
                if pt:
                    _native.check(lib.fr_escape_rows_de_pt_state_device(C.byref(cfg_n), plo, None, 0, h, p["z"], p["it"], p["dz"], p["m"],
                                                                        p["der"], s))
                    call = lambda: lib.fr_escape_extend_de_pt_device(C.byref(cfg), plo, None, 0, h, n_cap, p["z"], p["it"], p["dz"],  # noqa: E731
                                                                     p["m"], p["der"], s)
                else:
                    _native.check(lib.fr_escape_rows_de_device(C.byref(cfg_n), 0, None, 0, h, p["z"], p["it"], p["der"], s))
                    call = lambda: lib.fr_escape_extend_de_device(C.byref(cfg), 0, 0, h, n_cap, p["z"], p["it"], p["der"], s)  # noqa: E731
                running = int((indices() == n_cap).sum())
                keep()
                ext, ek = kernel_ms(lib, call, args.reps, before=restore)
                ext_ms = statistics.median(ext)
                after = indices()
                assert np.array_equal(after, final), "the extended escape indices are not the fresh render's"
                steps = int((np.where(after < m_cap, after + 1, m_cap) - n_cap)[after >= n_cap].sum())
                lines.append(json.dumps({"view": vname, "road": road, "from": n_cap, "to": m_cap, "pixels": n, "running": running,
                                         "running_share": round(running / n, 4), "extension_pixel_iterations": steps,
                                         "share_of_fresh_pixel_iterations": round(steps / total, 4), "extend_kernel": ek,
                                         "extend_ms_median": round(ext_ms, 4), "extend_ms_all": [round(t, 4) for t in ext],
                                         "fresh_de_ms_median": round(fresh_ms, 4), "extend_over_fresh": round(ext_ms / fresh_ms, 3)}))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
