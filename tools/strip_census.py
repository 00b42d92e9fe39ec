#!/usr/bin/env python3
"""Census of a view's 8x8 tiles and a model of the strip kernel's loop policy, from the CPU oracle alone (no GPU).

Prices an idea for escape_strip_kernel before any asm is written.  For a Config (default: C2, Mandelbrot 16384^2, default
view, cap 1024, f64) it prints

  * the census: interior (all 64 lanes reach the cap) / exterior (none does) / boundary (mixed) tiles, their
    wave-iterations (sum over tiles of the longest lane), idle lane-iterations, and how many exterior tiles are done within
    k iterations;
  * the loop model: vector instructions the four-iteration scaled loop with speculative blocks (fr_kernels.hip: FR_SC_ASM
    with FR_SC_SPEC_BODY) issues per tile class under a block policy (quiet stretch, longest block, regrowth after a
    rollback), for each --maxlen given.  Costs are read off the compiled ISA: a block of four 26, a checked iteration 8
    (+1 per distinct escape index recorded), a speculative block of L iterations 6 L + 2, four moves when a block ends or
    is thrown away in the second register set.  The one approximation: a lane is taken to pass T `--lag` iterations before
    it escapes (4; 3 moves the totals by a per mille).

Usage: python tools/strip_census.py [--edge 16384] [--cap 1024] [--maxlen 16 64 128 1024] [--quiet 16] [--regrow]
       [--lag 4] [--pos RE IM] [--scale S]       (C2 at full size: ten minutes on 16 cores)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402

M = 16  # FR_SPEC_M: the shortest speculative block


def interior_cost(cap, quiet, maxlen):
    """Vector instructions of a tile whose lanes all reach the cap (no rollback ever)."""
    c, si = 2, 0
    while si < min(quiet, cap) or cap - si < M:
        if si >= cap:
            return c
        c += 26
        si += 4
    length, blocks = M, 0
    while cap - si >= M:
        while length > cap - si:
            length //= 2
        c += 6 * length + 2
        si += length
        blocks += 1
        length = min(2 * length, maxlen)
    if blocks % 2 == 1:
        c += 4  # the state ends in the second register set
    while si < cap:
        c += 26
        si += 4
    return c


def simulate(n, cap, quiet, maxlen, regrow, lag):
    """n: (tiles, 64) executed iterations per lane -> (vector instructions of the loop, of them thrown away) per tile."""
    tiles = n.shape[0]
    pT = np.where(n >= cap, 1 << 30, np.maximum(n - lag, 0)).astype(np.int32)  # iteration at which the lane passes T
    si = np.zeros(tiles, np.int32)
    specq = np.full(tiles, quiet, np.int64)
    sspec = np.full(tiles, min(quiet, cap), np.int32)
    mode = np.zeros(tiles, np.int8)  # 0 blocks of four, 1 checked iterations, 2 speculative blocks
    par = np.zeros(tiles, np.int8)   # which register set holds the state
    length = np.full(tiles, M, np.int32)
    lcap = np.full(tiles, maxlen, np.int32)
    cost = np.full(tiles, 2, np.int64)
    waste = np.zeros(tiles, np.int64)
    mode[(pT <= 0).any(1)] = 1
    act = np.arange(tiles)
    while act.size:
        a = act
        nn, pp = n[a], pT[a]
        live = nn > si[a][:, None]
        md = mode[a]
        done = np.zeros(a.size, bool)

        def mark(sel, flags):
            tmp = np.zeros(a.size, bool)
            tmp[sel] = flags
            return tmp

        f = md == 0
        if f.any():
            ia, lv = a[f], live[f]
            s4 = si[ia] + 4
            ex = (lv & (pp[f] <= s4[:, None])).any(1)  # a lane above T at the block's end
            cost[ia] += 26
            ie = ia[ex]
            d = np.zeros(ia.size, bool)
            if ie.size:
                nne, s4e = nn[f][ex], s4[ex]
                rec = (lv[ex] & (nne <= s4e[:, None])).any(1)
                cost[ie] += 1 + rec
                si[ie] = s4e
                sspec[ie] = np.minimum(cap, s4e + specq[ie]).astype(np.int32)
                mode[ie] = 1
                d[ex] = ~(nne > s4e[:, None]).any(1) | (s4e >= cap)
            io = ia[~ex]
            if io.size:
                s4o = s4[~ex]
                si[io] = s4o
                cont = s4o < sspec[io]
                fin = ~cont & (s4o >= cap)
                sp = ~cont & ~fin & (cap - s4o >= M)
                rest = ~cont & ~fin & ~sp
                mode[io[sp]] = 2
                length[io[sp]] = M  # every entry from the checked code starts at M
                sspec[io[rest]] = cap
                d[~ex] = fin
            done |= mark(f, d)
        f = md == 1
        if f.any():
            ia, lv, nnf = a[f], live[f], nn[f]
            s0 = si[ia]
            s4 = s0 + 4
            inblk = lv & (nnf <= s4[:, None])
            rec = np.zeros(ia.size, np.int64)
            for k in range(1, 5):
                rec += (inblk & (nnf == (s0 + k)[:, None])).any(1)
            still = (nnf > s4[:, None]).any(1)
            lastn = np.where(lv, nnf, 0).max(1)
            cost[ia] += 8 * np.where(still, 4, np.clip(lastn - s0, 1, 4)) + rec
            si[ia] = s4
            dn = ~still | (s4 >= cap)
            cost[ia[~dn]] += 1
            again = ~dn & ((nnf > s4[:, None]) & (pT[ia] <= s4[:, None])).any(1)
            it = ia[~dn & ~again]
            sspec[it] = np.minimum(cap, s4[~dn & ~again] + specq[it]).astype(np.int32)
            mode[it] = 0
            done |= mark(f, dn)
        f = md == 2
        if f.any():
            ia, lv = a[f], live[f]
            s0 = si[ia]
            ln = np.minimum(length[ia], lcap[ia])
            while (ln > cap - s0).any():
                ln = np.where(ln > cap - s0, ln // 2, ln)
            s1 = s0 + ln
            fail = (lv & (pp[f] <= s1[:, None])).any(1)
            c = 6 * ln.astype(np.int64) + 2
            cost[ia] += c
            ifl = ia[fail]
            if ifl.size:
                waste[ifl] += c[fail]
                cost[ifl] += 4 * (par[ifl] == 1)
                specq[ifl] = np.minimum(specq[ifl] * 2, 32768)
                sspec[ifl] = np.minimum(cap, s0[fail] + specq[ifl]).astype(np.int32)
                mode[ifl] = 0
                par[ifl] = 0
                if not regrow:
                    lcap[ifl] = M
            iok = ia[~fail]
            d = np.zeros(ia.size, bool)
            if iok.size:
                s1o = s1[~fail]
                si[iok] = s1o
                length[iok] = np.minimum(2 * ln[~fail], lcap[iok])
                p_after = 1 - par[iok]
                out = (cap - s1o) < M
                io = iok[out]
                cost[io] += 4 * (p_after[out] == 1)
                sspec[io] = cap
                mode[io] = 0
                par[io] = 0
                par[iok[~out]] = p_after[~out]
                d[~fail] = out & (s1o >= cap)
            done |= mark(f, d)
        act = a[~done]
    return cost, waste


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--edge", type=int, default=16384)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--maxlen", type=int, nargs="*", default=[16, 64, 128, 1024])
    ap.add_argument("--quiet", type=int, default=16)
    ap.add_argument("--regrow", action="store_true", help="a tile that threw a block away may grow its blocks again")
    ap.add_argument("--lag", type=int, default=4)
    ap.add_argument("--pos", type=float, nargs=2, default=None)
    ap.add_argument("--scale", type=float, default=None)
    ap.add_argument("--band", type=int, default=256)
    args = ap.parse_args()
    edge, cap = args.edge, args.cap
    assert edge % 8 == 0 and args.band % 8 == 0
    kw = {}
    if args.pos:
        kw["pos"] = tuple(args.pos)
    if args.scale:
        kw["scale"] = (args.scale, args.scale)
    cfg = O.cli_config(edge, edge, iterations=cap, **kw)
    cls = ("interior", "exterior", "boundary")
    tiles = dict.fromkeys(cls, 0)
    wave_it = dict.fromkeys(cls, 0)
    lane_it = 0
    ext_hist = np.zeros(cap + 1, np.int64)
    model = {ml: dict(exterior=0, boundary=0, exterior_waste=0, boundary_waste=0) for ml in args.maxlen}
    t0 = time.time()
    for y0 in range(0, edge, args.band):
        y1 = min(edge, y0 + args.band)
        _, it = O.escape_rows(cfg, O.F64, y0, y1, 0)
        n = np.where(it < cap, it + 1, cap).astype(np.int32)
        t = n.reshape((y1 - y0) // 8, 8, edge // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
        mx, mn = t.max(1), t.min(1)
        sel = dict(interior=mn >= cap, exterior=mx < cap)
        sel["boundary"] = ~sel["interior"] & ~sel["exterior"]
        for k in cls:
            tiles[k] += int(sel[k].sum())
            wave_it[k] += int(mx[sel[k]].sum(dtype=np.int64))
        lane_it += int(t.sum(dtype=np.int64))
        ext_hist += np.bincount(mx[sel["exterior"]], minlength=cap + 1)
        ragged = t[~sel["interior"]]
        is_b = sel["boundary"][~sel["interior"]]
        for ml in args.maxlen:
            c, w = simulate(ragged, cap, args.quiet, ml, args.regrow, args.lag)
            r = model[ml]
            r["exterior"] += int(c[~is_b].sum())
            r["boundary"] += int(c[is_b].sum())
            r["exterior_waste"] += int(w[~is_b].sum())
            r["boundary_waste"] += int(w[is_b].sum())
        print("rows %d / %d  (%.0f s)" % (y1, edge, time.time() - t0), file=sys.stderr, flush=True)
    total_tiles, total_wave = sum(tiles.values()), sum(wave_it.values())
    print("# tools/strip_census.py: %d x %d, cap %d, f64, pos %s scale %s" % (edge, edge, cap, args.pos or "default", args.scale or "default"))
    print("executed pixel-iterations %d; idle lane-iterations %d (%.2f %% of 64 x wave-iterations)" % (
        lane_it, 64 * total_wave - lane_it, 100.0 * (1.0 - lane_it / (64.0 * total_wave))))
    print("%-10s %10s %18s %7s" % ("8x8 tiles", "count", "wave-iterations", "share"))
    for k in cls:
        print("%-10s %10d %18d %6.1f %%" % (k, tiles[k], wave_it[k], 100.0 * wave_it[k] / total_wave))
    cum = np.cumsum(ext_hist)
    print("exterior tiles finished within k iterations: " + ", ".join("%d: %d" % (k, cum[min(k, cap)]) for k in (4, 8, 16, 32, 64, 128, 256)))
    print("floor: 6.125 vector instructions x lane-iterations / 64 = %.4e" % (6.125 * lane_it / 64.0))
    print("# loop model: quiet %d, lag %d, %s" % (args.quiet, args.lag, "blocks regrow after a rollback" if args.regrow else "blocks of 16 for good after a tile's first rollback"))
    print("%-7s %14s %12s %12s %12s %12s %12s %12s" % ("maxlen", "interior/tile", "interior", "exterior", "boundary", "ext wasted", "bnd wasted", "LOOP TOTAL"))
    base = None
    for ml in args.maxlen:
        ic, r = interior_cost(cap, args.quiet, ml), model[ml]
        total = ic * tiles["interior"] + r["exterior"] + r["boundary"]
        base = total if base is None else base
        print("%-7d %14d %12.4e %12.4e %12.4e %12.4e %12.4e %12.4e  (%+.4e vs maxlen %d)" % (
            ml, ic, ic * tiles["interior"], r["exterior"], r["boundary"], r["exterior_waste"], r["boundary_waste"], total, total - base, args.maxlen[0]))
    print("(%d tiles in all; what the kernel issues outside the loops is not modelled: measured total minus LOOP TOTAL)" % total_tiles)


if __name__ == "__main__":
    main()
