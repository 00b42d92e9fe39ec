/*
 * fr_dispatch.hip — host only: which kernel a render gets.  fr_launch_escape and its launch_precision (the selector
 * semantics documented at fr_set_tile, include/fractal_hip.h), the kernel-name strings fr_last_kernel_name reports,
 * run_two_pass, fr_wants_work_queue, fr_wants_two_pass, fr_two_pass_bytes.  Includes fr_launch.h: the kernels' launchers
 * live beside their kernels, in fr_kernels.hip.
 */
#include "fr_kernels.h"

#include <cmath>

#include "fr_launch.h"

namespace {

#define FR_KNAME(base, k) (precision == 1 ? base "<float, " k ">" : base "<double, " k ">")

const char *first_pass_name(const fr_kparams &p, int precision) {
    /* which form of the first pass runs (fr_kernels.hip: launch_first_pass): the one whose later episodes may speculate, or the plain one */
    const bool spec = fr_first_pass_speculates(p);
#define FR_FIRST_NAMES(SUFFIX)                                                                                                       \
    (p.strip_tiles == 4                                                                                                              \
         ? (p.first_only ? FR_KNAME("escape_first_kernel", "4-tile strips in episodes, every tile finished in place" SUFFIX)         \
                         : FR_KNAME("escape_first_kernel + escape_second_kernel",                                                    \
                                    "4-tile strips, then persistent waves over the survivor lists" SUFFIX))                          \
         : (p.first_only ? FR_KNAME("escape_first_kernel", "7-tile strips in episodes, every tile finished in place" SUFFIX)         \
                         : FR_KNAME("escape_first_kernel + escape_second_kernel",                                                    \
                                    "7-tile strips, then persistent waves over the survivor lists" SUFFIX)))
    return spec ? FR_FIRST_NAMES("; speculative blocks in the later episodes") : FR_FIRST_NAMES("");
#undef FR_FIRST_NAMES
}

/* are the two-pass kernels available to this launch? */
bool two_pass_ready(const fr_kparams &p, int mode) {
    return mode == FR_OUT_RGB && p.first_cap != 0 && (p.first_only || (p.surv_counts && p.work_counter));
}

/* Two passes under selector `tile` — 12: round 2's first pass, 14: round 2's second pass (the host set p.second_v1), any
 * other: this round's kernels.  RGB output only; needs the survivor lists and p.work_counter (all counters zeroed on the
 * launch stream by the caller) and 0 < p.first_cap < p.iterations: two_pass_ready.  p.strip_tiles = 4: the first pass in
 * 4-tile strips (GUI-sized launches: four times as many workgroups to balance over the chip), else 7. */
hipError_t run_two_pass(const fr_kparams &p, int precision, int tile, const fr_kout &out, hipStream_t stream, const char *&name) {
    name = tile == 12   ? FR_KNAME("escape_first_v1_kernel + escape_queue_kernel", "round 2's first pass, then persistent waves over the survivor lists")
           : tile == 14 ? FR_KNAME("escape_first_kernel + escape_queue_kernel", "7-tile strips, then round 2's persistent waves over the survivor lists")
                        : first_pass_name(p, precision);
    if (p.ncols == 0 || p.nrows == 0) return hipSuccess;
    const hipError_t e = fr_launch_first_pass(p, precision, tile == 12, out, stream);
    if (e != hipSuccess) return e;
    if (p.first_only) return hipSuccess; /* nothing was handed over: there are no lists */
    if (p.debug_ablate & 2u) return hipSuccess; /* measurement aid: the first pass's cost on its own */
    return fr_launch_queue(p, precision, 1, out, stream);
}

/* The strip kernel in strips of the longest length of 7 / 4 / 2 / 1 tiles that `k_len` reaches: the one ladder of the
 * default dispatch (k_len from the view's statistics or the launch size) and of the selectors 1, 2, 4 and 8 (= 7 tiles). */
hipError_t run_strips(const fr_kparams &p, int precision, int mode, uint32_t k_len, const fr_kout &out, hipStream_t stream,
                      const char *&name) {
    const int k = k_len >= 7u ? 7 : k_len >= 4u ? 4 : k_len >= 2u ? 2 : 1;
    name = k == 7   ? FR_KNAME("escape_strip_kernel", "7 tiles")
           : k == 4 ? FR_KNAME("escape_strip_kernel", "4 tiles")
           : k == 2 ? FR_KNAME("escape_strip_kernel", "2 tiles")
                    : FR_KNAME("escape_strip_kernel", "1 tile");
    return fr_launch_strips(p, precision, mode, k, out, stream);
}

hipError_t run_refill(const fr_kparams &p, int precision, int mode, const fr_kout &out, hipStream_t stream, const char *&name) {
    name = FR_KNAME("escape_refill_kernel", "7x2-tile patches");
    return fr_launch_refill(p, precision, mode, out, stream);
}

/* what the selectors 9, 10, 11, 14 and 15 fall back to: refilling strips; only the escape-time algorithms have orbits to
 * refill, the others get 7-tile strips */
hipError_t run_refill_or_strips(const fr_kparams &p, int precision, int mode, const fr_kout &out, hipStream_t stream,
                                const char *&name) {
    if (p.algo != 0 && p.algo != 2) return run_strips(p, precision, mode, 7u, out, stream, name);
    return run_refill(p, precision, mode, out, stream, name);
}

hipError_t launch_precision(const fr_kparams &p, int precision, int mode, const fr_kout &out, int tile, hipStream_t stream,
                            const char *&name) {
    if (p.out_in_place && tile > 16) tile = 0; /* only the strip kernels know in-place addressing */
    switch (tile) {
    case 6401:
    case 3202:
    case 1604:
    case 808:
        name = tile == 6401   ? FR_KNAME("escape_kernel", "64x1")
               : tile == 3202 ? FR_KNAME("escape_kernel", "32x2")
               : tile == 1604 ? FR_KNAME("escape_kernel", "16x4")
                              : FR_KNAME("escape_kernel", "8x8");
        return fr_launch_tile(p, precision, mode, tile, out, stream);
    case 0: {
        /* strip length by image size: long strips amortise the per-workgroup setup, short ones
         * keep every SIMD supplied with several waves when the image is small (GUI frames) */
        const uint64_t tiles = (((uint64_t)p.ncols + 7) / 8) * (((uint64_t)p.nrows + 7) / 8);
        /* Julia views are mostly short orbits with a heavy tail: two passes (see escape_first_kernel; the
         * host asks for it from 65 536 tiles up: fr_wants_two_pass) */
        if (two_pass_ready(p, mode)) return run_two_pass(p, precision, 0, out, stream, name);
        /* patch refill: behind the periodicity shortcut, and for the COUNT / ESCAPE outputs of Julia images
         * (RGB renders of Julia images this large take the two-pass kernels above) */
        if (tiles >= 262144 && ((p.algo == 2 && mode != FR_OUT_RGB) || p.cycle_shortcut)) return run_refill(p, precision, mode, out, stream, name);
        /* p.strip_tiles: the length the view's own statistics call for (fr_api.hip: choose_kernel); else by launch size */
        /* By size (round 4, tools/strip_length_study.py -> profiles/r04_strip_length_by_size.txt): ONE tile per workgroup up to
         * 4096^2 — below that a launch has too few workgroups for longer strips to fill and balance the chip's 8192 wave
         * slots (1920 x 1080, default view, f64: 0.122 ms against 0.158 / 0.244 / 0.294 for 2 / 4 / 7 tiles; still 13-23 %
         * at 4096^2) — and the longest strips from 8192 x 4096 up, where the per-workgroup costs they amortise are what is
         * left (8192^2: 7 tiles best on six views of eight).  Views of very short orbits prefer long strips at every size;
         * the view's statistics say so from the second frame on (strip_tiles). */
        const uint32_t k_len = (mode == FR_OUT_RGB && p.strip_tiles) ? p.strip_tiles : tiles >= 524288 ? 7u : 1u;
        return run_strips(p, precision, mode, k_len, out, stream, name);
    }
    case 1:
    case 2:
    case 4:
    case 8: /* 7 tiles */
        return run_strips(p, precision, mode, (uint32_t)tile, out, stream, name);
    case 13: /* the first pass alone: no tile is handed over, no lists, no second kernel */
    case 16: /* ... in 4-tile strips */
    case 12: /* two passes with round 2's first pass (comparison only) */
    case 14: /* two passes with round 2's second-pass kernel (comparison only) */
    case 15: /* two passes, the first in 4-tile strips */
    case 11: /* two passes: strips to first_cap, then persistent waves over the survivors (otherwise as 9) */
        if (two_pass_ready(p, mode)) return run_two_pass(p, precision, tile, out, stream, name);
        return run_refill_or_strips(p, precision, mode, out, stream, name);
    case 10: /* the work-queue kernel (RGB output of an escape-time algorithm; otherwise as 9) */
        if (mode == FR_OUT_RGB && p.work_counter && fr_wants_work_queue(p, 10)) {
            name = FR_KNAME("escape_queue_kernel", "persistent waves, 64x32-px patches");
            return fr_launch_queue(p, precision, 0, out, stream);
        }
        [[fallthrough]];
    case 9: /* refilling strips */
        return run_refill_or_strips(p, precision, mode, out, stream, name);
    default:
        return hipErrorInvalidValue;
    }
}

} /* namespace */

hipError_t fr_launch_escape(const fr_kparams &p, int precision, int mode, const fr_kout &out, int tile,
                            hipStream_t stream, const char **kernel_name) {
    const char *name = "";
    const hipError_t e = launch_precision(p, precision, mode, out, tile, stream, name);
    if (kernel_name) *kernel_name = name;
    return e;
}

bool fr_wants_work_queue(const fr_kparams &p, int tile) {
    if (p.cycle_shortcut || (p.algo != 0 && p.algo != 2)) return false;
    /* its main loop is the scaled form in blocks of loop_mode iterations, counted in an f32 */
    if (p.loop_mode == 0 || p.iterations >= (1u << 24)) return false;
    /* only on request: over a whole image (BASELINE C4) it runs 3.5 ms (f32) / 4.9 ms (f64) against the patch-refill
     * kernel's 3.1 / 4.5; the default for large Julia images is the two-pass render, whose second pass this kernel
     * is (fr_wants_two_pass) */
    return tile == 10;
}

bool fr_wants_two_pass(fr_kparams &p, int precision, int tile, int hint) {
    p.first_cap = 0;
    p.first_only = 0;
    if (p.cycle_shortcut || (p.algo != 0 && p.algo != 2)) return false;
    if (p.loop_mode == 0 || p.iterations >= (1u << 24)) return false; /* as for the work-queue kernel */
    if (p.ncols == 0 || p.nrows == 0 || (uint64_t)p.ncols * p.nrows > 0xFFF00000ull) return false;
    if (p.algo == 2 && tile == 0) {
        /* a Julia constant the scaled loop may not run with (a component that is zero, tiny or huge — the dendrite c = i):
         * the first pass would take its plain-loop fallback on every strip; the strip kernel is the better plain loop */
        const double lo = precision == 1 ? 0x1p-30 : 0x1p-300, hi = precision == 1 ? 0x1p30 : 0x1p400;
        const double jr = precision == 1 ? std::fabs((double)(float)p.julia_re) : std::fabs(p.julia_re);
        const double ji = precision == 1 ? std::fabs((double)(float)p.julia_im) : std::fabs(p.julia_im);
        if (!(jr >= lo && jr <= hi && ji >= lo && ji <= hi)) return false;
    }
    if (tile == 0) {
        /* the default dispatch: Julia images from 2048^2 up.  Measured (tools/two_pass_sizes.py, C4's view, f32 /
         * f64, against the strips the default would otherwise pick): 65 536 tiles 0.17 / 0.21 ms against 0.18 / 0.30,
         * 131 072 tiles 0.17 / 0.22 against 0.20 / 0.33; at 32 768 tiles and below the strips win in f32 */
        const uint64_t tiles = (((uint64_t)p.ncols + 7) / 8) * (((uint64_t)p.nrows + 7) / 8);
        if (tiles < 262144 && hint < 1) return false; /* (a MEASURED view may ask for them from 4096 tiles up) */
        if (tiles < 4096) return false;
        /* which of the two suits the IMAGE is measured where that pays (hint: 1 two passes, 0 strips — fr_api.hip:
         * choose_kernel); without a measurement, by the algorithm: Julia views are mostly short orbits with a heavy tail */
        if (hint == 0 || (hint < 0 && p.algo != 2)) return false;
        /* ... and only where a tail can be long: under a cap of 512 the lists have nothing to save (a 256-iteration dust at
         * 2048^2: 0.055 ms in two passes, 0.039 in strips; profiles/r03_kernel_choice_views.txt, mid-size section) */
        if (hint < 0 && p.iterations < 512u) return false;
        p.first_only = hint == 2 ? 1u : 0u;
    } else if (tile == 13 || tile == 16) {
        p.first_only = 1u;
    } else if (tile != 11 && tile != 12 && tile != 14 && tile != 15) {
        return false;
    }
    if (tile == 15 || tile == 16) p.strip_tiles = 4u;
    /* first_cap: a multiple of the loop's block length; the second pass must have something left to do */
    uint32_t k1 = p.two_pass_cap ? p.two_pass_cap : 64u; /* measured on C4: 64 / 48 (tools/sweep_two_pass.py) */
    k1 = (k1 + 3u) & ~3u;
    if (k1 + 8u > p.iterations) return false;
    p.first_cap = k1;
    if (p.first_keep == 0 || p.first_keep > 64) p.first_keep = 48;
    return true;
}

fr_two_pass_layout fr_two_pass_bytes(const fr_kparams &p, int precision, uint32_t sub_capacity) {
    const size_t entries = (size_t)sub_capacity * FR_SURV_QUEUES;
    const size_t pair = precision == 1 ? 8 : 16;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    fr_two_pass_layout l{};
    l.z_off = 0;
    l.pos_off = up(entries * pair);
    l.cnt_off = l.pos_off + up(entries * 8);
    l.c_off = l.cnt_off + up(entries * 4);
    l.counts_off = l.c_off + (p.algo == 2 ? 0 : up(entries * pair));
    l.total = l.counts_off + FR_SURV_QUEUES * FR_SURV_COUNT_STRIDE * sizeof(uint32_t);
    return l;
}

