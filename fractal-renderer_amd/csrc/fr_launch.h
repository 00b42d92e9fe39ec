/*
 * fr_launch.h — the launchers that cross translation units: fr_dispatch.hip (host only) calls these, each defined beside
 * its kernels in fr_kernels.hip.  Plain functions; precision: 1 = f32, otherwise f64 (as fr_launch_escape).
 * It also carries the one predicate both sides evaluate, fr_first_pass_speculates: the launcher picks the instantiation by
 * it and the dispatch picks the name fr_last_kernel_name reports by it, and the two must agree.
 */
#ifndef FR_LAUNCH_H
#define FR_LAUNCH_H

#include "fr_kernels.h"

/* the strip renderers.  tile = 6401 / 3202 / 1604 / 808 (the 4-wave kernel's tile shape); strip_tiles = 1 / 2 / 4 / 7 */
hipError_t fr_launch_tile(const fr_kparams &p, int precision, int mode, int tile, const fr_kout &out, hipStream_t stream);
hipError_t fr_launch_strips(const fr_kparams &p, int precision, int mode, int strip_tiles, const fr_kout &out, hipStream_t stream);
hipError_t fr_launch_refill(const fr_kparams &p, int precision, int mode, const fr_kout &out, hipStream_t stream);

/* the two-pass render's first pass.  v1: round 2's first pass (comparison only) */
hipError_t fr_launch_first_pass(const fr_kparams &p, int precision, bool v1, const fr_kout &out, hipStream_t stream);

/* the persistent-wave kernels.  src 0: the work queue over the image; 1: the second pass over the survivor lists.  RGB output only; needs
 * p.work_counter (zeroed on the launch stream by the caller) */
hipError_t fr_launch_queue(const fr_kparams &p, int precision, int src, const fr_kout &out, hipStream_t stream);

/* the first-pass kernel's form: later episodes in speculative blocks where the plan allows them, unless this is the two-pass
 * render (tiles hand their stragglers over) of a view whose statistics say that nothing stays */
inline bool fr_first_pass_speculates(const fr_kparams &p) {
    return p.loop_mode == 4 && p.loop_spec != 0 && !(p.first_no_spec && !p.first_only);
}

#endif
