/*
 * fr_de.hip — distance estimation (include/fractal_hip.h, "DE"): the orbit's derivative carried beside the escape loop on the
 * F64 road and on PT (dd or wide centre), the exterior distance estimate b = |z| ln|z| / |z'| in pixels, and the colour map
 * with distance shading.  tests/de_model.c restates all of it; tests/test_gpu_de.py compares the two bit for bit.
 * RESUMABLE DE (include/fractal_hip.h): the same derivative kept as state, so that a DE view's cap is raised in place;
 * tests/de_state_model.c restates it and tests/test_gpu_de_extend.py compares the two bit for bit.
 *
 * Every operation of the definition is one correctly rounded f64 operation (the build has -ffp-contract=off; fma only where
 * the definition says fma), so the derivative, overflow to inf and NaN included, is the same on every conforming machine.
 *
 * Kernels, one lane per pixel, 256-lane workgroups (cdna_hip_programming: LDS for what a workgroup shares):
 *   escape_de_kernel<JULIA>     the F64 road: recursive() (calc/src/lib.rs:245-257) as written, 9 f64 operations a step, plus
 *                               2 adds, 1 multiply and 3 fma for d' = 2 z d + b0.  The deep kernels' workgroup (fr_kernels.h:
 *                               kDeep*, fr_deep_grid): 16 x 16 pixels, the 16 column and 16 row coordinates computed once by
 *                               32 lanes and staged in LDS.  A lane that escapes leaves EXEC and the wave ends its loop when
 *                               its last lane has.  64-bit output offsets.
 *   escape_pt_de_kernel<JULIA>  PT's loop as fr_pt.hip's orbit_pt states it — same operations, same rebases, the load of
 *                               X_{m+2} issued a step ahead — with d beside it, from the z the loop holds.  The orbits are the
 *                               context's (fr_ctx.h: pt_orbit_view): a dd and a wide centre differ only there.
 *   escape_extend_de_kernel<JULIA>     RESUMABLE DE on the F64 road: escape_de_kernel's step continued in place from the stored
 *                               (z, der) of the pixels whose iters is the old cap, c staged as the render stages it.
 *   escape_pt_de_state_kernel<JULIA>   escape_pt_de_kernel with RESUMABLE PT's rebase rule, storing (z, iters, dz, m, der);
 *   escape_extend_pt_de_kernel<JULIA>  continues that state in place on the orbits of the new cap.  Both run orbit_pt_de_state,
 *                               the one copy of the state step with the derivative.  The two extend kernels read iters first and
 *                               a workgroup with no pixel at the old cap ends before it stages or loads anything.
 *   ss_refine_de_f64_kernel<JULIA>, ss_refine_de_pt_kernel<JULIA>   ADAPTIVE SUPERSAMPLED DE's refine pass (fr_ss_adaptive_de.hip;
 *                               fr_ss_list.h: the claim loop): persistent waves run escape_de_kernel's loop / orbit_pt_de (the
 *                               one copy of escape_pt_de_kernel's loop) on the s x s samples of the listed edge pixels and
 *                               colour and shade each as colour_de_rows_kernel does (fr_ss_de_sample.h).
 *   distance_rows_kernel        (z, iters, der) -> D, one double per pixel; the log2 table in LDS.
 *   colour_de_rows_kernel       fr_colour.h's colour_of, the renders' own map, then the shading: every byte times
 *                               s = D / thickness where s < 1.  RGBA leaves as one dword, RGB as three bytes at any alignment.
 * No kernel here uses scratch (profiles/de_inner_loop_isa.txt, profiles/de_state_inner_loop_isa.txt).
 */
#include <cmath>
#include <memory>

#include "fr_ctx.h"
#include "fr_de.h"
#include "fr_math.h"
#include "fr_ss_list.h"
#include "fr_wide.h"

namespace {

#include "fr_colour.h"
#include "fr_de_shade.h" /* kHalfLn2, de_distance */
#include "fr_ss_de_sample.h" /* ss_de_sample_colour */

constexpr uint32_t kDeThreads = 64 * kDeepWaves;

/* the workgroup's 16 x 16 pixels: this lane's local column and row (fr_kernels.h: kDeep*) */
struct DeLane {
    uint32_t col0, row0, lx, ly, cx, r;
    bool valid;
};

__device__ __forceinline__ DeLane de_lane(const fr_kparams &p, uint32_t tid) {
    DeLane l;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kDeepBlockW - 1) / kDeepBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    l.col0 = bx * kDeepBlockW, l.row0 = by * kDeepBlockH;
    const uint32_t wave = tid >> 6, lane = tid & 63;
    l.lx = (wave % kDeepWavesX) * kDeepTileW + lane % kDeepTileW;
    l.ly = (wave / kDeepWavesX) * kDeepTileH + lane / kDeepTileW;
    l.cx = l.col0 + l.lx, l.r = l.row0 + l.ly;
    l.valid = l.cx < p.ncols && l.r < p.nrows;
    return l;
}

/* The 16 column and 16 row coordinates of the workgroup into LDS: coord_to_space (calc/src/lib.rs:181-197), and for PT
 * (`off`) without its final `+ pos` — DD's off.  The caller synchronises. */
template <bool OFF>
__device__ __forceinline__ void de_stage(const fr_kparams &p, uint32_t tid, uint32_t col0, uint32_t row0, double *s_re, double *s_im) {
    if (tid < kDeepBlockW + kDeepBlockH) {
        const double width = (double)p.width, height = (double)p.height;
        if (tid < kDeepBlockW) {
            const uint64_t x = (uint64_t)p.x_first + (uint64_t)(col0 + tid) * p.x_stride;
            const double v = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re;
            s_re[tid] = OFF ? v : v + p.pos_re;
        } else {
            const uint32_t r = row0 + (tid - kDeepBlockW);
            const uint64_t y = (uint64_t)p.y_first + (uint64_t)(r / p.block_rows) * p.y_stride + r % p.block_rows;
            const double v = (((double)y / height) - 0.5) / p.scale_im;
            s_im[tid - kDeepBlockW] = OFF ? v : v + p.pos_im;
        }
    }
}

__device__ __forceinline__ void de_store(const fr_kparams &p, const DeLane &l, double *z, uint32_t *iters, double *der, double zr,
                                         double zi, uint32_t it, double dr, double di) {
    const uint64_t k = (uint64_t)l.r * p.ncols + l.cx;
    z[2 * k] = zr;
    z[2 * k + 1] = zi;
    iters[k] = it;
    der[2 * k] = dr;
    der[2 * k + 1] = di;
}

/* ---- the F64 road ----------------------------------------------------------------------------------------------------- */

template <bool JULIA>
__global__ __launch_bounds__(kDeThreads) void escape_de_kernel(const fr_kparams p, double *__restrict__ z, uint32_t *__restrict__ iters,
                                                               double *__restrict__ der) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];
    const uint32_t tid = threadIdx.x;
    const DeLane l = de_lane(p, tid);
    de_stage<false>(p, tid, l.col0, l.row0, s_re, s_im);
    __syncthreads();
    if (!l.valid) return;
    const bool escape_algo = JULIA ? p.algo == 2 : p.algo == 0; /* the host picks JULIA from the algorithm */
    double re = 0.0, im = 0.0, dr = 0.0, di = 0.0; /* an algorithm without orbits writes zeros */
    uint32_t i = 0;
    if (escape_algo) {
        re = s_re[l.lx], im = s_im[l.ly];
        const double cre = JULIA ? p.julia_re : re, cim = JULIA ? p.julia_im : im; /* calc/src/lib.rs:209-210 */
        const double b0 = JULIA ? 0.0 : 1.0;
        const double squared = p.limit * p.limit; /* :246 */
        const uint32_t iterations = p.iterations;
        dr = 1.0;
        for (; i < iterations; i++) {
            const double tr = re + re, ti = im + im;
            const double nre = (re * re - im * im) + cre; /* square() + c, :87-91 */
            const double nim = tr * im + cim;             /* 2.0 * re is re + re, exactly */
            const double ndr = __builtin_fma(tr, dr, __builtin_fma(-ti, di, b0));
            const double ndi = __builtin_fma(tr, di, ti * dr);
            re = nre, im = nim, dr = ndr, di = ndi;
            if (nre * nre + nim * nim > squared) break; /* (next, i, nd); this lane leaves EXEC */
        }
    }
    de_store(p, l, z, iters, der, re, im, i, dr, di);
}

/* ---- PT (include/fractal_hip.h, fr_precision: PT; fr_pt.hip: orbit_pt) with d beside it ------------------------------------- */

/* escape_pt_de_kernel's pixel: PT's loop as orbit_pt states it with d beside it, from `off`.  Returns the escape index (or
 * `iterations`), leaves the final z in (zr, zi) and the derivative in (dr, di). */
template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_pt_de(uint32_t iterations, double off_re, double off_im, const double2 *__restrict__ x_orbit,
                                                const double2 *__restrict__ k_orbit, uint32_t x_last, uint32_t k_last, double squared,
                                                double &zr, double &zi, double &dr, double &di) {
    const double b0 = JULIA ? 0.0 : 1.0;
    const double2 *X = x_orbit;
    uint32_t last = x_last;
    uint32_t m = JULIA ? 0u : 1u;
    double dzr = off_re, dzi = off_im;
    const double dcr = JULIA ? 0.0 : off_re, dci = JULIA ? 0.0 : off_im;
    /* m <= last - 1 at the top of every step: X_{m+1} exists; the clamp is for a cap of 0, where R has two entries */
    double2 Z = X[m], N = X[min(m + 1u, last)];
    const double2 K1 = k_orbit[1];  /* the entry after a rebase; K_0 = R_0 = 0 */
    zr = Z.x + dzr, zi = Z.y + dzi;
    dr = 1.0, di = 0.0;
    uint32_t i = 0;
    for (; i < iterations; i++) {
        const double2 P = X[min(m + 2u, last)]; /* X_{m+2}: next step's X_{m+1} if it does not rebase */
        const double tr = Z.x + zr, ti = Z.y + zi;
        const double ur = zr + zr, ui = zi + zi; /* the derivative's t: from the z before the step */
        const double ndr = __builtin_fma(tr, dzr, __builtin_fma(-ti, dzi, dcr));
        const double ndi = __builtin_fma(tr, dzi, __builtin_fma(ti, dzr, dci));
        const double ner = __builtin_fma(ur, dr, __builtin_fma(-ui, di, b0));
        const double nei = __builtin_fma(ur, di, ui * dr);
        m++;
        zr = N.x + ndr;
        zi = N.y + ndi;
        dzr = ndr;
        dzi = ndi;
        dr = ner;
        di = nei;
        const double dist = zr * zr + zi * zi;
        if (dist > squared) break;
        if (dist < dzr * dzr + dzi * dzi || m == last) {
            dzr = zr;
            dzi = zi;
            m = 0;
            if (JULIA) {
                X = k_orbit;
                last = k_last;
            }
            Z = make_double2(0.0, 0.0);
            N = K1;
        } else {
            Z = N;
            N = P;
        }
    }
    return i;
}

template <bool JULIA>
__global__ __launch_bounds__(kDeThreads) void escape_pt_de_kernel(const fr_kparams p, double *__restrict__ z, uint32_t *__restrict__ iters,
                                                                  double *__restrict__ der, const double2 *__restrict__ x_orbit,
                                                                  const double2 *__restrict__ k_orbit, const uint32_t x_last,
                                                                  const uint32_t k_last) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];
    const uint32_t tid = threadIdx.x;
    const DeLane l = de_lane(p, tid);
    de_stage<true>(p, tid, l.col0, l.row0, s_re, s_im);
    __syncthreads();
    if (!l.valid) return;
    const bool escape_algo = JULIA ? p.algo == 2 : p.algo == 0;
    double zr = 0.0, zi = 0.0, dr = 0.0, di = 0.0;
    uint32_t i = 0;
    if (escape_algo)
        i = orbit_pt_de<JULIA>(p.iterations, s_re[l.lx], s_im[l.ly], x_orbit, k_orbit, x_last, k_last, p.limit * p.limit, zr, zi, dr, di);
    de_store(p, l, z, iters, der, zr, zi, i, dr, di);
}

/* ---- ADAPTIVE SUPERSAMPLED DE's refine pass (include/fractal_hip.h; fr_ss_list.h: the claim loop) ----------------------------- */

/* Persistent waves over the edge list of an adaptive DE render of cfg_s (`p` holds cfg_s).  The F64 road: each lane computes its
 * sample's c by coord_to_space on cfg_s — escape_de_kernel's de_stage operations on the same (x, y), hence the same bits — runs
 * escape_de_kernel's loop and colours and shades the sample as colour_de_rows_kernel does (fr_ss_de_sample.h).  The log2 table is
 * staged before the loop, which holds no barrier. */
template <bool JULIA, bool LINEAR>
__global__ __launch_bounds__(kSsRefineThreads) void ss_refine_de_f64_kernel(const fr_kparams p, const fr_ss_refine a,
                                                                            const fr_ss_de_shade sh) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    const double *gt = &g_log2_tab[0][0];
    for (uint32_t k = threadIdx.x; k < FR_LOG2_N * 3; k += kSsRefineThreads) s_tab[k] = gt[k];
    const uint16_t *const s_lt = ss_refine_tables<LINEAR>(); /* LINEAR-LIGHT SUPERSAMPLING: staged with the log2 table */
    __syncthreads();
    const double width = (double)p.width, height = (double)p.height;
    const double squared = p.limit * p.limit; /* :246 */
    const uint32_t iterations = p.iterations;
    ss_refine_loop<LINEAR>(a, s_lt, [&](uint64_t x, uint64_t y) {
        double re = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re + p.pos_re; /* de_stage<false> */
        double im = (((double)y / height) - 0.5) / p.scale_im + p.pos_im;
        const double cre = JULIA ? p.julia_re : re, cim = JULIA ? p.julia_im : im;
        const double b0 = JULIA ? 0.0 : 1.0;
        double dr = 1.0, di = 0.0;
        uint32_t i = 0;
        for (; i < iterations; i++) { /* escape_de_kernel's step */
            const double tr = re + re, ti = im + im;
            const double nre = (re * re - im * im) + cre;
            const double nim = tr * im + cim;
            const double ndr = __builtin_fma(tr, dr, __builtin_fma(-ti, di, b0));
            const double ndi = __builtin_fma(tr, di, ti * dr);
            re = nre, im = nim, dr = ndr, di = ndi;
            if (nre * nre + nim * nim > squared) break;
        }
        return ss_de_sample_colour(p, re, im, dr, di, i, sh.pixels, sh.thickness, s_tab);
    });
}

/* PT: `off` by de_stage<true>'s formula on cfg_s, then orbit_pt_de on the context's orbits */
template <bool JULIA, bool LINEAR>
__global__ __launch_bounds__(kSsRefineThreads) void ss_refine_de_pt_kernel(const fr_kparams p, const fr_ss_refine a, const fr_ss_de_shade sh,
                                                                           const double2 *__restrict__ x_orbit,
                                                                           const double2 *__restrict__ k_orbit, const uint32_t x_last,
                                                                           const uint32_t k_last) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    const double *gt = &g_log2_tab[0][0];
    for (uint32_t k = threadIdx.x; k < FR_LOG2_N * 3; k += kSsRefineThreads) s_tab[k] = gt[k];
    const uint16_t *const s_lt = ss_refine_tables<LINEAR>(); /* LINEAR-LIGHT SUPERSAMPLING: staged with the log2 table */
    __syncthreads();
    const double width = (double)p.width, height = (double)p.height;
    const double squared = p.limit * p.limit;
    ss_refine_loop<LINEAR>(a, s_lt, [&](uint64_t x, uint64_t y) {
        const double off_re = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re;
        const double off_im = (((double)y / height) - 0.5) / p.scale_im;
        double zr, zi, dr, di;
        const uint32_t it = orbit_pt_de<JULIA>(p.iterations, off_re, off_im, x_orbit, k_orbit, x_last, k_last, squared, zr, zi, dr, di);
        return ss_de_sample_colour(p, zr, zi, dr, di, it, sh.pixels, sh.thickness, s_tab);
    });
}

/* ---- RESUMABLE DE (include/fractal_hip.h): a DE view's cap raised in place ------------------------------------------------------ */

/* The F64 road.  Exhaustion stored (previous, N, d) and c is a function of the pixel, so the loop goes on from i = from.  `iters`
 * is read first; a workgroup with no pixel at `from` ends there (escape_extend_pt_kernel's early-out), and a finished pixel's z
 * and der are neither loaded nor stored.  The host launches it only for an escape-time algorithm and from < p.iterations. */
template <bool JULIA>
__global__ __launch_bounds__(kDeThreads) void escape_extend_de_kernel(const fr_kparams p, double *z, uint32_t *iters, double *der,
                                                                      const uint32_t from) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];
    const uint32_t tid = threadIdx.x;
    const DeLane l = de_lane(p, tid);
    const uint64_t k = (uint64_t)l.r * p.ncols + l.cx;
    uint32_t done = 0;
    if (l.valid) done = iters[k];
    const bool running = l.valid && done == from;
    if (!__syncthreads_or(running ? 1 : 0)) return; /* whole workgroup (uniform) */
    if (!JULIA) { /* c = the pixel's coordinate, staged as the render stages it; Julia's c is the constant */
        de_stage<false>(p, tid, l.col0, l.row0, s_re, s_im);
        __syncthreads();
    }
    if (!running) return;
    const double cre = JULIA ? p.julia_re : s_re[l.lx], cim = JULIA ? p.julia_im : s_im[l.ly];
    const double b0 = JULIA ? 0.0 : 1.0;
    const double squared = p.limit * p.limit;
    const uint32_t iterations = p.iterations;
    double re = z[2 * k], im = z[2 * k + 1], dr = der[2 * k], di = der[2 * k + 1];
    uint32_t i = from;
    for (; i < iterations; i++) { /* escape_de_kernel's step */
        const double tr = re + re, ti = im + im;
        const double nre = (re * re - im * im) + cre;
        const double nim = tr * im + cim;
        const double ndr = __builtin_fma(tr, dr, __builtin_fma(-ti, di, b0));
        const double ndi = __builtin_fma(tr, di, ti * dr);
        re = nre, im = nim, dr = ndr, di = ndi;
        if (nre * nre + nim * nim > squared) break;
    }
    de_store(p, l, z, iters, der, re, im, i, dr, di); /* i == iterations on exhaustion: the new cap */
}

/* PT.  A pixel's state between steps is RESUMABLE PT's (z, dz, m, onK; fr_pt.hip: orbit_pt_state) with the derivative d beside
 * it.  orbit_pt_de_state runs `steps` steps from it — escape_pt_de_kernel's operations with the state rule's rebase condition:
 * dist < |dz|^2, or m == last of an orbit ENDED BY ESCAPE (x_end / k_end: that last index, or ~0 for an orbit cut by the cap,
 * which m never equals) — and leaves the state after the last step in `s`; on escape that is (next, 0, 0, nd).  Returns the
 * steps completed before the escape (`steps`: none).  x_last / k_last only clamp the loads. */
struct PtDeState {
    double zr, zi, dzr, dzi, dr, di;
    uint32_t m;
    bool on_k;
};

constexpr uint32_t kDeOnK = 0x80000000u; /* bit 31 of the stored m: the pixel follows K (fr_pt.hip: kPtOnK) */

template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_pt_de_state(uint32_t steps, double dcr, double dci, const double2 *x_orbit,
                                                      const double2 *k_orbit, uint32_t x_last, uint32_t k_last, uint32_t x_end,
                                                      uint32_t k_end, double squared, PtDeState &s) {
    const bool on_k = JULIA && s.on_k;
    const double2 *X = on_k ? k_orbit : x_orbit;
    uint32_t last = on_k ? k_last : x_last, end = on_k ? k_end : x_end;
    uint32_t m = s.m;
    bool k_now = on_k;
    const double b0 = JULIA ? 0.0 : 1.0;
    double dzr = s.dzr, dzi = s.dzi, zr = s.zr, zi = s.zi, dr = s.dr, di = s.di;
    double2 Z = X[min(m, last)], N = X[min(m + 1u, last)]; /* m < last at the top of every step */
    const double2 K1 = k_orbit[1];                         /* the entry after a rebase; K_0 = R_0 = 0 */
    uint32_t i = 0;
    for (; i < steps; i++) {
        const double2 P = X[min(m + 2u, last)]; /* X_{m+2}: next step's X_{m+1} if it does not rebase */
        const double tr = Z.x + zr, ti = Z.y + zi;
        const double ur = zr + zr, ui = zi + zi; /* the derivative's t: from the z before the step */
        const double ndr = __builtin_fma(tr, dzr, __builtin_fma(-ti, dzi, dcr));
        const double ndi = __builtin_fma(tr, dzi, __builtin_fma(ti, dzr, dci));
        const double ner = __builtin_fma(ur, dr, __builtin_fma(-ui, di, b0));
        const double nei = __builtin_fma(ur, di, ui * dr);
        m++;
        zr = N.x + ndr;
        zi = N.y + ndi;
        dzr = ndr;
        dzi = ndi;
        dr = ner;
        di = nei;
        const double dist = zr * zr + zi * zi;
        if (dist > squared) break; /* this lane leaves EXEC; the wave goes on while any lane is left */
        if (dist < dzr * dzr + dzi * dzi || m == end) {
            dzr = zr;
            dzi = zi;
            m = 0;
            if (JULIA) {
                X = k_orbit;
                last = k_last;
                end = k_end;
                k_now = true;
            }
            Z = make_double2(0.0, 0.0);
            N = K1;
        } else {
            Z = N;
            N = P;
        }
    }
    const bool escaped = i < steps;
    s.zr = zr;
    s.zi = zi;
    s.dzr = escaped ? 0.0 : dzr;
    s.dzi = escaped ? 0.0 : dzi;
    s.dr = dr;
    s.di = di;
    s.m = escaped ? 0u : m;
    s.on_k = !escaped && k_now;
    return i;
}

__device__ __forceinline__ void de_state_store(uint64_t k, double *z, uint32_t *iters, double *dz, uint32_t *mm, double *der,
                                               const PtDeState &s, uint32_t it) {
    z[2 * k] = s.zr;
    z[2 * k + 1] = s.zi;
    iters[k] = it;
    dz[2 * k] = s.dzr;
    dz[2 * k + 1] = s.dzi;
    mm[k] = s.m | (s.on_k ? kDeOnK : 0u);
    der[2 * k] = s.dr;
    der[2 * k + 1] = s.di;
}

/* escape_pt_state_kernel's shape with the derivative: the whole state, 56 bytes per pixel.  `ended`: bit 0 = X, bit 1 = K is
 * ended by escape.  An algorithm without orbits writes zeros into all five arrays. */
template <bool JULIA>
__global__ __launch_bounds__(kDeThreads) void escape_pt_de_state_kernel(const fr_kparams p, double *__restrict__ z,
                                                                        uint32_t *__restrict__ iters, double *__restrict__ dz,
                                                                        uint32_t *__restrict__ mm, double *__restrict__ der,
                                                                        const double2 *__restrict__ x_orbit,
                                                                        const double2 *__restrict__ k_orbit, const uint32_t x_last,
                                                                        const uint32_t k_last, const uint32_t ended) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];
    const uint32_t tid = threadIdx.x;
    const DeLane l = de_lane(p, tid);
    de_stage<true>(p, tid, l.col0, l.row0, s_re, s_im);
    __syncthreads();
    if (!l.valid) return;
    const bool escape_algo = JULIA ? p.algo == 2 : p.algo == 0;
    PtDeState s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u, false};
    uint32_t it = 0;
    if (escape_algo) {
        const double off_re = s_re[l.lx], off_im = s_im[l.ly];
        s.m = JULIA ? 0u : 1u;
        s.dzr = off_re;
        s.dzi = off_im;
        const double2 X0 = x_orbit[min(s.m, x_last)];
        s.zr = X0.x + s.dzr;
        s.zi = X0.y + s.dzi;
        s.dr = 1.0;
        it = orbit_pt_de_state<JULIA>(p.iterations, JULIA ? 0.0 : off_re, JULIA ? 0.0 : off_im, x_orbit, k_orbit, x_last, k_last,
                                      (ended & 1u) ? x_last : ~0u, (ended & 2u) ? k_last : ~0u, p.limit * p.limit, s);
    }
    de_state_store((uint64_t)l.r * p.ncols + l.cx, z, iters, dz, mm, der, s, it);
}

/* escape_extend_pt_kernel's shape with the derivative: the stored state continued from cap `from` to p.iterations in place, on
 * the orbits of the new cap.  `iters` is read first and a workgroup with no pixel at `from` ends there, having written nothing;
 * a finished pixel's z, dz, m and der are neither loaded nor stored. */
template <bool JULIA>
__global__ __launch_bounds__(kDeThreads) void escape_extend_pt_de_kernel(const fr_kparams p, double *z, uint32_t *iters, double *dz,
                                                                         uint32_t *mm, double *der, const uint32_t from,
                                                                         const double2 *__restrict__ x_orbit,
                                                                         const double2 *__restrict__ k_orbit, const uint32_t x_last,
                                                                         const uint32_t k_last, const uint32_t ended) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];
    const uint32_t tid = threadIdx.x;
    const DeLane l = de_lane(p, tid);
    const uint64_t k = (uint64_t)l.r * p.ncols + l.cx;
    uint32_t done = 0;
    if (l.valid) done = iters[k];
    const bool running = l.valid && done == from;
    if (!__syncthreads_or(running ? 1 : 0)) return; /* whole workgroup (uniform) */
    if (!JULIA) { /* dc = the pixel's offset, staged as the render stages it; Julia's dc is 0 */
        de_stage<true>(p, tid, l.col0, l.row0, s_re, s_im);
        __syncthreads();
    }
    if (!running) return;
    const uint32_t word = mm[k];
    PtDeState s;
    s.zr = z[2 * k];
    s.zi = z[2 * k + 1];
    s.dzr = dz[2 * k];
    s.dzi = dz[2 * k + 1];
    s.dr = der[2 * k];
    s.di = der[2 * k + 1];
    s.on_k = JULIA && (word & kDeOnK) != 0;
    /* m < last of the orbit followed in every state this view produces; the clamp keeps foreign data inside the orbit */
    s.m = min(word & ~kDeOnK, (s.on_k ? k_last : x_last) - 1u);
    const uint32_t it = orbit_pt_de_state<JULIA>(p.iterations - from, JULIA ? 0.0 : s_re[l.lx], JULIA ? 0.0 : s_im[l.ly], x_orbit, k_orbit,
                                                 x_last, k_last, (ended & 1u) ? x_last : ~0u, (ended & 2u) ? k_last : ~0u,
                                                 p.limit * p.limit, s);
    de_state_store(k, z, iters, dz, mm, der, s, from + it); /* it == M - N on exhaustion: the new cap */
}

/* ---- distance and shaded colour over stored results ------------------------------------------------------------------------- */

__device__ __forceinline__ void de_stage_table(double *s_tab) {
    const double *gt = &g_log2_tab[0][0];
    for (uint32_t k = threadIdx.x; k < FR_LOG2_N * 3; k += kDeThreads) s_tab[k] = gt[k];
    __syncthreads();
}

__global__ __launch_bounds__(kDeThreads) void distance_rows_kernel(const double *__restrict__ z, const uint32_t *__restrict__ iters,
                                                                   const double *__restrict__ der, const size_t n, const uint32_t iterations,
                                                                   const double pixels, double *__restrict__ out) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    de_stage_table(s_tab);
    for (size_t k = (size_t)blockIdx.x * kDeThreads + threadIdx.x; k < n; k += (size_t)gridDim.x * kDeThreads)
        out[k] = de_distance(z[2 * k], z[2 * k + 1], der[2 * k], der[2 * k + 1], iters[k], iterations, pixels, s_tab);
}

/* kernel arguments re-read where the colour map uses them (fr_kernels.hip: FR_COLD_PARAMS; `p` is argument 0) */
typedef const __attribute__((address_space(4))) fr_kparams *DeKArgs;

__global__ __launch_bounds__(kDeThreads) void colour_de_rows_kernel(const fr_kparams p, const double *__restrict__ z,
                                                                    const uint32_t *__restrict__ iters, const double *__restrict__ der,
                                                                    const size_t n, const double pixels, const double thickness,
                                                                    const uint32_t bpp, uint8_t *__restrict__ out) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    de_stage_table(s_tab);
    const bool escape_algo = p.algo == 0 || p.algo == 2;
    for (size_t base = (size_t)blockIdx.x * kDeThreads; base < n; base += (size_t)gridDim.x * kDeThreads) {
        const size_t k = base + threadIdx.x;
        if (k >= n) continue;
        uint32_t r = 0, g = 0, b = 0;
        if (escape_algo) {
            const double zr = z[2 * k], zi = z[2 * k + 1];
            const uint32_t it = iters[k];
            uint8_t rgb[3] = {0, 0, 0};
            {
                DeKArgs kp = (DeKArgs)__builtin_amdgcn_kernarg_segment_ptr();
                asm volatile("" : "+s"(kp));
                const ColourConsts cc = make_colour_consts(*kp);
                colour_of(cc, zr * zr + zi * zi, it, s_tab, nullptr, rgb); /* fr_colour_rows_device's bytes */
            }
            r = rgb[0], g = rgb[1], b = rgb[2];
            if (it < p.iterations && thickness > 0.0) {
                const double s = de_distance(zr, zi, der[2 * k], der[2 * k + 1], it, p.iterations, pixels, s_tab) / thickness;
                if (s < 1.0) { /* 0 <= byte * s < 255: the cast truncates, nothing saturates */
                    r = (uint32_t)((double)r * s);
                    g = (uint32_t)((double)g * s);
                    b = (uint32_t)((double)b * s);
                }
            }
        }
        if (bpp == 4u) {
            reinterpret_cast<uint32_t *>(out)[k] = r | (g << 8) | (b << 16) | 0xFF000000u;
        } else {
            uint8_t *o = out + 3 * k;
            o[0] = (uint8_t)r;
            o[1] = (uint8_t)g;
            o[2] = (uint8_t)b;
        }
    }
}

constexpr size_t kDeMaxN = (size_t)1 << 40;

/* a grid for n pixels, a lane a pixel; the kernels stride on past 2^31 - 1 workgroups */
uint32_t de_blocks(size_t n) {
    const size_t blocks = (n + kDeThreads - 1) / kDeThreads;
    return (uint32_t)(blocks < 0x7FFFFFFFull ? blocks : 0x7FFFFFFFull);
}

/* pixels per unit of the plane along the tighter axis: one multiplication */
double de_pixels(const fr_config *cfg) { return (double)cfg->height * std::fmin(std::fabs(cfg->scale.re), std::fabs(cfg->scale.im)); }

} /* namespace */

using namespace fr;

namespace {

const char *const kDeScope =
    "distance estimation is defined for FR_PRECISION_F64 and FR_PRECISION_PT (dd or wide centre) on one device; FR_PRECISION_F32, "
    "FR_PRECISION_DD, BLA-PT, SCALED PT, block-cyclic and multi-device renders and fr_pixel are out of scope (BLA-PT has "
    "fr_escape_rows_de_pt_bla, supersampling fr_render_rows_ss_de), and so is "
    "raising a DE view's cap with fr_escape_extend* on (z, iters) alone: fr_escape_extend_de(_device) (F64) and "
    "fr_escape_extend_de_pt(_device) (PT) continue the derivative with them";

/* the domain of the F64 extension short of its arrays */
int de_extend_f64_domain(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1) {
    const int rc = check_rows(cfg, y0, y1);
    if (rc != FR_OK) return rc;
    if (precision == FR_PRECISION_PT)
        return fail(FR_ERR_INVALID_ARGUMENT, "FR_PRECISION_PT: a DE view's PT state is (z, iters, dz, m, der), not the three arrays of "
                                             "fr_escape_rows_de; fr_escape_rows_de_pt_state(_device) stores that state and "
                                             "fr_escape_extend_de_pt(_device) continues it");
    if (precision != FR_PRECISION_F64) return fail(FR_ERR_INVALID_ARGUMENT, kDeScope);
    return check_de_limit(cfg);
}

/* the domain of the PT state calls short of their arrays: PT's with a dd centre, WIDE PT's with a wide one, and DE's limit */
int de_pt_state_domain(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1) {
    int rc = check_rows(cfg, y0, y1);
    if (rc != FR_OK) return rc;
    if (c.wide && c.pos_lo) return fail(FR_ERR_INVALID_ARGUMENT, "distance estimation: pos_lo must be NULL when a wide centre is given");
    rc = c.check(cfg, FR_PRECISION_PT);
    if (rc != FR_OK) return rc;
    return check_de_limit(cfg);
}

/* de_state_device's / de_state_host's callable: the F64 extension of rows [y0, y1) between the profiling events (there is no
 * d and no m); arguments already checked, there is work */
auto de_extend_f64_rows(const fr_config *cfg, uint32_t y0, uint32_t y1, uint32_t from) {
    return [=](Ctx &, double *d_z, uint32_t *d_iters, double *, uint32_t *, double *d_der, hipStream_t stream) {
        return profiled_rows(cfg, default_opts(), y0, y1, 0, stream, [&](fr_kparams &p, const char *&kname) -> int {
            kname = "escape_extend_de_kernel";
            if (p.ncols == 0 || p.nrows == 0 || p.iterations <= from) return FR_OK;
            dim3 grid, block;
            HIP_TRY(fr_deep_grid(p, grid, block));
            if (cfg->algo == FR_ALGO_JULIA)
                escape_extend_de_kernel<true><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_der, from);
            else
                escape_extend_de_kernel<false><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_der, from);
            HIP_TRY(hipGetLastError());
            return FR_OK;
        });
    };
}

/* the same for the PT state render (from == nullptr) or its extension from *from, on the context's orbits of cfg's cap, which
 * the cache continues from those of a lower cap of the same view (fr_pt.hip: orbit_for) */
auto de_pt_state_rows(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1, const uint32_t *from) {
    return [=](Ctx &ctx, double *d_z, uint32_t *d_iters, double *d_dz, uint32_t *d_m, double *d_der, hipStream_t stream) {
        return profiled_rows(cfg, default_opts(), y0, y1, 0, stream, [&](fr_kparams &p, const char *&kname) -> int {
            kname = from ? "escape_extend_pt_de_kernel" : "escape_pt_de_state_kernel";
            const bool julia = cfg->algo == FR_ALGO_JULIA;
            const bool orbits = julia || cfg->algo == FR_ALGO_MANDELBROT;
            if (p.ncols == 0 || p.nrows == 0 || (from && (!orbits || p.iterations <= *from))) return FR_OK;
            dim3 grid, block;
            HIP_TRY(fr_deep_grid(p, grid, block));
            std::shared_ptr<PtOrbit> keep; /* alive until the launch is enqueued */
            PtOrbitView v;
            if (orbits) {
                const int rc = pt_orbit_view(ctx, cfg, c, keep, v);
                if (rc != FR_OK) return rc;
            }
            if (from) {
                if (julia)
                    escape_extend_pt_de_kernel<true><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_dz, d_m, d_der, *from, v.x, v.k, v.x_last,
                                                                                 v.k_last, v.ended);
                else
                    escape_extend_pt_de_kernel<false><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_dz, d_m, d_der, *from, v.x, v.k, v.x_last,
                                                                                  v.k_last, v.ended);
            } else if (julia) {
                escape_pt_de_state_kernel<true><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_dz, d_m, d_der, v.x, v.k, v.x_last, v.k_last,
                                                                            v.ended);
            } else {
                escape_pt_de_state_kernel<false><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_dz, d_m, d_der, v.x, v.k, v.x_last, v.k_last,
                                                                             v.ended);
            }
            HIP_TRY(hipGetLastError());
            return FR_OK;
        });
    };
}

int de_pt_state_device(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1, const uint32_t *from, void *d_z, void *d_iters,
                       void *d_dz, void *d_m, void *d_der, void *hip_stream) {
    const int rc = de_pt_state_domain(cfg, c, y0, y1);
    if (rc != FR_OK) return rc;
    return de_state_device(cfg, y0, y1, from, d_z, d_iters, d_dz, d_m, d_der, hip_stream, "PT", "dz", de_pt_state_rows(cfg, c, y0, y1, from));
}

int de_pt_state_host(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1, const uint32_t *from, double *z, uint32_t *iters,
                     double *dz, uint32_t *m, double *der) {
    const int rc = de_pt_state_domain(cfg, c, y0, y1);
    if (rc != FR_OK) return rc;
    return de_state_host(cfg, y0, y1, from, z, iters, dz, m, der, "PT", "dz", de_pt_state_rows(cfg, c, y0, y1, from));
}

/* the domain of the calls over stored results, short of their output */
int de_stored_check(const fr_config *cfg, const void *z, const void *iters, const void *der, size_t n) {
    if (!cfg) return fail(FR_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (n > kDeMaxN) return fail(FR_ERR_INVALID_ARGUMENT, "n > 2^40: one call covers one array of at most 2^40 pixels");
    if (n == 0) return FR_OK;
    return check_de_arrays(z, iters, der, "NULL array: the distance needs z, iters and der, all three");
}

int de_thickness_check(double thickness) {
    if (!(thickness >= 0.0 && thickness <= 0x1p20))
        return fail(FR_ERR_INVALID_ARGUMENT, "thickness must be finite and within [0, 2^20] (pixels; 0 = no shading)");
    return FR_OK;
}

hipError_t launch_distance(const fr_config *cfg, const double *z, const uint32_t *iters, const double *der, size_t n, double *out,
                           hipStream_t stream) {
    distance_rows_kernel<<<dim3(de_blocks(n)), dim3(kDeThreads), 0, stream>>>(z, iters, der, n, cfg->iterations, de_pixels(cfg), out);
    return hipGetLastError();
}

hipError_t launch_colour_de(const fr_config *cfg, const double *z, const uint32_t *iters, const double *der, size_t n, double thickness,
                            uint32_t channels, void *out, hipStream_t stream) {
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    return fr_launch_colour_de_rows(p, z, iters, der, n, de_pixels(cfg), thickness, channels, out, stream);
}

} /* namespace */

hipError_t fr_launch_colour_de_rows(const fr_kparams &p, const double *z, const uint32_t *iters, const double *der, size_t n, double pixels,
                                    double thickness, uint32_t channels, void *out, hipStream_t stream) {
    colour_de_rows_kernel<<<dim3(de_blocks(n)), dim3(kDeThreads), 0, stream>>>(p, z, iters, der, n, pixels, thickness, channels,
                                                                              static_cast<uint8_t *>(out));
    return hipGetLastError();
}

/* fr_de.h: DE's own rules, the road of F64 and PT, and what is left of a state call's domain */
namespace fr {

int check_de_limit(const fr_config *cfg) {
    if (!(cfg->limit <= 0x1p20))
        return fail(FR_ERR_INVALID_ARGUMENT, "distance estimation: limit must be <= 2^20 (the bound that keeps the derivative's overflow "
                                             "below one pixel rests on it)");
    return FR_OK;
}

int check_de_arrays(const void *z, const void *iters, const void *der, const char *null_text) {
    if (!z || !iters || !der)
        return fail(FR_ERR_INVALID_ARGUMENT, null_text ? null_text : "NULL array: a DE render writes z, iters and der, all three");
    if ((reinterpret_cast<uintptr_t>(z) & 7u) || (reinterpret_cast<uintptr_t>(der) & 7u) || (reinterpret_cast<uintptr_t>(iters) & 3u))
        return fail(FR_ERR_INVALID_ARGUMENT, "z and der must be 8-byte aligned, iters 4-byte aligned");
    return FR_OK;
}

/* DE's domain on top of the road's own */
int de_domain(const fr_config *cfg, int precision, const Centre &c, bool wide_call, uint32_t y0, uint32_t y1) {
    int rc = check_rows(cfg, y0, y1);
    if (rc != FR_OK) return rc;
    if (wide_call) {
        if (!c.wide) return fail(FR_ERR_INVALID_ARGUMENT, "FR_PRECISION_PT, wide centre: centre is NULL");
    } else if (precision != FR_PRECISION_F64 && precision != FR_PRECISION_PT) {
        return fail(FR_ERR_INVALID_ARGUMENT, kDeScope);
    } else if (precision == FR_PRECISION_F64 && c.pos_lo) {
        return fail(FR_ERR_INVALID_ARGUMENT, "distance estimation: pos_lo is for FR_PRECISION_PT only; the F64 road takes none");
    }
    if (precision == FR_PRECISION_PT) {
        rc = c.check(cfg, FR_PRECISION_PT); /* PT's domain, or WIDE PT's with its |scale| <= 2^440 */
        if (rc != FR_OK) return rc;
    }
    return check_de_limit(cfg);
}

int de_launch(Ctx &ctx, const fr_config *cfg, int precision, const Centre &c, const fr_kparams &p, double *d_z, uint32_t *d_iters,
              double *d_der, hipStream_t stream, const char *&kname) {
    const bool julia = cfg->algo == FR_ALGO_JULIA;
    const bool orbits = julia || cfg->algo == FR_ALGO_MANDELBROT;
    kname = precision == FR_PRECISION_PT ? "escape_pt_de_kernel" : "escape_de_kernel";
    if (p.ncols == 0 || p.nrows == 0) return FR_OK;
    dim3 grid, block;
    HIP_TRY(fr_deep_grid(p, grid, block));
    if (precision == FR_PRECISION_PT) {
        std::shared_ptr<PtOrbit> keep; /* alive until the launch is enqueued */
        PtOrbitView v;
        if (orbits) {
            const int rc = pt_orbit_view(ctx, cfg, c, keep, v);
            if (rc != FR_OK) return rc;
        }
        if (julia)
            escape_pt_de_kernel<true><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_der, v.x, v.k, v.x_last, v.k_last);
        else
            escape_pt_de_kernel<false><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_der, v.x, v.k, v.x_last, v.k_last);
    } else if (julia) {
        escape_de_kernel<true><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_der);
    } else {
        escape_de_kernel<false><<<grid, block, 0, stream>>>(p, d_z, d_iters, d_der);
    }
    HIP_TRY(hipGetLastError());
    return FR_OK;
}

int de_state_check(const fr_config *cfg, uint32_t y0, uint32_t y1, const uint32_t *from, const void *z, const void *iters, const void *d,
                   const void *m, const void *der, const char *road, const char *d_name, bool *work) {
    *work = false;
    if (from && cfg->iterations < *from)
        return fail(FR_ERR_INVALID_ARGUMENT, "cfg->iterations < from_iterations: a lower cap cannot be derived from a stored state");
    if ((size_t)cfg->width * (size_t)(y1 - y0) == 0) return FR_OK;
    if (road) {
        if (!z || !iters || !d || !m || !der)
            return fail(FR_ERR_INVALID_ARGUMENT, std::string("NULL array: the DE state of ") + road + " is z, iters, " + d_name + ", m and der, all five");
        if ((reinterpret_cast<uintptr_t>(z) & 7u) || (reinterpret_cast<uintptr_t>(d) & 7u) || (reinterpret_cast<uintptr_t>(der) & 7u) ||
            (reinterpret_cast<uintptr_t>(iters) & 3u) || (reinterpret_cast<uintptr_t>(m) & 3u))
            return fail(FR_ERR_INVALID_ARGUMENT, std::string("z, ") + d_name + " and der must be 8-byte aligned, iters and m 4-byte aligned");
    } else {
        const int rc = check_de_arrays(z, iters, der, "NULL array: the extension of a DE view needs z, iters and der, all three");
        if (rc != FR_OK) return rc;
    }
    *work = !from || (cfg->iterations != *from && (cfg->algo == FR_ALGO_MANDELBROT || cfg->algo == FR_ALGO_JULIA));
    return FR_OK;
}

/* fr_ss_list.h: ADAPTIVE SUPERSAMPLED DE's refine pass on the F64 road and PT, on the orbits the probe made */
int de_ss_refine(Ctx &ctx, const fr_config *cfg, int precision, const Centre &c, const fr_ss_refine &a, const fr_ss_de_shade &sh,
                 uint32_t groups, hipStream_t stream) {
    const bool julia = cfg->algo == FR_ALGO_JULIA;
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    const dim3 grid(groups), block(kSsRefineThreads);
    if (precision == FR_PRECISION_PT) {
        std::shared_ptr<PtOrbit> keep; /* alive until the launch is enqueued */
        PtOrbitView v;
        const int rc = pt_orbit_view(ctx, cfg, c, keep, v);
        if (rc != FR_OK) return rc;
        ss_refine_instance(julia, a.linear, [&](auto J, auto L) {
            ss_refine_de_pt_kernel<J(), L()><<<grid, block, 0, stream>>>(p, a, sh, v.x, v.k, v.x_last, v.k_last);
        });
    } else {
        ss_refine_instance(julia, a.linear, [&](auto J, auto L) { ss_refine_de_f64_kernel<J(), L()><<<grid, block, 0, stream>>>(p, a, sh); });
    }
    HIP_TRY(hipGetLastError());
    return FR_OK;
}

}  // namespace fr

extern "C" {

int fr_escape_rows_de_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, void *d_z,
                             void *d_iters, void *d_der, void *hip_stream) {
    const Centre c{pos_lo, nullptr};
    const int rc = de_domain(cfg, precision, c, false, y0, y1);
    if (rc != FR_OK) return rc;
    return de_rows_device(cfg, y0, y1, d_z, d_iters, d_der, hip_stream, de_rows(cfg, y0, y1, de_road(de_launch, cfg, precision, c)));
}

int fr_escape_rows_de(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, double *z, uint32_t *iters,
                      double *der) {
    const Centre c{pos_lo, nullptr};
    const int rc = de_domain(cfg, precision, c, false, y0, y1);
    if (rc != FR_OK) return rc;
    return de_rows_host(cfg, y0, y1, z, iters, der, de_rows(cfg, y0, y1, de_road(de_launch, cfg, precision, c)));
}

int fr_escape_rows_de_pt_wide_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, void *d_z, void *d_iters,
                                     void *d_der, void *hip_stream) {
    const Centre c{nullptr, centre};
    const int rc = de_domain(cfg, FR_PRECISION_PT, c, true, y0, y1);
    if (rc != FR_OK) return rc;
    return de_rows_device(cfg, y0, y1, d_z, d_iters, d_der, hip_stream, de_rows(cfg, y0, y1, de_road(de_launch, cfg, (int)FR_PRECISION_PT, c)));
}

int fr_escape_rows_de_pt_wide(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, double *z, uint32_t *iters,
                              double *der) {
    const Centre c{nullptr, centre};
    const int rc = de_domain(cfg, FR_PRECISION_PT, c, true, y0, y1);
    if (rc != FR_OK) return rc;
    return de_rows_host(cfg, y0, y1, z, iters, der, de_rows(cfg, y0, y1, de_road(de_launch, cfg, (int)FR_PRECISION_PT, c)));
}

/* ---- RESUMABLE DE (include/fractal_hip.h) ---- */

int fr_escape_extend_de_device(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, uint32_t from_iterations, void *d_z,
                               void *d_iters, void *d_der, void *hip_stream) {
    const int rc = de_extend_f64_domain(cfg, precision, y0, y1);
    if (rc != FR_OK) return rc;
    return de_state_device(cfg, y0, y1, &from_iterations, d_z, d_iters, nullptr, nullptr, d_der, hip_stream, nullptr, nullptr,
                           de_extend_f64_rows(cfg, y0, y1, from_iterations));
}

int fr_escape_extend_de(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, uint32_t from_iterations, double *z, uint32_t *iters,
                        double *der) {
    const int rc = de_extend_f64_domain(cfg, precision, y0, y1);
    if (rc != FR_OK) return rc;
    /* z and der share the context's z scratch, as in fr_escape_rows_de; uploaded first, as fr_escape_extend does */
    return de_state_host(cfg, y0, y1, &from_iterations, z, iters, nullptr, nullptr, der, nullptr, nullptr,
                         de_extend_f64_rows(cfg, y0, y1, from_iterations));
}

int fr_escape_rows_de_pt_state_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, uint32_t y0,
                                      uint32_t y1, void *d_z, void *d_iters, void *d_dz, void *d_m, void *d_der, void *hip_stream) {
    return de_pt_state_device(cfg, Centre{pos_lo, centre}, y0, y1, nullptr, d_z, d_iters, d_dz, d_m, d_der, hip_stream);
}

int fr_escape_rows_de_pt_state(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, uint32_t y0, uint32_t y1,
                               double *z, uint32_t *iters, double *dz, uint32_t *m, double *der) {
    return de_pt_state_host(cfg, Centre{pos_lo, centre}, y0, y1, nullptr, z, iters, dz, m, der);
}

int fr_escape_extend_de_pt_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, uint32_t y0, uint32_t y1,
                                  uint32_t from_iterations, void *d_z, void *d_iters, void *d_dz, void *d_m, void *d_der,
                                  void *hip_stream) {
    return de_pt_state_device(cfg, Centre{pos_lo, centre}, y0, y1, &from_iterations, d_z, d_iters, d_dz, d_m, d_der, hip_stream);
}

int fr_escape_extend_de_pt(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, uint32_t y0, uint32_t y1,
                           uint32_t from_iterations, double *z, uint32_t *iters, double *dz, uint32_t *m, double *der) {
    return de_pt_state_host(cfg, Centre{pos_lo, centre}, y0, y1, &from_iterations, z, iters, dz, m, der);
}

int fr_distance_rows_device(const fr_config *cfg, const void *d_z, const void *d_iters, const void *d_der, size_t n, void *d_out,
                            void *hip_stream) {
    const int rc = de_stored_check(cfg, d_z, d_iters, d_der, n);
    if (rc != FR_OK || n == 0) return rc;
    if (!d_out) return fail(FR_ERR_INVALID_ARGUMENT, "d_out is NULL");
    if (reinterpret_cast<uintptr_t>(d_out) & 7u) return fail(FR_ERR_INVALID_ARGUMENT, "d_out must be 8-byte aligned");
    HIP_TRY(launch_distance(cfg, static_cast<const double *>(d_z), static_cast<const uint32_t *>(d_iters), static_cast<const double *>(d_der), n,
                            static_cast<double *>(d_out), static_cast<hipStream_t>(hip_stream)));
    return FR_OK;
}

int fr_distance_rows(const fr_config *cfg, const double *z, const uint32_t *iters, const double *der, size_t n, double *out) {
    int rc = de_stored_check(cfg, z, iters, der, n);
    if (rc != FR_OK || n == 0) return rc;
    if (!out) return fail(FR_ERR_INVALID_ARGUMENT, "out is NULL");
    const size_t zb = n * 2 * sizeof(double), ib = n * sizeof(uint32_t);
    LifeShared ls;
    Ctx *ctx;
    rc = primary(&ctx);
    if (rc != FR_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    rc = ctx->reserve(ctx->z, 2 * zb); /* z, then der */
    if (rc == FR_OK) rc = ctx->reserve(ctx->iters, ib);
    if (rc == FR_OK) rc = ctx->reserve(ctx->misc, n * sizeof(double));
    if (rc != FR_OK) return rc;
    double *const d_z = static_cast<double *>(ctx->z.ptr), *const d_der = d_z + 2 * n, *const d_out = static_cast<double *>(ctx->misc.ptr);
    HIP_TRY(hipMemcpyAsync(d_z, z, zb, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_der, der, zb, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->iters.ptr, iters, ib, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_distance(cfg, d_z, static_cast<const uint32_t *>(ctx->iters.ptr), d_der, n, d_out, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, d_out, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FR_OK;
}

int fr_colour_de_rows_device(const fr_config *cfg, const void *d_z, const void *d_iters, const void *d_der, size_t n, double thickness,
                             int channels, void *d_out, void *hip_stream) {
    int rc = de_stored_check(cfg, d_z, d_iters, d_der, n);
    if (rc == FR_OK) rc = de_thickness_check(thickness);
    if (rc == FR_OK) rc = check_channels(channels);
    if (rc != FR_OK || n == 0) return rc;
    if (!d_out) return fail(FR_ERR_INVALID_ARGUMENT, "d_out is NULL");
    if (channels == 4 && (reinterpret_cast<uintptr_t>(d_out) & 3u)) return fail(FR_ERR_INVALID_ARGUMENT, "RGBA8 output must be 4-byte aligned");
    HIP_TRY(launch_colour_de(cfg, static_cast<const double *>(d_z), static_cast<const uint32_t *>(d_iters), static_cast<const double *>(d_der), n,
                             thickness, (uint32_t)channels, d_out, static_cast<hipStream_t>(hip_stream)));
    return FR_OK;
}

int fr_colour_de_rgb8(const fr_config *cfg, const double *z, const uint32_t *iters, const double *der, size_t n, double thickness,
                      uint8_t *out, size_t out_len) {
    int rc = de_stored_check(cfg, z, iters, der, n);
    if (rc == FR_OK) rc = de_thickness_check(thickness);
    if (rc != FR_OK || n == 0) return rc;
    if (!out) return fail(FR_ERR_INVALID_ARGUMENT, "out is NULL");
    if (out_len < 3 * n) return fail(FR_ERR_BUFFER_TOO_SMALL, "out_len < 3*n");
    const size_t zb = n * 2 * sizeof(double), ib = n * sizeof(uint32_t);
    LifeShared ls;
    Ctx *ctx;
    rc = primary(&ctx);
    if (rc != FR_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    rc = ctx->reserve(ctx->z, 2 * zb); /* z, then der */
    if (rc == FR_OK) rc = ctx->reserve(ctx->iters, ib);
    if (rc == FR_OK) rc = ctx->reserve(ctx->rgb, 3 * n);
    if (rc != FR_OK) return rc;
    double *const d_z = static_cast<double *>(ctx->z.ptr), *const d_der = d_z + 2 * n;
    HIP_TRY(hipMemcpyAsync(d_z, z, zb, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_der, der, zb, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->iters.ptr, iters, ib, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_colour_de(cfg, d_z, static_cast<const uint32_t *>(ctx->iters.ptr), d_der, n, thickness, 3u, ctx->rgb.ptr, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, ctx->rgb.ptr, 3 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FR_OK;
}

} /* extern "C" */
