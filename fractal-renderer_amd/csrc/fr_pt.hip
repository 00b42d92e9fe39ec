/*
 * fr_pt.hip — FR_PRECISION_PT: deep zooms by perturbation.  The view's reference orbit is iterated once on the host in
 * double-double arithmetic (DD's operations) and stored as its f64 hi parts; every pixel then iterates in f64 only its
 * offset dz from that orbit, dz' = (2Z + dz) dz + dc, and rebases (dz = z, back to the orbit's start) when |z| < |dz|
 * or the orbit runs out, so one orbit serves the whole view (include/fractal_hip.h, fr_precision, states the sequence;
 * tests/pt_model.c restates it; tests/test_gpu_pt.py compares the two bit for bit).
 *
 * Host part: the orbits (R for Mandelbrot; V and K for Julia), computed with -ffp-contract=off and std::fma exactly where
 * the definition has fma, uploaded into device memory owned by the context and kept there for the next call of the same
 * view (Ctx::pt_orbit, guarded by Ctx::pt_mu).
 *
 * Device part, escape_pt_kernel<MODE, JULIA> (cdna_hip_programming: one lane per pixel, LDS for what a workgroup
 * shares):
 *   - a workgroup of 4 waves renders 16 x 16 pixels, each wave one 8 x 8 tile (DD's shape);
 *   - the 16 column and 16 row offsets `off` are computed once per workgroup by 32 lanes and staged in LDS, as is the
 *     log2 table for RGB;
 *   - one step is 4 fma + 4 add for dz' and z', 3 + 3 for the escape and rebase tests: ~14 f64 VALU operations against
 *     DD's ~89.  Each step needs the orbit entries X_m and X_{m+1}; the next index is m + 1 or, after a rebase, 0, so
 *     X_0 = 0 and X_1 (of the orbit rebased onto) stay in registers and the load of X_{m+2} is issued one step ahead,
 *     its latency hidden behind the step's arithmetic.  While no lane of a wave has rebased, the lanes share m and the
 *     16-byte load of an interleaved (re, im) entry is one cache line for the whole wave; afterwards it gathers, from
 *     an orbit that the L2 holds (16 B per entry);
 *   - outputs as escape_dd_kernel's: RGB / RGBA, ESCAPE (z, index), COUNT; 64-bit output offsets.
 *
 * Resumable PT (include/fractal_hip.h, "RESUMABLE PT"; tests/pt_state_model.c restates it): escape_pt_state_kernel<JULIA>
 * is the ESCAPE render with the state rule — no rebase at the end of an orbit that the cap cut — and stores the whole
 * state (z, iters, dz, m); escape_extend_pt_kernel<JULIA> continues such a state to a higher cap in place, on orbits that
 * the host continued from their dd tails instead of recomputing them (orbit_for).  escape_pt_kernel and orbit_pt are the
 * PT definition's and stay as they are.
 *
 * ADAPTIVE SUPERSAMPLING (include/fractal_hip.h; fr_ss_adaptive.hip): ss_refine_pt_kernel<JULIA>, persistent waves that run
 * orbit_pt on the s x s samples of the listed edge pixels (fr_ss_list.h: the claim loop), and pt_ss_refine, its launch.
 *
 * The entry points that only PT has live here beside their launches, at the end of the file: the state render and its
 * extension, and every fr_*_pt_wide call (WIDE PT: the same launches with a Centre that holds a wide centre; fr_ctx.h).
 * Each builds its Centre and checks PT's domain; the state calls then hand pt_state_rows, their launch, to the state road
 * of fr_ctx.h (state_device, state_host), the others go to the row calls' bodies in fr_api.hip.  The workgroup's geometry and
 * the launches' grid are the deep kernels' (fr_kernels.h: kDeep*, fr_deep_grid).
 */
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "fr_ctx.h"
#include "fr_math.h"
#include "fr_ss_list.h"
#include "fr_wide.h"

namespace {

#include "fr_colour.h"

/* ---- device: the pixel loop (include/fractal_hip.h, fr_precision: PT), operation for operation ------------------- */

/* X: the orbit the pixel starts on (R or V), K: the one it rebases onto (R or K); *_last: index of the last entry.
 * Returns the escape index (or `iterations`), the final z in (out_re, out_im). */
template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_pt(uint32_t iterations, double off_re, double off_im, const double2 *x_orbit,
                                             const double2 *k_orbit, uint32_t x_last, uint32_t k_last, double squared,
                                             double &out_re, double &out_im) {
    const double2 *X = x_orbit;
    uint32_t last = x_last;
    uint32_t m = JULIA ? 0u : 1u;
    double dzr = off_re, dzi = off_im;
    const double dcr = JULIA ? 0.0 : off_re, dci = JULIA ? 0.0 : off_im;
    double2 Z = X[m], N = X[m + 1]; /* m <= last - 1 at the top of every step: X_{m+1} exists */
    const double2 K1 = k_orbit[1];  /* the entry after a rebase; K_0 = R_0 = 0 */
    double zr = Z.x + dzr, zi = Z.y + dzi;
    uint32_t i = 0;
    for (; i < iterations; i++) {
        const double2 P = X[min(m + 2u, last)]; /* X_{m+2}: next step's X_{m+1} if it does not rebase */
        const double tr = Z.x + zr, ti = Z.y + zi;
        const double ndr = __builtin_fma(tr, dzr, __builtin_fma(-ti, dzi, dcr));
        const double ndi = __builtin_fma(tr, dzi, __builtin_fma(ti, dzr, dci));
        m++;
        zr = N.x + ndr;
        zi = N.y + ndi;
        dzr = ndr;
        dzi = ndi;
        const double dist = zr * zr + zi * zi;
        if (dist > squared) break; /* this lane leaves EXEC; the wave goes on while any lane is left */
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
    out_re = zr;
    out_im = zi;
    return i;
}

template <int MODE, bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_pt_kernel(const fr_kparams p, const fr_kout out,
                                                                    const double2 *__restrict__ x_orbit,
                                                                    const double2 *__restrict__ k_orbit, const uint32_t x_last,
                                                                    const uint32_t k_last) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];

    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kDeepBlockW - 1) / kDeepBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t col0 = bx * kDeepBlockW, row0 = by * kDeepBlockH;

    if (MODE == FR_OUT_RGB) {
        const double *gt = &g_log2_tab[0][0];
        for (uint32_t k = tid; k < FR_LOG2_N * 3; k += 64 * kDeepWaves) s_tab[k] = gt[k];
    }
    if (tid < kDeepBlockW + kDeepBlockH) {
        /* off: coord_to_space (calc/src/lib.rs:181-197) without the final `+ pos`, DD's off */
        const double width = (double)p.width, height = (double)p.height;
        if (tid < kDeepBlockW) {
            const uint64_t x = (uint64_t)p.x_first + (uint64_t)(col0 + tid) * p.x_stride;
            s_re[tid] = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re;
        } else {
            const uint32_t r = row0 + (tid - kDeepBlockW);
            const uint64_t y = (uint64_t)p.y_first + (uint64_t)(r / p.block_rows) * p.y_stride + r % p.block_rows;
            s_im[tid - kDeepBlockW] = (((double)y / height) - 0.5) / p.scale_im;
        }
    }
    __syncthreads();

    const uint32_t wave = tid >> 6, lane = tid & 63;
    const uint32_t lx = (wave % kDeepWavesX) * kDeepTileW + lane % kDeepTileW;
    const uint32_t ly = (wave / kDeepWavesX) * kDeepTileH + lane / kDeepTileW;
    const uint32_t cx = col0 + lx, r = row0 + ly;
    const bool valid = cx < p.ncols && r < p.nrows;
    const bool escape_algo = JULIA ? p.algo == 2 : p.algo == 0; /* the host picks JULIA from the algorithm */

    double zr = 0.0, zi = 0.0;
    uint32_t iters = 0;
    if (valid && escape_algo) {
        const double squared = p.limit * p.limit; /* calc/src/lib.rs:246 */
        iters = orbit_pt<JULIA>(p.iterations, s_re[lx], s_im[ly], x_orbit, k_orbit, x_last, k_last, squared, zr, zi);
    }

    if constexpr (MODE == FR_OUT_RGB) {
        if (valid) {
            uint8_t rgb[3] = {0, 0, 0};
            if (escape_algo) {
                const ColourConsts cc = make_colour_consts(p);
                const double r2 = zr * zr, i2 = zi * zi;
                colour_pixel<double>(cc, zr, zi, r2, i2, iters, s_tab, nullptr, rgb); /* :214-234 on the f64 z */
            }
            uint64_t row_out = r;
            if (p.out_in_place) row_out = (uint64_t)p.y_first + (uint64_t)(r / p.block_rows) * p.y_stride + r % p.block_rows;
            const uint64_t k = row_out * p.ncols + cx;
            if (p.out_rgba) {
                reinterpret_cast<uint32_t *>(out.rgb)[k] =
                    (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16) | 0xFF000000u;
            } else {
                uint8_t *o = out.rgb + 3ull * k;
                o[0] = rgb[0];
                o[1] = rgb[1];
                o[2] = rgb[2];
            }
        }
    } else if constexpr (MODE == FR_OUT_ESCAPE) {
        if (valid) {
            const uint64_t k = (uint64_t)r * p.ncols + cx;
            if (out.z) {
                out.z[2 * k] = zr;
                out.z[2 * k + 1] = zi;
            }
            if (out.iters) out.iters[k] = iters;
        }
    } else {
        unsigned long long n = 0;
        if (valid && escape_algo) n = iters < p.iterations ? (unsigned long long)iters + 1ull : p.iterations;
        for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
        if (lane == 0 && n) atomicAdd(out.count + ((blockIdx.x + 131u * wave) % FR_COUNT_SLOTS), n);
    }
}

template <bool JULIA>
hipError_t launch(const fr_kparams &p, int mode, const fr_kout &out, const double2 *x_orbit, const double2 *k_orbit,
                  uint32_t x_last, uint32_t k_last, hipStream_t stream) {
    dim3 grid, block;
    const hipError_t e = fr_deep_grid(p, grid, block);
    if (e != hipSuccess) return e;
    if (mode == FR_OUT_RGB)
        escape_pt_kernel<FR_OUT_RGB, JULIA><<<grid, block, 0, stream>>>(p, out, x_orbit, k_orbit, x_last, k_last);
    else if (mode == FR_OUT_ESCAPE)
        escape_pt_kernel<FR_OUT_ESCAPE, JULIA><<<grid, block, 0, stream>>>(p, out, x_orbit, k_orbit, x_last, k_last);
    else
        escape_pt_kernel<FR_OUT_COUNT, JULIA><<<grid, block, 0, stream>>>(p, out, x_orbit, k_orbit, x_last, k_last);
    return hipGetLastError();
}

/* ---- device: ADAPTIVE SUPERSAMPLING's refine pass (include/fractal_hip.h; fr_ss_list.h: the claim loop) --------------- */

/* Persistent waves over the edge list of an adaptive render of cfg_s (`p` holds cfg_s): each lane computes its sample's `off`
 * by escape_pt_kernel's formula — the same operations on the same (x, y), hence the same bits — runs orbit_pt and colours
 * the f64 z as the render does.  The log2 table is staged before the loop, which holds no barrier. */
template <bool JULIA, bool LINEAR>
__global__ __launch_bounds__(kSsRefineThreads) void ss_refine_pt_kernel(const fr_kparams p, const fr_ss_refine a,
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
        double zr, zi;
        const uint32_t iters = orbit_pt<JULIA>(p.iterations, off_re, off_im, x_orbit, k_orbit, x_last, k_last, squared, zr, zi);
        uint8_t rgb[3] = {0, 0, 0};
        const ColourConsts cc = make_colour_consts(p);
        colour_pixel<double>(cc, zr, zi, zr * zr, zi * zi, iters, s_tab, nullptr, rgb);
        return (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16);
    });
}

/* ---- device: the resumable state (include/fractal_hip.h, "resumable perturbation") --------------------------------- */

/* A pixel's state between steps: z, dz, the index m into the orbit it follows and whether that orbit is K (Julia after a
 * rebase).  orbit_pt_state runs `steps` steps of the PT sequence from it with the state rule's rebase condition — dist <
 * |dz|^2, or m == last of an orbit that is ENDED BY ESCAPE (x_end / k_end: that last index, or ~0 for an orbit cut by the
 * cap, which m never equals) — and leaves the state after the last step in `s`; on escape the state is (z, 0, 0).  Returns
 * the steps completed before the escape (`steps`: none).  x_last / k_last only clamp the loads. */
struct PtState {
    double zr, zi, dzr, dzi;
    uint32_t m;
    bool on_k;
};

template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_pt_state(uint32_t steps, double dcr, double dci, const double2 *x_orbit,
                                                   const double2 *k_orbit, uint32_t x_last, uint32_t k_last, uint32_t x_end,
                                                   uint32_t k_end, double squared, PtState &s) {
    const bool on_k = JULIA && s.on_k;
    const double2 *X = on_k ? k_orbit : x_orbit;
    uint32_t last = on_k ? k_last : x_last, end = on_k ? k_end : x_end;
    uint32_t m = s.m;
    bool k_now = on_k;
    double dzr = s.dzr, dzi = s.dzi, zr = s.zr, zi = s.zi;
    double2 Z = X[min(m, last)], N = X[min(m + 1u, last)]; /* m < last at the top of every step */
    const double2 K1 = k_orbit[1];                         /* the entry after a rebase; K_0 = R_0 = 0 */
    uint32_t i = 0;
    for (; i < steps; i++) {
        const double2 P = X[min(m + 2u, last)]; /* X_{m+2}: next step's X_{m+1} if it does not rebase */
        const double tr = Z.x + zr, ti = Z.y + zi;
        const double ndr = __builtin_fma(tr, dzr, __builtin_fma(-ti, dzi, dcr));
        const double ndi = __builtin_fma(tr, dzi, __builtin_fma(ti, dzr, dci));
        m++;
        zr = N.x + ndr;
        zi = N.y + ndi;
        dzr = ndr;
        dzi = ndi;
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
    const bool escaped = i < steps; /* (z, 0, 0) for an escaped lane */
    s.zr = zr;
    s.zi = zi;
    s.dzr = escaped ? 0.0 : dzr;
    s.dzi = escaped ? 0.0 : dzi;
    s.m = escaped ? 0u : m;
    s.on_k = !escaped && k_now;
    return i;
}

constexpr uint32_t kPtOnK = 0x80000000u; /* bit 31 of the stored m: the pixel follows K */

/* 16 column and 16 row offsets of the workgroup's pixels into LDS (escape_pt_kernel's staging); the caller synchronises */
__device__ __forceinline__ void stage_offsets(const fr_kparams &p, uint32_t tid, uint32_t col0, uint32_t row0, double *s_re,
                                              double *s_im) {
    if (tid < kDeepBlockW + kDeepBlockH) {
        const double width = (double)p.width, height = (double)p.height;
        if (tid < kDeepBlockW) {
            const uint64_t x = (uint64_t)p.x_first + (uint64_t)(col0 + tid) * p.x_stride;
            s_re[tid] = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re;
        } else {
            const uint32_t r = row0 + (tid - kDeepBlockW);
            const uint64_t y = (uint64_t)p.y_first + (uint64_t)(r / p.block_rows) * p.y_stride + r % p.block_rows;
            s_im[tid - kDeepBlockW] = (((double)y / height) - 0.5) / p.scale_im;
        }
    }
}

/* escape_pt_kernel<FR_OUT_ESCAPE>'s shape with the state rule, storing the whole state: z and dz as re, im per pixel, iters,
 * m (bit 31: on K).  `ended`: bit 0 = X, bit 1 = K is ended by escape.  An algorithm without orbits writes zeros. */
template <bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_pt_state_kernel(const fr_kparams p, double *__restrict__ z,
                                                                          uint32_t *__restrict__ iters, double *__restrict__ dz,
                                                                          uint32_t *__restrict__ mm,
                                                                          const double2 *__restrict__ x_orbit,
                                                                          const double2 *__restrict__ k_orbit, const uint32_t x_last,
                                                                          const uint32_t k_last, const uint32_t ended) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];

    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kDeepBlockW - 1) / kDeepBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t col0 = bx * kDeepBlockW, row0 = by * kDeepBlockH;
    stage_offsets(p, tid, col0, row0, s_re, s_im);
    __syncthreads();

    const uint32_t wave = tid >> 6, lane = tid & 63;
    const uint32_t lx = (wave % kDeepWavesX) * kDeepTileW + lane % kDeepTileW;
    const uint32_t ly = (wave / kDeepWavesX) * kDeepTileH + lane / kDeepTileW;
    const uint32_t cx = col0 + lx, r = row0 + ly;
    if (cx >= p.ncols || r >= p.nrows) return;
    const bool escape_algo = JULIA ? p.algo == 2 : p.algo == 0; /* the host picks JULIA from the algorithm */

    PtState s{0.0, 0.0, 0.0, 0.0, 0u, false};
    uint32_t it = 0;
    if (escape_algo) {
        const double off_re = s_re[lx], off_im = s_im[ly];
        s.m = JULIA ? 0u : 1u;
        s.dzr = off_re;
        s.dzi = off_im;
        const double2 X0 = x_orbit[min(s.m, x_last)];
        s.zr = X0.x + s.dzr;
        s.zi = X0.y + s.dzi;
        it = orbit_pt_state<JULIA>(p.iterations, JULIA ? 0.0 : off_re, JULIA ? 0.0 : off_im, x_orbit, k_orbit, x_last, k_last,
                                   (ended & 1u) ? x_last : ~0u, (ended & 2u) ? k_last : ~0u, p.limit * p.limit, s);
    }
    const uint64_t k = (uint64_t)r * p.ncols + cx;
    z[2 * k] = s.zr;
    z[2 * k + 1] = s.zi;
    iters[k] = it;
    dz[2 * k] = s.dzr;
    dz[2 * k + 1] = s.dzi;
    mm[k] = s.m | (s.on_k ? kPtOnK : 0u);
}

/* Continue a stored state from cap `from` to p.iterations in place (escape_extend_dd_kernel's early-out): `iters` is read
 * first and a workgroup with no pixel at `from` ends there, having written nothing; a finished pixel's z, dz and m are
 * neither loaded nor stored.  The orbits are those of the new cap. */
template <bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_extend_pt_kernel(const fr_kparams p, double *z, uint32_t *iters, double *dz,
                                                                           uint32_t *mm, const uint32_t from,
                                                                           const double2 *__restrict__ x_orbit,
                                                                           const double2 *__restrict__ k_orbit, const uint32_t x_last,
                                                                           const uint32_t k_last, const uint32_t ended) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];

    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kDeepBlockW - 1) / kDeepBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t col0 = bx * kDeepBlockW, row0 = by * kDeepBlockH;
    const uint32_t wave = tid >> 6, lane = tid & 63;
    const uint32_t lx = (wave % kDeepWavesX) * kDeepTileW + lane % kDeepTileW;
    const uint32_t ly = (wave / kDeepWavesX) * kDeepTileH + lane / kDeepTileW;
    const uint32_t cx = col0 + lx, r = row0 + ly;
    const bool valid = cx < p.ncols && r < p.nrows;
    const uint64_t k = (uint64_t)r * p.ncols + cx;
    uint32_t done = 0;
    if (valid) done = iters[k];
    const bool running = valid && done == from;
    if (!__syncthreads_or(running ? 1 : 0)) return; /* whole workgroup (uniform) */

    if (!JULIA) { /* dc = the pixel's offset, staged as the render stages it; Julia's dc is 0 */
        stage_offsets(p, tid, col0, row0, s_re, s_im);
        __syncthreads();
    }
    if (running) {
        const uint32_t word = mm[k];
        PtState s;
        s.zr = z[2 * k];
        s.zi = z[2 * k + 1];
        s.dzr = dz[2 * k];
        s.dzi = dz[2 * k + 1];
        s.on_k = JULIA && (word & kPtOnK) != 0;
        /* m < last of the orbit followed in every state this view produces; the clamp keeps foreign data inside the orbit */
        s.m = min(word & ~kPtOnK, (s.on_k ? k_last : x_last) - 1u);
        const uint32_t it = orbit_pt_state<JULIA>(p.iterations - from, JULIA ? 0.0 : s_re[lx], JULIA ? 0.0 : s_im[ly], x_orbit, k_orbit,
                                                  x_last, k_last, (ended & 1u) ? x_last : ~0u, (ended & 2u) ? k_last : ~0u,
                                                  p.limit * p.limit, s);
        z[2 * k] = s.zr;
        z[2 * k + 1] = s.zi;
        dz[2 * k] = s.dzr;
        dz[2 * k + 1] = s.dzi;
        mm[k] = s.m | (s.on_k ? kPtOnK : 0u);
        iters[k] = from + it; /* it == M - N on exhaustion: the new cap */
    }
}

/* ---- host: the reference orbits, DD's operations (include/fractal_hip.h) with std::fma where the definition has fma -- */

struct ddh {
    double hi, lo;
};

ddh two_sum(double a, double b) {
    const double s = a + b;
    const double bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}

ddh fast_two_sum(double a, double b) {
    const double s = a + b;
    return {s, b - (s - a)};
}

ddh add_dd(ddh a, ddh b) {
    ddh s = two_sum(a.hi, b.hi);
    const ddh t = two_sum(a.lo, b.lo);
    s.lo = s.lo + t.hi;
    s = fast_two_sum(s.hi, s.lo);
    s.lo = s.lo + t.lo;
    return fast_two_sum(s.hi, s.lo);
}

ddh add_d(ddh a, double d) {
    ddh s = two_sum(a.hi, d);
    s.lo = s.lo + a.lo;
    return fast_two_sum(s.hi, s.lo);
}

ddh sqr(ddh x) {
    const double p = x.hi * x.hi;
    double e = std::fma(x.hi, x.hi, -p);
    e = std::fma(x.hi + x.hi, x.lo, e);
    return fast_two_sum(p, e);
}

ddh twice_mul(ddh x, ddh y) {
    const double p = x.hi * y.hi;
    double e = std::fma(x.hi, y.hi, -p);
    e = std::fma(x.hi, y.lo, e);
    e = std::fma(x.lo, y.hi, e);
    const ddh h = fast_two_sum(p, e);
    return {h.hi + h.hi, h.lo + h.lo};
}

ddh neg(ddh x) { return {-x.hi, -x.lo}; }

/* how an orbit's last stored entry came about, and that entry in dd: what continuing the recurrence needs */
struct OrbitEnd {
    bool ended = false; /* ended by escape (identical at every higher cap); false: cut by the cap at k == kmax */
    ddh re{0.0, 0.0}, im{0.0, 0.0};
    fr::WideTail wide; /* that entry as integers, for a view with a wide centre (fr_wide.hip) */
};

/* Orbit `which` (0: R or V, 1: K) of the view as re, im pairs of the hi parts, appended to `out`; at most iterations + 2
 * entries in all.  from == nullptr: the whole orbit, entry 0 first.  Otherwise entries 0 .. last of an orbit CUT BY THE CAP
 * exist already (`last` = its kmax, *from its end) and the recurrence goes on from entry last + 1: the same operations on
 * the same dd values, so the entries are those of the whole orbit at cfg's cap. */
void reference_orbit(const fr_config *cfg, double lo_re, double lo_im, int which, std::vector<double> &out, OrbitEnd &end,
                     const OrbitEnd *from = nullptr, uint32_t last = 0) {
    const bool julia = cfg->algo == 2;
    const uint32_t kmin = julia ? 1u : 2u;
    const uint32_t kmax = julia ? (cfg->iterations > 1 ? cfg->iterations : 1u) : cfg->iterations + 1u;
    const ddh cre{cfg->pos.re, lo_re}, cim{cfg->pos.im, lo_im};
    ddh zr{0.0, 0.0}, zi{0.0, 0.0};
    if (julia && which == 0) zr = cre, zi = cim;
    bool stored = false; /* entry k is in the orbit already and has passed its tests */
    uint32_t k = 0;
    if (from) {
        end = *from;
        if (from->ended || last >= kmax) return;
        zr = from->re, zi = from->im, k = last, stored = true;
    }
    out.reserve(out.size() + 2 * ((size_t)(kmax - k) + 1));
    for (;; k++) {
        if (!stored) {
            out.push_back(zr.hi);
            out.push_back(zi.hi);
            end.ended = k >= kmin && zr.hi * zr.hi + zi.hi * zi.hi > 4.0;
            if (end.ended || k == kmax) break;
        }
        stored = false;
        if (!julia && k == 0) {
            zr = cre, zi = cim; /* R_1 = C */
        } else {
            const ddh a = add_dd(sqr(zr), neg(sqr(zi)));
            const ddh b = twice_mul(zr, zi);
            if (julia) {
                zr = add_d(a, cfg->julia_set.re);
                zi = add_d(b, cfg->julia_set.im);
            } else {
                zr = add_dd(a, cre);
                zi = add_dd(b, cim);
            }
        }
    }
    end.re = zr, end.im = zi;
}

/* reference_orbit for a view with a wide centre (include/fractal_hip.h, "WIDE PT"): the same contract, the recurrence in
 * fixed point from the stored integer tail */
void reference_orbit_wide(const fr_config *cfg, const fr_wide_centre *wide, int which, std::vector<double> &out, OrbitEnd &end,
                          const OrbitEnd *from = nullptr, uint32_t last = 0) {
    if (from) {
        end = *from;
        if (from->ended) return;
    }
    fr::wide_reference_orbit(cfg, wide, which, out, end.ended, end.wide, from ? &from->wide : nullptr, last);
}

}  // namespace

namespace fr {

/* the orbits of one view in device memory: X (R or V) at dev[0 ..], K (Julia) after it */
struct PtOrbit {
    uint32_t algo = 0, iterations = 0;
    double key[6] = {}; /* pos.re, pos.im, pos_lo.re, pos_lo.im, julia_set.re, julia_set.im, compared bit for bit */
    std::vector<uint64_t> wide_key; /* a wide centre's n and words (then key[0 .. 3] are 0); empty: a dd view */
    double2 *dev = nullptr;
    uint32_t x_last = 0, k_last = 0;
    size_t k_offset = 0; /* entries */
    OrbitEnd x_end, k_end;  /* Mandelbrot: k_end = x_end */
    uint32_t computed = 0;  /* entries the last request for this view computed on the host (fr_debug_pt_orbit_cache) */
    uint32_t ended() const { return (x_end.ended ? 1u : 0u) | (k_end.ended ? 2u : 0u); } /* the kernels' `ended` */
    ~PtOrbit() {
        if (dev) (void)hipFree(dev); /* hipFree waits for the device: no kernel still reads the orbit */
    }
};

namespace {

void view_key(const fr_config *cfg, const Centre &c, double key[6]) {
    key[0] = c.wide ? 0.0 : cfg->pos.re; /* a wide view does not read cfg->pos */
    key[1] = c.wide ? 0.0 : cfg->pos.im;
    key[2] = c.lo_re();
    key[3] = c.lo_im();
    key[4] = cfg->algo == 2 ? cfg->julia_set.re : 0.0;
    key[5] = cfg->algo == 2 ? cfg->julia_set.im : 0.0;
}

/* The view's orbits, from the context's cache or computed and uploaded; the caller keeps `out` alive until its launch
 * has been enqueued (a later view may replace the cache entry meanwhile; the last reference frees it).
 * The same view at a HIGHER cap continues what the cache holds (include/fractal_hip.h, "resumable perturbation"): an orbit
 * ended by escape is the same at every cap, so if all are, the entry is re-keyed and nothing is computed; otherwise the
 * recurrence goes on from the stored dd tail for the missing entries only, into a NEW PtOrbit — launches in flight hold the
 * old one — whose old entries arrive by a device-to-device copy. */
int orbit_for(Ctx &ctx, const fr_config *cfg, const Centre &centre, std::shared_ptr<PtOrbit> &out) {
    const fr_wide_centre *wide = centre.wide;
    double key[6];
    view_key(cfg, centre, key);
    std::vector<uint64_t> wkey; /* one slot, two roads: a wide view never matches a dd view, nor other words or another n */
    if (wide) wide_key(wide, wkey);
    const bool julia = cfg->algo == 2;
    std::lock_guard<std::mutex> lk(ctx.pt_mu);
    const std::shared_ptr<PtOrbit> c = ctx.pt_orbit;
    const bool same_view = c && c->algo == cfg->algo && memcmp(c->key, key, sizeof key) == 0 && c->wide_key == wkey;
    if (same_view && c->iterations == cfg->iterations) {
        c->computed = 0;
        out = c;
        return FR_OK;
    }
    const bool resume = same_view && c->iterations < cfg->iterations;
    if (resume && c->x_end.ended && c->k_end.ended) {
        c->iterations = cfg->iterations; /* only orbit_for reads it, under pt_mu */
        c->computed = 0;
        out = c;
        return FR_OK;
    }
    std::vector<double> x, k; /* the entries to upload: all of them, or those behind the cached ones */
    auto o = std::make_shared<PtOrbit>();
    if (wide) {
        reference_orbit_wide(cfg, wide, 0, x, o->x_end, resume ? &c->x_end : nullptr, resume ? c->x_last : 0u);
        if (julia) reference_orbit_wide(cfg, wide, 1, k, o->k_end, resume ? &c->k_end : nullptr, resume ? c->k_last : 0u);
    } else {
        reference_orbit(cfg, key[2], key[3], 0, x, o->x_end, resume ? &c->x_end : nullptr, resume ? c->x_last : 0u);
        if (julia) reference_orbit(cfg, key[2], key[3], 1, k, o->k_end, resume ? &c->k_end : nullptr, resume ? c->k_last : 0u);
    }
    const size_t x_old = resume ? (size_t)c->x_last + 1 : 0, k_old = resume && julia ? (size_t)c->k_last + 1 : 0;
    const size_t x_n = x_old + x.size() / 2, k_n = k_old + k.size() / 2;
    o->algo = cfg->algo;
    o->iterations = cfg->iterations;
    memcpy(o->key, key, sizeof key);
    o->wide_key = std::move(wkey);
    o->x_last = (uint32_t)(x_n - 1);
    o->k_offset = x_n;
    o->k_last = julia ? (uint32_t)(k_n - 1) : o->x_last;
    if (!julia) o->k_end = o->x_end;
    o->computed = (uint32_t)(x.size() / 2 + k.size() / 2);
    if (!resume) ctx.pt_orbit.reset(); /* the previous view's orbit goes first: its memory is free for this one */
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&o->dev), (x_n + k_n) * sizeof(double2)));
    if (x_old) HIP_TRY(hipMemcpyAsync(o->dev, c->dev, x_old * sizeof(double2), hipMemcpyDeviceToDevice, nullptr));
    if (k_old) HIP_TRY(hipMemcpyAsync(o->dev + o->k_offset, c->dev + c->k_offset, k_old * sizeof(double2), hipMemcpyDeviceToDevice, nullptr));
    if (x_old || k_old) HIP_TRY(hipStreamSynchronize(nullptr)); /* the copies are done before a launch on any stream reads them */
    if (!x.empty()) HIP_TRY(hipMemcpy(o->dev + x_old, x.data(), x.size() * sizeof(double), hipMemcpyHostToDevice));
    if (!k.empty()) HIP_TRY(hipMemcpy(o->dev + o->k_offset + k_old, k.data(), k.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx.pt_orbit = o;
    out = std::move(o);
    return FR_OK;
}

template <bool JULIA>
hipError_t launch_state(const fr_kparams &p, uint32_t from, bool extend, double *z, uint32_t *iters, double *dz, uint32_t *m,
                        const PtOrbit *o, hipStream_t stream) {
    dim3 grid, block;
    const hipError_t e = fr_deep_grid(p, grid, block);
    if (e != hipSuccess) return e;
    const double2 *x = o ? o->dev : nullptr, *k = o ? (JULIA ? o->dev + o->k_offset : o->dev) : nullptr;
    const uint32_t x_last = o ? o->x_last : 0u, k_last = o ? o->k_last : 0u, ended = o ? o->ended() : 0u;
    if (extend)
        escape_extend_pt_kernel<JULIA><<<grid, block, 0, stream>>>(p, z, iters, dz, m, from, x, k, x_last, k_last, ended);
    else
        escape_pt_state_kernel<JULIA><<<grid, block, 0, stream>>>(p, z, iters, dz, m, x, k, x_last, k_last, ended);
    return hipGetLastError();
}

}  // namespace

/* what fr_bla.hip needs of this file: the view's orbits in device memory (orbit_for's), and one orbit on the host */
int pt_orbit_view(Ctx &ctx, const fr_config *cfg, const Centre &c, std::shared_ptr<PtOrbit> &keep, PtOrbitView &v) {
    const int rc = orbit_for(ctx, cfg, c, keep);
    if (rc != FR_OK) return rc;
    const bool julia = cfg->algo == 2;
    v.x = keep->dev;
    v.k = julia ? keep->dev + keep->k_offset : keep->dev;
    v.x_last = keep->x_last;
    v.k_last = julia ? keep->k_last : keep->x_last;
    v.ended = keep->ended();
    return FR_OK;
}

void pt_host_orbit(const fr_config *cfg, const Centre &c, int which, std::vector<double> &out) {
    OrbitEnd end;
    if (c.wide)
        reference_orbit_wide(cfg, c.wide, which, out, end);
    else
        reference_orbit(cfg, c.lo_re(), c.lo_im(), which, out, end);
}

int launch_pt(Ctx &ctx, const fr_config *cfg, const Centre &c, const fr_kparams &p, int mode, const fr_kout &out, hipStream_t stream,
              const char **kernel_name) {
    if (kernel_name) *kernel_name = "escape_pt_kernel";
    if (p.ncols == 0 || p.nrows == 0) return FR_OK;
    const bool julia = cfg->algo == 2;
    if (cfg->algo != 0 && !julia) { /* no escape-time algorithm: every pixel is black / zero, as DD's kernel gives */
        HIP_TRY(launch<false>(p, mode, out, nullptr, nullptr, 0, 0, stream));
        return FR_OK;
    }
    std::shared_ptr<PtOrbit> o;
    const int rc = orbit_for(ctx, cfg, c, o);
    if (rc != FR_OK) return rc;
    if (julia) {
        HIP_TRY(launch<true>(p, mode, out, o->dev, o->dev + o->k_offset, o->x_last, o->k_last, stream));
    } else {
        HIP_TRY(launch<false>(p, mode, out, o->dev, o->dev, o->x_last, o->x_last, stream));
    }
    return FR_OK;
}

/* fr_ss_list.h: the refine pass of an adaptive render on plain PT (dd or wide centre), on the orbits the probe made */
int pt_ss_refine(Ctx &ctx, const fr_config *cfg, const Centre &c, const fr_ss_refine &a, uint32_t groups, hipStream_t stream) {
    std::shared_ptr<PtOrbit> o;
    const int rc = orbit_for(ctx, cfg, c, o);
    if (rc != FR_OK) return rc;
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    const bool julia = cfg->algo == 2; /* Mandelbrot: K is X */
    const double2 *const k_orbit = julia ? o->dev + o->k_offset : o->dev;
    const uint32_t k_last = julia ? o->k_last : o->x_last;
    ss_refine_instance(julia, a.linear, [&](auto J, auto L) {
        ss_refine_pt_kernel<J(), L()><<<dim3(groups), dim3(kSsRefineThreads), 0, stream>>>(p, a, o->dev, k_orbit, o->x_last, k_last);
    });
    HIP_TRY(hipGetLastError());
    return FR_OK;
}

/* FR_PRECISION_PT with its resumable state (escape_pt_state_kernel, escape_extend_pt_kernel; include/fractal_hip.h, "resumable
 * perturbation"): the local grid from `p` as launch_pt takes it, z and dz as re, im per pixel, m with bit 31 = on K.  The
 * extension continues the arrays from from_iterations to p.iterations on the orbits of the new cap, which the context's
 * cache continues from those of the old one. */
static int launch_pt_state(Ctx &ctx, const fr_config *cfg, const Centre &c, const fr_kparams &p, double *z, uint32_t *iters, double *dz,
                           uint32_t *m, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "escape_pt_state_kernel";
    if (p.ncols == 0 || p.nrows == 0) return FR_OK;
    const bool julia = cfg->algo == 2;
    if (cfg->algo != 0 && !julia) { /* no escape-time algorithm: zeros in all four arrays */
        HIP_TRY(launch_state<false>(p, 0, false, z, iters, dz, m, nullptr, stream));
        return FR_OK;
    }
    std::shared_ptr<PtOrbit> o;
    const int rc = orbit_for(ctx, cfg, c, o);
    if (rc != FR_OK) return rc;
    HIP_TRY(julia ? launch_state<true>(p, 0, false, z, iters, dz, m, o.get(), stream)
                  : launch_state<false>(p, 0, false, z, iters, dz, m, o.get(), stream));
    return FR_OK;
}

static int launch_pt_extend(Ctx &ctx, const fr_config *cfg, const Centre &c, const fr_kparams &p, uint32_t from_iterations, double *z,
                            uint32_t *iters, double *dz, uint32_t *m, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "escape_extend_pt_kernel";
    const bool julia = cfg->algo == 2;
    if (p.ncols == 0 || p.nrows == 0 || p.iterations <= from_iterations || (cfg->algo != 0 && !julia)) return FR_OK;
    std::shared_ptr<PtOrbit> o;
    const int rc = orbit_for(ctx, cfg, c, o);
    if (rc != FR_OK) return rc;
    HIP_TRY(julia ? launch_state<true>(p, from_iterations, true, z, iters, dz, m, o.get(), stream)
                  : launch_state<false>(p, from_iterations, true, z, iters, dz, m, o.get(), stream));
    return FR_OK;
}

/* ---- resumable perturbation: FR_PRECISION_PT rows with their state, and that state continued to a higher cap ------- */

/* The launch of the state road (fr_ctx.h: state_device, state_host).  from == nullptr: the state render; else the extension
 * from *from.  Into the arrays it is given, between the profiling events. */
static auto pt_state_rows(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1, const uint32_t *from) {
    return [=](Ctx &ctx, double *d_z, uint32_t *d_iters, double *d_dz, uint32_t *d_m, hipStream_t stream) {
        return profiled_rows(cfg, default_opts(), y0, y1, 0, stream, [&](fr_kparams &p, const char *&kname) {
            return from ? launch_pt_extend(ctx, cfg, c, p, *from, d_z, d_iters, d_dz, d_m, stream, &kname)
                        : launch_pt_state(ctx, cfg, c, p, d_z, d_iters, d_dz, d_m, stream, &kname);
        });
    };
}

static int check_pt_rows(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1) {
    const int rc = check_rows(cfg, y0, y1);
    return rc == FR_OK ? c.check(cfg, FR_PRECISION_PT) : rc;
}

static int pt_state_device(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1, const uint32_t *from, void *d_z, void *d_iters,
                           void *d_dz, void *d_m, void *hip_stream) {
    const int rc = check_pt_rows(cfg, c, y0, y1);
    if (rc != FR_OK) return rc;
    return state_device(cfg, y0, y1, from, d_z, d_iters, d_dz, d_m, hip_stream, "PT", "dz", pt_state_rows(cfg, c, y0, y1, from));
}

static int pt_state_host(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1, const uint32_t *from, double *z,
                         uint32_t *iters, double *dz, uint32_t *m) {
    const int rc = check_pt_rows(cfg, c, y0, y1);
    if (rc != FR_OK) return rc;
    return state_host(cfg, y0, y1, from, z, iters, dz, m, "PT", "dz", pt_state_rows(cfg, c, y0, y1, from));
}

/* WIDE PT: a NULL centre must not fall through to the dd road */
static int need_centre(const fr_wide_centre *centre) {
    if (!centre) return fail(FR_ERR_INVALID_ARGUMENT, "FR_PRECISION_PT, wide centre: centre is NULL");
    return FR_OK;
}

}  // namespace fr

int fr_debug_pt_orbit_cache(uint32_t out[4]) {
    using namespace fr;
    if (!out) return fail(FR_ERR_INVALID_ARGUMENT, "out is NULL");
    out[0] = out[1] = out[2] = out[3] = 0;
    LifeShared ls;
    Ctx *ctx = primary_if_created();
    if (!ctx) return FR_OK;
    std::lock_guard<std::mutex> lk(ctx->pt_mu);
    const PtOrbit *o = ctx->pt_orbit.get();
    if (!o) return FR_OK;
    out[0] = o->iterations;
    out[1] = o->x_last + 1;
    out[2] = o->algo == 2 ? o->k_last + 1 : 0;
    out[3] = o->computed;
    return FR_OK;
}

int fr_debug_reference_orbit(const fr_config *cfg, const fr_imaginary *pos_lo, int which, double *out, size_t cap,
                             uint32_t *len) {
    using namespace fr;
    int rc = check_pt(cfg, pos_lo);
    if (rc != FR_OK) return rc;
    if (cfg->algo != 0 && cfg->algo != 2) return fail(FR_ERR_INVALID_ARGUMENT, "FR_PRECISION_PT: orbits exist for Mandelbrot and Julia");
    if (which != 0 && !(which == 1 && cfg->algo == 2))
        return fail(FR_ERR_INVALID_ARGUMENT, "which must be 0 (R or V) or, for Julia, 1 (K)");
    if (!len) return fail(FR_ERR_INVALID_ARGUMENT, "len is NULL");
    if (cap && !out) return fail(FR_ERR_INVALID_ARGUMENT, "out is NULL");
    std::vector<double> v;
    OrbitEnd end;
    reference_orbit(cfg, pos_lo ? pos_lo->re : 0.0, pos_lo ? pos_lo->im : 0.0, which, v, end);
    *len = (uint32_t)(v.size() / 2);
    const size_t n = std::min(cap, v.size() / 2);
    if (n) memcpy(out, v.data(), n * 2 * sizeof(double));
    return FR_OK;
}

/* ---- the calls of the resumable state --------------------------------------------------------------------------------- */

using namespace fr;

int fr_escape_rows_pt_state_device(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, void *d_z,
                                   void *d_iters, void *d_dz, void *d_m, void *hip_stream) {
    return pt_state_device(cfg, Centre{pos_lo, nullptr}, y0, y1, nullptr, d_z, d_iters, d_dz, d_m, hip_stream);
}

int fr_escape_extend_pt_device(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, uint32_t from_iterations,
                               void *d_z, void *d_iters, void *d_dz, void *d_m, void *hip_stream) {
    return pt_state_device(cfg, Centre{pos_lo, nullptr}, y0, y1, &from_iterations, d_z, d_iters, d_dz, d_m, hip_stream);
}

int fr_escape_rows_pt_state(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, double *z, uint32_t *iters,
                            double *dz, uint32_t *m) {
    return pt_state_host(cfg, Centre{pos_lo, nullptr}, y0, y1, nullptr, z, iters, dz, m);
}

int fr_escape_extend_pt(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, uint32_t from_iterations,
                        double *z, uint32_t *iters, double *dz, uint32_t *m) {
    return pt_state_host(cfg, Centre{pos_lo, nullptr}, y0, y1, &from_iterations, z, iters, dz, m);
}

/* ---- WIDE PT (include/fractal_hip.h): the PT calls with a fixed-point view centre in place of (pos, pos_lo) ------------- */

int fr_render_rows_pt_wide(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, int channels, uint8_t *out,
                           size_t out_len) {
    int rc = check_channels(channels);
    if (rc == FR_OK) rc = need_centre(centre);
    if (rc != FR_OK) return rc;
    return fr_host_render_rows_deep(cfg, FR_PRECISION_PT, Centre{nullptr, centre}, y0, y1, out, out_len, (unsigned)channels, nullptr);
}

int fr_render_rows_pt_wide_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, int channels,
                                  void *d_out, size_t out_len, void *hip_stream) {
    int rc = check_channels(channels);
    if (rc == FR_OK) rc = need_centre(centre);
    if (rc != FR_OK) return rc;
    return render_rows_device(cfg, FR_PRECISION_PT, Centre{nullptr, centre}, y0, y1, d_out, out_len, hip_stream, (unsigned)channels, nullptr);
}

int fr_escape_rows_pt_wide(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, double *z, uint32_t *iters) {
    const int rc = need_centre(centre);
    if (rc != FR_OK) return rc;
    return escape_rows(cfg, FR_PRECISION_PT, Centre{nullptr, centre}, y0, y1, z, iters, 2);
}

int fr_escape_rows_pt_wide_state_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, void *d_z,
                                        void *d_iters, void *d_dz, void *d_m, void *hip_stream) {
    const int rc = need_centre(centre);
    if (rc != FR_OK) return rc;
    return pt_state_device(cfg, Centre{nullptr, centre}, y0, y1, nullptr, d_z, d_iters, d_dz, d_m, hip_stream);
}

int fr_escape_extend_pt_wide_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1,
                                    uint32_t from_iterations, void *d_z, void *d_iters, void *d_dz, void *d_m, void *hip_stream) {
    const int rc = need_centre(centre);
    if (rc != FR_OK) return rc;
    return pt_state_device(cfg, Centre{nullptr, centre}, y0, y1, &from_iterations, d_z, d_iters, d_dz, d_m, hip_stream);
}

int fr_escape_rows_pt_wide_state(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, double *z,
                                 uint32_t *iters, double *dz, uint32_t *m) {
    const int rc = need_centre(centre);
    if (rc != FR_OK) return rc;
    return pt_state_host(cfg, Centre{nullptr, centre}, y0, y1, nullptr, z, iters, dz, m);
}

int fr_escape_extend_pt_wide(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, uint32_t from_iterations,
                             double *z, uint32_t *iters, double *dz, uint32_t *m) {
    const int rc = need_centre(centre);
    if (rc != FR_OK) return rc;
    return pt_state_host(cfg, Centre{nullptr, centre}, y0, y1, &from_iterations, z, iters, dz, m);
}
