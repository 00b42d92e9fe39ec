/*
 * fr_de_scaled.hip — DE ON SCALED PT (include/fractal_hip.h, "DE ON SCALED PT"): SCALED PT's pixel loops (fr_scaled.hip:
 * orbit_pt_scaled, orbit_bla_scaled) with a SCALED derivative u = d 2^-e carried beside them, e the exponent of the view's scale.
 * Past a scale of 2^440 the derivative d itself is of the order 2^e at a pixel near the set, so dn2 = |d|^2 leaves f64 from
 * e = 512; u stays where d stays at a scale of 1.  The recurrence is linear in d, so scaling it scales only the constant term:
 * u' = 2 z u + b0 2^-e through a plain step and u' = A u + B 2^-e through a skip.  tests/de_scaled_model.c restates the
 * definition; tests/test_gpu_de_scaled.py compares the two bit for bit.
 *
 * Host part: nothing of its own.  Orbits and tables are the context's (fr_scaled.h: scaled_dev_fill), so a fr_*_pt_scaled call
 * and a DE call of the same view and bits share them.  The distance and the shading are DE's own kernels, run on the scaled view
 * that fr_de_scaled_view writes: no distance or colour kernel is added.
 *
 * Device part: escape_pt_scaled_de_kernel<JULIA> (bits = -1) and escape_bla_scaled_de_kernel<JULIA>, the escape mode of
 * escape_pt_scaled_kernel and escape_bla_scaled_kernel in their shape — a workgroup of 4 waves renders 16 x 16 pixels, each wave
 * one 8 x 8 tile, woff staged in LDS, the level search by bisection over R, a skip's loads behind the branch, 64-bit output
 * offsets, plain vector loads and stores — writing z, iters and der.  The step of w, the search and the tests are the siblings'
 * operation for operation: the derivative only reads, so z and iters are fr_escape_rows_pt_scaled's bit for bit.  The table form
 * keeps escape_bla_de_kernel's ONE arithmetic path for the derivative: nu = (fma(g.re, u.re, fma(-g.im, u.im, b.re)),
 * fma(g.re, u.im, fma(g.im, u.re, b.im))), where a lane that skips takes g = A and b = B Sinv (Julia: (+0, +0)) and a lane that
 * steps takes g = z + z and b = (bs0, -0); fma(x, y, -0) is x * y in every bit, so the stepping lane's imaginary part is the
 * definition's fma(t.re, u.im, t.im * u.re).  The registers, the occupancy and the inner loop:
 * profiles/de_scaled_inner_loop_isa.txt.
 *
 * RESUMABLE SCALED DE (include/fractal_hip.h, "RESUMABLE SCALED DE"; tests/de_scaled_state_model.c restates it;
 * tests/test_gpu_de_scaled_state.py compares the two bit for bit): escape_pt_scaled_de_state_kernel<JULIA> is the plain loop's DE
 * render with RESUMABLE SCALED PT's state rule — no rebase at the end of an orbit that the cap cut — and stores the whole state
 * (z, iters, w, m, der); escape_extend_pt_scaled_de_kernel<JULIA> continues such a state to a higher cap in place, on orbits that
 * fr_pt.hip's cache continued from their integer tails.  They are fr_scaled.hip's escape_pt_scaled_state_kernel and
 * escape_extend_pt_scaled_kernel in their shape, with (ur, ui) carried as orbit_pt_scaled_de carries them; both run
 * orbit_pt_scaled_de_state, the one copy of the state step with the derivative.  escape_pt_scaled_de_kernel and orbit_pt_scaled_de
 * stay as they are.  The table form has no state (BLA-PT's reason: i + 2^k <= iterations).  Registers and occupancy: DESIGN.md 3.27.
 *
 * The host half, at the end of the file, is the three things fr_de.h asks of a road — scaled_de_domain (SCALED PT's domain check,
 * fr_bla.h: scaled_check), scaled_de_launch (the kernel on given parameters, on the context's orbits and tables) and
 * scaled_de_ss_refine — and the calls: the rows are the domain and fr_de.h's device or host form of a three-array row call, the
 * state calls hand their launch, a callable, to RESUMABLE DE's five-array forms (fr_de.h: de_state_device, de_state_host).
 * SUPERSAMPLED SCALED DE (fr_ss_de.hip) renders through the same domain and launch.
 *
 * ADAPTIVE SUPERSAMPLED SCALED DE (include/fractal_hip.h; fr_ss_adaptive_de.hip): ss_refine_de_scaled_kernel<JULIA, BLA, LINEAR>,
 * persistent waves that run orbit_pt_scaled_de / orbit_bla_scaled_de on the s x s samples of the listed pixels through fr_ss_list.h's
 * claim loop, each sample coloured and shaded through fr_ss_de_sample.h; the probe is scaled_de_launch over the strided map
 * (fr_ss_list.h: de_render_map), and scaled_de_ss_refine is the refine launch.  Registers and occupancy: DESIGN.md 3.34.
 */
#include <cmath>
#include <memory>

#include "fr_bla.h"
#include "fr_ctx.h"
#include "fr_de.h"
#include "fr_math.h"
#include "fr_scaled.h"
#include "fr_ss_list.h"
#include "fr_wide.h"

namespace {

#include "fr_colour.h"       /* the refine kernel's colour map and the log2 table */
#include "fr_de_shade.h"     /* de_distance */
#include "fr_ss_de_sample.h" /* ss_de_sample_colour */

/* ---- device: the plain scaled loop with the scaled derivative (bits = -1) ------------------------------------------------ */

/* orbit_pt_scaled (fr_scaled.hip) with u = (ur, ui) beside it.  Returns the escape index (or `iterations`), the final z in
 * (out_re, out_im) and the scaled derivative in (out_ur, out_ui): the returned step's on escape, the last one's on exhaustion,
 * (Sinv, 0) for a cap of 0. */
template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_pt_scaled_de(uint32_t iterations, double woff_re, double woff_im, const ScaledDev &t,
                                                       double squared, double &out_re, double &out_im, double &out_ur, double &out_ui) {
    const double S = t.S, Sinv = t.Sinv;
    const double2 *X = t.x_orbit;
    uint32_t last = t.x_last;
    uint32_t m = JULIA ? 0u : 1u;
    double wr = woff_re, wi = woff_im;
    const double wcr = JULIA ? 0.0 : woff_re, wci = JULIA ? 0.0 : woff_im;
    const double bs0 = JULIA ? 0.0 : Sinv;
    double2 Z = X[m], N = X[min(m + 1u, last)]; /* m <= last - 1 at the top of every step (a cap of 0 takes none) */
    const double2 K1 = t.k_orbit[1];            /* the entry after a rebase; K_0 = R_0 = 0 */
    double zr = __builtin_fma(wr, Sinv, Z.x), zi = __builtin_fma(wi, Sinv, Z.y);
    double ur = Sinv, ui = 0.0; /* u0 = (Sinv, 0) */
    uint32_t i = 0;
    for (; i < iterations; i++) {
        const double2 P = X[min(m + 2u, last)]; /* X_{m+2}: next step's X_{m+1} if it does not rebase */
        const double tr = Z.x + zr, ti = Z.y + zi;
        const double gr = zr + zr, gi = zi + zi; /* the derivative's t: from the z before the step */
        const double nwr = __builtin_fma(tr, wr, __builtin_fma(-ti, wi, wcr));
        const double nwi = __builtin_fma(tr, wi, __builtin_fma(ti, wr, wci));
        const double nur = __builtin_fma(gr, ur, __builtin_fma(-gi, ui, bs0));
        const double nui = __builtin_fma(gr, ui, gi * ur);
        m++;
        zr = __builtin_fma(nwr, Sinv, N.x);
        zi = __builtin_fma(nwi, Sinv, N.y);
        wr = nwr;
        wi = nwi;
        ur = nur; /* escape returns nu; otherwise u = nu */
        ui = nui;
        const double dist = zr * zr + zi * zi;
        if (dist > squared) break; /* this lane leaves EXEC; the wave goes on while any lane is left */
        if (rebase_test(zr, zi, wr, wi, S, Sinv) || m == last) { /* a rebase never touches u */
            wr = zr * S;
            wi = zi * S;
            m = 0;
            if (JULIA) {
                X = t.k_orbit;
                last = t.k_last;
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
    out_ur = ur;
    out_ui = ui;
    return i;
}

/* ---- device: the scaled loop with table skips and the scaled derivative (bits >= 0) ------------------------------------------ */

/* orbit_bla_scaled (fr_scaled.hip) with u beside it, as orbit_bla_de (fr_de_bla.hip) carries d beside orbit_bla */
template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_bla_scaled_de(uint32_t iterations, double woff_re, double woff_im, const ScaledDev &t,
                                                        double squared, double &out_re, double &out_im, double &out_ur, double &out_ui) {
    const double S = t.S, Sinv = t.Sinv;
    const double2 *X = t.x_orbit;
    const double *R = t.x_R, *CF = t.x_coef;
    uint32_t last = t.x_last, n0 = t.x_n0;
    uint32_t m = JULIA ? 0u : 1u;
    double wr = woff_re, wi = woff_im;
    const double wcr = JULIA ? 0.0 : woff_re, wci = JULIA ? 0.0 : woff_im;
    const double bs0 = JULIA ? 0.0 : Sinv;
    double2 Z = X[m]; /* X_m of the orbit followed */
    double zr = __builtin_fma(wr, Sinv, Z.x), zi = __builtin_fma(wi, Sinv, Z.y);
    double ur = Sinv, ui = 0.0; /* u0 = (Sinv, 0) */
    uint32_t i = 0, result = iterations;
    while (i < iterations) {
        /* 1. the level: the largest k in 1 .. kc with (w f)^2 < (R f)^2 (orbit_bla_scaled's search) */
        const uint32_t j = m - 1u;
        uint32_t K = 0;
        if (m >= 1u && j < n0) {
            const double f = is_big(wr, wi) ? Sinv : 1.0;
            const double ar = wr * f, ai = wi * f;
            const double d2 = ar * ar + ai * ai;
            uint32_t kc = j ? (uint32_t)__builtin_ctz(j) : 31u;          /* j % 2^k == 0 */
            kc = min(kc, 31u - (uint32_t)__builtin_clz(n0 - j));         /* (j >> k) < n_k, that is j + 2^k <= n0 */
            kc = min(kc, 31u - (uint32_t)__builtin_clz(iterations - i)); /* i + 2^k <= iterations */
            uint32_t lo = 0, hi = kc;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1u) >> 1;
                const double Rf = R[bla_level_offset(n0, mid) + (j >> mid)] * f;
                if (d2 < Rf * Rf)
                    lo = mid;
                else
                    hi = mid - 1u;
            }
            K = lo;
        }
        /* 2. the step w' = A w + c and the derivative's u' = g u + b — one arithmetic path each, only the loads behind the branch */
        double ar, ai, cr = wcr, ci = wci;
        double gr, gi, br = bs0, bi = -0.0; /* a plain step: fma(g.im, u.re, -0) is g.im * u.re, the definition's product */
        uint32_t step = 1u;
        if (K) {
            const uint32_t e = bla_level_offset(n0, K) + (j >> K);
            if (JULIA) { /* B wc is +0 = wc for every finite B; the derivative's b is (+0, +0) by definition */
                const double2 A = reinterpret_cast<const double2 *>(CF)[e];
                ar = A.x, ai = A.y;
                br = 0.0, bi = 0.0;
            } else {
                const double4 AB = reinterpret_cast<const double4 *>(CF)[e];
                ar = AB.x, ai = AB.y;
                cr = __builtin_fma(AB.z, wcr, -(AB.w * wci));
                ci = __builtin_fma(AB.z, wci, AB.w * wcr);
                br = AB.z * Sinv, bi = AB.w * Sinv;
            }
            gr = ar, gi = ai;
            step = 1u << K;
        } else {
            ar = Z.x + zr, ai = Z.y + zi; /* t = X_m + z */
            gr = zr + zr, gi = zi + zi;   /* the derivative's t: from the z before the step */
        }
        const double nwr = __builtin_fma(ar, wr, __builtin_fma(-ai, wi, cr));
        const double nwi = __builtin_fma(ar, wi, __builtin_fma(ai, wr, ci));
        const double nur = __builtin_fma(gr, ur, __builtin_fma(-gi, ui, br));
        const double nui = __builtin_fma(gr, ui, __builtin_fma(gi, ur, bi));
        m += step;
        i += step;
        const double2 N = X[min(m, last)]; /* m <= last: 1 + ((j >> K) + 1) 2^K <= 1 + n0 */
        zr = __builtin_fma(nwr, Sinv, N.x);
        zi = __builtin_fma(nwi, Sinv, N.y);
        wr = nwr;
        wi = nwi;
        ur = nur; /* escape returns nu; otherwise u = nu */
        ui = nui;
        /* 3. the tests, the plain scaled loop's; a rebase never touches u */
        const double dist = zr * zr + zi * zi;
        if (dist > squared) { /* this lane leaves EXEC; the wave goes on while any lane is left */
            result = i - 1u;
            break;
        }
        if (rebase_test(zr, zi, wr, wi, S, Sinv) || m == last) {
            wr = zr * S;
            wi = zi * S;
            m = 0;
            if (JULIA) {
                X = t.k_orbit;
                R = t.k_R;
                CF = t.k_coef;
                last = t.k_last;
                n0 = t.k_n0;
            }
            Z = make_double2(0.0, 0.0); /* K_0 = R_0 = 0 */
        } else {
            Z = N;
        }
    }
    out_re = zr;
    out_im = zi;
    out_ur = ur;
    out_ui = ui;
    return result;
}

/* ---- device: the kernels: one body, the loop chosen by BLA ----------------------------------------------------------------- */

template <bool JULIA, bool BLA>
__device__ __forceinline__ void scaled_de_body(const fr_kparams &p, double *__restrict__ z, uint32_t *__restrict__ iters,
                                               double *__restrict__ der, const ScaledDev &t) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];

    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kDeepBlockW - 1) / kDeepBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t col0 = bx * kDeepBlockW, row0 = by * kDeepBlockH;
    stage_woff(p, tid, col0, row0, s_re, s_im);
    __syncthreads();

    const uint32_t wave = tid >> 6, lane = tid & 63;
    const uint32_t lx = (wave % kDeepWavesX) * kDeepTileW + lane % kDeepTileW;
    const uint32_t ly = (wave / kDeepWavesX) * kDeepTileH + lane / kDeepTileW;
    const uint32_t cx = col0 + lx, r = row0 + ly;
    if (!(cx < p.ncols && r < p.nrows)) return;
    const bool escape_algo = JULIA ? p.algo == 2 : p.algo == 0; /* the host picks JULIA from the algorithm */

    double zr = 0.0, zi = 0.0, ur = 0.0, ui = 0.0; /* an algorithm without orbits writes zeros */
    uint32_t it = 0;
    if (escape_algo) {
        const double squared = p.limit * p.limit; /* calc/src/lib.rs:246 */
        if constexpr (BLA)
            it = orbit_bla_scaled_de<JULIA>(p.iterations, s_re[lx], s_im[ly], t, squared, zr, zi, ur, ui);
        else
            it = orbit_pt_scaled_de<JULIA>(p.iterations, s_re[lx], s_im[ly], t, squared, zr, zi, ur, ui);
    }
    const uint64_t k = (uint64_t)r * p.ncols + cx;
    z[2 * k] = zr;
    z[2 * k + 1] = zi;
    iters[k] = it;
    der[2 * k] = ur;
    der[2 * k + 1] = ui;
}

template <bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_pt_scaled_de_kernel(const fr_kparams p, double *__restrict__ z,
                                                                              uint32_t *__restrict__ iters, double *__restrict__ der,
                                                                              const ScaledDev t) {
    scaled_de_body<JULIA, false>(p, z, iters, der, t);
}

template <bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_bla_scaled_de_kernel(const fr_kparams p, double *__restrict__ z,
                                                                               uint32_t *__restrict__ iters, double *__restrict__ der,
                                                                               const ScaledDev t) {
    scaled_de_body<JULIA, true>(p, z, iters, der, t);
}

hipError_t launch(bool julia, bool bla, const fr_kparams &p, double *z, uint32_t *iters, double *der, const ScaledDev &t,
                  hipStream_t stream) {
    dim3 grid, block;
    const hipError_t e = fr_deep_grid(p, grid, block);
    if (e != hipSuccess) return e;
    if (bla) {
        if (julia)
            escape_bla_scaled_de_kernel<true><<<grid, block, 0, stream>>>(p, z, iters, der, t);
        else
            escape_bla_scaled_de_kernel<false><<<grid, block, 0, stream>>>(p, z, iters, der, t);
    } else {
        if (julia)
            escape_pt_scaled_de_kernel<true><<<grid, block, 0, stream>>>(p, z, iters, der, t);
        else
            escape_pt_scaled_de_kernel<false><<<grid, block, 0, stream>>>(p, z, iters, der, t);
    }
    return hipGetLastError();
}

/* ---- device: ADAPTIVE SUPERSAMPLED SCALED DE's refine pass (include/fractal_hip.h; fr_ss_list.h: the claim loop) --------------- */

/* ss_refine_de_bla_kernel (fr_de_bla.hip) with the scaled DE loops: `woff` by stage_woff's formula on cfg_s (`p` holds cfg_s with
 * the scaled divisors sre, sim, as ss_refine_scaled_kernel has them), the loop chosen by BLA, the table built with Dw over the
 * whole image of cfg_s; sh.pixels is the scaled view's last factor of D, sh.thickness is Ts */
template <bool JULIA, bool BLA, bool LINEAR>
__global__ __launch_bounds__(kSsRefineThreads) void ss_refine_de_scaled_kernel(const fr_kparams p, const fr_ss_refine a,
                                                                               const fr_ss_de_shade sh, const ScaledDev t) {
    __shared__ double s_tab[FR_LOG2_N * 3];
    const double *gt = &g_log2_tab[0][0];
    for (uint32_t k = threadIdx.x; k < FR_LOG2_N * 3; k += kSsRefineThreads) s_tab[k] = gt[k];
    const uint16_t *const s_lt = ss_refine_tables<LINEAR>(); /* LINEAR-LIGHT SUPERSAMPLING: staged with the log2 table */
    __syncthreads();
    const double width = (double)p.width, height = (double)p.height;
    const double squared = p.limit * p.limit;
    ss_refine_loop<LINEAR>(a, s_lt, [&](uint64_t x, uint64_t y) {
        const double woff_re = (((double)x / height) - ((width / height) / 2.0)) / p.scale_re;
        const double woff_im = (((double)y / height) - 0.5) / p.scale_im;
        double zr, zi, ur, ui;
        uint32_t it;
        if constexpr (BLA)
            it = orbit_bla_scaled_de<JULIA>(p.iterations, woff_re, woff_im, t, squared, zr, zi, ur, ui);
        else
            it = orbit_pt_scaled_de<JULIA>(p.iterations, woff_re, woff_im, t, squared, zr, zi, ur, ui);
        return ss_de_sample_colour(p, zr, zi, ur, ui, it, sh.pixels, sh.thickness, s_tab);
    });
}

hipError_t launch_refine(bool julia, bool bla, const fr_kparams &p, const fr_ss_refine &a, const fr_ss_de_shade &sh, const ScaledDev &t,
                         uint32_t groups, hipStream_t stream) {
    const dim3 grid(groups), block(kSsRefineThreads);
    if (bla)
        fr::ss_refine_instance(julia, a.linear, [&](auto J, auto L) {
            ss_refine_de_scaled_kernel<J(), true, L()><<<grid, block, 0, stream>>>(p, a, sh, t);
        });
    else
        fr::ss_refine_instance(julia, a.linear, [&](auto J, auto L) {
            ss_refine_de_scaled_kernel<J(), false, L()><<<grid, block, 0, stream>>>(p, a, sh, t);
        });
    return hipGetLastError();
}

/* ---- device: the resumable state of the plain scaled loop with the scaled derivative (include/fractal_hip.h, "RESUMABLE SCALED
 * DE") ------------------------------------------------------------------------------------------------------------------------- */

/* A pixel's state between steps: RESUMABLE SCALED PT's (z, w, m, onK) with u beside it.  orbit_pt_scaled_de_state is
 * orbit_pt_scaled_state (fr_scaled.hip) with (ur, ui) carried as orbit_pt_scaled_de carries them: `steps` steps of the plain
 * scaled loop from the state with the state rule's rebase condition — the scaled rebase test, or m == last of an orbit that is
 * ENDED BY ESCAPE (x_end / k_end: that last index, or ~0 for an orbit cut by the cap, which m never equals) — and the state
 * after the last step left in `s`; on escape that is (z, 0, 0) with nu kept.  Returns the steps completed before the escape
 * (`steps`: none).  t.x_last / t.k_last only clamp the loads. */
struct ScaledDeState {
    double zr, zi, wr, wi, ur, ui;
    uint32_t m;
    bool on_k;
};

template <bool JULIA>
__device__ __forceinline__ uint32_t orbit_pt_scaled_de_state(uint32_t steps, double wcr, double wci, const ScaledDev &t, uint32_t x_end,
                                                             uint32_t k_end, double squared, ScaledDeState &s) {
    const double S = t.S, Sinv = t.Sinv;
    const bool on_k = JULIA && s.on_k;
    const double2 *X = on_k ? t.k_orbit : t.x_orbit;
    uint32_t last = on_k ? t.k_last : t.x_last, end = on_k ? k_end : x_end;
    uint32_t m = s.m;
    bool k_now = on_k;
    const double bs0 = JULIA ? 0.0 : Sinv;
    double wr = s.wr, wi = s.wi, zr = s.zr, zi = s.zi, ur = s.ur, ui = s.ui;
    double2 Z = X[min(m, last)], N = X[min(m + 1u, last)]; /* m < last at the top of every step */
    const double2 K1 = t.k_orbit[1];                       /* the entry after a rebase; K_0 = R_0 = 0 */
    uint32_t i = 0;
    for (; i < steps; i++) {
        const double2 P = X[min(m + 2u, last)]; /* X_{m+2}: next step's X_{m+1} if it does not rebase */
        const double tr = Z.x + zr, ti = Z.y + zi;
        const double gr = zr + zr, gi = zi + zi; /* the derivative's t: from the z before the step */
        const double nwr = __builtin_fma(tr, wr, __builtin_fma(-ti, wi, wcr));
        const double nwi = __builtin_fma(tr, wi, __builtin_fma(ti, wr, wci));
        const double nur = __builtin_fma(gr, ur, __builtin_fma(-gi, ui, bs0));
        const double nui = __builtin_fma(gr, ui, gi * ur);
        m++;
        zr = __builtin_fma(nwr, Sinv, N.x);
        zi = __builtin_fma(nwi, Sinv, N.y);
        wr = nwr;
        wi = nwi;
        ur = nur; /* escape keeps nu; otherwise u = nu */
        ui = nui;
        const double dist = zr * zr + zi * zi;
        if (dist > squared) break; /* this lane leaves EXEC; the wave goes on while any lane is left */
        if (rebase_test(zr, zi, wr, wi, S, Sinv) || m == end) { /* a rebase never touches u */
            wr = zr * S;
            wi = zi * S;
            m = 0;
            if (JULIA) {
                X = t.k_orbit;
                last = t.k_last;
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
    const bool escaped = i < steps; /* (z, 0, 0) for an escaped lane, nu kept */
    s.zr = zr;
    s.zi = zi;
    s.wr = escaped ? 0.0 : wr;
    s.wi = escaped ? 0.0 : wi;
    s.ur = ur;
    s.ui = ui;
    s.m = escaped ? 0u : m;
    s.on_k = !escaped && k_now;
    return i;
}

__device__ __forceinline__ void scaled_de_state_store(uint64_t k, double *z, uint32_t *iters, double *w, uint32_t *mm, double *der,
                                                      const ScaledDeState &s, uint32_t it) {
    z[2 * k] = s.zr;
    z[2 * k + 1] = s.zi;
    iters[k] = it;
    w[2 * k] = s.wr;
    w[2 * k + 1] = s.wi;
    mm[k] = s.m | (s.on_k ? kOnK : 0u);
    der[2 * k] = s.ur;
    der[2 * k + 1] = s.ui;
}

/* escape_pt_scaled_state_kernel's shape (fr_scaled.hip) with the derivative: the whole state, 56 bytes per pixel, five stores.
 * `ended`: bit 0 = X, bit 1 = K is ended by escape.  An algorithm without orbits writes zeros into all five arrays. */
template <bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_pt_scaled_de_state_kernel(const fr_kparams p, double *__restrict__ z,
                                                                                    uint32_t *__restrict__ iters, double *__restrict__ w,
                                                                                    uint32_t *__restrict__ mm, double *__restrict__ der,
                                                                                    const ScaledDev t, const uint32_t ended) {
    __shared__ double s_re[kDeepBlockW];
    __shared__ double s_im[kDeepBlockH];

    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)p.ncols + kDeepBlockW - 1) / kDeepBlockW);
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const uint32_t col0 = bx * kDeepBlockW, row0 = by * kDeepBlockH;
    stage_woff(p, tid, col0, row0, s_re, s_im);
    __syncthreads();

    const uint32_t wave = tid >> 6, lane = tid & 63;
    const uint32_t lx = (wave % kDeepWavesX) * kDeepTileW + lane % kDeepTileW;
    const uint32_t ly = (wave / kDeepWavesX) * kDeepTileH + lane / kDeepTileW;
    const uint32_t cx = col0 + lx, r = row0 + ly;
    if (cx >= p.ncols || r >= p.nrows) return;
    const bool escape_algo = JULIA ? p.algo == 2 : p.algo == 0; /* the host picks JULIA from the algorithm */

    ScaledDeState s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u, false};
    uint32_t it = 0;
    if (escape_algo) {
        const double woff_re = s_re[lx], woff_im = s_im[ly];
        s.m = JULIA ? 0u : 1u;
        s.wr = woff_re;
        s.wi = woff_im;
        const double2 X0 = t.x_orbit[min(s.m, t.x_last)];
        s.zr = __builtin_fma(s.wr, t.Sinv, X0.x);
        s.zi = __builtin_fma(s.wi, t.Sinv, X0.y);
        s.ur = t.Sinv; /* u0 = (Sinv, 0) */
        it = orbit_pt_scaled_de_state<JULIA>(p.iterations, JULIA ? 0.0 : woff_re, JULIA ? 0.0 : woff_im, t, (ended & 1u) ? t.x_last : ~0u,
                                             (ended & 2u) ? t.k_last : ~0u, p.limit * p.limit, s);
    }
    scaled_de_state_store((uint64_t)r * p.ncols + cx, z, iters, w, mm, der, s, it);
}

/* escape_extend_pt_scaled_kernel's shape (fr_scaled.hip) with the derivative: the stored state continued from cap `from` to
 * p.iterations in place, on the orbits of the new cap.  `iters` is read first and a workgroup with no pixel at `from` ends there,
 * having written nothing; a finished pixel's z, w, m and der are neither loaded nor stored. */
template <bool JULIA>
__global__ __launch_bounds__(64 * kDeepWaves) void escape_extend_pt_scaled_de_kernel(const fr_kparams p, double *z, uint32_t *iters, double *w,
                                                                                     uint32_t *mm, double *der, const uint32_t from,
                                                                                     const ScaledDev t, const uint32_t ended) {
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

    if (!JULIA) { /* wc = the pixel's woff, staged as the render stages it; Julia's wc is 0 */
        stage_woff(p, tid, col0, row0, s_re, s_im);
        __syncthreads();
    }
    if (!running) return;
    const uint32_t word = mm[k];
    ScaledDeState s;
    s.zr = z[2 * k];
    s.zi = z[2 * k + 1];
    s.wr = w[2 * k];
    s.wi = w[2 * k + 1];
    s.ur = der[2 * k];
    s.ui = der[2 * k + 1];
    s.on_k = JULIA && (word & kOnK) != 0;
    /* m < last of the orbit followed in every state this view produces; the clamp keeps foreign data inside the orbit */
    s.m = min(word & ~kOnK, (s.on_k ? t.k_last : t.x_last) - 1u);
    const uint32_t it = orbit_pt_scaled_de_state<JULIA>(p.iterations - from, JULIA ? 0.0 : s_re[lx], JULIA ? 0.0 : s_im[ly], t,
                                                        (ended & 1u) ? t.x_last : ~0u, (ended & 2u) ? t.k_last : ~0u, p.limit * p.limit, s);
    scaled_de_state_store(k, z, iters, w, mm, der, s, from + it); /* it == M - N on exhaustion: the new cap */
}

/* the state render, or — extend — the extension from `from` */
template <bool JULIA>
hipError_t launch_state(const fr_kparams &p, uint32_t from, bool extend, double *z, uint32_t *iters, double *w, uint32_t *m, double *der,
                        const ScaledDev &t, uint32_t ended, hipStream_t stream) {
    dim3 grid, block;
    const hipError_t e = fr_deep_grid(p, grid, block);
    if (e != hipSuccess) return e;
    if (extend)
        escape_extend_pt_scaled_de_kernel<JULIA><<<grid, block, 0, stream>>>(p, z, iters, w, m, der, from, t, ended);
    else
        escape_pt_scaled_de_state_kernel<JULIA><<<grid, block, 0, stream>>>(p, z, iters, w, m, der, t, ended);
    return hipGetLastError();
}

}  // namespace

using namespace fr;

namespace {

/* ---- RESUMABLE SCALED DE: the plain loop's rows with their DE state, and that state continued to a higher cap ---------------- */

/* de_state_device's / de_state_host's callable (fr_de.h): the state render (from == nullptr) or its extension from *from between
 * the profiling events, on the context's orbits of cfg's cap, which pt_orbit_view's cache continues from those of a lower cap of
 * the same view and shares with every other scaled or wide call of it */
auto scaled_de_state_rows(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1, const uint32_t *from) {
    return [=](Ctx &ctx, double *d_z, uint32_t *d_iters, double *d_w, uint32_t *d_m, double *d_der, hipStream_t stream) {
        return profiled_rows(cfg, default_opts(), y0, y1, 0, stream, [&](fr_kparams &p, const char *&kname) -> int {
            kname = from ? "escape_extend_pt_scaled_de_kernel" : "escape_pt_scaled_de_state_kernel";
            const bool julia = cfg->algo == FR_ALGO_JULIA, extend = from != nullptr;
            if (p.ncols == 0 || p.nrows == 0) return FR_OK;
            if (cfg->algo != FR_ALGO_MANDELBROT && !julia) { /* no escape-time algorithm: zeros in all five arrays (the extension never gets here) */
                HIP_TRY(launch_state<false>(p, 0, false, d_z, d_iters, d_w, d_m, d_der, ScaledDev{}, 0, stream));
                return FR_OK;
            }
            const ScaledConsts k = scaled_consts(cfg);
            p.scale_re = k.sre;
            p.scale_im = k.sim;
            std::shared_ptr<PtOrbit> orbit; /* alive until the launch is enqueued */
            PtOrbitView v;
            const int rc = pt_orbit_view(ctx, cfg, c, orbit, v);
            if (rc != FR_OK) return rc;
            ScaledDev t{};
            t.x_orbit = v.x;
            t.k_orbit = v.k;
            t.x_last = v.x_last;
            t.k_last = v.k_last;
            t.S = k.S;
            t.Sinv = k.Sinv;
            const uint32_t n = extend ? *from : 0u;
            HIP_TRY(julia ? launch_state<true>(p, n, extend, d_z, d_iters, d_w, d_m, d_der, t, v.ended, stream)
                          : launch_state<false>(p, n, extend, d_z, d_iters, d_w, d_m, d_der, t, v.ended, stream));
            return FR_OK;
        });
    };
}

/* the state calls are the plain loop's: SCALED PT's domain with bits = -1 and the centre required */
int scaled_de_state_domain(const fr_config *cfg, const Centre &c, uint32_t y0, uint32_t y1) {
    int bits = -1;
    return scaled_check(cfg, c, bits, y0, y1);
}

int scaled_de_state_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, const uint32_t *from, void *d_z,
                           void *d_iters, void *d_w, void *d_m, void *d_der, void *hip_stream) {
    const Centre c{nullptr, centre, true};
    const int rc = scaled_de_state_domain(cfg, c, y0, y1);
    if (rc != FR_OK) return rc;
    return de_state_device(cfg, y0, y1, from, d_z, d_iters, d_w, d_m, d_der, hip_stream, "SCALED PT", "w",
                           scaled_de_state_rows(cfg, c, y0, y1, from));
}

int scaled_de_state_host(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, const uint32_t *from, double *z,
                         uint32_t *iters, double *w, uint32_t *m, double *der) {
    const Centre c{nullptr, centre, true};
    const int rc = scaled_de_state_domain(cfg, c, y0, y1);
    if (rc != FR_OK) return rc;
    return de_state_host(cfg, y0, y1, from, z, iters, w, m, der, "SCALED PT", "w", scaled_de_state_rows(cfg, c, y0, y1, from));
}

}  // namespace

/* fr_de.h: the road's domain and its launch; fr_ss_list.h: its refine launch */
namespace fr {

/* SCALED PT's domain (bits resolved in place; its limit <= 2^20 is DE's too) */
int scaled_de_domain(const fr_config *cfg, const Centre &c, int &bits, uint32_t y0, uint32_t y1) { return scaled_check(cfg, c, bits, y0, y1); }

/* on the context's orbits and tables; `p` holds the view's scale, the kernels get a copy with the scaled divisors */
int scaled_de_launch(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_kparams &p, double *d_z, uint32_t *d_iters,
                     double *d_der, hipStream_t stream, const char *&kname) {
    kname = bits < 0 ? "escape_pt_scaled_de_kernel" : "escape_bla_scaled_de_kernel";
    if (p.ncols == 0 || p.nrows == 0) return FR_OK;
    const bool julia = cfg->algo == FR_ALGO_JULIA, bla = bits >= 0;
    if (cfg->algo != FR_ALGO_MANDELBROT && !julia) { /* no escape-time algorithm: zeros, and no orbit is asked for */
        HIP_TRY(launch(false, bla, p, d_z, d_iters, d_der, ScaledDev{}, stream));
        return FR_OK;
    }
    const ScaledConsts k = scaled_consts(cfg);
    fr_kparams ps = p;
    ps.scale_re = k.sre;
    ps.scale_im = k.sim;
    std::shared_ptr<PtOrbit> orbit; /* alive until the launch is enqueued, like the table */
    std::shared_ptr<BlaTable> table;
    ScaledDev t;
    const int rc = scaled_dev_fill(ctx, cfg, c, bits, k, orbit, table, t);
    if (rc != FR_OK) return rc;
    HIP_TRY(launch(julia, bla, ps, d_z, d_iters, d_der, t, stream));
    return FR_OK;
}

int scaled_de_ss_refine(Ctx &ctx, const fr_config *cfg, const Centre &c, int bits, const fr_ss_refine &a, const fr_ss_de_shade &sh,
                        uint32_t groups, hipStream_t stream) {
    const ScaledConsts k = scaled_consts(cfg);
    fr_kparams p;
    fill_params(cfg, default_opts(), p);
    p.scale_re = k.sre;
    p.scale_im = k.sim;
    std::shared_ptr<PtOrbit> orbit; /* alive until the launch is enqueued, like the table */
    std::shared_ptr<BlaTable> table;
    ScaledDev t;
    const int rc = scaled_dev_fill(ctx, cfg, c, bits, k, orbit, table, t);
    if (rc != FR_OK) return rc;
    HIP_TRY(launch_refine(cfg->algo == FR_ALGO_JULIA, bits >= 0, p, a, sh, t, groups, stream));
    return FR_OK;
}

}  // namespace fr

extern "C" {

/* ---- the calls of RESUMABLE SCALED DE (the plain loop's: no bits) -------------------------------------------------------------- */

int fr_escape_rows_de_pt_scaled_state_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, void *d_z,
                                             void *d_iters, void *d_w, void *d_m, void *d_der, void *hip_stream) {
    return scaled_de_state_device(cfg, centre, y0, y1, nullptr, d_z, d_iters, d_w, d_m, d_der, hip_stream);
}

int fr_escape_rows_de_pt_scaled_state(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, double *z,
                                      uint32_t *iters, double *w, uint32_t *m, double *der) {
    return scaled_de_state_host(cfg, centre, y0, y1, nullptr, z, iters, w, m, der);
}

int fr_escape_extend_de_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1,
                                         uint32_t from_iterations, void *d_z, void *d_iters, void *d_w, void *d_m, void *d_der,
                                         void *hip_stream) {
    return scaled_de_state_device(cfg, centre, y0, y1, &from_iterations, d_z, d_iters, d_w, d_m, d_der, hip_stream);
}

int fr_escape_extend_de_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, uint32_t from_iterations,
                                  double *z, uint32_t *iters, double *w, uint32_t *m, double *der) {
    return scaled_de_state_host(cfg, centre, y0, y1, &from_iterations, z, iters, w, m, der);
}

int fr_escape_rows_de_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1, void *d_z,
                                       void *d_iters, void *d_der, void *hip_stream) {
    const Centre c{nullptr, centre, true};
    const int rc = scaled_de_domain(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return de_rows_device(cfg, y0, y1, d_z, d_iters, d_der, hip_stream, de_rows(cfg, y0, y1, de_road(scaled_de_launch, cfg, c, bits)));
}

int fr_escape_rows_de_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1, double *z,
                                uint32_t *iters, double *der) {
    const Centre c{nullptr, centre, true};
    const int rc = scaled_de_domain(cfg, c, bits, y0, y1);
    if (rc != FR_OK) return rc;
    return de_rows_host(cfg, y0, y1, z, iters, der, de_rows(cfg, y0, y1, de_road(scaled_de_launch, cfg, c, bits)));
}

int fr_de_scaled_view(const fr_config *cfg, fr_config *view) {
    if (!cfg) return fail(FR_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (!view) return fail(FR_ERR_INVALID_ARGUMENT, "view is NULL");
    /* SCALED PT's rules about the scale (fr_wide.hip: check_pt_wide), which are what the constants of a view rest on */
    const double sre = std::fabs(cfg->scale.re), sim = std::fabs(cfg->scale.im);
    if (!std::isfinite(sre) || !std::isfinite(sim)) return fail(FR_ERR_INVALID_ARGUMENT, "SCALED PT: the scale of the view must be finite");
    if (sre < 0x1p-64 || sim < 0x1p-64) return fail(FR_ERR_INVALID_ARGUMENT, "SCALED PT: |scale| must be >= 2^-64 on both axes");
    if ((sre < sim ? sre : sim) < 0x1p-32 * (sre > sim ? sre : sim))
        return fail(FR_ERR_INVALID_ARGUMENT, "SCALED PT: min |scale| must be >= 2^-32 max |scale| over the two axes");
    const ScaledConsts k = scaled_consts(cfg);
    if (view != cfg) *view = *cfg;
    view->scale.re = k.sre;
    view->scale.im = k.sim;
    return FR_OK;
}

} /* extern "C" */
